"""The fence protocol's own controls (tests/fence.py), on the CPU: stand-in `calls` in plain torch that each break one clause of
the memory contract must fail with that clause's message, a clean one must pass under both patterns at both placements; the
layout the arena promises; and a completeness check over text: every streamed entry point of include/dff.h has a Spec in a
test file that fences.  No GPU, no library."""
import glob
import os
import re

import pytest
import torch

import fence
from fence import BAND, COMBINATIONS, fenced
from stream_gate import Spec

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = 37                                                  # (no multiple of anything)


def _neighbour(t, k):
    """The element `k` places after the END of t (k = 0: the first one past it; k < 0 counts back from its START) as a
    one-element view of the same storage, or None where the storage ends first -- the separate allocations of the reference
    run, where the stray access of a real kernel would have hit the allocator's padding."""
    o = t.storage_offset() + (t.numel() + k if k >= 0 else k)
    if o < 0 or o >= t.untyped_storage().nbytes() // t.element_size():
        return None
    return torch.as_strided(t, (1,), (1,), o)


def clean(_, b):
    torch.add(b["x"], 1.0, out=b["y"])
    b["acc"] += b["x"].double().sum()
    b["ws"][1:] = 3.0                                   # a workspace may be written (element 0 stays as it arrived)


def writes_past_output(_, b):
    clean(_, b)
    byte = _neighbour(b["y"].view(torch.uint8), 0)
    if byte is not None:
        byte.fill_(1)


def writes_before_workspace(_, b):
    clean(_, b)
    byte = _neighbour(b["ws"].view(torch.uint8), -1)
    if byte is not None:
        byte.fill_(1)


def writes_input(_, b):
    clean(_, b)
    b["x"][3] = 7.0


def reads_past_input(_, b):
    clean(_, b)
    stray = _neighbour(b["x"], 0)
    if stray is not None:
        b["y"][0] += stray[0]


def reads_workspace(_, b):
    first = b["ws"][0].clone()
    clean(_, b)
    b["y"][0] += first


def leaves_output_unwritten(_, b):
    torch.add(b["x"][:-1], 1.0, out=b["y"][:-1])
    b["acc"] += b["x"].double().sum()


def spec(fn):
    """x a pure input, y an output, acc in-out, ws a workspace of N floats that arrives zeroed in the reference run"""
    x = torch.arange(N, dtype=torch.float32) * 0.5 + 0.25              # (x + 1 is never the sentinel)
    return Spec("control", {"x": (x, float("nan")), "acc": (torch.tensor([2.0], dtype=torch.float64), float("nan"))},
                {"y": ((N,), torch.float32)}, fn, inout=("acc",), work={"ws": torch.zeros(N, dtype=torch.float32)})


@pytest.mark.parametrize("pattern,placement", COMBINATIONS)
def test_control_a_clean_call_passes(pattern, placement):
    got = fenced(spec(clean), pattern=pattern, placement=placement)
    assert torch.equal(got.bufs["y"], spec(clean).ins["x"][0] + 1.0) and float(got.bufs["acc"]) == 2.0 + float(spec(clean).ins["x"][0].sum())


@pytest.mark.parametrize("pattern,placement", COMBINATIONS)
@pytest.mark.parametrize("fn,message", [
    (writes_past_output, r"guard band damaged: 1 byte\(s\), the first 1 byte\(s\) past the end of y, the last 1 byte\(s\) past the end of y"),
    (writes_before_workspace, r"guard band damaged: 1 byte\(s\), the first 1 byte\(s\) before the start of ws, the last 1 byte"),
    (writes_input, "the pure input x was written to"),
    (leaves_output_unwritten, "a sentinel survives in y"),
], ids=["a-past-an-output", "b-before-a-workspace", "c-into-an-input", "f-output-unwritten"])
def test_control_the_fence_catches(fn, message, pattern, placement):
    """(a), (b), (c), (f): caught under either pattern at either placement."""
    with pytest.raises(AssertionError, match=message):
        fenced(spec(fn), pattern=pattern, placement=placement)


@pytest.mark.parametrize("placement", fence.PLACEMENTS)
@pytest.mark.parametrize("fn", [reads_past_input, reads_workspace], ids=["d-past-an-input", "e-workspace-contents"])
def test_control_the_fence_catches_a_stray_read(fn, placement):
    """(d), (e): a stray read that finds zeros adds nothing -- that is how such a bug hides in the allocator's padding, and why
    every fence runs under 0xFF as well, where the same read finds a NaN and the result differs."""
    fenced(spec(fn), pattern=0x00, placement=placement)
    with pytest.raises(AssertionError, match="y differs from the same call on separate allocations"):
        fenced(spec(fn), pattern=0xFF, placement=placement)


def test_control_a_long_overrun_lands_in_checked_memory():
    """An overrun longer than a band: it runs through the next buffer into the band after it; first and last are reported
    against the buffers they are nearest to."""
    def fn(_, b):
        clean(_, b)
        yb = b["y"].view(torch.uint8)
        o = yb.storage_offset() + yb.numel()
        if o + 2 * BAND < yb.untyped_storage().nbytes():
            wb = b["ws"].view(torch.uint8)
            torch.as_strided(yb, (wb.storage_offset() + wb.numel() + 5 - o,), (1,), o).fill_(1)     # the band, ws, five bytes more
    with pytest.raises(AssertionError, match=r"the first 1 byte\(s\) past the end of y, the last 5 byte\(s\) past the end of ws"):
        fenced(spec(fn), pattern=0xFF, placement="tight")


def test_the_layout():
    """natural: every buffer at a multiple of 256; tight: at its documented alignment and at no larger one (an 8-byte aligned
    workspace at 8 mod 16, an array at sizeof(element) mod 16); either way at least BAND bytes between two buffers and at both
    ends, every byte a buffer or a band, every buffer exactly its own length."""
    sp = Spec("layout", {"f": (torch.zeros(5), 0.0), "d": (torch.zeros(3, dtype=torch.float64), 0.0), "b": (torch.zeros(7, dtype=torch.uint8), 0),
                         "st": (torch.zeros(8, dtype=torch.int32), 0)},
              {"l": ((3, 3), torch.int64), "h": ((9,), torch.int32)}, lambda _, b: (b["l"].zero_(), b["h"].zero_()),
              work={"ws": torch.zeros(41, dtype=torch.uint8)})
    want = {"f": 4, "d": 8, "b": 1, "st": 8, "l": 8, "h": 4, "ws": 8}
    for pattern, placement in COMBINATIONS:
        got = fenced(sp, pattern=pattern, placement=placement, align={"st": 8})
        base, at = got.arena.data_ptr(), 0
        assert [s.name for s in got.slots] == list(want)
        for s in got.slots:
            p = got.bufs[s.name].data_ptr()
            assert p == base + s.start and s.start - at >= BAND and s.nbytes == got.bufs[s.name].numel() * got.bufs[s.name].element_size()
            assert p % 256 == 0 if placement == "natural" else p % 16 == want[s.name], (s.name, placement, p % 256)
            at = s.end
        assert got.total - at == BAND and got.arena.numel() == got.total
        assert got.slots[-1].nbytes == 41                                        # the workspace is not rounded up
    with pytest.raises(AssertionError, match="buffers the Spec does not have"):
        fenced(sp, align={"nope": 8})


def test_every_streamed_entry_point_is_fenced():
    """Text only: an entry point of include/dff.h that takes a `void* stream` must appear as Spec("name" in a tests/*.py file
    that calls fenced( -- a new ABI call cannot ship without a fence."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dff.h")).read(), flags=re.S)
    streamed = [m.group(1) for m in re.finditer(r"\b(dff_\w+)\s*\(([^;{}]*?)\)\s*;", text) if re.search(r"void\s*\*\s*stream\b", m.group(2))]
    assert len(streamed) >= 38 and "dff_score" in streamed and "dff_resampled_js" in streamed and "dff_model_create" not in streamed
    fencing = [open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))]
    fencing = [t for t in fencing if re.search(r"\bfenced\(", t)]
    missing = [name for name in streamed if not any(f'Spec("{name}"' in t for t in fencing)]
    assert not missing, f"entry points without a fence test: {missing}"
