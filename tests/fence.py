"""The fence protocol: how a test shows that an ABI call touches no memory but its own buffers, that the contents of its
workspace are irrelevant, and that the alignments include/dff.h states are enough ("The memory contract of a call").
It runs a stream_gate.Spec -- the description of one call that the stream-order protocol already uses -- so the test of a
call sits next to its stream-order test, in the file that owns the Spec; tests/test_fence.py holds the harness's own controls.

Every other GPU test hands a call tensors that come straight from PyTorch's caching allocator: blocks rounded up to 512
bytes, carved out of large segments.  A kernel that writes a few elements past an output or past *_workspace_bytes, or
reads past an input, lands in padding or in a neighbour; nothing faults and nothing fails.  Here ALL buffers of a call --
inputs, outputs, in-out buffers, workspaces -- are views into ONE uint8 ARENA:

    | band | buffer | band | buffer | ... | buffer | band |          every band >= BAND = 64 KiB

A band ends at the exact last byte of the buffer before it and starts at the exact first byte of the one after it, so every
byte of the arena is a buffer or a band, and an overrun too long for one band lands in another checked region.  A workspace
is passed at exactly the length of the Spec's own (what *_workspace_bytes returned for its shape).

PLACEMENT "natural": every buffer at a multiple of 256 bytes, as callers place them today.  "tight": every buffer at the
smallest alignment the header documents for it and at no larger one -- a workspace ("8-byte aligned") at 8 mod 16, an
array at sizeof(element) mod 16; `align` (name -> bytes) names what the header states where that is not the element size
(the 32-byte dff_hmm_fit_state travels as int32 words and is documented as 8-byte aligned).
PATTERN 0x00 or 0xFF fills the bands and the workspaces: 0xFF is NaN in every float type and -1 in every integer type.  Only
these two: a large finite integer read out of bounds and used as an index would turn a silent bug into a wild access; zero
and -1 stay inside the arena.  Outputs are filled with stream_gate's sentinel.

CHECKED after the call, each with its own message (pytest does not rewrite the asserts of this module):
  1. every band still holds its pattern; else the first and last damaged byte, relative to the nearest buffer, by name;
  2. every pure input is bit-identical to what was uploaded;
  3. every result (spec.results) is bit-identical to stream_gate.reference(spec): the same call on ordinary separate
     allocations -- and therefore identical across both patterns and both placements.  An out-of-bounds read that reaches a
     result, a dependence on the workspace's contents and a dependence on alignment all fail here (under 0xFF at the latest:
     a stray zero may be harmless, a stray NaN or -1 is not);
  4. no sentinel survives in an output that is not listed in spec.unwritten.
There is no tolerance anywhere: the oracle tests stay the judge of correctness; this protocol is about whose memory it is.
It works on CPU tensors too (the stand-in calls of tests/test_fence.py)."""
import torch

from stream_gate import bits_equal, device_of, reference, sentinel

BAND = 64 * 1024
PATTERNS = (0x00, 0xFF)
PLACEMENTS = ("natural", "tight")
COMBINATIONS = tuple((p, q) for q in PLACEMENTS for p in PATTERNS)
WORKSPACE_ALIGN = 8          # "workspace_dev ... 8-byte aligned": what include/dff.h states for every workspace


class Slot:
    def __init__(self, name, kind, shape, dtype, align):
        self.name, self.kind, self.shape, self.dtype, self.align = name, kind, tuple(shape), dtype, align
        n = 1
        for s in self.shape:
            n *= s
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.start = None

    @property
    def end(self):
        return self.start + self.nbytes


def _slots(spec, align):
    align = dict(align or {})
    item = lambda dtype: torch.empty((), dtype=dtype).element_size()  # noqa: E731
    out = []
    for k, (real, _) in spec.ins.items():
        out.append(Slot(k, "inout" if k in spec.inout else "in", real.shape, real.dtype, align.pop(k, item(real.dtype))))
    for k, (shape, dtype) in spec.outs.items():
        out.append(Slot(k, "out", shape, dtype, align.pop(k, item(dtype))))
    for k, w in spec.work.items():
        out.append(Slot(k, "work", w.shape, w.dtype, align.pop(k, max(WORKSPACE_ALIGN, item(w.dtype)))))
    assert not align, f"{spec.name}: alignments given for buffers the Spec does not have: {sorted(align)}"
    return out


def _place(slots, placement):
    """Offsets relative to a 256-byte aligned base.  natural: multiples of 256.  tight: start = align mod 16 for an alignment
    below 16, align mod 2 align above: aligned as documented and not one bit better."""
    assert placement in PLACEMENTS, f"placement {placement!r}: one of {PLACEMENTS}"
    at = 0
    for s in slots:
        lo = at + BAND
        if placement == "natural":
            s.start = (lo + 255) // 256 * 256
        else:
            assert s.align & (s.align - 1) == 0 and s.align >= 1, f"{s.name}: alignment {s.align} is no power of two"
            period = max(16, 2 * s.align)
            s.start = lo + (s.align - lo) % period
            assert s.start % s.align == 0 and s.start % (2 * s.align) != 0
        at = s.end
    return at + BAND


def _where(slots, byte):
    """`byte` (inside a band) relative to the nearest buffer."""
    before = [s for s in slots if s.end <= byte]
    after = [s for s in slots if s.start > byte]
    past = byte - before[-1].end + 1 if before else None
    ahead = after[0].start - byte if after else None
    if ahead is None or (past is not None and past <= ahead):
        return f"{past} byte(s) past the end of {before[-1].name}"
    return f"{ahead} byte(s) before the start of {after[0].name}"


class Fenced:
    """What fenced() returns: the layout (slots), the arena and the buffers, for a test that wants to look further."""

    def __init__(self, slots, arena, bufs, total):
        self.slots, self.arena, self.bufs, self.total = slots, arena, bufs, total


def fenced(spec, nat=None, pattern=0xFF, placement="natural", ref=None, align=None):
    """One call of `spec` inside an arena (the module's docstring); `ref`: stream_gate.reference(spec, nat) when the caller has
    it already -- it is the same for every pattern and placement."""
    assert pattern in PATTERNS, f"pattern {pattern!r}: one of {PATTERNS}"
    dev = device_of(spec)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    what = f"{spec.name} [fence {pattern:#04x}, {placement}]"
    if ref is None:
        ref = reference(spec, nat)

    slots = _slots(spec, align)
    total = _place(slots, placement)
    raw = torch.full((total + 256,), pattern, dtype=torch.uint8, device=dev)
    skew = -raw.data_ptr() % 256
    arena = raw[skew:skew + total]
    bufs, uploaded = {}, {}
    for s in slots:
        view = arena[s.start:s.end].view(s.dtype).view(s.shape)
        if s.nbytes:                                            # (an empty tensor has no address)
            assert view.data_ptr() == arena.data_ptr() + s.start and view.data_ptr() % s.align == 0
        if s.nbytes and placement == "tight":
            assert view.data_ptr() % (2 * s.align) != 0, f"{what}: {s.name} sits at a larger alignment than {s.align}"
        if s.kind in ("in", "inout"):
            view.copy_(spec.ins[s.name][0])
            if s.kind == "in":
                uploaded[s.name] = spec.ins[s.name][0].clone()
        elif s.kind == "out":
            view.fill_(sentinel(s.dtype))
        bufs[s.name] = view                                     # a workspace keeps the pattern
    sync()

    spec.fn(nat, bufs)
    sync()

    at, damaged, first, last = 0, 0, None, None
    for s in slots + [None]:                                    # 1. the bands, all of them: an overrun may span several
        hi = s.start if s is not None else total
        bad = (arena[at:hi] != pattern).nonzero()
        if bad.numel():
            damaged += bad.numel()
            first, last = (at + int(bad[0]) if first is None else first), at + int(bad[-1])
        at = s.end if s is not None else total
    if damaged:
        raise AssertionError(f"{what}: guard band damaged: {damaged} byte(s), the first {_where(slots, first)}, "
                             f"the last {_where(slots, last)}")
    for k, v in uploaded.items():                               # 2. the pure inputs
        assert bits_equal(bufs[k], v), f"{what}: the pure input {k} was written to"
    for k in spec.results:                                      # 3. the results
        assert bits_equal(bufs[k], ref[k]), f"{what}: {k} differs from the same call on separate allocations"
    for k, (_, dtype) in spec.outs.items():                     # 4. the sentinel
        if k not in spec.unwritten:
            assert not bool((bufs[k] == sentinel(dtype)).any()), f"{what}: a sentinel survives in {k}"
    print(f"[fence] {spec.name} {pattern:#04x} {placement}: {len(slots)} buffers, arena of {total} bytes")
    return Fenced(slots, arena, bufs, total)
