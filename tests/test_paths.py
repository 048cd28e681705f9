"""dff_path_states on the GPU against the plain-loop oracle of tests/paths_cases.py (the definitions of include/dff.h, frame by
frame).  Everything is integer work: every comparison is array_equal, there is no tolerance anywhere.

What is compared how:
- every output   prev, next, t_prev, t_next, cls and the path table equal the oracle's, with the dtypes of the binding, at the
                 sizes around the wave (64), a thread's frames (8), the workgroup (2048) and more than one workgroup, and with the
                 workspace handed over dirty (0xFF) at exactly dff_path_states_workspace_bytes;
- invariants     prev == dff_core_states' labels; the paths of each direction number dwell_summary's events of dff_label_runs
                 run on those labels; the frames of class 2 (3) number the sum of duration - 1 over the paths of that direction;
                 reversing time inside every trajectory swaps prev and next;
- scripted folding   the frames of oracle.kinetics.scripted_frames (see tests/test_kinetics.py): the script fixes the number,
                 the direction and the duration of the paths.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle.kinetics import native_q, scripted_frames
from fence import COMBINATIONS, fenced
from paths_cases import (CARRY_STRETCH, HI, KEYS_FRAME, KEYS_PATH, LO, M, carry_case, cv_series, path_states_oracle, ragged,
                         reverse_within, reversed_times)
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

DTYPES = {"prev": np.int8, "next": np.int8, "cls": np.int8, "t_prev": np.int64, "t_next": np.int64, "exit": np.int64,
          "entry": np.int64, "direction": np.int8}


def dirty_workspace(n):
    return torch.full((B().path_states_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")


def paths_gpu(cv, lengths, lo=LO, hi=HI):
    """binding.path_states with a dirty workspace of exactly the bytes asked for -> the outputs on the host, the table cut to
    the true count"""
    cv = np.asarray(cv, np.float32)
    res = B().path_states(to_dev(cv), lengths, lo, hi, workspace=dirty_workspace(len(cv)))
    k = int(res["n_paths"].cpu())
    assert 0 <= k <= len(cv)
    got = {key: res[key].cpu().numpy() for key in KEYS_FRAME}
    got.update({key: res[key][:k].cpu().numpy() for key in KEYS_PATH})
    return got


def assert_paths(cv, lengths, what, lo=LO, hi=HI):
    want = path_states_oracle(cv, lo, hi, lengths)
    got = paths_gpu(cv, lengths, lo, hi)
    for key in KEYS_PATH + KEYS_FRAME:
        assert got[key].dtype == DTYPES[key] == want[key].dtype, (what, key)
        bad = np.flatnonzero(got[key] != want[key]) if got[key].shape == want[key].shape else None
        assert np.array_equal(got[key], want[key]), \
            f"{what}: {key} differs" + (f" at {bad[:5]}: {got[key][bad[:5]]}, the oracle has {want[key][bad[:5]]}" if bad is not None
                                        else f": {len(got[key])} entries, the oracle has {len(want[key])}")
    return want


# ---------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 6145])
def test_sizes(dev, n):
    for seed, step in ((500 + n, 0.08), (900 + n, 0.5)):           # slow: long excursions; fast: many short paths, direct jumps
        want = assert_paths(cv_series(n, seed, step), [n], f"n={n} step={step}")
    if n >= 255:
        assert len(want["entry"]) > 10 and {0, 1} == set(want["direction"].tolist()) and (np.diff(want["entry"]) > 0).all()
        assert (want["entry"] - want["exit"] == 1).any() and set(want["cls"].tolist()) == {-1, 0, 1, 2, 3, 4, 5}
    for c in (0.0, 1.0, 0.5, np.nan):                               # one core only, no core at all
        want = assert_paths(np.full(n, c, np.float32), [n], f"n={n} constant {c}")
        assert len(want["entry"]) == 0


# ---------------------------------------------------------------- 2. the carry through a whole block without a decisive frame
def test_carry_through_empty_blocks(dev):
    """excursions of 4600 frames between the cores: the 2048-frame workgroup in their middle holds no decisive frame, and both
    the forward and the backward carry pass through it"""
    gap = [M] * 4600
    cv = np.array([1.0] + gap + [0.0] + gap + [0.0] + gap + [1.0] + gap + [1.0] + gap, np.float32)
    n = len(cv)
    want = assert_paths(cv, [n], "long excursions")
    assert want["exit"].tolist() == [0, 9202] and want["entry"].tolist() == [4601, 13803] and want["direction"].tolist() == [0, 1]
    cls = want["cls"]
    assert (cls[1:4601] == 3).all() and (cls[4602:9202] == 4).all() and (cls[9203:13803] == 2).all()
    assert (cls[13804:18404] == 5).all() and (cls[18405:] == -1).all() and (want["next"][18405:] == -1).all()
    assert (want["t_next"][1:4601] == 4601).all() and (want["t_prev"][18405:] == 18404).all()
    # the same frames cut so that every excursion loses a flank: nothing is determined between the cores
    lengths = [2301, 4601, 4601, 4601, 4601, n - 2301 - 4 * 4601]
    want = assert_paths(cv, lengths, "long excursions, cut in the middle")
    assert len(want["entry"]) == 0 and not np.isin(want["cls"], (2, 3, 4, 5)).any()


# ---------------------------------------------------------------- 3. trajectory shapes
def assert_table_continues(want, lengths, group=64):
    """paths on both sides of the first launch group's end (`group` non-empty unequal trajectories), in one ascending table"""
    nonempty = np.flatnonzero(np.asarray(lengths) > 0)
    cut = int(np.cumsum(lengths)[nonempty[group - 1]])
    assert (want["entry"] < cut).sum() > 5 and (want["entry"] >= cut).sum() > 5 and (np.diff(want["entry"]) > 0).all()


def test_trajectory_shapes(dev):
    cv = cv_series(24000, 77, 0.3)
    assert_paths(cv[:6147], [0, 1, 2047, 1, 0, 2048, 2, 2048, 0], "lengths 0 and 1, boundaries at block edges")
    assert_paths(cv[:4096], [2048, 2048], "a boundary exactly at the block edge")
    assert_paths(cv[:5], [1, 1, 1, 1, 1], "single frames")
    r70 = ragged(24000, 70, 70)
    assert len(r70) == 70 and 0 in r70 and 1 in r70
    want = assert_paths(cv, r70, "70 unequal trajectories: two launch groups")
    assert_table_continues(want, r70)
    one = path_states_oracle(cv, LO, HI)
    assert len(one["entry"]) > len(want["entry"])                   # the boundaries matter on this series
    want = assert_paths(cv, [300] * 80, "80 equal trajectories: the periodic path")
    assert len(want["entry"]) > 100
    assert_paths(cv, [300] * 40 + [0] + [300] * 40, "80 equal trajectories and an empty one")
    assert_paths(cv, [299] * 40 + [301] * 40, "80 unequal trajectories of nearly equal length")


@pytest.mark.parametrize("case", ["one", "periodic", "groups"])
def test_carry_scan_second_chunk(dev, case):
    """more than 256 blocks in one launch (paths_cases.carry_case): the carry scan runs two chunks, upwards and downwards"""
    cv, lengths = carry_case(case)
    assert sum(lengths[:64] if case == "groups" else lengths) > 256 * 2048      # the frames of the first launch
    want = assert_paths(cv, lengths, f"carry scan, {case}")
    assert len(want["entry"]) > 10000 and set(want["cls"].tolist()) == {-1, 0, 1, 2, 3, 4, 5}
    if case == "one":
        s = CARRY_STRETCH
        assert (want["prev"][s] == 0).all() and (want["next"][s] == 1).all() and (want["cls"][s] == 2).all()
        assert (want["t_prev"][s] == s.start - 1).all() and (want["t_next"][s] == s.stop).all()
        assert len(want["entry"]) == 34198
        assert (want["exit"][-1], want["entry"][-1], want["direction"][-1]) == (s.start - 1, s.stop, 1)
    if case == "groups":
        assert_table_continues(want, lengths)


# ---------------------------------------------------------------- 4. edge values
def test_edge_values(dev):
    lo32, hi32 = np.float32(LO), np.float32(HI)
    # exactly lo and exactly hi are inside the cores, the neighbouring floats are not
    cv = np.array([M, lo32, M, np.nextafter(hi32, np.float32(0)), hi32, M, np.nextafter(lo32, np.float32(1)), lo32, hi32, lo32], np.float32)
    want = assert_paths(cv, [len(cv)], "thresholds")
    assert want["cls"].tolist() == [-1, 0, 2, 2, 1, 3, 3, 0, 1, 0] and want["exit"].tolist() == [1, 4, 7, 8]
    assert want["entry"].tolist() == [4, 7, 8, 9] and want["direction"].tolist() == [1, 0, 1, 0]      # the last two: direct jumps
    # non-finite values at the first and last frame of trajectories and on both sides of a block edge
    for bad in (np.nan, np.inf, -np.inf):
        lengths = [2040, 16, 2040, 4100]
        cv = cv_series(sum(lengths), 31, 0.4)
        cv[np.isnan(cv) | np.isinf(cv)] = M
        ends = np.cumsum(lengths)
        for t in (0, ends[0] - 1, ends[0], ends[1] - 1, 2047, 2048, 4095, 4096, 6143, 6144, ends[3] - 1):
            cv[t] = bad
        want = assert_paths(cv, lengths, f"{bad} at trajectory ends and block edges")
        assert (want["cls"][[0, 2047, 2048, 4095, 4096]] == -1).all() and len(want["entry"]) > 10
        cv = np.array([1.0, M, bad, M, 0.0, M, 1.0, bad, 0.0], np.float32)
        want = assert_paths(cv, [len(cv)], f"{bad} inside a path")
        assert want["cls"].tolist() == [1, -1, -1, -1, 0, 2, 1, -1, 0] and want["entry"].tolist() == [6]
    # negative thresholds, through evaluate
    st = ev().path_states(np.array([-3.0, -1.5, 0.0, -1.5, -2.0], np.float32), -2.0, -1.0)
    assert st.cls.cpu().tolist() == [0, 2, 1, 3, 0] and st.t_next.cpu().tolist() == [0, 2, 2, 4, 4]
    p = ev().transition_paths(np.array([-3.0, -1.5, 0.0, -1.5, -2.0], np.float32), -2.0, -1.0)
    assert p["duration"].tolist() == [2, 2] and p["direction"].tolist() == [1, 0] and p["duration"].dtype == np.int64
    with pytest.raises(ValueError, match="lo must be < hi"):
        B().path_states(to_dev(np.zeros(4, np.float32)), [4], 0.9, 0.2)
    empty = B().path_states(torch.empty(0, dtype=torch.float32, device="cuda"), [], LO, HI)
    assert int(empty["n_paths"].cpu()) == 0 and empty["cls"].numel() == 0


# ---------------------------------------------------------------- 5. invariants against the kinetics calls on the GPU
@pytest.mark.parametrize("layout", ["one", "ragged", "equal"])
def test_invariants(dev, layout):
    n = 24000
    cv = cv_series(n, 123, 0.3)
    lengths = {"one": [n], "ragged": ragged(n, 70, 5), "equal": [300] * 80}[layout]
    got = paths_gpu(cv, lengths)
    labels = B().core_states(to_dev(cv), lengths, LO, HI)
    assert np.array_equal(got["prev"], labels.cpu().numpy().astype(np.int8))                       # 1
    events = ev().dwell_summary(ev().label_runs(labels, lengths))["events"]
    n_ab, n_ba = int((got["direction"] == 1).sum()), int((got["direction"] == 0).sum())
    assert (n_ab, n_ba) == (events[(0, 1)], events[(1, 0)]) and n_ab > 10 and n_ba > 10            # 2
    duration = got["entry"] - got["exit"]
    assert (duration >= 1).all()
    assert int((got["cls"] == 2).sum()) == int((duration[got["direction"] == 1] - 1).sum()) > 0    # 3
    assert int((got["cls"] == 3).sum()) == int((duration[got["direction"] == 0] - 1).sum()) > 0
    # reversing time inside every trajectory swaps prev and next, and the classes 2 and 3
    rev = paths_gpu(reverse_within(cv, lengths), lengths)
    assert np.array_equal(rev["prev"], reverse_within(got["next"], lengths))
    assert np.array_equal(rev["next"], reverse_within(got["prev"], lengths))
    assert np.array_equal(rev["t_prev"], reversed_times(got["t_next"], lengths))
    assert np.array_equal(rev["t_next"], reversed_times(got["t_prev"], lengths))
    swap = np.array([-1, 0, 1, 3, 2, 4, 5], np.int8)               # class c -> swap[c + 1]
    assert np.array_equal(rev["cls"], swap[reverse_within(got["cls"], lengths).astype(np.int64) + 1])
    assert len(rev["entry"]) == len(got["entry"]) and int((rev["direction"] == 1).sum()) == n_ba


# ---------------------------------------------------------------- 6. max_paths and NULL outputs
def raw_call(cvd, ln, outs, max_paths, ws):
    g = lambda k: ptr(outs[k]) if outs.get(k) is not None else None     # noqa: E731
    raw("dff_path_states", 0, ptr(cvd), cvd.numel(), ln.ctypes.data, len(ln), LO, HI, g("prev"), g("next"), g("t_prev"), g("t_next"),
        g("cls"), max_paths, g("exit"), g("entry"), g("direction"), g("n_paths"), ptr(ws), ws.numel(), stream_of(cvd))


def sentinel_outs(n, size, keys):
    shape = {"prev": n, "next": n, "cls": n, "t_prev": n, "t_next": n, "exit": size, "entry": size, "direction": size, "n_paths": 1}
    return {k: torch.full((shape[k],), 123, dtype=torch.int64 if k == "n_paths" else getattr(torch, np.dtype(DTYPES[k]).name), device="cuda")
            for k in keys}


def test_max_paths(dev):
    n = 6145
    cv = cv_series(n, 66, 0.4)
    lengths = [100, 2000, 1, 4044]
    want = path_states_oracle(cv, LO, HI, lengths)
    k = len(want["entry"])
    assert k > 20
    cvd, ln, ws = to_dev(cv), np.asarray(lengths, np.int64), dirty_workspace(n)
    for max_paths in (0, 1, k - 1, k, k + 5):
        outs = sentinel_outs(n, k + 16, KEYS_FRAME + KEYS_PATH + ("n_paths",))
        raw_call(cvd, ln, outs, max_paths, ws)
        assert int(outs["n_paths"].cpu()) == k, max_paths           # the true count, whatever fits
        m = min(max_paths, k)
        for key in KEYS_PATH:
            assert np.array_equal(outs[key][:m].cpu().numpy(), want[key][:m]), (max_paths, key)
            assert bool((outs[key][m:] == 123).all()), f"max_paths={max_paths}: {key} touched beyond the paths written"
        for key in KEYS_FRAME:
            assert np.array_equal(outs[key].cpu().numpy(), want[key]), (max_paths, key)
    # max_paths = 0 takes no table arrays
    outs = sentinel_outs(n, 0, ("n_paths",))
    raw_call(cvd, ln, outs, 0, ws)
    assert int(outs["n_paths"].cpu()) == k
    got = B().path_states(cvd, lengths, LO, HI, frames=False, times=False, max_paths=3)
    assert got["entry"].cpu().tolist() == want["entry"][:3].tolist() and int(got["n_paths"].cpu()) == k and set(got) == {
        "exit", "entry", "direction", "n_paths"}


def test_every_combination_of_null_outputs(dev):
    n = 6145
    cv = cv_series(n, 67, 0.4)
    lengths = [100, 2000, 1, 4044]
    want = path_states_oracle(cv, LO, HI, lengths)
    k = len(want["entry"])
    cvd, ln, ws = to_dev(cv), np.asarray(lengths, np.int64), dirty_workspace(n)
    for mask in itertools.product((False, True), repeat=6):
        keys = tuple(key for key, on in zip(KEYS_FRAME, mask) if on) + ((KEYS_PATH + ("n_paths",)) if mask[5] else ())
        outs = sentinel_outs(n, k, keys)
        raw_call(cvd, ln, outs, k, ws)
        for key in keys:
            assert np.array_equal(outs[key].cpu().numpy(), want[key] if key != "n_paths" else [k]), (keys, key)


# ---------------------------------------------------------------- 7. scripted folding
SCRIPT = [[0.3, 0.0, 0.3, 1.0, 0.3, 0.0], [1.0, 0.3, 0.0, 0.3], [0.0, 0.3, 1.0, 1.0, 0.3]]     # one list per trajectory
REPEAT = 40
# w = 0 folded (Q >= HI, core 1), w = 1 unfolded (Q <= LO, core 0), w = 0.3 between.  Trajectory 1: - F p U p F (unfolds, folds),
# 2: U p F - (folds), 3: F p U U - (unfolds); every path crosses one stretch of REPEAT frames
N_FOLDING, N_UNFOLDING = 2, 2


def test_scripted_folding(dev, golden):
    f = golden("struct_folded.npz")["chignolin"].astype(np.float64)
    x, w = scripted_frames(f, sum(SCRIPT, []), REPEAT, 0.05, len(f))
    lengths = [len(s) * REPEAT for s in SCRIPT]
    pairs, r0 = ev().native_pairs(f)
    q = native_q(x, pairs, r0)
    assert np.abs(q - LO).min() > 1e-3 and np.abs(q - HI).min() > 1e-3, "an oracle Q lies within 1e-3 of a threshold"
    assert (q[w == 0.0] > HI).all() and (q[w == 1.0] < LO).all() and ((q[w == 0.3] > LO) & (q[w == 0.3] < HI)).all()
    e = ev().TransitionPathEvaluator("chignolin", f, cv="q", lo=LO, hi=HI, frame_time=0.2, nbins=10, ref_data=x, ref_traj_lengths=lengths)
    res = e.eval(x, lengths)
    s = e.series["samples"]
    want = path_states_oracle(s["cv"], LO, HI, lengths)             # the oracle on the GPU's own series
    for key in KEYS_FRAME:
        assert np.array_equal(s["states"][key], want[key]), key
    for key in KEYS_PATH:
        assert np.array_equal(s["paths"][key], want[key]), key
    assert res["n_paths_folding"] == N_FOLDING and res["n_paths_unfolding"] == N_UNFOLDING
    assert s["paths"]["direction"].tolist() == [0, 1, 1, 0] and s["paths"]["duration"].tolist() == [REPEAT + 1] * 4
    for key in ("mean_path_time_folding", "mean_path_time_unfolding", "median_path_time_folding", "median_path_time_unfolding"):
        assert res[key] == pytest.approx((REPEAT + 1) * 0.2, rel=1e-12), key
    n = len(x)
    assert res["path_frames_share"] == 4 * REPEAT / n and res["loop_frames_share"] == 0.0
    assert res["undetermined_share"] == 3 * REPEAT / n and res["samples_nonfinite"] == 0.0
    # the committor rises from 0 in core A to 1 in core B; of the 5 stretches between the cores that reach a core, 3 reach core B
    p_b, centres = s["p_b"]["p_b"], e.centres
    ok = np.isfinite(p_b)
    assert (p_b[ok & (centres < LO)] == 0.0).all() and (p_b[ok & (centres > HI)] == 1.0).all() and (np.diff(p_b[ok]) >= 0).all()
    assert (ok & (centres < LO)).any() and (ok & (centres > HI)).any()
    mid = ok & (centres > LO) & (centres < HI)
    assert mid.sum() == 1 and p_b[mid][0] == 3 * REPEAT / (5 * REPEAT) and s["p_b"]["count"][mid][0] == 5 * REPEAT
    xs, k = centres[ok], int(np.flatnonzero(centres[ok] == centres[mid][0])[0])
    assert res["committor_half"] == pytest.approx(xs[k - 1] + (xs[k] - xs[k - 1]) * 0.5 / 0.6, rel=1e-12)
    assert res["ptp_max"] == 1.0 and res["ptp_max_at"] == centres[mid][0]       # every determined frame between the cores is on a path
    # the reference data are the samples
    for key in e.KEYS:
        assert res[key + "_ref"] == res[key], key
    assert res["log10_path_time_ratio_folding"] == 0.0 and res["ptp_max_diff"] == 0.0 and res["committor_rmsd"] == 0.0


# ---------------------------------------------------------------- 8. stream order and the fence
KIN_N = 5000                                                        # three workgroups
KIN_LENGTHS = np.array([1, 2047, 1, 2000, 951], np.int64)


def path_states_spec():
    b, n = B(), KIN_N
    cv = cv_series(n, 71, 0.3)
    k = len(path_states_oracle(cv, LO, HI, KIN_LENGTHS)["entry"])   # a table of exactly the paths: every entry is written
    ws = torch.empty(b.path_states_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    names = ("prev", "next", "t_prev", "t_next", "cls", "exit", "entry", "direction", "n_paths")

    def wrap(_, bufs):
        res = b.path_states(bufs["cv"], KIN_LENGTHS, LO, HI, max_paths=k)
        return {key: res[key].view(torch.uint8) if res[key].dtype == torch.int8 else res[key] for key in names}
    # the int8 outputs are handed over as bytes (the gate has sentinels for uint8, not int8): -1 reads 255, never the sentinel 0x7b
    return Spec("dff_path_states", {"cv": (to_dev(cv), 0.5)},
                {"prev": ((n,), torch.uint8), "next": ((n,), torch.uint8), "t_prev": ((n,), torch.int64), "t_next": ((n,), torch.int64),
                 "cls": ((n,), torch.uint8), "exit": ((k,), torch.int64), "entry": ((k,), torch.int64), "direction": ((k,), torch.uint8),
                 "n_paths": ((1,), torch.int64)},
                lambda _, bufs: raw("dff_path_states", 0, ptr(bufs["cv"]), n, KIN_LENGTHS.ctypes.data, len(KIN_LENGTHS), LO, HI,
                                    ptr(bufs["prev"]), ptr(bufs["next"]), ptr(bufs["t_prev"]), ptr(bufs["t_next"]), ptr(bufs["cls"]), k,
                                    ptr(bufs["exit"]), ptr(bufs["entry"]), ptr(bufs["direction"]), ptr(bufs["n_paths"]),
                                    ptr(bufs["ws"]), bufs["ws"].numel(), stream_of(bufs["cv"])),
                work={"ws": ws}, wrap=wrap), k


def test_stream_order_path_states(gate, side):  # noqa: F811
    spec, k = path_states_spec()
    ref = analysis_call(spec, gate, side)
    assert int(ref["n_paths"]) == k > 10                            # the poison (constant 0.5) has no path


def test_fence():
    """The memory contract (tests/fence.py): every buffer in one arena, the carries at exactly dff_path_states_workspace_bytes,
    the table arrays at exactly the number of paths."""
    spec, _ = path_states_spec()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)
