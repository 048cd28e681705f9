"""Host side of dff_path_states: the symbols, the refusals of bad arguments (on the host, before any device call: they run on a
machine without one), the oracle on hand-written series, path_time_summary / tp_probability / empirical_committor on hand-made
counts (the min_count rule and the weighted path included), path_histograms and TransitionPathEvaluator over numpy stand-ins
for the device calls, the package's re-exports and the --paths arguments of tools_eval_samples.py.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from dff_amd import binding, evaluate
from oracle.kinetics import core_states, label_runs, native_q
from paths_cases import HI, KEYS_FRAME, LO, M, cv_series, path_states_by_walking, path_states_oracle, ragged, reverse_within
from support import refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN, INF = float("nan"), float("inf")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dff.h")).read(), flags=re.S)
    lib = binding.load_library()
    for name in ("dff_path_states_workspace_bytes", "dff_path_states"):
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, header)
        assert m, name
        assert len(binding.SYMBOLS[name][1]) == len(m.group(1).split(",")), name      # one ctypes type per argument of the header
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_path_states"][1]) == 20 and binding.SYMBOLS["dff_path_states"][0] is C.c_int
    assert binding.SYMBOLS["dff_path_states_workspace_bytes"] == (C.c_longlong, [C.c_longlong])


def test_workspace_bytes():
    lib = binding.load_library()
    assert lib.dff_path_states_workspace_bytes(-1) == -1
    with pytest.raises(ValueError, match="negative frame count"):
        binding.path_states_workspace_bytes(-1)
    # one 32-byte carry per 2048 frames
    assert binding.path_states_workspace_bytes(0) == 0
    assert binding.path_states_workspace_bytes(1) == binding.path_states_workspace_bytes(2048) == 32
    assert binding.path_states_workspace_bytes(2049) == 64 and binding.path_states_workspace_bytes(819200) == 400 * 32


def test_path_states_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n = 5000
    need = binding.path_states_workspace_bytes(n)
    cv, i8, i64, cnt, ws = np.zeros(n, np.float32), np.zeros(n, np.int8), np.zeros(n, np.int64), np.zeros(1, np.int64), np.zeros(need + 8, np.uint8)
    one = np.array([n], np.int64)

    def call(n_=n, lengths=one, lo=0.2, hi=0.9, cv_=p(cv), max_paths=n, exit_=p(i64), dir_=p(i8), cnt_=p(cnt), ws_=p(ws), ws_bytes=need):
        return lib.dff_path_states(0, cv_, n_, p(lengths) if lengths is not None else None, len(lengths) if lengths is not None else 1,
                                   lo, hi, p(i8), p(i8), p(i64), p(i64), p(i8), max_paths, exit_, p(i64), dir_, cnt_, ws_, ws_bytes, None)

    cases = [("negative frame count", dict(n_=-1)), ("lo must be < hi", dict(lo=0.9, hi=0.2)), ("lo must be < hi", dict(lo=0.5, hi=0.5)),
             ("negative max_paths", dict(max_paths=-1)),
             ("sum to 4999, not n = 5000", dict(lengths=np.array([4000, 999], np.int64))),
             ("trajectory 1 has negative length", dict(lengths=np.array([5001, -1], np.int64))),
             ("null / negative trajectory lengths", dict(lengths=None)),
             ("null cv", dict(cv_=None)), ("null path output", dict(exit_=None)), ("null path output", dict(dir_=None)),
             ("workspace of %d bytes, %d needed" % (need - 1, need), dict(ws_bytes=need - 1)),
             ("workspace of 0 bytes", dict(ws_=None, ws_bytes=0)),
             ("8-byte aligned", dict(ws_=C.c_void_p(ws.ctypes.data + 4)))]
    for bad in (NAN, INF, -INF):
        cases += [("lo and hi must be finite", dict(lo=bad)), ("lo and hi must be finite", dict(hi=bad))]
    for what, kw in cases:
        refused(lib, call(**kw), what)
    none = [None] * 5
    assert lib.dff_path_states(0, None, 0, None, 0, 0.2, 0.9, *none, 0, None, None, None, None, None, 0, None) == 0          # n == 0
    empty = np.array([0, 0], np.int64)
    assert lib.dff_path_states(0, None, 0, p(empty), 2, 0.2, 0.9, *none, 5, None, None, None, None, None, 0, None) == 0
    # nothing asked for: no device call either (this machine has no device)
    assert lib.dff_path_states(0, p(cv), n, p(one), 1, 0.2, 0.9, *none, 0, None, None, None, None, p(ws), need, None) == 0
    with pytest.raises(ValueError, match="cv"):
        binding.path_states(torch.zeros(5), [5], 0.2, 0.9)                          # not a CUDA tensor


# ---------------------------------------------------------------- the oracle on hand-written series
def test_oracle_on_a_hand_written_series():
    #                 0    1  2  3    4    5  6    7    8  9    10
    cv = np.array([M, 0.0, M, M, 1.0, 1.0, M, 1.0, NAN, M, 0.0, M], np.float32)
    o = path_states_oracle(cv, LO, HI)
    assert o["prev"].tolist() == [-1, 0, 0, 0, 1, 1, 1, 1, -1, -1, 0, 0]
    assert o["next"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, -1, 0, 0, -1]
    assert o["t_prev"].tolist() == [-1, 1, 1, 1, 4, 5, 5, 7, -1, -1, 10, 10]
    assert o["t_next"].tolist() == [1, 1, 4, 4, 4, 5, 7, 7, -1, 10, 10, -1]
    assert o["cls"].tolist() == [-1, 0, 2, 2, 1, 1, 5, 1, -1, -1, 0, -1]
    assert (o["exit"].tolist(), o["entry"].tolist(), o["direction"].tolist()) == ([1], [4], [1])
    # a boundary after frame 3 cuts the path; a direct jump inside the second trajectory is a path of duration 1
    o = path_states_oracle(np.array([0.0, M, M, M, 1.0, 0.0], np.float32), LO, HI, [4, 2])
    assert o["cls"].tolist() == [0, -1, -1, -1, 1, 0] and o["next"].tolist() == [0, -1, -1, -1, 1, 0]
    assert (o["exit"].tolist(), o["entry"].tolist(), o["direction"].tolist()) == ([4], [5], [0])
    assert len(path_states_oracle([], LO, HI, [0, 0])["cls"]) == 0


def test_oracle_equals_the_definitions_walked_out():
    for n, seed, lengths in ((700, 1, None), (900, 2, [0, 1, 300, 2, 597]), (500, 3, [250, 250])):
        for step in (0.08, 0.5):
            cv = cv_series(n, seed, step)
            a, b = path_states_oracle(cv, LO, HI, lengths), path_states_by_walking(cv, LO, HI, lengths)
            assert set(a) == set(b) and len(a["entry"]) > 3
            for key in a:
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (n, step, key)


def test_oracle_invariants():
    """prev is core_states' label; the paths number dwell_summary's events; class 2 (3) frames number sum(duration - 1); time
    reversal swaps prev and next: the invariants the GPU test asserts, here between the oracles"""
    n = 6000
    cv = cv_series(n, 9, 0.3)
    for lengths in ([n], ragged(n, 12, 3)):
        o = path_states_oracle(cv, LO, HI, lengths)
        lab, _ = core_states(cv, LO, HI, lengths)
        assert np.array_equal(o["prev"], lab.astype(np.int8))
        events = evaluate.dwell_summary(label_runs(lab, lengths))["events"]
        assert ((o["direction"] == 1).sum(), (o["direction"] == 0).sum()) == (events[(0, 1)], events[(1, 0)])
        d = o["entry"] - o["exit"]
        assert (o["cls"] == 2).sum() == (d[o["direction"] == 1] - 1).sum() > 0 and (o["cls"] == 3).sum() == (d[o["direction"] == 0] - 1).sum() > 0
        r = path_states_oracle(reverse_within(cv, lengths), LO, HI, lengths)
        assert np.array_equal(r["prev"], reverse_within(o["next"], lengths)) and np.array_equal(r["next"], reverse_within(o["prev"], lengths))


# ---------------------------------------------------------------- path_time_summary, tp_probability, empirical_committor
def test_path_time_summary():
    paths = {"direction": np.array([1, 0, 1, 1, 1], np.int8), "duration": np.array([1, 7, 3, 5, 11], np.int64)}
    s = evaluate.path_time_summary(paths, frame_time=0.5)
    assert s[1] == {"n": 4, "mean": 2.5, "median": 2.0, "p10": float(np.percentile([0.5, 1.5, 2.5, 5.5], 10)),
                    "p90": float(np.percentile([0.5, 1.5, 2.5, 5.5], 90))}
    assert s[0] == {"n": 1, "mean": 3.5, "median": 3.5, "p10": 3.5, "p90": 3.5}
    s = evaluate.path_time_summary({"direction": np.zeros(0, np.int8), "duration": np.zeros(0, np.int64)})
    for d in (0, 1):
        assert s[d]["n"] == 0 and all(math.isnan(s[d][k]) for k in ("mean", "median", "p10", "p90"))
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="frame_time"):
            evaluate.path_time_summary(paths, bad)
    with pytest.raises(ValueError, match="one entry per path"):
        evaluate.path_time_summary({"direction": [1], "duration": [1, 2]})


def hand_hist():
    """two units, three bins; classes (U, 3, 6), next (U, 3, 2)"""
    classes = np.array([[[4, 0, 0, 0, 0, 0], [0, 0, 2, 1, 1, 0], [0, 0, 0, 0, 0, 0]],
                        [[6, 0, 1, 0, 1, 0], [0, 0, 2, 3, 0, 1], [0, 1, 0, 0, 0, 0]]], np.int64)
    nxt = np.array([[[4, 0], [2, 2], [0, 0]],
                    [[7, 1], [3, 3], [0, 1]]], np.int64)
    return {"classes": classes, "next": nxt}


def test_tp_probability_and_the_min_count_rule():
    r = evaluate.tp_probability(hand_hist())
    assert r["count"].tolist() == [12, 10, 1]
    assert r["p_tp"].tolist() == [1 / 12, 8 / 10, 0.0] and r["p_tp_ab"].tolist() == [1 / 12, 4 / 10, 0.0] and r["p_tp_ba"].tolist() == [0.0, 4 / 10, 0.0]
    r = evaluate.tp_probability(hand_hist(), min_count=2)           # a condition on the counts: the bin with one frame is NaN
    assert r["p_tp"][:2].tolist() == [1 / 12, 8 / 10] and math.isnan(r["p_tp"][2]) and math.isnan(r["p_tp_ab"][2])
    r = evaluate.tp_probability(hand_hist(), min_count=11)
    assert r["p_tp"][0] == 1 / 12 and np.isnan(r["p_tp"][1:]).all()
    h = hand_hist()
    h["classes"][:, 2] = 0                                          # an empty bin is NaN at the default
    assert math.isnan(evaluate.tp_probability(h)["p_tp"][2])
    with pytest.raises(ValueError, match="min_count"):
        evaluate.tp_probability(hand_hist(), min_count=0)


def test_empirical_committor():
    r = evaluate.empirical_committor(hand_hist())
    assert r["count"].tolist() == [12, 10, 1] and r["p_b"].tolist() == [1 / 12, 5 / 10, 1.0]
    r = evaluate.empirical_committor(hand_hist(), min_count=2)
    assert math.isnan(r["p_b"][2]) and r["p_b"][1] == 0.5
    assert "p_b_lo" not in r


def test_the_weighted_path():
    h = hand_hist()
    w = np.array([[1, 1], [2, 0], [0, 2], [0, 0]], np.uint32)        # the data; unit 0 twice; unit 1 twice; nothing
    r = evaluate.tp_probability(h, weights=w, confidence=0.5)
    assert r["p_tp"].tolist() == [1 / 12, 8 / 10, 0.0]              # the point estimate does not depend on the weights
    want = np.array([[1 / 12, 8 / 10, 0.0], [0.0, 6 / 8, NAN], [2 / 16, 10 / 12, 0.0], [NAN, NAN, NAN]])
    assert np.array_equal(r["p_tp_resamples"], want, equal_nan=True)
    lo, hi = evaluate.percentile_interval(want, 0.5)
    assert np.array_equal(r["p_tp_lo"], lo) and np.array_equal(r["p_tp_hi"], hi) and lo[0] == np.percentile([1 / 12, 0.0, 2 / 16], 25)
    c = evaluate.empirical_committor(h, min_count=2, weights=w, confidence=0.5)
    want = np.array([[1 / 12, 0.5, NAN], [0.0, 0.5, NAN], [2 / 16, 0.5, 1.0], [NAN, NAN, NAN]])     # min_count holds per resample
    assert np.array_equal(c["p_b_resamples"], want, equal_nan=True) and c["p_b_lo"][1] == c["p_b_hi"][1] == 0.5
    # the weights of bootstrap_weights, every unit once on average
    w = evaluate.bootstrap_weights(2, 50, 0)
    r = evaluate.tp_probability(h, weights=w)
    assert r["p_tp_resamples"].shape == (50, 3) and (r["p_tp_lo"][:2] <= r["p_tp"][:2]).all() and (r["p_tp"][:2] <= r["p_tp_hi"][:2]).all()
    with pytest.raises(ValueError, match="weights"):
        evaluate.tp_probability(h, weights=np.ones((4, 3), np.uint32))


def test_half_crossing():
    x = np.array([0.1, 0.3, 0.5, 0.7, 0.9])
    assert evaluate._half_crossing(x, [0.0, 0.0, 0.25, 0.75, 1.0]) == pytest.approx(0.6)
    assert evaluate._half_crossing(x, [0.0, NAN, NAN, 1.0, 1.0]) == pytest.approx(0.4)          # across bins without an estimate
    assert evaluate._half_crossing(x, [0.0, 0.5, 1.0, 1.0, 1.0]) == 0.3
    assert math.isnan(evaluate._half_crossing(x, [0.0, 0.1, 0.2, 0.3, 0.4])) and math.isnan(evaluate._half_crossing(x, [NAN] * 5))


# ---------------------------------------------------------------- path_histograms and the evaluator over numpy stand-ins
def host_path_states(cv, lengths, lo, hi, frames=True, times=True, paths=True, max_paths=None, workspace=None):
    """binding.path_states from the oracle, on CPU tensors"""
    o = path_states_oracle(cv.numpy(), lo, hi, lengths)
    out = {k: torch.from_numpy(o[k]) for k in KEYS_FRAME}
    out.update({k: torch.from_numpy(o[k]) for k in ("exit", "entry", "direction")})
    out["n_paths"] = torch.tensor([len(o["entry"])])
    return out


def host_unit_hist(bins, unit_lengths, nbins, ld=None, workspace=None):
    """binding.unit_hist by numpy: (U, C, max(nbins)) counts"""
    b = bins.numpy()
    ld = max(nbins)
    out = np.zeros((len(unit_lengths), b.shape[1], ld), np.int32)
    o = 0
    for u, ln in enumerate(unit_lengths):
        for c in range(b.shape[1]):
            v = b[o:o + ln, c]
            out[u, c, :nbins[c]] = np.bincount(v[(v >= 0) & (v < nbins[c])], minlength=nbins[c])
        o += ln
    return torch.from_numpy(out)


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(binding, "path_states", host_path_states)
    monkeypatch.setattr(binding, "unit_hist", host_unit_hist)
    monkeypatch.setattr(binding, "struct_native_q", lambda x, pairs, r0, beta, lam: torch.from_numpy(
        native_q(x.numpy(), pairs, r0, beta, lam).astype(np.float32)))


def test_path_histograms_on_the_stand_in(on_host):
    n = 3000
    cv = cv_series(n, 4, 0.3)
    lengths = [1000, 500, 1500]
    st = evaluate.path_states(cv, LO, HI, lengths, device="cpu")
    o = path_states_oracle(cv, LO, HI, lengths)
    assert np.array_equal(st.cls.numpy(), o["cls"]) and np.array_equal(st.numpy()["t_next"], o["t_next"])
    edges = np.linspace(0.0, 1.0, 11)
    h = evaluate.path_histograms(cv, edges, st, lengths)
    assert h["classes"].shape == (3, 10, 6) and h["next"].shape == (3, 10, 2) and h["classes"].dtype == np.int64
    b = np.clip(np.searchsorted(edges, cv.astype(np.float64), side="right") - 1, None, 9)
    b[~np.isfinite(cv)] = -1
    unit = np.repeat(np.arange(3), lengths)
    want_c, want_n = np.zeros((3, 10, 6), np.int64), np.zeros((3, 10, 2), np.int64)
    for t in range(n):
        if b[t] >= 0 and o["cls"][t] >= 0:
            want_c[unit[t], b[t], o["cls"][t]] += 1
        if b[t] >= 0 and o["next"][t] >= 0:
            want_n[unit[t], b[t], o["next"][t]] += 1
    assert np.array_equal(h["classes"], want_c) and np.array_equal(h["next"], want_n)
    assert h["classes"].sum() == (o["cls"][np.isfinite(cv)] >= 0).sum()
    one = evaluate.path_histograms(cv, edges, st)                   # one unit of all frames
    assert np.array_equal(one["classes"][0], want_c.sum(axis=0)) and one["unit_lengths"].tolist() == [n]
    # another coordinate of the same frames: integer microstate labels
    labels = (np.arange(n) % 7).astype(np.int32)
    labels[5] = -1
    hs = evaluate.path_histograms(labels, None, st, lengths, n_states=7)
    assert hs["classes"].shape == (3, 7, 6) and hs["classes"][:, 3].sum() == (o["cls"][labels == 3] >= 0).sum()
    assert hs["next"].sum() == (o["next"][labels >= 0] >= 0).sum()
    for kw in (dict(coordinate=cv[:-1], edges=edges), dict(coordinate=cv, edges=None), dict(coordinate=labels, edges=None)):
        with pytest.raises(ValueError, match="path_histograms"):
            evaluate.path_histograms(states=st, **kw)
    p = evaluate.transition_paths(cv, LO, HI, lengths, device="cpu")
    assert np.array_equal(p["entry"], o["entry"]) and np.array_equal(p["duration"], o["entry"] - o["exit"])


def test_summarize():
    summary = {1: {"n": 3, "mean": 2.0, "median": 1.5, "p10": 1.0, "p90": 3.0}, 0: {"n": 0, "mean": NAN, "median": NAN, "p10": NAN, "p90": NAN}}
    centres = np.array([0.1, 0.3, 0.5, 0.7, 0.9])
    cls_counts = [10, 30, 40, 6, 4, 7, 3]                           # class -1, 0 .. 5
    args = (summary, cls_counts, [0.0, NAN, 0.4, 0.2, 0.0], [0.0, NAN, 0.25, 0.75, 1.0], centres)
    q = evaluate.TransitionPathEvaluator.summarize(*args, 1, samples_nonfinite=2)                # Q: folded is core 1
    assert tuple(q) == evaluate.TransitionPathEvaluator.KEYS
    assert q["n_paths_folding"] == 3.0 and q["n_paths_unfolding"] == 0.0 and q["mean_path_time_folding"] == 2.0
    assert math.isnan(q["median_path_time_unfolding"]) and q["median_path_time_folding"] == 1.5
    assert q["path_frames_share"] == 0.1 and q["loop_frames_share"] == 0.1 and q["undetermined_share"] == 0.1
    assert q["ptp_max"] == 0.4 and q["ptp_max_at"] == 0.5 and q["committor_half"] == pytest.approx(0.6) and q["samples_nonfinite"] == 2.0
    r = evaluate.TransitionPathEvaluator.summarize(*args, 0)                                     # RMSD: folded is core 0
    assert r["n_paths_folding"] == 0.0 and r["n_paths_unfolding"] == 3.0 and r["mean_path_time_unfolding"] == 2.0
    e = evaluate.TransitionPathEvaluator.summarize(summary, [0] * 7, [NAN] * 5, [NAN] * 5, centres, 1)
    assert all(math.isnan(e[k]) for k in ("path_frames_share", "ptp_max", "ptp_max_at", "committor_half"))


def folding_frames(golden, script, repeat=20):
    from oracle.kinetics import scripted_frames
    f = golden("struct_folded.npz")["chignolin"].astype(np.float64)
    x, _ = scripted_frames(f, sum(script, []), repeat, 0.05, len(f))
    return f, x, [len(s) * repeat for s in script]


def test_evaluator_on_the_stand_in(on_host, golden):
    script = [[0.3, 0.0, 0.3, 1.0, 0.3, 0.0], [1.0, 0.3, 0.0, 0.3], [0.0, 0.3, 1.0, 1.0, 0.3]]
    f, x, lengths = folding_frames(golden, script)
    e = evaluate.TransitionPathEvaluator("chignolin", f, lo=LO, hi=HI, frame_time=0.5, nbins=10, n_resamples=20, device="cpu")
    res = e.eval(x, lengths)
    s = e.series["samples"]
    assert res["n_paths_folding"] == 2.0 and res["n_paths_unfolding"] == 2.0 and s["paths"]["duration"].tolist() == [21] * 4
    assert res["mean_path_time_folding"] == 10.5 and res["median_path_time_unfolding"] == 10.5
    assert res["path_frames_share"] == 80 / 300 and res["loop_frames_share"] == 0.0 and res["undetermined_share"] == 60 / 300
    assert res["ptp_max"] == 1.0 and res["ptp_max_at"] == pytest.approx(0.85) and 0.0 <= res["ptp_max_lo"] <= res["ptp_max_hi"] == 1.0
    # a resample without the stretches that go back to core 0 crosses 1 / 2 before the bin between the cores, one without those
    # that go on to core 1 after it: always between the centres of the outermost estimated bins
    assert e.centres[0] < res["committor_half_lo"] <= res["committor_half"] <= res["committor_half_hi"] < e.centres[-1]
    assert s["hist"]["classes"].shape == (3, 10, 6) and s["hist"]["unit_lengths"].tolist() == lengths
    assert s["p_b"]["p_b_resamples"].shape == (20, 10) and set(s) == {"cv", "states", "paths", "summary", "hist", "p_tp", "p_b"}
    assert set(res) == set(e.KEYS) | {"ptp_max_lo", "ptp_max_hi", "committor_half_lo", "committor_half_hi"}
    # against a reference that folds slower: twice the frames between the cores
    slow = [[1.0, 0.3, 0.3, 0.0, 0.3, 0.3, 1.0]]
    _, xr, lr = folding_frames(golden, slow)
    e = evaluate.TransitionPathEvaluator("chignolin", f, lo=LO, hi=HI, nbins=10, ref_data=xr, ref_traj_lengths=lr, device="cpu")
    res = e.eval(x, lengths)
    assert res["mean_path_time_folding_ref"] == 41.0 and res["n_paths_unfolding_ref"] == 1.0
    assert res["log10_path_time_ratio_folding"] == pytest.approx(math.log10(21 / 41)) and res["ptp_max_diff"] == 0.0
    assert res["committor_rmsd"] == pytest.approx(math.sqrt((0.6 - 0.5) ** 2 / 3))           # three bins estimated in both
    assert set(res) == set(e.KEYS) | {k + "_ref" for k in e.KEYS} | {"log10_path_time_ratio_folding", "log10_path_time_ratio_unfolding",
                                                                     "ptp_max_diff", "committor_rmsd"}
    # the RMSD: folded is core 0, so a path that enters core 0 folds
    e = evaluate.TransitionPathEvaluator("chignolin", f, cv="rmsd", lo=1.0, hi=4.0, device="cpu")
    assert (e.folded_label, e.unfolded_label) == (0, 1) and e.edges[0] == 0.0 and e.edges[-1] == 6.0 and len(e.edges) == 51


def test_evaluator_checks_its_arguments(monkeypatch, golden):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    f = golden("struct_folded.npz")["chignolin"]
    for kw, what in ((dict(cv="tic", lo=0.2, hi=0.9), "cv"), (dict(lo=0.9, hi=0.2), "lo"), (dict(lo=NAN, hi=0.9), "lo"),
                     (dict(lo=0.2, hi=0.9, frame_time=0.0), "frame_time"), (dict(lo=0.2, hi=0.9, nbins=0), "nbins"),
                     (dict(lo=0.2, hi=0.9, nbins=2.5), "nbins"), (dict(lo=0.2, hi=0.9, cv_range=(1.0, 0.0)), "cv_range"),
                     (dict(lo=0.2, hi=0.9, min_count=0), "min_count"), (dict(lo=0.2, hi=0.9, n_resamples=-1), "n_resamples")):
        with pytest.raises(ValueError, match=what):
            evaluate.TransitionPathEvaluator("chignolin", f, **kw, device="cpu")
    with pytest.raises(ValueError, match="lo"):
        evaluate.path_states(np.zeros(3), 0.9, 0.2)
    with pytest.raises(ValueError, match="lo"):
        evaluate.transition_paths(np.zeros(3), NAN, 0.2)

    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.TransitionPathEvaluator("chignolin", f, lo=0.2, hi=0.9, device="cpu")


# ---------------------------------------------------------------- the package, the tool
def test_package_reexports():
    for name in ("path_states", "PathStates", "transition_paths", "path_time_summary", "path_histograms", "tp_probability",
                 "empirical_committor", "TransitionPathEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__


def test_paths_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.paths is None and a.paths_bins is None and a.kinetics is None          # the existing defaults stand
    tool.paths_arguments(a)
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--paths", "--folded-pdb", "f.pdb", "--parallel-sim", "8"])
    assert a.paths == "" and a.paths_bins is None and a.folded_pdb == "f.pdb" and a.kinetics is None
    tool.paths_arguments(a)
    assert tool.kinetics_cores(a) == (0.2, 0.9)
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--paths", "heldout.pt", "--paths-bins", "25", "--kinetics-cv", "rmsd",
                       "--kinetics-cores", "1.5,4", "--frame-time", "0.2", "--folded-pdb", "f.pdb"])
    assert a.paths == "heldout.pt" and a.paths_bins == 25 and a.kinetics_cv == "rmsd" and a.kinetics_cores == (1.5, 4.0) and a.frame_time == 0.2
    for bad in (["--paths-bins", "0"], ["--paths-bins", "2.5"], ["--paths-bins", "65537"], ["--kinetics-cores", "4,1.5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--paths"] + bad)
    with pytest.raises(SystemExit, match="--paths needs --folded-pdb"):
        tool.paths_arguments(ap.parse_args(["s.pt", "chignolin", "refs", "--paths"]))
    with pytest.raises(SystemExit, match="--paths-bins needs --paths"):
        tool.paths_arguments(ap.parse_args(["s.pt", "chignolin", "refs", "--paths-bins", "10", "--folded-pdb", "f.pdb"]))
    with pytest.raises(SystemExit):                                                  # the RMSD has no default cores
        tool.kinetics_cores(ap.parse_args(["s.pt", "chignolin", "refs", "--paths", "--kinetics-cv", "rmsd", "--folded-pdb", "f.pdb"]))
