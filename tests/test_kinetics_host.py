"""Host side of the folding-kinetics calls (dff_struct_native_q / dff_core_states / dff_label_runs): the symbols, the refusals
of bad arguments (on the host, before any device call: they run on a machine without one), the numpy oracle on hand-written
series, dwell_summary on hand-built runs, native_pairs on the golden folded structures, the evaluator's argument checks, the
package's re-exports and the --kinetics arguments of tools_eval_samples.py.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from dff_amd import binding, evaluate
from oracle.kinetics import core_states, core_states_scan, label_runs, native_q
from support import refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_struct_native_q", "dff_kinetics_workspace_bytes", "dff_core_states", "dff_label_runs")
NAN, INF = float("nan"), float("inf")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_struct_native_q"][1]) == 11
    assert len(binding.SYMBOLS["dff_core_states"][1]) == 12
    assert len(binding.SYMBOLS["dff_label_runs"][1]) == 14
    assert binding.SYMBOLS["dff_kinetics_workspace_bytes"][0] is C.c_longlong


def test_workspace_bytes():
    lib = binding.load_library()
    assert lib.dff_kinetics_workspace_bytes(-1) == -1
    with pytest.raises(ValueError, match="negative frame count"):
        binding.kinetics_workspace_bytes(-1)
    # one 16-byte carry per 2048 frames
    assert binding.kinetics_workspace_bytes(0) == 0
    assert binding.kinetics_workspace_bytes(1) == binding.kinetics_workspace_bytes(2048) == 16
    assert binding.kinetics_workspace_bytes(2049) == 32
    assert binding.kinetics_workspace_bytes(819200) == 400 * 16


def test_native_q_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n, N, P = 100, 10, 5
    x, pairs, r0, q = np.zeros((n, N, 3), np.float32), np.zeros((P, 2), np.int32), np.ones(P, np.float32), np.zeros(n, np.float32)

    def call(n_=n, N_=N, P_=P, beta=5.0, lam=1.2, x_=p(x), pairs_=p(pairs), r0_=p(r0), q_=p(q)):
        return lib.dff_struct_native_q(0, x_, n_, N_, pairs_, r0_, P_, beta, lam, q_, None)

    cases = [("n_beads must be 4..64", dict(N_=3)), ("n_beads must be 4..64", dict(N_=65)),
             ("negative count", dict(n_=-1)), ("n_pairs must be 1..45", dict(P_=0)), ("n_pairs must be 1..45", dict(P_=46)),
             ("null input", dict(x_=None)), ("null output", dict(q_=None)),
             ("null pair list", dict(pairs_=None)), ("null pair list", dict(r0_=None))]
    for bad in (NAN, INF, 0.0, -1.0):
        cases += [("beta must be finite and > 0", dict(beta=bad)), ("lambda must be finite and > 0", dict(lam=bad))]
    for what, kw in cases:
        refused(lib, call(**kw), what)
    assert call(n_=0, x_=None, pairs_=None, r0_=None, q_=None) == 0                 # n == 0: a valid no-op
    with pytest.raises(ValueError):
        binding.struct_native_q(torch.zeros((5, 4, 3)), pairs, r0)                  # not a CUDA tensor


def test_core_states_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n = 5000
    need = binding.kinetics_workspace_bytes(n)
    cv, lab, ws = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(need + 8, np.uint8)
    one = np.array([n], np.int64)

    def call(n_=n, lengths=one, lo=0.2, hi=0.9, cv_=p(cv), lab_=p(lab), ws_=p(ws), ws_bytes=need):
        return lib.dff_core_states(0, cv_, n_, p(lengths) if lengths is not None else None,
                                   len(lengths) if lengths is not None else 1, lo, hi, lab_, None, ws_, ws_bytes, None)

    cases = [("negative frame count", dict(n_=-1)), ("lo must be < hi", dict(lo=0.9, hi=0.2)), ("lo must be < hi", dict(lo=0.5, hi=0.5)),
             ("sum to 4999, not n = 5000", dict(lengths=np.array([4000, 999], np.int64))),
             ("trajectory 1 has negative length", dict(lengths=np.array([5001, -1], np.int64))),
             ("null / negative trajectory lengths", dict(lengths=None)),
             ("null cv / labels", dict(cv_=None)), ("null cv / labels", dict(lab_=None)),
             ("workspace of %d bytes, %d needed" % (need - 1, need), dict(ws_bytes=need - 1)),
             ("workspace of 0 bytes", dict(ws_=None, ws_bytes=0)),
             ("8-byte aligned", dict(ws_=C.c_void_p(ws.ctypes.data + 4)))]
    for bad in (NAN, INF, -INF):
        cases += [("lo and hi must be finite", dict(lo=bad)), ("lo and hi must be finite", dict(hi=bad))]
    for what, kw in cases:
        refused(lib, call(**kw), what)
    assert lib.dff_core_states(0, None, 0, None, 0, 0.2, 0.9, None, None, None, 0, None) == 0       # n == 0
    empty = np.array([0, 0], np.int64)
    assert lib.dff_core_states(0, None, 0, p(empty), 2, 0.2, 0.9, None, None, None, 0, None) == 0
    with pytest.raises(ValueError, match="cv"):
        binding.core_states(torch.zeros(5), [5], 0.2, 0.9)                         # not a CUDA tensor


def test_label_runs_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n = 5000
    need = binding.kinetics_workspace_bytes(n)
    lab, ws = np.zeros(n, np.int32), np.zeros(need + 8, np.uint8)
    i64, i32, u8, cnt = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(1, np.int64)
    one = np.array([n], np.int64)

    def call(n_=n, lengths=one, max_runs=n, lab_=p(lab), start=p(i64), cnt_=p(cnt), ws_=p(ws), ws_bytes=need):
        return lib.dff_label_runs(0, lab_, n_, p(lengths), len(lengths), max_runs, start, p(i64), p(i32), p(u8), cnt_, ws_,
                                  ws_bytes, None)

    for what, kw in (("negative frame count", dict(n_=-1)), ("negative max_runs", dict(max_runs=-1)),
                     ("sum to 4999, not n = 5000", dict(lengths=np.array([4000, 999], np.int64))),
                     ("trajectory 0 has negative length", dict(lengths=np.array([-1, 5001], np.int64))),
                     ("null labels / n_runs", dict(lab_=None)), ("null labels / n_runs", dict(cnt_=None)),
                     ("null run output", dict(start=None)),
                     ("workspace of %d bytes, %d needed" % (need - 1, need), dict(ws_bytes=need - 1)),
                     ("workspace of 0 bytes", dict(ws_=None, ws_bytes=0)),
                     ("8-byte aligned", dict(ws_=C.c_void_p(ws.ctypes.data + 1)))):
        refused(lib, call(**kw), what)
    assert lib.dff_label_runs(0, None, 0, None, 0, 0, None, None, None, None, None, None, 0, None) == 0   # n == 0
    with pytest.raises(ValueError, match="labels"):
        binding.label_runs(torch.zeros(5, dtype=torch.int32), [5])                 # not a CUDA tensor


# ---------------------------------------------------------------- the oracle on hand-written series
LO, HI = np.float32(0.2), np.float32(0.9)
M = 0.5                                       # between the cores


def test_oracle_equality_at_both_thresholds():
    below, above = np.nextafter(LO, np.float32(1)), np.nextafter(HI, np.float32(0))
    lab, core = core_states([M, LO, M, above, HI, M, below, LO], LO, HI)
    assert lab.tolist() == [-1, 0, 0, 0, 1, 1, 1, 0] and core.tolist() == [-1, 0, -1, -1, 1, -1, -1, 0]


def test_oracle_resets_on_non_finite_values():
    for bad in (NAN, INF, -INF):
        lab, core = core_states([1.0, M, bad, M, 0.0, bad, 1.0], LO, HI)
        assert lab.tolist() == [1, 1, -1, -1, 0, -1, 1], bad
        assert core.tolist() == [1, -1, -1, -1, 0, -1, 1], bad


def test_oracle_trajectory_boundaries():
    # the previous trajectory ended in a core: the next one starts from nothing
    lab, _ = core_states([M, 1.0, 1.0, M, M, 0.0], LO, HI, [3, 3])
    assert lab.tolist() == [-1, 1, 1, -1, -1, 0]
    # a trajectory that never visits a core; trajectories of one frame; an empty one
    lab, _ = core_states([1.0, M, M, M, 0.0, M, 1.0], LO, HI, [1, 3, 1, 0, 1, 1])
    assert lab.tolist() == [1, -1, -1, -1, 0, -1, 1]
    assert core_states([], LO, HI, [])[0].shape == (0,) and core_states([], LO, HI, [0, 0])[0].shape == (0,)


def test_oracle_loop_equals_the_max_accumulate_formulation():
    rng = np.random.default_rng(11)
    cv = (0.55 + np.cumsum(rng.standard_normal(5000)) * 0.05).astype(np.float32)
    cv = np.abs((cv % 2.0) - 1.0).astype(np.float32)                   # folded back into 0 .. 1
    cv[rng.integers(0, 5000, 40)] = np.nan
    cv[rng.integers(0, 5000, 10)] = np.inf
    lengths = [1, 7, 2000, 2992]
    lab, _ = core_states(cv, LO, HI, lengths)
    assert {-1, 0, 1} == set(lab.tolist())
    assert np.array_equal(lab, core_states_scan(cv, LO, HI, lengths))
    assert np.array_equal(core_states(cv, LO, HI)[0], core_states_scan(cv, LO, HI))
    assert not np.array_equal(lab, core_states(cv, LO, HI)[0])         # the boundaries matter on this series


def test_oracle_runs():
    r = label_runs([0, 0, 1, -1, -1, 1, 1, 1, 7], [4, 1, 0, 4])
    assert r["start"].tolist() == [0, 2, 3, 4, 5, 8] and r["length"].tolist() == [2, 1, 1, 1, 3, 1]
    assert r["label"].tolist() == [0, 1, -1, -1, 1, 7] and r["flags"].tolist() == [1, 0, 2, 3, 1, 2]
    assert len(label_runs([], [])["start"]) == 0
    r = label_runs([5, 5, 5])
    assert r["start"].tolist() == [0] and r["length"].tolist() == [3] and r["flags"].tolist() == [3]


def test_oracle_native_q():
    x = np.zeros((3, 4, 3), np.float32)
    x[:, :, 0] = np.arange(4) * 4.0                                    # a straight chain, 4 A apart
    x[1] *= 2.0
    x[2, 0, 0] = np.nan
    q = native_q(x, [[0, 3]], [12.0], beta=5.0, lam=1.0)
    assert q[0] == 0.5 and q[1] == pytest.approx(1 / (1 + math.exp(60.0))) and np.isnan(q[2])
    assert native_q(x[:1] * 1e30, [[0, 3], [0, 1]], [12.0, 4.0])[0] == 0.0
    for bad in ([[0, 4]], [[-1, 2]], [[2, 2]]):
        assert np.isnan(native_q(x, bad, [1.0])).all()


# ---------------------------------------------------------------- dwell_summary
def runs_of(*trajs):
    lab = np.concatenate([np.asarray(t, np.int32) for t in trajs])
    return label_runs(lab, [len(t) for t in trajs])


def test_dwell_summary_censoring():
    # 0 0 0 | 1 1 | 0 0 0 0 | 1: the first and the last dwell are censored, the two in the middle completed
    s = evaluate.dwell_summary(runs_of([0, 0, 0, 1, 1, 0, 0, 0, 0, 1]), frame_time=0.5)
    assert s["labels"] == [0, 1] and s["frames"] == {0: 7, 1: 3} and s["events"] == {(0, 1): 2, (1, 0): 1}
    assert s["rates"][(0, 1)] == 2 / (7 * 0.5) and s["rates"][(1, 0)] == 1 / (3 * 0.5)
    assert s["n_completed"] == {0: 1, 1: 1} and s["mean_dwell"] == {0: 2.0, 1: 1.0} and s["median_dwell"] == {0: 2.0, 1: 1.0}
    assert s["total_frames"] == 10 and s["undetermined_frames"] == 0
    # the same frames cut into two trajectories at the 1 -> 0 step: that event is gone, and no dwell is completed
    s = evaluate.dwell_summary(runs_of([0, 0, 0, 1, 1], [0, 0, 0, 0, 1]))
    assert s["frames"] == {0: 7, 1: 3} and s["events"] == {(0, 1): 2, (1, 0): 0} and s["n_completed"] == {0: 0, 1: 0}
    assert math.isnan(s["mean_dwell"][0]) and math.isnan(s["median_dwell"][1])


def test_dwell_summary_undetermined_run_breaks_the_event():
    s = evaluate.dwell_summary(runs_of([0, 0, -1, 1, 1, 0]))
    assert s["events"] == {(0, 1): 0, (1, 0): 1} and s["frames"] == {0: 3, 1: 2} and s["undetermined_frames"] == 1
    assert s["rates"][(0, 1)] == 0.0 and s["rates"][(1, 0)] == 0.5
    # the dwell of 1 has an exit but no entry event: not completed
    assert s["n_completed"] == {0: 0, 1: 0}


def test_dwell_summary_without_time():
    s = evaluate.dwell_summary(runs_of([-1, -1, -1]))
    assert s["labels"] == [] and s["events"] == {} and s["rates"] == {} and s["total_frames"] == 3
    s = evaluate.dwell_summary(label_runs([], []))
    assert s["total_frames"] == 0 and s["labels"] == []
    r = evaluate.FoldingKineticsEvaluator.summarize(s, 1, 0)
    assert all(math.isnan(r[k]) for k in ("folded_share", "rate_folding", "rate_unfolding", "mean_dwell_folded",
                                          "free_energy_folding_kT")) and r["n_folding"] == 0.0
    # one state only: there is no other state to go to or to come from
    s = evaluate.dwell_summary(runs_of([1, 1, 1]))
    r = evaluate.FoldingKineticsEvaluator.summarize(s, 1, 0)
    assert r["folded_share"] == 1.0 and r["unfolded_share"] == 0.0 and math.isnan(r["rate_folding"])
    assert math.isnan(r["rate_unfolding"]) and math.isnan(r["free_energy_folding_kT"])
    with pytest.raises(ValueError, match="frame_time"):
        evaluate.dwell_summary(runs_of([0]), frame_time=0.0)


def test_summarize_keys_and_labels():
    s = evaluate.dwell_summary(runs_of([0, 0, 0, 1, 1, 0, 0, 0, 0, 1]))
    q = evaluate.FoldingKineticsEvaluator.summarize(s, 1, 0, samples_nonfinite=2)       # Q: folded is label 1
    assert set(q) == set(evaluate.FoldingKineticsEvaluator.KEYS)
    assert q["folded_share"] == 0.3 and q["unfolded_share"] == 0.7 and q["undetermined_share"] == 0.0
    assert q["n_folding"] == 2.0 and q["n_unfolding"] == 1.0 and q["rate_folding"] == 2 / 7 and q["rate_unfolding"] == 1 / 3
    assert q["free_energy_folding_kT"] == pytest.approx(-math.log(3 / 7)) and q["samples_nonfinite"] == 2.0
    r = evaluate.FoldingKineticsEvaluator.summarize(s, 0, 1)                             # RMSD: folded is label 0
    assert r["folded_share"] == 0.7 and r["n_folding"] == 1.0 and r["rate_unfolding"] == 2 / 7
    assert r["mean_dwell_folded"] == 4.0 and r["mean_dwell_unfolded"] == 2.0


# ---------------------------------------------------------------- native_pairs, the evaluator, the package, the tool
def test_native_pairs_on_the_golden_folded_structures(golden):
    folded = golden("struct_folded.npz")
    for mol, want in (("chignolin", 22), ("trp_cage", 71), ("bba", 93), ("villin", 136), ("protein_g", 277)):
        f = folded[mol]
        pairs, r0 = evaluate.native_pairs(f)
        assert pairs.dtype == np.int32 and r0.dtype == np.float32 and pairs.shape == (want, 2) and r0.shape == (want,), mol
        assert np.all(pairs[:, 1] >= pairs[:, 0] + 3) and pairs.max() < len(f) and np.all(r0 < 10.0)
        d = np.linalg.norm(f[pairs[:, 0]].astype(np.float64) - f[pairs[:, 1]], axis=1)
        assert np.abs(d - r0).max() < 1e-5
        assert len(evaluate.native_pairs(f, cutoff=1e3, offset=1)[0]) == len(f) * (len(f) - 1) // 2


def test_native_pairs_checks_its_arguments():
    f = np.arange(30, dtype=np.float64).reshape(10, 3)
    for kw, what in ((dict(cutoff=NAN), "cutoff"), (dict(cutoff=0.0), "cutoff"), (dict(offset=0), "offset"),
                     (dict(offset=10), "offset"), (dict(offset=1.5), "offset"), (dict(cutoff=1.0), "no pair")):
        with pytest.raises(ValueError, match=what):
            evaluate.native_pairs(f, **kw)
    for bad in (np.zeros((3, 3)), np.zeros((65, 3)), np.zeros((10, 2)), np.full((10, 3), NAN)):
        with pytest.raises(ValueError, match="native_pairs"):
            evaluate.native_pairs(bad)


def test_evaluator_checks_its_arguments(monkeypatch, golden):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    f = golden("struct_folded.npz")["chignolin"]
    for kw, what in ((dict(cv="tic", lo=0.2, hi=0.9), "cv"), (dict(lo=0.9, hi=0.2), "lo"), (dict(lo=0.5, hi=0.5), "lo"),
                     (dict(lo=NAN, hi=0.9), "lo"), (dict(lo=0.2, hi=INF), "hi"), (dict(lo=0.2, hi=0.9, frame_time=0.0), "frame_time"),
                     (dict(lo=0.2, hi=0.9, beta=-1.0), "beta"), (dict(lo=0.2, hi=0.9, lam=NAN), "lam")):
        with pytest.raises(ValueError, match=what):
            evaluate.FoldingKineticsEvaluator("chignolin", f, **kw, device="cpu")
    ev = evaluate.FoldingKineticsEvaluator("chignolin", f, lo=0.2, hi=0.9, device="cpu")
    assert (ev.folded_label, ev.unfolded_label) == (1, 0) and ev.pairs.shape == (22, 2)
    ev = evaluate.FoldingKineticsEvaluator("chignolin", f, cv="rmsd", lo=1.0, hi=4.0, device="cpu")
    assert (ev.folded_label, ev.unfolded_label) == (0, 1)
    with pytest.raises(NotImplementedError):
        ev.eval(np.zeros((3, 10, 3)), plot_dynamics=True)
    with pytest.raises(ValueError, match="lo"):
        evaluate.core_states(np.zeros(3), 0.9, 0.2)


def test_evaluator_raises_without_library(monkeypatch, golden):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.FoldingKineticsEvaluator("chignolin", golden("struct_folded.npz")["chignolin"], lo=0.2, hi=0.9, device="cpu")


def test_package_reexports():
    for name in ("native_pairs", "native_contacts_q", "core_states", "label_runs", "dwell_summary", "FoldingKineticsEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__


def test_kinetics_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.kinetics is None and a.kinetics_cv == "q" and a.kinetics_cores is None and a.frame_time == 1.0
    assert a.clusters is None and a.parallel_sim is None and a.folded_pdb is None          # the existing defaults stand
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--kinetics", "--folded-pdb", "f.pdb", "--parallel-sim", "8"])
    assert a.kinetics == "" and a.folded_pdb == "f.pdb" and a.parallel_sim == 8
    assert tool.kinetics_cores(a) == (0.2, 0.9)
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--kinetics", "heldout.pt", "--kinetics-cv", "rmsd", "--kinetics-cores",
                       "1.5,4", "--frame-time", "0.2"])
    assert a.kinetics == "heldout.pt" and a.kinetics_cv == "rmsd" and a.kinetics_cores == (1.5, 4.0) and a.frame_time == 0.2
    for bad in (["--kinetics-cores", "4,1.5"], ["--kinetics-cores", "1"], ["--kinetics-cores", "a,b"],
                ["--kinetics-cores", "nan,1"], ["--kinetics-cv", "tic"], ["--frame-time", "0"], ["--frame-time", "inf"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--kinetics"] + bad)
    with pytest.raises(SystemExit):                                                         # the RMSD has no default cores
        tool.kinetics_cores(ap.parse_args(["s.pt", "chignolin", "refs", "--kinetics", "--kinetics-cv", "rmsd"]))


def test_log10_ratio_is_nan_unless_both_are_finite_and_positive():
    assert evaluate._log10_ratio(2, 1) == np.log10(2.0) and evaluate._log10_ratio(1.0, 4.0) == np.log10(0.25)
    for a, b in ((0, 1), (1, 0), (NAN, 1), (INF, 1), (-1, 1), (1, NAN), (1, INF), (1, -1)):
        assert np.isnan(evaluate._log10_ratio(a, b)), (a, b)
    got = evaluate._log10_ratio([2.0, 0.0, 1.0, NAN], [1.0, 1.0, 0.0, 1.0])
    assert got[0] == np.log10(2.0) and np.isnan(got[1:]).all() and len(got) == 4 and isinstance(got, list)
    assert evaluate._log10_ratio([], []) == []
    for a, b in (([1.0, 2.0], 1.0), (1.0, [1.0]), ([1.0, 2.0], [1.0])):
        with pytest.raises(ValueError):
            evaluate._log10_ratio(a, b)
