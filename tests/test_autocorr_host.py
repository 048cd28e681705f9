"""Host side of dff_autocorr and of the relaxation analysis on top of it: the symbols, the refusals of bad arguments (on the
host, before any device call: they run on a machine without one), Sokal's window and the 1 / e crossing on geometric ACFs,
the algebra of the effective sample size and the standard error, both estimators from hand-made sums, the numpy oracle on a
hand-written series, the evaluator's argument checks, the package's re-exports and the --relaxation arguments of
tools_eval_samples.py.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from dff_amd import binding, evaluate
from oracle.autocorr import Acf, estimate, lagged_sums
from support import refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_autocorr_workspace_bytes", "dff_autocorr")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_autocorr"][1]) == 15
    assert len(binding.SYMBOLS["dff_autocorr_workspace_bytes"][1]) == 3
    assert binding.SYMBOLS["dff_autocorr_workspace_bytes"][0] is C.c_longlong


def test_workspace_bytes():
    lib = binding.load_library()
    for bad in ((-1, 1, 10), (10, 0, 10), (10, 9, 10), (10, 1, -1), (10, 1, 65536)):
        assert lib.dff_autocorr_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="d must be 1..8"):
        binding.autocorr_workspace_bytes(10, 9, 10)
    with pytest.raises(ValueError, match="max_lag must be 0..65535"):
        binding.autocorr_workspace_bytes(10, 1, 65536)
    assert binding.autocorr_workspace_bytes(0, 1, 10) == 0
    # 4 bytes per frame (rounded up to 8) + one slot of 3 d + 1 sums per lag and tile of 512 frames, while the tiles are few
    assert binding.autocorr_workspace_bytes(1, 1, 0) == 8 + 4 * 8
    assert binding.autocorr_workspace_bytes(513, 2, 10) == 2056 + 2 * 7 * 11 * 8
    # bounded in n: the partials stop growing once there are ~2048 workgroups
    at = lambda n: binding.autocorr_workspace_bytes(n, 2, 4096) - 4 * n           # noqa: E731
    assert at(10 ** 6) == at(10 ** 7) == at(10 ** 9) and at(10 ** 6) + 4 * 10 ** 6 < 256 * 2 ** 20
    for d, L in ((1, 65535), (8, 65535), (8, 511), (3, 20000)):
        assert binding.autocorr_workspace_bytes(10 ** 6, d, L) - 4 * 10 ** 6 < 64 * 2 ** 20, (d, L)
    assert all(binding.autocorr_workspace_bytes(n, 3, 77) % 8 == 0 for n in (1, 2, 3, 511, 512, 513))


def test_autocorr_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n, d, L = 5000, 2, 100
    need = binding.autocorr_workspace_bytes(n, d, L)
    ws = np.zeros(need + 8, np.uint8)
    one = np.array([n], np.int64)
    null = None                      # the device pointers: refused before anything would read them

    def call(n_=n, d_=d, L_=L, lengths=one, series=C.c_void_p(8), sxy=C.c_void_p(8), ws_=p(ws), ws_bytes=need):
        return lib.dff_autocorr(0, series, n_, d_, p(lengths) if lengths is not None else None,
                                len(lengths) if lengths is not None else 1, L_, null, sxy, null, null, null, ws_, ws_bytes, None)

    # a short workspace is sized for the call's own shape, so every case below keeps (n, d, L) unless it is the case
    for what, kw in (("d must be 1..8", dict(d_=0)), ("d must be 1..8", dict(d_=9)),
                     ("max_lag must be 0..65535", dict(L_=-1)), ("max_lag must be 0..65535", dict(L_=65536)),
                     ("negative frame count", dict(n_=-1)),
                     ("sum to 4999, not n = 5000", dict(lengths=np.array([4000, 999], np.int64))),
                     ("trajectory 1 has negative length", dict(lengths=np.array([5001, -1], np.int64))),
                     ("null / negative trajectory lengths", dict(lengths=None)),
                     ("null series", dict(series=None)), ("null sxy", dict(sxy=None)),
                     ("workspace of %d bytes, %d needed" % (need - 1, need), dict(ws_bytes=need - 1)),
                     ("workspace of 0 bytes", dict(ws_=None, ws_bytes=0)),
                     ("8-byte aligned", dict(ws_=C.c_void_p(ws.ctypes.data + 4)))):
        refused(lib, call(**kw), what)
    refused(lib, lib.dff_autocorr(0, None, 0, 1, None, 0, 5, None, None, None, None, None, None, 0, None), "null sxy")
    with pytest.raises(ValueError, match="series"):
        binding.autocorr(torch.zeros((5, 1), dtype=torch.float64), [5], 2)      # not a CUDA tensor


# ---------------------------------------------------------------- Sokal's window and the 1 / e crossing
@pytest.mark.parametrize("phi", [0.5, 0.9, 0.99])
def test_integrated_autocorr_time_on_a_geometric_acf(phi):
    L, c = 2048, 5.0
    rho = phi ** np.arange(L + 1)
    tau, W, converged = evaluate.integrated_autocorr_time(rho, c)
    assert converged and 1 <= W <= L
    tau_of = lambda w: 0.5 + sum(phi ** l for l in range(1, w + 1))     # noqa: E731
    assert tau == pytest.approx(tau_of(W), rel=1e-12)
    assert W >= c * tau_of(W) and not (W - 1 >= c * tau_of(W - 1))
    exact = 0.5 + phi / (1 - phi)                                       # the full sum: the window cuts off phi^(W+1) / (1 - phi)
    assert exact - phi ** (W + 1) / (1 - phi) == pytest.approx(tau, rel=1e-9) and tau < exact
    # (L, 1) is taken as one component; two components are refused
    assert evaluate.integrated_autocorr_time(rho[:, None], c) == (tau, W, True)
    with pytest.raises(ValueError):
        evaluate.integrated_autocorr_time(np.stack([rho, rho], 1))


def test_integrated_autocorr_time_without_a_window():
    phi = 0.99                                                          # tau = 99.5: the window closes near 5 tau
    rho = phi ** np.arange(101)
    tau, W, converged = evaluate.integrated_autocorr_time(rho)
    assert not converged and W == 100 and tau == pytest.approx(0.5 + rho[1:].sum(), rel=1e-12)
    # lags without a pair (NaN) are not available: the sum stops before the first of them
    rho[41:] = np.nan
    tau, W, converged = evaluate.integrated_autocorr_time(rho)
    assert not converged and W == 40 and tau == pytest.approx(0.5 + rho[1:41].sum(), rel=1e-12)
    assert evaluate.integrated_autocorr_time(np.ones(1)) == (0.5, 0, False)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="c must be"):
            evaluate.integrated_autocorr_time(rho, bad)


@pytest.mark.parametrize("phi", [0.5, 0.9, 0.99])
def test_crossing_time_on_a_geometric_acf(phi):
    """phi^x is convex: the chord lies above it, so the interpolated crossing comes late, by at most max f'' / 8 over the chord's
    slope on the interval of the crossing = ln(phi)^2 / (8 (1 - phi)) frames."""
    rho = phi ** np.arange(2049)
    t = evaluate.crossing_time(rho)
    exact = -1.0 / math.log(phi)
    assert -1e-12 <= t - exact <= math.log(phi) ** 2 / (8 * (1 - phi)) + 1e-12, (t, exact)
    assert evaluate.crossing_time(rho, 0.25) == pytest.approx(math.log(0.25) / math.log(phi), abs=math.log(phi) ** 2 / (8 * (1 - phi)) + 1e-12)
    assert evaluate.crossing_time(rho, 2.0) == 0.0                      # below the level from the start


def test_crossing_time_without_a_crossing():
    assert math.isnan(evaluate.crossing_time(np.ones(100)))
    assert math.isnan(evaluate.crossing_time(np.array([1.0, 0.9, np.nan, 0.1])))
    assert evaluate.crossing_time(np.array([1.0, 0.5, 0.25]), 0.375) == 1.5


def test_sample_size_algebra():
    assert evaluate.effective_sample_size(819200, 50.0) == 8192.0
    assert evaluate.effective_sample_size(10, 0.5) == 10.0              # uncorrelated frames: tau = 1/2
    assert evaluate.standard_error(4.0, 100, 0.5) == pytest.approx(0.2)
    v, n, tau = 2.5, 1000, 7.0
    assert evaluate.standard_error(v, n, tau) == pytest.approx(math.sqrt(v / evaluate.effective_sample_size(n, tau)), rel=1e-15)


# ---------------------------------------------------------------- the estimators, the oracle
def test_estimators_from_hand_made_sums():
    # x = 1 2 3 4 6, shift 0, one component: lag 0 and lag 1 by hand
    sxy = np.array([[1 + 4 + 9 + 16 + 36.0], [2 + 6 + 12 + 24.0], [0.0]])
    sx = np.array([[16.0], [10.0], [0.0]])
    sy = np.array([[16.0], [15.0], [0.0]])
    count = np.array([5, 4, 0])
    per = evaluate.autocorr_estimate(sxy, sx, sy, count, "per_lag").numpy()
    assert per[0, 0] == pytest.approx(66 / 5 - 3.2 ** 2) and per[1, 0] == pytest.approx(44 / 4 - 2.5 * 3.75) and np.isnan(per[2, 0])
    glo = evaluate.autocorr_estimate(sxy, sx, sy, count, "global").numpy()
    want = sum((a - 3.2) * (b - 3.2) for a, b in ((1, 2), (2, 3), (3, 4), (4, 6))) / 4
    assert glo[0, 0] == pytest.approx(per[0, 0]) and glo[1, 0] == pytest.approx(want) and np.isnan(glo[2, 0])
    with pytest.raises(ValueError, match="estimator"):
        evaluate.autocorr_estimate(sxy, sx, sy, count, "fft")
    # and the oracle's own estimators agree on its own sums
    s = lagged_sums([1, 2, 3, 4, 6], 2)
    assert np.array_equal(s["count"], [5, 4, 3]) and s["sxy"][1, 0] == 44 and s["sx"][1, 0] == 10 and s["sy"][1, 0] == 15
    assert np.allclose(estimate(s, "per_lag")[:2], per[:2]) and np.allclose(estimate(s, "global")[:2], glo[:2])


def test_oracle_boundaries_and_non_finite_frames():
    x = np.array([[1, 1], [2, 1], [np.nan, 1], [4, 1], [5, np.inf], [6, 1], [7, 1]], np.float64)
    s = lagged_sums(x, 3, [4, 0, 3], shift=[1.0, 0.0])
    # usable: 0 1 3 | 5 6 (frames 2 and 4 are out); trajectories [0, 4) and [4, 7)
    assert s["count"].tolist() == [5, 2, 1, 1]          # lag 1: (0, 1), (5, 6); lag 2: (1, 3); lag 3: (0, 3)
    assert s["sxy"][:, 0].tolist() == [0 + 1 + 9 + 25 + 36, 0 * 1 + 5 * 6, 1 * 3, 0 * 3] and s["sxy"][:, 1].tolist() == [5, 2, 1, 1]
    assert s["sx"][:, 0].tolist() == [15, 5, 1, 0] and s["sy"][:, 0].tolist() == [15, 7, 3, 3]
    assert s["sabs"][:, 0].tolist() == s["sxy"][:, 0].tolist()
    a = Acf(x[:, 0], 3, [4, 0, 3])
    assert a.counts.tolist() == [6, 3, 2, 1] and a.mean[0] == pytest.approx((1 + 2 + 4 + 5 + 6 + 7) / 6) and a.acf[0, 0] == 1.0


# ---------------------------------------------------------------- the evaluator, the package, the tool
def test_evaluator_checks_its_arguments(monkeypatch, golden):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    f = golden("struct_folded.npz")["chignolin"]
    for kw, what in ((dict(cv="phi", max_lag=10), "cv"), (dict(max_lag=0), "max_lag"), (dict(max_lag=65536), "max_lag"),
                     (dict(max_lag=2.5), "max_lag"), (dict(max_lag=10, frame_time=0.0), "frame_time"),
                     (dict(max_lag=10, frame_time=float("nan")), "frame_time"), (dict(cv="tic", max_lag=10), "tica")):
        with pytest.raises(ValueError, match=what):
            evaluate.RelaxationEvaluator("chignolin", f, **kw, device="cpu")
    with pytest.raises(ValueError, match="folded"):
        evaluate.RelaxationEvaluator("chignolin", None, cv="rmsd", max_lag=10, device="cpu")
    e = evaluate.RelaxationEvaluator("chignolin", f, max_lag=10, device="cpu")
    assert e.pairs.shape == (22, 2) and e.max_lag == 10 and e.ref_result is None
    F = binding.DFF_MAX_BEADS          # any (mean, coeff) pair of matching shapes
    e = evaluate.RelaxationEvaluator("chignolin", cv="tic", tica=(np.zeros(F), np.zeros((F, 3))), max_lag=10, device="cpu")
    assert e.coeff.shape == (F, 3)
    with pytest.raises(ValueError, match="estimator"):
        evaluate.autocorrelation(np.zeros(5), 2, estimator="fft", device="cpu")
    for bad, what in ((np.zeros((5, 9)), "d must be"), (np.zeros((5, 2, 2)), "series"), (np.zeros(5, np.int64), "series")):
        with pytest.raises(ValueError, match=what):
            evaluate.autocorrelation(bad, 2, device="cpu")
    for bad in (-1, 65536, 1.5):
        with pytest.raises(ValueError, match="max_lag"):
            evaluate.autocorrelation(np.zeros(5), bad, device="cpu")
    with pytest.raises(ValueError, match="trajectory lengths"):
        evaluate.autocorrelation(np.zeros(5), 2, [2, 2], device="cpu")


def test_summarize_from_an_oracle_acf():
    rng = np.random.default_rng(3)
    x = np.zeros(4000)
    for t in range(1, len(x)):
        x[t] = 0.8 * x[t - 1] + rng.standard_normal()
    a = Acf(x, 100, [2000, 2000])
    r = evaluate.RelaxationEvaluator.summarize(a, frame_time=0.5)
    tau, W, conv = evaluate.integrated_autocorr_time(a.acf[:, 0])
    assert set(r) == set(evaluate.RelaxationEvaluator.KEYS) - {"samples_nonfinite"}
    assert r["tau_int"] == tau * 0.5 and r["window_converged"] == float(conv) == 1.0 and r["tau_e"] == evaluate.crossing_time(a.acf[:, 0]) * 0.5
    assert r["ess"] == pytest.approx(4000 / (2 * tau)) and r["ess_share"] == pytest.approx(1 / (2 * tau))
    assert r["mean"] == pytest.approx(x.mean()) and r["stderr"] == pytest.approx(math.sqrt(x.var() * 2 * tau / 4000))
    assert 3.0 < tau < 6.5                                              # 1/2 + 0.8 / 0.2 = 4.5
    lists = evaluate.RelaxationEvaluator.summarize(a, frame_time=0.5, as_list=True)
    assert all(lists[k] == [r[k]] for k in r)


def test_evaluator_raises_without_library(monkeypatch, golden):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.RelaxationEvaluator("chignolin", golden("struct_folded.npz")["chignolin"], max_lag=10, device="cpu")


def test_package_reexports():
    for name in ("autocorrelation", "integrated_autocorr_time", "crossing_time", "effective_sample_size", "standard_error",
                 "RelaxationEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__


def test_relaxation_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.relaxation is None and a.relaxation_cv == "q" and a.max_lag is None and a.frame_time == 1.0
    assert a.kinetics is None and a.kinetics_cv == "q"                                      # the existing defaults stand
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--relaxation", "--max-lag", "500", "--folded-pdb", "f.pdb"])
    assert a.relaxation == "" and a.max_lag == 500
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--relaxation", "heldout.pt", "--relaxation-cv", "tic", "--max-lag", "64",
                       "--frame-time", "0.2"])
    assert a.relaxation == "heldout.pt" and a.relaxation_cv == "tic" and a.max_lag == 64 and a.frame_time == 0.2
    for bad in (["--relaxation-cv", "phi"], ["--max-lag", "0"], ["--max-lag", "65536"], ["--max-lag", "x"], ["--frame-time", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--relaxation"] + bad)
    with pytest.raises(SystemExit):                                                         # the lags have no default
        tool.relaxation_max_lag(ap.parse_args(["s.pt", "chignolin", "refs", "--relaxation"]))
