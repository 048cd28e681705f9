"""Host side of the Markov state models: the symbols and refusals of the dff_micro_* / dff_msm_* calls (on the host, before any
device call: they run on a machine without one), largest_connected_set against scipy, the properties of the oracle's
reversible estimator (oracle/msm.py), MarkovStateModel on top of the oracle's sweeps, timescales of a known matrix, the
evaluator's argument checks and dict keys, the package's re-exports and the --msm arguments of tools_eval_samples.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dff_amd
from dff_amd import binding, evaluate
from oracle import msm as oracle
from support import refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_micro_chunk", "dff_micro_kmeans_workspace_bytes", "dff_micro_kmeans_step", "dff_micro_transition_counts",
         "dff_msm_workspace_bytes", "dff_msm_reversible_steps", "dff_debug_msm_driver", "dff_msm_driver_for")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+DFF_MSM_MAXK\s+1024\b", header) and binding.MSM_MAX_STATES == evaluate.MSM_MAX_STATES == 1024
    assert len(binding.SYMBOLS["dff_micro_kmeans_step"][1]) == len(binding.SYMBOLS["dff_kmeans_step"][1]) == 14
    assert len(binding.SYMBOLS["dff_micro_transition_counts"][1]) == len(binding.SYMBOLS["dff_transition_counts"][1]) == 10
    assert len(binding.SYMBOLS["dff_msm_reversible_steps"][1]) == 10
    assert binding.SYMBOLS["dff_msm_workspace_bytes"][0] is C.c_longlong
    chunk = binding.MICRO_CHUNK
    assert chunk == lib.dff_micro_chunk() and chunk >= 256 and chunk % 256 == 0


def test_workspace_bytes():
    lib = binding.load_library()
    Cn = binding.MICRO_CHUNK
    for bad in ((-1, 1, 1), (10, 0, 1), (10, 9, 1), (10, 1, 0), (10, 1, 1025)):
        assert lib.dff_micro_kmeans_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="centres must be 1..1024"):
        binding.micro_kmeans_workspace_bytes(10, 2, 1025)
    assert binding.micro_kmeans_workspace_bytes(0, 2, 5) == 0
    for n, rows in ((1, 1), (Cn, 1), (Cn + 1, 2), (2 * Cn + 1, 3)):
        assert binding.micro_kmeans_workspace_bytes(n, 2, 5) == rows * (5 * 3 + 1) * 8
    assert binding.micro_kmeans_workspace_bytes(819200, 8, 1024) == -(-819200 // Cn) * (1024 * 9 + 1) * 8
    assert binding.msm_workspace_bytes(1) == 16 and binding.msm_workspace_bytes(1024) == 16384
    for bad in (0, 1025, -3):
        assert lib.dff_msm_workspace_bytes(bad) == -1
        with pytest.raises(ValueError, match="states must be 1..1024"):
            binding.msm_workspace_bytes(bad)


def test_refusals_before_any_device_call():
    lib = binding.load_library()
    km = lambda n, d, K, ws=FAKE, wsb=1 << 30: lib.dff_micro_kmeans_step(0, FAKE, n, d, FAKE, K, FAKE, FAKE, FAKE, FAKE, FAKE, ws, wsb, None)  # noqa: E731
    refused(lib, km(10, 2, 0), "centres must be 1..1024")
    refused(lib, km(10, 2, 1025), "centres must be 1..1024")
    refused(lib, km(10, 0, 4), "d must be 1..8")
    refused(lib, km(10, 9, 4), "d must be 1..8")
    refused(lib, km(-1, 2, 4), "negative point count")
    refused(lib, km(10, 2, 4, FAKE, 8), "workspace of 8 bytes")
    refused(lib, km(10, 2, 4, C.c_void_p(4097)), "8-byte aligned")
    refused(lib, lib.dff_micro_kmeans_step(0, None, 10, 2, FAKE, 4, FAKE, FAKE, None, None, None, None, 0, None), "null points")
    one, lag1 = np.array([10], np.int64), np.array([1], np.int32)
    tc = lambda K, lags, lengths=one, n=10: lib.dff_micro_transition_counts(0, FAKE, n, p(lengths), len(lengths), p(lags), len(lags), K, FAKE, None)  # noqa: E731
    refused(lib, tc(0, lag1), "states must be 1..1024")
    refused(lib, tc(1025, lag1), "states must be 1..1024")
    refused(lib, tc(4, np.array([0], np.int32)), "must be >= 1")
    refused(lib, tc(4, np.arange(1, 10, dtype=np.int32)), "lag times must be 1..8")
    refused(lib, tc(4, lag1, np.array([4, 5], np.int64)), "sum to 9, not n = 10")
    ms = lambda K, steps=1, wsb=1 << 20, ws=FAKE: lib.dff_msm_reversible_steps(0, FAKE, FAKE, K, FAKE, steps, None, ws, wsb, None)  # noqa: E731
    refused(lib, ms(0), "states must be 1..1024")
    refused(lib, ms(1025), "states must be 1..1024")
    refused(lib, ms(4, -1), "negative n_steps")
    refused(lib, ms(4, 1, 63), "workspace of 63 bytes, 64 needed")
    refused(lib, ms(4, 1, 64, C.c_void_p(4100)), "8-byte aligned")
    refused(lib, lib.dff_debug_msm_driver(3), "debug_msm_driver")
    assert lib.dff_debug_msm_driver(0) == 0
    assert [binding.msm_driver_for(K) for K in (1, 32, 33, 1024)] == [2, 2, 1, 1]       # the measured crossover
    for forced in (1, 2):
        assert lib.dff_debug_msm_driver(forced) == 0 and [binding.msm_driver_for(K) for K in (1, 1024)] == [forced, forced]
    assert lib.dff_debug_msm_driver(0) == 0 and lib.dff_msm_driver_for(0) == -1 and lib.dff_msm_driver_for(1025) == -1


# ---------------------------------------------------------------- the largest strongly connected set
def random_digraph(K, seed, density):
    rng = np.random.default_rng(seed)
    return (rng.random((K, K)) < density) * rng.integers(1, 9, (K, K))


def scipy_largest(sp, counts):
    n, lab = sp.connected_components(np.asarray(counts) > 0, directed=True, connection="strong")
    sizes = np.bincount(lab, minlength=n)
    firsts = np.array([np.flatnonzero(lab == c)[0] for c in range(n)])
    best = max(range(n), key=lambda c: (sizes[c], -firsts[c]))
    return np.flatnonzero(lab == best)


DENSITIES = (0.0, 0.5, 1.0, 1.5, 3.0)            # expected out-degree; and half of all edges
TWO_TRIPLES = ((4, 5), (5, 6), (6, 4), (1, 3), (3, 2), (2, 1), (3, 4))      # {1, 2, 3} -> {4, 5, 6}: two components of three


def digraphs(K):
    for seed, density in enumerate(tuple(v / K for v in DENSITIES) + (0.5,)):
        yield density, random_digraph(K, 100 * K + seed, density)


def two_triples():
    c = np.zeros((7, 7))
    for a, b in TWO_TRIPLES:
        c[a, b] = 2
    return c


@pytest.mark.parametrize("K", [1, 2, 7, 50, 300])
def test_largest_connected_set_equals_scipy(K):
    sp = pytest.importorskip("scipy.sparse.csgraph")
    for density, c in digraphs(K):
        assert np.array_equal(evaluate.largest_connected_set(c), scipy_largest(sp, c)), (K, density)


def test_largest_connected_set_equals_scipy_on_ties_and_empty_graphs():
    sp = pytest.importorskip("scipy.sparse.csgraph")
    for c in (two_triples(), np.zeros((5, 5)), np.zeros((1, 1))):
        assert np.array_equal(evaluate.largest_connected_set(c), scipy_largest(sp, c))
    assert scipy_largest(sp, two_triples()).tolist() == [1, 2, 3]


@pytest.mark.parametrize("K", [1, 2, 7, 50, 300])
def test_largest_connected_set_equals_the_oracle(K):
    for density, c in digraphs(K):
        got = evaluate.largest_connected_set(c)
        assert got.dtype == np.int64 and np.array_equal(got, np.sort(got))
        assert np.array_equal(got, oracle.largest_connected_set(c)), (K, density)


def test_largest_connected_set_ties_and_empty_graphs():
    c = two_triples()
    assert evaluate.largest_connected_set(c).tolist() == [1, 2, 3]
    c[0, 0] = 5                                                                 # a self-loop is a component of one
    assert evaluate.largest_connected_set(c).tolist() == [1, 2, 3]
    assert evaluate.largest_connected_set(np.zeros((5, 5))).tolist() == [0]      # all singletons: the lowest index
    assert evaluate.largest_connected_set(np.zeros((0, 0))).tolist() == []
    chain = np.diag(np.ones(2999), 1)                                           # a 3000-state path: deep, no recursion
    assert evaluate.largest_connected_set(chain).tolist() == [0]
    chain[2999, 0] = 1
    assert len(evaluate.largest_connected_set(chain)) == 3000
    with pytest.raises(ValueError, match="square"):
        evaluate.largest_connected_set(np.zeros((2, 3)))


# ---------------------------------------------------------------- the oracle's estimator
check_reversible = oracle.check_reversible


@pytest.mark.parametrize("K", [2, 3, 5, 64, 65])
def test_oracle_estimator_properties(K):
    C = oracle.connected_counts(K, 7 * K, diag=1e2)
    T, pi, x, n_iter = oracle.reversible_mle(C)
    assert n_iter > 1 or K == 2
    check_reversible(C, T, pi, f"K = {K}")


def test_oracle_symmetric_counts_are_a_fixed_point():
    C = oracle.connected_counts(9, 3, diag=50.0)
    C = C + C.T
    S, c = C + C.T, C.sum(axis=1)
    x, err = oracle.sweep(S, c, oracle.start(S))
    assert err < 13 * 2.0 ** -53
    T, pi = oracle.transition_matrix_from_x(S, c, x)
    assert np.abs(T - oracle.row_normalised(C)).max() < 1e-14 and np.abs(pi - c / c.sum()).max() < 1e-15


# ---------------------------------------------------------------- MarkovStateModel on the oracle's sweeps
class OracleSweeps:
    calls = 0

    def __init__(self, S, c, device):
        self.S, self.c = np.array(S), np.array(c)

    def __call__(self, x, n):
        OracleSweeps.calls += 1
        return oracle.sweeps(self.S, self.c, np.array(x), n)


@pytest.fixture
def on_oracle(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    OracleSweeps.calls = 0


@pytest.mark.parametrize("K", [2, 3, 5, 64])
def test_model_reproduces_the_oracle(on_oracle, K):
    C = oracle.connected_counts(K, 7 * K, diag=1e2)
    m = evaluate.MarkovStateModel(3, tol=1e-13, steps_per_sync=16).fit_counts(C)
    assert m.converged and m.active_set.tolist() == list(range(K)) and m.active_count_share == 1.0
    T, pi, x, n_iter = oracle.reversible_mle(C)
    assert m.n_iter == n_iter and OracleSweeps.calls == -(-n_iter // 16)
    check_reversible(C, m.transition_matrix, m.stationary_distribution, f"model, K = {K}")
    assert np.abs(m.transition_matrix - T).max() < 1e-11 and np.abs(m.stationary_distribution - pi).max() < 1e-11
    assert m.log_likelihood() == pytest.approx(oracle.log_likelihood(C, T), rel=1e-12)
    ts = m.timescales(4)
    want = oracle.timescales(T, pi, 3, 4)
    assert ts.shape == (4,) and np.array_equal(np.isnan(ts), np.isnan(want))
    assert np.allclose(ts[~np.isnan(ts)], want[~np.isnan(want)], rtol=1e-8)
    if K == 2:
        assert np.isnan(ts[1:]).all()


def test_model_active_set_and_max_iter(on_oracle):
    C = np.zeros((6, 6))
    C[np.ix_([1, 3, 4], [1, 3, 4])] = oracle.connected_counts(3, 5, diag=10.0)
    C[0, 1] = 4                                        # 0 feeds the set, 5 is isolated, 2 only receives
    C[3, 2] = 3
    m = evaluate.MarkovStateModel(1).fit_counts(C)
    assert m.active_set.tolist() == [1, 3, 4] and m.transition_matrix.shape == (3, 3) and m.count_matrix.shape == (6, 6)
    assert m.active_count_share == pytest.approx(1 - 7 / C.sum())
    check_reversible(C[np.ix_([1, 3, 4], [1, 3, 4])], m.transition_matrix, m.stationary_distribution, "active set")
    slow = evaluate.MarkovStateModel(1, max_iter=3, steps_per_sync=2).fit_counts(oracle.connected_counts(5, 35, diag=1e2))
    assert not slow.converged and slow.n_iter == 3 and OracleSweeps.calls >= 2
    one = evaluate.MarkovStateModel(1).fit_counts(np.zeros((4, 4)))
    assert one.active_set.tolist() == [0] and one.transition_matrix.tolist() == [[1.0]] and one.active_count_share == 0.0
    assert np.isnan(one.timescales(2)).all()
    nonrev = evaluate.MarkovStateModel(2, reversible=False).fit_counts(C)
    assert np.allclose(nonrev.transition_matrix, oracle.row_normalised(C[np.ix_([1, 3, 4], [1, 3, 4])]))
    assert np.allclose(nonrev.stationary_distribution @ nonrev.transition_matrix, nonrev.stationary_distribution)
    for bad in (np.zeros((2, 3)), -np.ones((2, 2)), np.full((2, 2), np.nan)):
        with pytest.raises(ValueError, match="counts"):
            evaluate.MarkovStateModel(1).fit_counts(bad)
    for kw in (dict(lagtime=0), dict(lagtime=1.5), dict(lagtime=1, tol=0.0), dict(lagtime=1, steps_per_sync=0)):
        with pytest.raises(ValueError):
            evaluate.MarkovStateModel(**kw)
    with pytest.raises(ValueError, match="not fitted"):
        evaluate.MarkovStateModel(1).timescales()


def test_timescales_of_a_known_three_state_matrix(on_oracle):
    """T = 0.8 I + 0.1 [[1, 1, 0], [1, 0, 1], [0, 1, 1]] is symmetric (reversible, pi uniform) with eigenvalues 1, 0.9, 0.7."""
    T = np.array([[0.9, 0.1, 0.0], [0.1, 0.8, 0.1], [0.0, 0.1, 0.9]])
    m = evaluate.MarkovStateModel(5).fit_counts(1000 * T)                 # symmetric counts: the fixed point at the start
    assert m.converged and m.n_iter == 1
    assert np.abs(m.transition_matrix - T).max() < 1e-15 and np.abs(m.stationary_distribution - 1 / 3).max() < 1e-15
    assert np.allclose(m.eigenvalues(), [1.0, 0.9, 0.7], rtol=0, atol=1e-14)
    ts = m.timescales(3)
    assert np.allclose(ts[:2], [-5 / np.log(0.9), -5 / np.log(0.7)], rtol=1e-12) and np.isnan(ts[2])
    neg = evaluate.MarkovStateModel(1).fit_counts(np.array([[1.0, 9.0], [9.0, 1.0]]))      # lambda_2 = -0.8: no timescale
    assert np.isnan(neg.timescales(1)[0])


# ---------------------------------------------------------------- the evaluator, the package, the tool
def test_evaluator_checks_its_arguments(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    F = binding.DFF_MAX_BEADS
    tica = (np.zeros(F), np.zeros((F, 2)))
    for kw, what in ((dict(), "lagtime"), (dict(lagtime=0), "lagtime"), (dict(lagtime=2.5), "lagtime"),
                     (dict(lagtime=1, n_microstates=0), "n_microstates"), (dict(lagtime=1, n_microstates=1025), "n_microstates"),
                     (dict(lagtime=1, n_timescales=0), "n_timescales"), (dict(lagtime=1, frame_time=0.0), "frame_time"),
                     (dict(lagtime=1, frame_time=float("inf")), "frame_time"),
                     (dict(lagtime=1, n_microstates=3, centers=np.zeros((4, 2))), "centers"),
                     (dict(lagtime=1, n_microstates=3, centers=np.full((3, 2), np.nan)), "centers")):
        with pytest.raises(ValueError, match=what):
            evaluate.MsmEvaluator("chignolin", tica, **kw, device="cpu")
    with pytest.raises(ValueError, match="coeff"):
        evaluate.MsmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 9))), lagtime=1, device="cpu")
    e = evaluate.MsmEvaluator("chignolin", tica, n_microstates=3, lagtime=4, centers=np.eye(3, 2), frame_time=0.5, device="cpu")
    assert e.centers.shape == (3, 2) and e.lagtime == 4 and e.ref_result is None and e.models == {}
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="n_clusters"):
            evaluate.MicrostateKMeans(bad, device="cpu")
    assert evaluate.MicrostateKMeans(1024, device="cpu").n_clusters == 1024
    with pytest.raises(ValueError, match="1..64"):
        evaluate.KMeans(65, device="cpu")                                   # the K <= 64 class keeps its limit


def test_the_two_kmeans_classes_keep_their_own_names_limits_and_seeding(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    with pytest.raises(ValueError, match=r"^KMeans: n_clusters must be 1\.\.64$"):
        evaluate.KMeans(65, device="cpu")
    with pytest.raises(ValueError, match=r"^MicrostateKMeans: n_clusters must be 1\.\.1024$"):
        evaluate.MicrostateKMeans(1025, device="cpu")
    with pytest.raises(ValueError, match="^MicrostateKMeans: not fitted$"):
        evaluate.MicrostateKMeans(3, device="cpu").transform(np.zeros((4, 2)))
    assert evaluate.MicrostateKMeans._seed_centers is not evaluate.KMeans._seed_centers


def test_evaluator_raises_without_library(monkeypatch):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.MsmEvaluator("chignolin", (np.zeros(64), np.zeros((64, 2))), lagtime=1, device="cpu")


def test_summarize_keys_and_stationary_js(on_oracle):
    a = evaluate.MarkovStateModel(2).fit_counts(np.array([[90.0, 10, 0], [10, 80, 10], [0, 10, 90]]))
    r = evaluate.MsmEvaluator.summarize(a, n_timescales=3, frame_time=0.5, samples_nonfinite=2)
    assert set(r) == set(evaluate.MsmEvaluator.KEYS)
    assert r["n_active"] == 3.0 and r["converged"] == 1.0 and r["samples_nonfinite"] == 2.0 and r["active_count_share"] == 1.0
    assert r["timescales"][:2] == pytest.approx([0.5 * -2 / np.log(0.9), 0.5 * -2 / np.log(0.7)]) and np.isnan(r["timescales"][2])
    assert evaluate.MsmEvaluator.stationary_js(a, a) == pytest.approx(0.0, abs=1e-15)
    c = np.zeros((3, 3))
    c[:2, :2] = [[50.0, 50], [50, 50]]
    b = evaluate.MarkovStateModel(2).fit_counts(c)                            # active set {0, 1}, pi = (1/2, 1/2)
    assert b.active_set.tolist() == [0, 1]
    want = evaluate.js_divergence(np.array([1 / 3, 1 / 3, 1 / 3]), np.array([0.5, 0.5, 0.0]))
    assert evaluate.MsmEvaluator.stationary_js(a, b) == pytest.approx(want, rel=1e-12) and want > 0.05


def test_package_reexports():
    for name in ("MicrostateKMeans", "largest_connected_set", "MarkovStateModel", "implied_timescales", "MsmEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    assert issubclass(evaluate.MicrostateKMeans, evaluate.KMeans)
    for name in ("micro_kmeans_step", "micro_kmeans_workspace_bytes", "micro_transition_counts", "msm_reversible_steps",
                 "msm_workspace_bytes"):
        assert callable(getattr(binding, name))


def test_msm_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.msm is None and a.msm_states is None and a.msm_lag is None and a.msm_lagtimes is None and a.frame_time == 1.0
    assert a.relaxation is None and a.kinetics is None                                      # the existing defaults stand
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--msm", "--msm-states", "200", "--msm-lag", "10"])
    assert a.msm == "" and tool.msm_arguments(a) == (200, 10)
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--msm", "heldout.pt", "--msm-states", "1024", "--msm-lag", "5",
                       "--msm-lagtimes", "1,2,5,10", "--frame-time", "0.2"])
    assert a.msm == "heldout.pt" and a.msm_lagtimes == [1, 2, 5, 10] and a.frame_time == 0.2
    for bad in (["--msm-states", "0"], ["--msm-states", "1025"], ["--msm-states", "x"], ["--msm-lag", "0"],
                ["--msm-lagtimes", "1,0"], ["--msm-lagtimes", "1,x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--msm"] + bad)
    for missing in ([], ["--msm-states", "10"], ["--msm-lag", "3"]):                        # neither has a default
        with pytest.raises(SystemExit):
            tool.msm_arguments(ap.parse_args(["s.pt", "chignolin", "refs", "--msm"] + missing))
