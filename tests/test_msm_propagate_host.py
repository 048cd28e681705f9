"""Host side of the propagation call: the symbols and refusals of dff_msm_propagate (refused on the host, before any device
call), the LDS arithmetic, and msm_propagate / msm_relaxation / msm_autocorrelation / metastable_sets / chapman_kolmogorov /
ChapmanKolmogorovEvaluator on a numpy stand-in behind evaluate.propagator (propagate_cases.host_propagate: `w @ T` with the
call's status rules), the re-exports and the tool's arguments.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import propagate_cases as pc
from dff_amd import binding, evaluate
from oracle import msm as oracle
from oracle import msm_bootstrap as boot
from oracle.msm_bootstrap import five_state_case
from standins import HostSpectral, OracleSweeps
from support import owning_unit, refused, same_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_msm_propagate_workspace_bytes", "dff_msm_propagate_lds_limit", "dff_msm_propagate", "dff_debug_msm_propagate_path")
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
    assert len(binding.SYMBOLS["dff_msm_propagate"][1]) == 18
    assert binding.SYMBOLS["dff_msm_propagate_workspace_bytes"] == (C.c_longlong, [C.c_int] * 4)
    assert binding.SYMBOLS["dff_msm_propagate_lds_limit"] == (C.c_int, [])
    assert binding.SYMBOLS["dff_debug_msm_propagate_path"] == (C.c_int, [C.c_int])
    assert binding.MSM_PROPAGATE_MAX_BATCH == evaluate.PROPAGATE_MAX_BATCH == 16384
    assert binding.MSM_PROPAGATE_MAX_ROWS == evaluate.PROPAGATE_MAX_ROWS == 16 and binding.MSM_PROPAGATE_MAX_STEPS == 65535
    text = owning_unit("dff_msm_propagate.hip")
    assert '#include "dff_msm_propagate.hip"' in text
    assert "dff_msm_propagate.hip" not in re.sub(r"(?m)^#.*$", "", open(os.path.join(ROOT, "build.sh")).read())   # comments only


def test_both_paths_fit_a_compute_unit():
    """the vectors (K x 16), the eight waves' partial sums, and on the LDS path the observables (K x 16) and the matrix"""
    L = binding.msm_propagate_lds_limit()
    assert 64 <= L < 1024
    assert 8 * (L * L + 2 * 16 * L + 8 * 256) <= 160 * 1024
    assert 8 * (16 * 1024 + 8 * 256) <= 160 * 1024                  # the streamed path at K = 1024


def test_workspace_bytes_and_refusals_before_any_device_call():
    lib = binding.load_library()
    assert binding.msm_propagate_workspace_bytes(1, 1, 1, 1) == 8 and binding.msm_propagate_workspace_bytes(48, 1024, 16, 16) == 48 * 8
    for bad in ((0, 4, 1, 1), (16385, 4, 1, 1), (4, 0, 1, 1), (4, 1025, 1, 1), (4, 4, 0, 1), (4, 4, 17, 1), (4, 4, 1, 0), (4, 4, 1, 17)):
        assert lib.dff_msm_propagate_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="problems must be 1..16384"):
        binding.msm_propagate_workspace_bytes(0, 4, 1, 1)

    def call(ks=(4, 3), Kmax=4, P=None, M=2, R=2, S=3, n_mat=2, mat_of=(0, 1), t=FAKE, w0=FAKE, obs=FAKE, out=FAKE, status=FAKE,
             ws=FAKE, wsb=1 << 20):
        ks = np.array(ks, np.int32)
        mo = p(np.array(mat_of, np.int32)) if mat_of is not None else None
        return lib.dff_msm_propagate(0, t, n_mat, mo, p(ks), len(ks) if P is None else P, Kmax, w0, M, obs, R, S, out, None, status,
                                     ws, wsb, None)
    refused(lib, call(P=0), "problems must be 1..16384")
    refused(lib, call(ks=[1] * 16385, mat_of=[0] * 16385, Kmax=1), "problems must be 1..16384")
    refused(lib, call(Kmax=0), "states must be 1..1024")
    refused(lib, call(Kmax=1025), "states must be 1..1024")
    for bad in (0, 17):
        refused(lib, call(M=bad), "start vectors must be 1..16")
        refused(lib, call(R=bad), "observables must be 1..16")
    refused(lib, call(S=-1), "steps must be 0..65535")
    refused(lib, call(S=65536), "steps must be 0..65535")
    refused(lib, call(ks=[1] * 16384, mat_of=[0] * 16384, Kmax=1, M=16, R=16, S=65535), "output values, at most 268435456 per call")
    refused(lib, call(n_mat=0), "matrices must be 1..16384")
    for null in ("t", "w0", "obs", "out", "status"):
        refused(lib, call(**{null: None}), "null matrices")
    refused(lib, call(mat_of=None, n_mat=1), "1 matrices for 2 problems and no mat_of")
    refused(lib, call(mat_of=(0, 2)), "problem 1 takes matrix 2 of 2")
    refused(lib, call(mat_of=(-1, 0)), "problem 0 takes matrix -1 of 2")
    refused(lib, call(mat_of=(1, 1)), "problem 1 reads matrix 1 with 3 states, an earlier problem with 4")
    refused(lib, call(ks=(4, 5)), "problem 1 has 5 states, must be 1..Kmax = 4")
    refused(lib, call(ks=(0, 4)), "problem 0 has 0 states")
    refused(lib, call(wsb=15), "workspace of 15 bytes, 16 needed")
    refused(lib, call(ws=None), f"workspace of {1 << 20} bytes, 16 needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    assert lib.dff_debug_msm_propagate_path(3) == 1 and "0 (by size), 1 (LDS) or 2 (workspace)" in lib.dff_last_error().decode()
    L = binding.msm_propagate_lds_limit()
    assert lib.dff_debug_msm_propagate_path(1) == 0
    try:
        refused(lib, call(ks=(4, L + 1), Kmax=L + 1), f"problem 1 has {L + 1} states, the forced LDS path takes at most {L}")
    finally:
        assert lib.dff_debug_msm_propagate_path(0) == 0
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)     # noqa: E731
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensors"):
        binding.msm_propagate(z(2, 4, 4), None, [4, 4], z(2, 1, 4), z(2, 1, 4), 3)


def test_package_reexports():
    for name in ("propagator", "msm_propagate", "msm_relaxation", "msm_autocorrelation", "MsmAutocorrelation", "pcca_memberships",
                 "metastable_sets", "chapman_kolmogorov", "chapman_kolmogorov_of_models", "ChapmanKolmogorov",
                 "ChapmanKolmogorovEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("msm_propagate", "msm_propagate_workspace_bytes", "msm_propagate_lds_limit", "debug_msm_propagate_path"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the Python layer on a stand-in
class HostPropagator:
    calls = 0
    problems = 0

    def __init__(self, device):
        pass

    def __call__(self, t, mat_of, ks, w0, obs, n_steps, want_last=False):
        HostPropagator.calls += 1
        HostPropagator.problems += len(ks)
        return pc.host_propagate(t, mat_of, ks, w0, obs, n_steps, want_last)


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "resampled_counter", boot.Counter)
    monkeypatch.setattr(evaluate, "batched_reversible_sweeper", boot.Sweeper)
    monkeypatch.setattr(evaluate, "spectral_solver", HostSpectral)
    monkeypatch.setattr(evaluate, "propagator", HostPropagator)
    monkeypatch.setattr(binding, "micro_transition_counts",
                        lambda lab, lengths, lags, K: torch.from_numpy(oracle.transition_counts(lab.numpy(), lengths, lags, K)))
    HostPropagator.calls = HostPropagator.problems = 0


def plain_model(T, lag=1, pad=0, scale=1000.0):
    """a reversible=False model whose transition matrix is T (counts T * scale), `pad` unvisited states in front of it"""
    C0 = np.zeros((len(T) + pad, len(T) + pad))
    C0[pad:, pad:] = np.asarray(T) * scale
    return evaluate.MarkovStateModel(lag, reversible=False, device="cpu").fit_counts(C0)


TWO = np.array([[0.9, 0.1], [0.25, 0.75]])
LINE = np.array([[0.9, 0.1, 0.0], [0.2, 0.7, 0.1], [0.0, 0.3, 0.7]])


def test_msm_propagate_drops_inactive_states_and_batches(on_host):
    a, b = plain_model(LINE, lag=2), plain_model(TWO, lag=3, pad=1)
    assert list(b.active_set) == [1, 2]
    start, obs = np.array([[1.0, 0.0, 0.0], [0.2, 0.3, 0.5]]), np.array([[1.0, 2.0, 3.0]])
    out = evaluate.msm_propagate([a, b], start, obs, 4, device="cpu")
    assert out.shape == (2, 5, 2, 1) and HostPropagator.calls == 1 and HostPropagator.problems == 2
    for s in range(5):
        assert np.allclose(out[0, s, :, 0], start @ np.linalg.matrix_power(a.transition_matrix, s) @ obs[0], rtol=1e-14)
        assert np.allclose(out[1, s, :, 0], start[:, 1:] @ np.linalg.matrix_power(b.transition_matrix, s) @ obs[0, 1:], rtol=1e-14)
    assert same_bits(evaluate.msm_propagate(b, start, obs, 4, device="cpu")[0], out[1])
    rel = evaluate.msm_relaxation(a, start[1], obs[0], 4, device="cpu")
    assert rel.shape == (5,) and same_bits(rel, out[0, :, 1, 0])
    assert evaluate.msm_relaxation(a, start[1], np.vstack([obs, obs]), 4, device="cpu").shape == (5, 2)
    for bad, text in (((a, np.ones((1, 2)), obs, 1), "start must be"), ((a, start, np.ones((17, 3)), 1), "observables must be"),
                      ((a, start, obs, -1), "n_steps"), ((a, start, obs, 65536), "n_steps"), ((a, start * np.nan, obs, 1), "finite"),
                      (([], start, obs, 1), "no model"), (([a, plain_model(TWO)], start, obs, 1), "one state index")):
        with pytest.raises(ValueError, match=text):
            evaluate.msm_propagate(*bad, device="cpu")
    with pytest.raises(ValueError, match="not fitted"):
        evaluate.msm_propagate(evaluate.MarkovStateModel(1, device="cpu"), start, obs, 1)


def test_autocorrelation_of_a_two_state_model(on_host):
    m = plain_model(TWO, lag=5)
    ac = evaluate.msm_autocorrelation(m, [3.0, -1.0], 6, device="cpu")
    lam = (1 - TWO[0, 1] - TWO[1, 0]) ** np.arange(7)
    assert list(ac.lags) == [0, 5, 10, 15, 20, 25, 30] and np.allclose(ac.acf, lam, rtol=1e-13)
    pi = m.stationary_distribution
    mean = pi @ [3.0, -1.0]
    assert np.isclose(ac.mean, mean) and np.isclose(ac.cov[0], pi @ (np.array([3.0, -1.0]) - mean) ** 2)
    two = evaluate.msm_autocorrelation(m, [[3.0, -1.0], [0.0, 1.0]], 6, device="cpu")
    assert two.acf.shape == (7, 2) and np.allclose(two.acf, lam[:, None], rtol=1e-13) and same_bits(two.cov[:, 0], ac.cov)


# ---------------------------------------------------------------- metastable sets
def test_inner_simplex_ordering_and_ties():
    psi = np.array([[1.0, 2.0], [1.0, 2.0], [1.0, -1.0], [1.0, 0.5], [1.0, -1.0]])
    assert list(evaluate.inner_simplex(psi)) == [0, 2]               # the lowest index wins both ties
    with pytest.raises(ValueError, match="fewer than"):
        evaluate.inner_simplex(np.ones((4, 2)))


def test_metastable_sets_of_block_models(on_host, monkeypatch):
    for K in (8, 40):
        C4, blocks = pc.four_block_counts(K)
        m = evaluate.MarkovStateModel(1, tol=1e-12, max_iter=100000, steps_per_sync=64, device="cpu").fit_counts(C4)
        sets = evaluate.metastable_sets(m, 4)
        assert all(np.array_equal(s, b) for s, b in zip(sets, blocks)), [s.tolist() for s in sets]
        chi = evaluate.pcca_memberships(m, 4)
        assert chi.shape == (K, 4) and np.abs(chi.sum(axis=1) - 1.0).max() < 1e-9 and chi.min() > -1e-6
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])                        # sets in no order of the states: ordered by their smallest state
    C4, blocks = pc.four_block_counts(8)
    Cp = np.zeros((9, 9))                                            # state 8 is never visited: the sets are on the FULL index
    Cp[np.ix_(perm, perm)] = C4
    m = evaluate.MarkovStateModel(1, tol=1e-12, max_iter=100000, steps_per_sync=64, device="cpu").fit_counts(Cp)
    sets = evaluate.metastable_sets(m, 4)
    want = sorted((np.sort(perm[b]) for b in blocks), key=lambda s: s[0])
    assert [s.tolist() for s in sets] == [s.tolist() for s in want] and [int(s[0]) for s in sets] == sorted(int(s[0]) for s in sets)
    assert [s.tolist() for s in evaluate.metastable_sets(m, 1)] == [list(range(8))]
    for bad in (0, 9, 17):
        with pytest.raises(ValueError, match="m must be 1.."):
            evaluate.pcca_memberships(m, bad)
    # a vertex has membership 1 in its own set, so a set of the inner simplex keeps at least that state; the refusal guards the rule
    monkeypatch.setattr(evaluate, "pcca_memberships", lambda model, m: np.array([[0.6, 0.4, 0.0]] * 5 + [[0.5, 0.5, 0.0]] * 3))
    with pytest.raises(ValueError, match="only 1 of 3 sets have a state"):     # 0.5 / 0.5: the lowest index wins the tie
        evaluate.metastable_sets(m, 3)


# ---------------------------------------------------------------- the Chapman-Kolmogorov test
def test_chapman_kolmogorov_definitions_by_hand(on_host):
    base, two = plain_model(LINE, lag=1), plain_model(LINE @ LINE, lag=2)
    sets = [np.array([0]), np.array([1, 2])]
    pred, est = evaluate.chapman_kolmogorov_of_models([(base, {1: base, 2: two})], [1, 2], sets, device="cpu")
    assert HostPropagator.calls == 1 and HostPropagator.problems == 3 and pred.shape == est.shape == (1, 2, 2, 2)
    pi = base.stationary_distribution
    w = np.array([[1.0, 0.0, 0.0], [0.0, pi[1], pi[2]] / (pi[1] + pi[2])])
    ind = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 1.0]])
    for i, k in enumerate((1, 2)):
        assert np.allclose(pred[0, i], w @ np.linalg.matrix_power(LINE, k) @ ind.T, rtol=1e-13)
    assert same_bits(pred[0, 0], est[0, 0])                          # k = 1: the same model
    assert np.allclose(pred[0, 1], est[0, 1], atol=1e-12)            # T(2 tau) = T(tau)^2 here: the test holds
    # differing active sets: the model at 2 tau lacks state 0 (pad), so set 0 has no active state there: its row is NaN
    small = plain_model(TWO, lag=2, pad=1)
    pred, est = evaluate.chapman_kolmogorov_of_models([(base, {2: small})], [2], sets, device="cpu")
    assert np.isfinite(pred).all() and np.isnan(est[0, 0, 0]).all() and est[0, 0, 1, 0] == 0.0 and np.isclose(est[0, 0, 1, 1], 1.0)


def test_chapman_kolmogorov_from_labels_and_its_refusals(on_host):
    labels, lengths, _ = five_state_case()
    kw = dict(traj_lengths=lengths, n_states=5, tol=1e-12, max_iter=100000, steps_per_sync=16, device="cpu")
    sets = [[0, 1], [3, 4]]
    ck = evaluate.chapman_kolmogorov(labels, 1, sets, (1, 2, 3), **kw)
    assert HostPropagator.calls == 1 and HostPropagator.problems == 4
    assert list(ck.lagtimes) == [1, 2, 3] and ck.predicted.shape == (3, 2, 2) and same_bits(ck.predicted[0], ck.estimated[0])
    assert sorted(ck.models) == [1, 2, 3] and ck.models[3].lagtime == 3 and ck.predicted_lo is None and np.isnan(ck.share_inside)
    d = (ck.predicted - ck.estimated)[np.isfinite(ck.predicted - ck.estimated)]
    assert ck.max_abs_diff == np.abs(d).max() and np.isclose(ck.rms_diff, np.sqrt(np.mean(d * d)))
    nr = evaluate.chapman_kolmogorov(labels, 1, sets, (2,), reversible=False, **kw)
    assert nr.predicted.shape == (1, 2, 2) and not nr.models[1].reversible
    for bad, text in (([[0, 1], [1, 2]], "overlap"), ([[0], []], "set 1 is empty"), ([[0], [5]], "outside 0 .. 4"), ([], "sets"),
                      ([[i] for i in range(5)] * 4, "sets")):
        with pytest.raises(ValueError, match=text):
            evaluate.chapman_kolmogorov(labels, 1, bad, (1, 2), **kw)
    for bad in ((), (0, 1), (1, 1), (1.5,)):
        with pytest.raises(ValueError, match="multiples"):
            evaluate.chapman_kolmogorov(labels, 1, sets, bad, **kw)
    with pytest.raises(ValueError, match="reversible"):
        evaluate.chapman_kolmogorov(labels, 1, sets, (1, 2), reversible=False, n_resamples=3, **kw)


def test_chapman_kolmogorov_bootstrap_and_share_inside(on_host):
    labels, lengths, _ = five_state_case()
    kw = dict(traj_lengths=lengths, n_states=5, tol=1e-12, max_iter=100000, steps_per_sync=16, device="cpu")
    sets, mult = [[0, 1], [3, 4]], (2, 3)
    ck = evaluate.chapman_kolmogorov(labels, 1, sets, mult, n_resamples=6, seed=2, resample_batch=4, **kw)
    assert HostPropagator.calls == 1 + 2                             # the point estimate, then one call per batch of resamples
    assert ck.predicted_resamples.shape == ck.estimated_resamples.shape == (6, 2, 2, 2)
    w = evaluate.bootstrap_weights(len(lengths), 6, 2)
    for b in range(6):
        models = {k: evaluate.MarkovStateModel(k, tol=1e-12, max_iter=100000, steps_per_sync=16, device="cpu")
                  .fit_counts(boot.weighted_counts(labels, lengths, lengths, k, 5, w[b:b + 1])[0]) for k in (1, 2, 3)}
        pred, est = evaluate.chapman_kolmogorov_of_models([(models[1], models)], mult, sets, device="cpu")
        assert same_bits(pred[0], ck.predicted_resamples[b]) and same_bits(est[0], ck.estimated_resamples[b]), b
    lo, hi = evaluate.percentile_interval(ck.estimated_resamples.reshape(6, -1), 0.95)
    assert same_bits(lo.reshape(2, 2, 2), ck.estimated_lo) and same_bits(hi.reshape(2, 2, 2), ck.estimated_hi)
    assert ck.share_inside == evaluate.share_inside(ck.predicted, ck.estimated_lo, ck.estimated_hi)
    point = np.array([0.5, 2.0, np.nan, 1.0])
    assert evaluate.share_inside(point, np.array([0.0, 0.0, 0.0, np.nan]), np.array([1.0, 1.0, 1.0, 2.0])) == 0.5
    assert np.isnan(evaluate.share_inside(point[2:3], np.zeros(1), np.ones(1)))


# ---------------------------------------------------------------- the evaluator
def test_the_evaluator_checks_its_arguments_and_fills_its_keys(on_host, monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.ChapmanKolmogorovEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None: {"labels": proj[:, 0].round().to(torch.int32)})

    def measured(series, max_lag, traj_lengths=None, **kw):         # autocorrelation() needs the GPU: the oracle's shape on numpy
        x = np.asarray(series, np.float64)
        x = x - x.mean()
        acf = np.array([np.mean(x[:len(x) - l] * x[l:]) for l in range(max_lag + 1)]) / np.mean(x * x)
        return evaluate.Autocorrelation(acf[:, None], acf[:, None], np.full(max_lag + 1, len(x)), np.zeros(1), np.ones(1), "per_lag")
    monkeypatch.setattr(evaluate, "autocorrelation", measured)

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        args = dict(n_microstates=5, lagtime=2, n_sets=2, multiples=(1, 2), frame_time=0.5, centers=np.arange(5.0).reshape(5, 1),
                    device="cpu")
        args.update(kw)
        return evaluate.ChapmanKolmogorovEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), **args)
    labels, lengths, _ = five_state_case()
    frames = np.where(labels < 0, 0, labels).astype(np.float64).reshape(-1, 1, 1)
    e = make()
    res = e.eval(frames, lengths)
    assert set(res) == set(evaluate.ChapmanKolmogorovEvaluator.KEYS)
    assert res["n_sets"] == 2.0 and len(e.sets) == 2 and np.array(res["ck_diagonal_predicted"]).shape == (2, 2)
    assert res["ck_diagonal_predicted"][0] == res["ck_diagonal_estimated"][0] and np.isfinite(res["acf_rms_diff"])
    assert res["ck_max_abs_diff"] == e.results["samples"].max_abs_diff
    with_ref = make(ref_data=frames, ref_traj_lengths=lengths, n_bootstrap=4).eval(frames, lengths)
    keys = set(evaluate.ChapmanKolmogorovEvaluator.KEYS) | {"ck_share_inside"}
    assert set(with_ref) == keys | {k + "_ref" for k in keys} | {"ck_max_abs_diff_minus_ref"}
    assert with_ref["ck_max_abs_diff_minus_ref"] == 0.0 and 0.0 <= with_ref["ck_share_inside"] <= 1.0
    for bad, text in ((dict(lagtime=None), "lagtime"), (dict(n_sets=0), "n_sets"), (dict(n_sets=17), "n_sets"),
                      (dict(multiples=()), "multiples"), (dict(multiples=(1, 1)), "multiples"), (dict(n_microstates=0), "n_microstates"),
                      (dict(n_bootstrap=-1), "n_bootstrap"), (dict(frame_time=0.0), "frame_time")):
        with pytest.raises(ValueError, match=text):
            make(**bad)


# ---------------------------------------------------------------- the tool
def test_ck_arguments_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    full = base + ["--parallel-sim", "4", "--ck", "--ck-states", "9", "--ck-lag", "2"]
    assert tool.ck_arguments(ap.parse_args(base)) is None
    assert tool.ck_arguments(ap.parse_args(full)) == (9, 2, 3, [1, 2, 3, 4, 5], 0)
    a = ap.parse_args(full + ["--ck-sets", "4", "--ck-multiples", "1,2,8", "--ck-bootstrap", "50"])
    assert tool.ck_arguments(a) == (9, 2, 4, [1, 2, 8], 50)
    assert ap.parse_args(base + ["--parallel-sim", "4", "--ck", "held.pt", "--ck-states", "9", "--ck-lag", "2"]).ck == "held.pt"
    for alone in (["--ck-states", "9"], ["--ck-lag", "2"], ["--ck-sets", "3"], ["--ck-multiples", "1,2"], ["--ck-bootstrap", "5"]):
        with pytest.raises(SystemExit, match="need --ck"):
            tool.ck_arguments(ap.parse_args(base + alone))
    with pytest.raises(SystemExit, match="--ck needs --parallel-sim"):
        tool.ck_arguments(ap.parse_args(base + ["--ck", "--ck-states", "9", "--ck-lag", "2"]))
    with pytest.raises(SystemExit, match="--ck needs --ck-states K and --ck-lag L"):
        tool.ck_arguments(ap.parse_args(base + ["--parallel-sim", "4", "--ck", "--ck-states", "9"]))
    for bad in (["--ck-sets", "0"], ["--ck-sets", "17"], ["--ck-multiples", "0,1"], ["--ck-multiples", "1,1"], ["--ck-multiples", "x"],
                ["--ck-bootstrap", "0"], ["--ck-states", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(full + bad)
