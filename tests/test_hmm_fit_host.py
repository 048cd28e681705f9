"""Host side of Baum-Welch on the device: the symbols and refusals of dff_hmm_fit_steps (on the host, before any device call),
the numpy statement of its M-step (tests/hmm_fit_cases.py) against HiddenMarkovModel._m_step's formulas, and the Python layer
-- HiddenMarkovModel(m_step="device"), resampled_labels, bootstrap_hmm, HmmEvaluator(n_bootstrap=...) -- on a stand-in behind
evaluate.hmm_fit_solver: hmm_fit_cases.replay over hmm_cases.host_estep.  No GPU.

M-step agreement.  mstep() adds in index order and sweeps the reversible estimator to the first err < tol; _m_step's formulas
are numpy's pairwise sums and reversible_transition_matrix on a vectorised numpy sweep to the same tol.  The two differ by
rounding and by at most one sweep.  MEASURED on the CPU over the cases below, the largest difference of A, B, p0, pi relative
to the array's largest magnitude: 1.14e-15 (pi; B 1.11e-15, A 3.9e-16, p0 2.8e-16).  The bar is 10 x that, 1.14e-14, and by
the rule of the issue must stay <= 1e-9."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import hmm_cases as hc
import hmm_fit_cases as fc
from dff_amd import binding, evaluate
from standins import HostEstep, OracleSweeps
from support import hmm_chunk, owning_unit, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used
MSTEP_MEASURED = 1.14e-15
MSTEP_BAR = 10 * MSTEP_MEASURED


# ---------------------------------------------------------------- symbols and refusals
def test_header_library_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in ("dff_hmm_fit_workspace_bytes", "dff_hmm_fit_steps"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in binding.SYMBOLS and getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_hmm_fit_steps"][1]) == 22 and len(binding.SYMBOLS["dff_hmm_fit_workspace_bytes"][1]) == 6
    struct = re.search(r"typedef struct \{([^{}]*)\} dff_hmm_fit_state;", header).group(1)
    fields = re.findall(r"(int32_t|double|long long)\s+(\w+);", struct)
    assert fields == [("int32_t", "n_estep"), ("int32_t", "stop"), ("int32_t", "estep_status"), ("int32_t", "flags"),
                      ("double", "last_loglik"), ("long long", "rev_sweeps")]
    assert binding.HMM_FIT_STATE.itemsize == 32 and list(binding.HMM_FIT_STATE.names) == [f for _, f in fields]
    text = owning_unit("dff_hmm_mstep.hip")
    assert '#include "dff_hmm_mstep.hip"' in text
    rec = np.zeros(1, binding.HMM_FIT_STATE)
    rec["n_estep"], rec["stop"], rec["flags"], rec["last_loglik"], rec["rev_sweeps"] = 7, 1, 3, -2.5, 1 << 40
    assert binding.hmm_fit_state_dict(rec.view(np.int32)) == {"n_estep": 7, "stop": 1, "estep_status": 0, "flags": 3, "last_loglik": -2.5,
                                                               "rev_sweeps": 1 << 40}


def test_refusals_before_any_device_call():
    lib = binding.load_library()
    L = np.array([3 * hmm_chunk() + 5, 0, 7], np.int64)
    n = int(L.sum())
    for lag, m, K in ((1, 1, 1), (3, 3, 5), (7, 8, 1024)):
        nstats = 1 + m * m + m + m * K
        assert binding.hmm_fit_workspace_bytes(n, L, lag, m, K) == binding.hmm_workspace_bytes(n, L, lag, m, K) + (8 * nstats + 15) // 16 * 16 + 16
    for bad, text in (((n, L, 1, 0, 4), "hidden states must be 1..8"), ((n, L, 1, 2, 1025), "symbols must be 1..1024"),
                      ((n, L, 0, 2, 4), "lag must be >= 1"), ((n + 1, L, 1, 2, 4), "trajectory lengths sum to")):
        with pytest.raises(ValueError, match=re.escape(text)):
            binding.hmm_fit_workspace_bytes(*bad)

    def call(n=n, lengths=L, lag=1, m=2, K=4, labels=FAKE, trans=FAKE, emit=FAKE, init=FAKE, reversible=1, n_steps=2, accuracy=1e-3,
             rev_tol=1e-12, rev_max=10, loglik=FAKE, state=FAKE, ws=FAKE, wsb=1 << 30):
        lengths = np.asarray(lengths, np.int64)
        return lib.dff_hmm_fit_steps(0, labels, n, p(lengths), len(lengths), lag, trans, emit, init, m, K, reversible, n_steps, accuracy,
                                     rev_tol, rev_max, loglik, None, state, ws, wsb, None)
    refused(lib, call(m=0), "hidden states must be 1..8")
    refused(lib, call(m=9), "hidden states must be 1..8")
    refused(lib, call(K=0), "symbols must be 1..1024")
    refused(lib, call(lag=0), "lag must be >= 1")
    refused(lib, call(n=n + 1), "trajectory lengths sum to")
    refused(lib, call(lengths=[n + 1, -1]), "trajectory 1 has negative length")
    refused(lib, call(labels=None), "null labels")
    for null in ("trans", "emit", "init", "loglik", "state"):
        refused(lib, call(**{null: None}), "null transition matrix")
    refused(lib, call(reversible=2), "reversible must be 0 or 1")
    refused(lib, call(n_steps=0), "n_steps must be >= 1")
    for bad in (0.0, -1.0, float("nan")):
        refused(lib, call(accuracy=bad), "accuracy must be > 0")
        refused(lib, call(rev_tol=bad), "rev_tol must be > 0")
    refused(lib, call(rev_max=0), "rev_max_sweeps must be >= 1")
    refused(lib, call(state=C.c_void_p(4100)), "state must be 8-byte aligned")
    want = binding.hmm_fit_workspace_bytes(n, L, 1, 2, 4)
    refused(lib, call(wsb=want - 1), f"workspace of {want - 1} bytes, {want} needed")
    refused(lib, call(ws=None), f"{want} needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    binding.debug_hmm_stages(3)
    try:
        refused(lib, call(), "dff_debug_hmm_stages is set")
    finally:
        binding.debug_hmm_stages(0)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)     # noqa: E731
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensors"):
        binding.hmm_fit_steps(torch.zeros(4, dtype=torch.int32), [4], 1, z(2, 2), z(2, 3), z(2), True, 2, 1e-3)


def test_package_reexports():
    for name in ("hmm_fit_solver", "resampled_labels", "bootstrap_hmm", "HmmBootstrap"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("hmm_fit_steps", "hmm_fit_workspace_bytes", "hmm_fit_state_dict"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the M-step's statement against _m_step's formulas
def numpy_sweeps(S, c, tol, max_sweeps):
    """the vectorised numpy sweep (numpy's own sums) to the first err < tol"""
    x = 0.5 * S.sum(axis=1)
    for _ in range(max_sweeps):
        q = c / x
        xn = np.divide(S, q[:, None] + q[None, :], out=np.zeros_like(S), where=S != 0).sum(axis=1)
        err = np.max(np.abs(xn - x) / x)
        x = xn
        if err < tol:
            break
    return x


def formulas(stats, A, B, p0, m, K, reversible, tol):
    """HiddenMarkovModel._m_step's expressions, with the reversible estimator as reversible_transition_matrix on numpy_sweeps"""
    xi, g0, gs = stats[1:1 + m * m].reshape(m, m), stats[1 + m * m:1 + m * m + m], stats[1 + m * m + m:].reshape(m, K)
    occ = gs.sum(axis=1)
    Bn = np.where(occ[:, None] > 0, gs / np.where(occ > 0, occ, 1.0)[:, None], B)
    pn = g0 / g0.sum() if g0.sum() > 0 else p0
    if reversible:
        if m == 1:
            return np.ones((1, 1)), Bn, pn, np.ones(1)
        S, c = xi + xi.T, xi.sum(axis=1)
        T, pi = evaluate.reversible_transition_matrix(S, c, numpy_sweeps(S, c, tol, 1_000_000))
        return T, Bn, pn, pi
    rows = xi.sum(axis=1)
    return np.where(rows[:, None] > 0, xi / np.where(rows > 0, rows, 1.0)[:, None], A), Bn, pn, None


MSTEP_CASES = ((1, 1, 1), (2, 5, 1), (3, 5, 3), (4, 64, 1), (5, 1024, 3), (8, 1024, 7), (8, 5, 1))


def test_the_statement_agrees_with_the_host_m_steps_formulas():
    worst = {}
    for m, K, lag in MSTEP_CASES:
        labels, lengths, A, B, p0 = hc.case_inputs(m, K, lag, False, hmm_chunk())
        lengths = [v for v in lengths if v <= lag * (2 * hmm_chunk() + 1) + 1]              # the chain of 20 chunks adds nothing here
        labels = labels[:sum(lengths)]
        stats = hc.host_estep(labels, lengths, lag, A, B, p0, hmm_chunk())[0]
        assert not np.isnan(stats).any()
        for reversible in (False, True):
            got = fc.mstep(stats, A, B, p0, m, K, reversible, 1e-12, 1_000_000)
            want = formulas(stats, A, B, p0, m, K, reversible, 1e-12)
            assert not got["lost"] and got["flags"] == 0
            for name, a, b in (("A", got["A"], want[0]), ("B", got["B"], want[1]), ("p0", got["p0"], want[2]), ("pi", got["pi"], want[3])):
                if b is None:
                    assert a is None
                    continue
                d = float(np.abs(a - b).max() / np.abs(b).max())
                worst[(name, reversible)] = max(worst.get((name, reversible), 0.0), d)
            if reversible and m > 1:
                assert np.allclose(got["A"].sum(axis=1), 1.0, atol=1e-9) and np.allclose(got["pi"] @ got["A"], got["pi"], atol=1e-9)
                assert 1 <= got["sweeps"] < 5000
    print("[hmm-fit] mstep against the host formulas, largest relative difference:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert MSTEP_BAR <= 1e-9
    assert max(worst.values()) <= MSTEP_BAR, worst


def test_kept_rows_lost_states_and_the_sweep_cap_in_the_statement():
    m, K = 2, 4
    stats = np.concatenate([[-10.0], [3.0, 0.0, 0.0, 0.0], [1.0, 0.0], [2.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    A, B, p0 = np.array([[0.5, 0.5], [0.25, 0.75]]), np.array([[0.5, 0.5, 0, 0], [0, 0, 0.5, 0.5]]), np.array([0.5, 0.5])
    got = fc.mstep(stats, A, B, p0, m, K, False)
    assert got["flags"] == 1 and np.array_equal(got["A"][1], A[1]) and np.array_equal(got["B"][1], B[1]) and np.array_equal(got["A"][0], [1.0, 0.0])
    lost = fc.mstep(stats, A, B, p0, m, K, True)
    assert lost["lost"] and lost["flags"] == 1 and all(np.array_equal(lost[k], v) for k, v in (("A", A), ("B", B), ("p0", p0)))
    xi = np.array([[50.0, 5.0, 1.0], [2.0, 40.0, 4.0], [3.0, 1.0, 30.0]])
    stats = np.concatenate([[-1.0], xi.ravel(), [1.0, 1.0, 1.0], np.ones(6)])
    capped = fc.mstep(stats, np.eye(3), np.full((3, 2), 0.5), np.ones(3) / 3, 3, 2, True, 1e-12, 3)
    free = fc.mstep(stats, np.eye(3), np.full((3, 2), 0.5), np.ones(3) / 3, 3, 2, True, 1e-12, 1_000_000)
    assert capped["sweeps"] == 3 and capped["flags"] == 2 and free["flags"] == 0 and free["sweeps"] > 3
    assert not fc.strongly_connected(np.array([[1.0, 1.0, 0], [0, 1.0, 1.0], [0, 0, 1.0]])) and fc.strongly_connected(np.array([[0, 1.0, 0], [0, 0, 1.0], [1.0, 0, 0]]))


# ---------------------------------------------------------------- the Python layer on the stand-in
@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    Cn, seen = hmm_chunk(), {}

    def estep(labels, lengths, lag, A, B, p0):
        """hc.host_estep, each distinct input computed once: fits that differ in steps_per_sync alone repeat their E-steps"""
        key = (np.asarray(labels).tobytes(), tuple(lengths), lag, A.tobytes(), B.tobytes(), p0.tobytes())
        if key not in seen:
            seen[key] = hc.host_estep(labels, lengths, lag, A, B, p0, Cn)
        return seen[key]
    monkeypatch.setattr(fc.ReplaySolver, "host_estep", staticmethod(estep))
    monkeypatch.setattr(evaluate, "hmm_fit_solver", fc.ReplaySolver)
    monkeypatch.setattr(evaluate, "hmm_estep_solver", HostEstep)


def em_case():
    A, B, p0 = hc.model(2, 6, seed=3)
    lengths = [150, 90, 0, 160]
    return hc.simulate(A, B, p0 / p0.sum(), lengths, seed=5), lengths


def start_of():
    return (np.array([[0.7, 0.3], [0.4, 0.6]]), np.array([[3.0, 2, 1, 1, 1, 1], [1, 1, 1, 1, 2, 3.0]]) / 9.0, np.array([0.5, 0.5]))


def device_fit(labels, lengths, **kw):
    args = dict(reversible=True, accuracy=1e-3, max_iter=200, device="cpu", m_step="device")
    initial = kw.pop("initial", start_of())
    renumber = kw.pop("renumber", True)
    args.update(kw)
    return evaluate.HiddenMarkovModel(2, 1, **args).fit(labels, lengths, 6, initial=initial, renumber=renumber)


def test_the_device_loop_does_not_depend_on_steps_per_sync(on_host):
    labels, lengths = em_case()
    for reversible in (True, False):
        for max_iter in (200, 10):                                  # 10: no multiple of 7 or 32, and not converged
            fits = [device_fit(labels, lengths, reversible=reversible, max_iter=max_iter, steps_per_sync=s) for s in (1, 7, 32)]
            a = fits[0]
            assert a.converged == (max_iter == 200) and a.n_iter == len(a.log_likelihoods) <= max_iter and a.message == ""
            assert (max_iter == 200) or a.n_iter == 10
            for b in fits[1:]:
                assert (b.n_iter, b.converged, b.message, b.log_likelihoods, b.rev_sweeps) == (a.n_iter, a.converged, a.message, a.log_likelihoods, a.rev_sweeps)
                for name in ("transition_matrix", "observation_probabilities", "initial_distribution", "stationary_distribution"):
                    assert np.array_equal(getattr(a, name), getattr(b, name)), name
            assert (a.rev_sweeps > 0) == reversible and not a.rev_unconverged and not a.degenerate
        # the host path's loop stops at the same E-step, on parameters that differ by the M-steps' rounding only
        host = evaluate.HiddenMarkovModel(2, 1, reversible=reversible, accuracy=1e-3, max_iter=200, device="cpu")
        host.fit(labels, lengths, 6, initial=start_of())
        d = device_fit(labels, lengths, reversible=reversible)
        assert d.n_iter == host.n_iter and d.converged and np.allclose(d.transition_matrix, host.transition_matrix, rtol=1e-9)
        assert np.allclose(d.log_likelihoods, host.log_likelihoods, rtol=1e-12)
        assert np.allclose(d.stationary_distribution, host.stationary_distribution, rtol=1e-9)


def test_failures_messages_flags_and_the_order_of_the_states(on_host):
    labels, lengths = em_case()
    a0, b0 = np.array([[1.0, 0.0], [0.5, 0.5]]), start_of()[1]
    g = device_fit(labels, lengths, reversible=False, max_iter=4, initial=(a0, b0, np.array([1.0, 0.0])))
    assert g.degenerate and np.array_equal(g.observation_probabilities[1], b0[1]) and np.array_equal(g.transition_matrix[1], a0[1])
    r = device_fit(labels, lengths, max_iter=40, steps_per_sync=7, initial=(a0, b0, np.array([1.0, 0.0])))
    assert not r.converged and r.message == evaluate.HiddenMarkovModel.LOST and "lost a hidden state" in r.message and r.n_iter == 1
    assert len(r.log_likelihoods) == 1 and r.degenerate
    bad = evaluate.HiddenMarkovModel(2, 1, reversible=False, device="cpu", m_step="device")
    bad.fit(np.array([0, 1, 0], np.int32), None, 2, initial=(np.eye(2), np.eye(2), np.array([0.5, 0.5])))
    assert not bad.converged and "likelihood zero" in bad.message and bad.log_likelihoods == [] and bad.n_iter == 1
    capped = device_fit(labels, lengths, max_iter=3, rev_max_sweeps=2)
    assert capped.rev_unconverged and capped.rev_sweeps == 6
    # renumber=False keeps the order of the initial parameters; the default sorts by population
    a, b, q = start_of()
    swapped = (a[::-1, ::-1].copy(), b[::-1].copy(), q[::-1].copy())
    kept, kept_swapped = device_fit(labels, lengths, renumber=False), device_fit(labels, lengths, renumber=False, initial=swapped)
    assert np.allclose(kept.stationary_distribution, kept_swapped.stationary_distribution[::-1], rtol=1e-9)
    assert np.allclose(kept.observation_probabilities, kept_swapped.observation_probabilities[::-1], rtol=1e-9, atol=1e-15)
    pops = (kept.stationary_distribution, kept_swapped.stationary_distribution)
    assert min(p_[0] - p_[1] for p_ in pops) < 0 < max(p_[0] - p_[1] for p_ in pops)         # one of the two is NOT sorted
    sorted_ = device_fit(labels, lengths, initial=swapped)
    assert sorted_.stationary_distribution[0] >= sorted_.stationary_distribution[1]
    for kw, text in ((dict(m_step="gpu"), "m_step"), (dict(steps_per_sync=0), "steps_per_sync"), (dict(rev_tol=0.0), "rev_tol"),
                     (dict(rev_max_sweeps=0), "rev_max_sweeps")):
        with pytest.raises(ValueError, match=text):
            evaluate.HiddenMarkovModel(2, 1, device="cpu", **kw)


def test_resampled_labels_on_the_host():
    labels = torch.arange(10, dtype=torch.int32)
    units = [3, 0, 4, 2, 1]
    lab, lengths = evaluate.resampled_labels(labels, units, [2, 3, 0, 1, 2])
    assert lab.dtype == torch.int32 and lab.tolist() == [0, 1, 2, 0, 1, 2, 7, 8, 9, 9]       # unit-major, copies adjacent
    assert lengths.tolist() == [3, 3, 0, 0, 0, 2, 1, 1] and lengths.dtype == np.int64        # an empty unit: empty trajectories
    same, ln = evaluate.resampled_labels(labels, units, np.ones(5, np.uint32))
    assert same.tolist() == labels.tolist() and ln.tolist() == units
    none, ln = evaluate.resampled_labels(labels, units, np.zeros(5, np.uint32))
    assert none.numel() == 0 and ln.size == 0
    for bad in (([3, 3], [1, 1]), (units, [1, 1]), (units, [1, 1, 1, 1, -1])):
        with pytest.raises(ValueError, match="resampled_labels"):
            evaluate.resampled_labels(labels, *bad)


def test_bootstrap_hmm_through_the_stand_in(on_host, monkeypatch):
    labels, lengths = em_case()
    point = device_fit(labels, lengths)
    start = (point.transition_matrix, point.observation_probabilities, point.initial_distribution)
    kw = dict(reversible=True, accuracy=1e-3, max_iter=200, device="cpu")
    w = np.array([[1, 1, 1, 1], [2, 0, 0, 2], [0, 3, 1, 0]])
    bs = evaluate.bootstrap_hmm(labels, 1, 2, lengths, 6, weights=w, point=point, **kw)
    assert bs.point is point and bs.weights.dtype == np.uint32 and bs.unit_lengths.tolist() == lengths and bs.n_failed == 0
    assert bs.timescales.shape == (3, 1) and bs.lifetimes.shape == bs.stationary.shape == (3, 2) and bs.transition_matrices.shape == (3, 2, 2)
    warm = device_fit(labels, lengths, initial=start, renumber=False)          # all ones: the warm-started fit of the original labels
    assert np.array_equal(bs.transition_matrices[0], warm.transition_matrix) and np.array_equal(bs.stationary[0], warm.stationary_distribution)
    assert bs.n_iter[0] == warm.n_iter and bs.converged[0] and bs.log_likelihood[0] == warm.log_likelihoods[-1]
    assert np.array_equal(bs.timescales[0], warm.timescales()) and np.array_equal(bs.lifetimes[0], warm.lifetimes())
    for b in (1, 2):
        lab_b, len_b = evaluate.resampled_labels(torch.from_numpy(labels), lengths, w[b])
        own = device_fit(lab_b, len_b, initial=start, renumber=False)
        assert np.array_equal(bs.transition_matrices[b], own.transition_matrix) and bs.n_iter[b] == own.n_iter
    assert bs.std().shape == (1,) and bs.std("lifetimes").shape == (2,) and np.isfinite(bs.std("stationary")).all()
    lo, hi = bs.interval("timescales", 0.9)
    assert lo[0] <= hi[0]
    with pytest.raises(ValueError, match="name must be"):
        bs.std("n_iter")
    # the default point and the seeded draws
    monkeypatch.setattr(evaluate, "initial_hmm", lambda *a, **k: start_of())
    auto = evaluate.bootstrap_hmm(labels, 1, 2, lengths, 6, n_resamples=2, seed=4, max_iter=20, device="cpu")
    assert auto.point.m_step == "device" and np.array_equal(auto.weights, evaluate.bootstrap_weights(4, 2, 4))
    # a failed resample: NaN rows, counted
    real = evaluate.resampled_labels

    def broken(lab, units, row):
        out, ln = real(lab, units, row)
        if int(row[0]) == 2:
            out = out.clone()
            out[0] = 6                                              # a label >= K: the E-step fails with status 3
        return out, ln
    monkeypatch.setattr(evaluate, "resampled_labels", broken)
    bs = evaluate.bootstrap_hmm(labels, 1, 2, lengths, 6, weights=w, point=point, **kw)
    assert bs.n_failed == 1 and bs.failed.tolist() == [False, True, False] and not bs.converged[1] and bs.n_iter[1] == 1
    for name in ("timescales", "lifetimes", "stationary", "transition_matrices", "log_likelihood"):
        v = getattr(bs, name)
        assert np.isnan(v[1]).all() and np.isfinite(v[[0, 2]]).all(), name
    assert np.isfinite(bs.std("lifetimes")).all()
    for bf in (1, 3):
        with pytest.raises(ValueError, match="block_frames must be at least 2 lagtime"):
            evaluate.bootstrap_hmm(labels, 2, 2, lengths, 6, block_frames=bf, point=point, **kw)
    blocks = evaluate.bootstrap_hmm(labels, 1, 2, lengths, 6, n_resamples=2, block_frames=50, point=point, **kw)
    assert blocks.unit_lengths.tolist() == [50, 50, 50, 50, 40, 50, 50, 50, 10] and blocks.weights.shape == (2, 9)
    with pytest.raises(ValueError, match="weights must be"):
        evaluate.bootstrap_hmm(labels, 1, 2, lengths, 6, weights=np.ones((2, 3)), point=point, **kw)


def test_the_evaluator_without_bootstrap_is_unchanged_and_with_it_adds_its_keys(on_host, monkeypatch):
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.HmmEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None: {"labels": proj[:, 0].round().to(torch.int32)})
    monkeypatch.setattr(evaluate, "label_runs", lambda labels, traj_lengths=None, device=None: {"labels": np.zeros(0, np.int64)})
    monkeypatch.setattr(evaluate, "dwell_summary", lambda runs, step: {})
    monkeypatch.setattr(evaluate, "initial_hmm", lambda *a, **k: start_of())

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        args = dict(n_microstates=6, n_hidden=2, lagtime=1, frame_time=0.5, centers=np.arange(6.0).reshape(6, 1), max_iter=30, device="cpu")
        args.update(kw)
        return evaluate.HmmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), **args)
    labels, lengths = em_case()
    frames = labels.astype(np.float64).reshape(-1, 1, 1)
    plain = make().eval(frames, lengths)
    assert list(plain) == list(evaluate.HmmEvaluator.KEYS)                     # today's keys, in today's order
    zero = make(n_bootstrap=0, block_frames=None, bootstrap_seed=3)
    assert zero.eval(frames, lengths) == plain and zero.bootstrap == {}
    e = make(n_bootstrap=4, bootstrap_seed=1, ref_data=frames, ref_traj_lengths=lengths)
    res = e.eval(frames, lengths)
    keys = set(evaluate.HmmEvaluator.KEYS) | set(evaluate.HmmEvaluator.BOOTSTRAP_KEYS)
    assert set(res) == keys | {k + "_ref" for k in keys} | {"log10_timescale_ratio", "log10_lifetime_ratio", "population_js"}
    assert {k: res[k] for k in plain} == plain
    bs = e.bootstrap["samples"]
    assert bs.point is e.models["samples"] and bs.weights.shape == (4, 4) and set(e.bootstrap) == {"samples", "refs"}
    assert res["timescales_std"] == [float(v) * 0.5 for v in bs.std("timescales")] and res["bootstrap_failed"] == float(bs.n_failed)
    assert res["hidden_populations_std"] == [float(v) for v in bs.std("stationary")] and len(res["lifetimes_std"]) == 2
    assert res["timescales_lo"][0] <= res["timescales_hi"][0] and res["timescales_std_ref"] == res["timescales_std"]
    for bad, text in ((dict(n_bootstrap=-1), "n_bootstrap"), (dict(n_bootstrap=2, block_frames=1), "block_frames")):
        with pytest.raises(ValueError, match=text):
            make(**bad)


def test_the_tool_refuses_the_bootstrap_options_without_hmm():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    full = base + ["--parallel-sim", "4", "--hmm", "--hmm-states", "50", "--hmm-hidden", "3", "--hmm-lag", "5"]
    for alone in (["--hmm-bootstrap", "10"], ["--hmm-block-frames", "40"], ["--hmm-bootstrap-seed", "2"]):
        with pytest.raises(SystemExit, match="need --hmm"):
            tool.hmm_arguments(ap.parse_args(base + alone))
    for alone in (["--hmm-block-frames", "40"], ["--hmm-bootstrap-seed", "2"]):
        with pytest.raises(SystemExit, match="need --hmm-bootstrap"):
            tool.hmm_arguments(ap.parse_args(full + alone))
    a = ap.parse_args(full + ["--hmm-bootstrap", "10", "--hmm-block-frames", "40", "--hmm-bootstrap-seed", "2"])
    assert tool.hmm_arguments(a) == (50, 3, 5) and (a.hmm_bootstrap, a.hmm_block_frames, a.hmm_bootstrap_seed) == (10, 40, 2)
    assert tool.hmm_arguments(ap.parse_args(full)) == (50, 3, 5) and ap.parse_args(full).hmm_bootstrap is None
    for bad in (["--hmm-bootstrap", "0"], ["--hmm-block-frames", "1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(full + bad)


def test_the_benchmark_lists_its_cases():
    import tools_bench_hmm_fit as bench
    assert bench.STEPS_PER_SYNC == (1, 8, 32, 128) and bench.CASE == dict(K=200, m=4, n_traj=80, length=1000, lag=10, max_iter=1000)
    assert bench.DIAGONALS == (None, 0.999)
    a = bench.build_parser().parse_args(["--resamples", "7", "--parts", "fit"])
    assert a.resamples == 7 and a.parts == ["fit"]
