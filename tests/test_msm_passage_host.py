"""Host side of the passage feature: the symbols and refusals of dff_msm_dirichlet_solve (refused on the host, before any
device call), MarkovStateModel.flux_matrix, mfpt / committor / reactive_flux / bootstrap_passage on a numpy stand-in behind
evaluate.dirichlet_solver (oracle/passage.py) on hand cases, the reversible=False fallback, set validation, states_by_cv,
the PassageBootstrap statistics, MsmPassageEvaluator's reductions, the re-exports and the tool's arguments.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from dff_amd import binding, evaluate
from oracle import msm_bootstrap as boot
from oracle import passage as po
from standins import OracleSweeps
from support import owning_unit, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_msm_dirichlet_workspace_bytes", "dff_msm_dirichlet_lds_limit", "dff_msm_dirichlet_solve", "dff_debug_msm_dirichlet_path")
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
    assert len(binding.SYMBOLS["dff_msm_dirichlet_solve"][1]) == 15
    assert binding.SYMBOLS["dff_msm_dirichlet_workspace_bytes"] == (C.c_longlong, [C.c_int, C.c_int])
    assert binding.MSM_DIRICHLET_MAX_BATCH == evaluate.DIRICHLET_MAX_BATCH == 16384
    text = owning_unit("dff_msm_passage.hip")
    assert '#include "dff_msm_passage.hip"' in text
    L = binding.msm_dirichlet_lds_limit()
    assert 64 <= L < 1024 and 8 * ((L + 1) * (L + 2) // 2 + (L + 1) + 2 * L) + 4096 <= 160 * 1024        # the triangle fits a CU's LDS


def test_workspace_bytes_and_refusals_before_any_device_call():
    lib = binding.load_library()
    assert binding.msm_dirichlet_workspace_bytes(1, 1) == (1 + 1 + 32) * 8
    assert binding.msm_dirichlet_workspace_bytes(48, 1024) == 48 * (1 + 1024 * 1024 + 32 * 1024) * 8
    for bad in ((0, 4), (16385, 4), (4, 0), (4, 1025)):
        assert lib.dff_msm_dirichlet_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="problems must be 1..16384"):
        binding.msm_dirichlet_workspace_bytes(0, 4)

    def call(ks=(4, 3), Kmax=4, P=None, n_flux=2, flux_of=None, flux=FAKE, ws=FAKE, wsb=1 << 20, status=FAKE):
        ks = np.array(ks, np.int32)
        fo = None if flux_of is None else p(np.array(flux_of, np.int32))
        return lib.dff_msm_dirichlet_solve(0, flux, n_flux, fo, p(ks), len(ks) if P is None else P, Kmax, FAKE, FAKE, FAKE, FAKE, status,
                                           ws, wsb, None)
    refused(lib, call(P=0), "problems must be 1..16384")
    refused(lib, call(ks=[1] * 16385, Kmax=1, n_flux=1, flux_of=[0] * 16385), "problems must be 1..16384")
    refused(lib, call(Kmax=0), "states must be 1..1024")
    refused(lib, call(Kmax=1025), "states must be 1..1024")
    refused(lib, call(n_flux=0), "flux matrices must be 1..16384")
    refused(lib, call(flux=None), "null flux")
    refused(lib, call(status=None), "null flux")
    refused(lib, call(n_flux=1), "1 flux matrices for 2 problems and no flux_of")
    refused(lib, call(ks=(4, 5)), "problem 1 has 5 states, must be 1..Kmax = 4")
    refused(lib, call(ks=(0, 4)), "problem 0 has 0 states")
    refused(lib, call(flux_of=[0, 2]), "problem 1 takes flux matrix 2 of 2")
    refused(lib, call(flux_of=[-1, 0]), "problem 0 takes flux matrix -1 of 2")
    need = 2 * (1 + 16 + 128) * 8
    refused(lib, call(wsb=need - 1), f"workspace of {need - 1} bytes, {need} needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    assert lib.dff_debug_msm_dirichlet_path(5) == 1 and "3 (global, VALU) or 4 (global, MFMA)" in lib.dff_last_error().decode()
    L = binding.msm_dirichlet_lds_limit()
    assert lib.dff_debug_msm_dirichlet_path(1) == 0
    try:
        refused(lib, call(ks=(4, L + 2), Kmax=L + 2, wsb=1 << 30), f"problem 1 has {L + 2} states, the forced LDS path takes at most {L + 1}")
    finally:
        assert lib.dff_debug_msm_dirichlet_path(0) == 0


def test_package_reexports():
    for name in ("mfpt", "committor", "reactive_flux", "ReactiveFlux", "bootstrap_passage", "PassageBootstrap", "states_by_cv",
                 "dirichlet_solver", "MsmPassageEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("msm_dirichlet_solve", "msm_dirichlet_workspace_bytes", "msm_dirichlet_lds_limit", "debug_msm_dirichlet_path"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the oracle's own pieces
def test_the_stand_in_elimination_solves_the_formulation():
    for K, nb, where in ((2, 1, "end"), (17, 3, "start"), (40, 6, "interleaved"), (70, 3, "middle")):
        X = po.ring(K, K) if K < 24 else po.two_well(K, seed=K)
        role = po.boundary_at(K, nb, where)
        for prob in (po.mfpt_problem(X, role, 3.0), po.committor_problem(X, role)):
            u, status = po.solve_one(*prob)
            W, b, I = po.system(*prob)
            if not b.any():                                          # one boundary state, g = 0: u = 0 exactly
                assert status == 0 and not u.any()
                continue
            assert status == 0 and po.backward_error(W, b, u[I]) <= po.eta_bar(len(I))
            assert po.forward_error(u[I], po.truth(W, b)) <= 64 * max(po.lapack_error(W, b), len(I) * po.U)
            T = prob[0] / prob[0].sum(axis=1, keepdims=True)         # and the package's host fallback solves the same problem
            assert np.allclose(evaluate._host_dirichlet(T, *prob[1:]), po.dirichlet(*prob), rtol=1e-6)
    off = np.random.default_rng(0).random((5, 130))
    assert np.allclose(po.row_sums(off), off.sum(axis=1), rtol=1e-14)
    X = po.ring(8, 1)
    cut = X.copy()
    cut[3, :] = cut[:, 3] = 0.0
    assert po.solve_one(cut, po.boundary_at(8, 1, "end"), np.zeros(8), np.ones(8))[1] == 1 + 3
    assert po.solve_one(X, np.zeros(8, np.int32), np.zeros(8), np.ones(8))[1] == -1
    assert po.solve_one(X, np.full(8, 2, np.int32), np.zeros(8), np.ones(8))[1] == -2


def test_forward_ratios_scatter_on_the_bridge():
    """What the forward bar's R = 32 of test_msm_passage.py rests on, reproduced: two_well K = 300, bridge 1e-6, MFPT to the last
    three states, five seeds of the generator.  At near-equal cond(W) 2^-53 (6.4 .. 7.0e-7) np.linalg.solve's own forward error
    spans a factor of about ten, and the ratio to it of LAPACK's Cholesky and of the numpy copy of the kernel's elimination
    scatters between about 1 and 10, every solve backward stable to a few 2^-53.  (The bars below leave room for another
    LAPACK build; measured here: LU 3.8e-9 .. 4.1e-8, potrf 0.7 .. 5.2, the copy 1.0 .. 10.3.)"""
    lu, chol, copy = [], [], []
    for seed in (300, 0, 1, 2, 3):
        prob = po.mfpt_problem(po.two_well(300, 1e-6, seed=seed), po.boundary_at(300, 3, "end"), 5.0)
        W, b, I = po.system(*prob)
        t = po.truth(W, b)
        el = po.lapack_error(W, b, t)
        xc, (xl, failed) = po.cholesky_solve(W, b), po.ldlt_solve(W, b)
        assert failed == -1 and binding.msm_dirichlet_lds_limit() < len(I)      # (the blocked path's size)
        for x in (xc, xl):
            assert po.backward_error(W, b, x) <= 16 * po.U
        lu.append(el), chol.append(po.forward_error(xc, t) / el), copy.append(po.forward_error(xl, t) / el)
        assert max(el, po.forward_error(xc, t), po.forward_error(xl, t)) <= np.linalg.cond(W) * po.U
        print(f"seed {seed}: LU {el:.2e}, potrf ratio {chol[-1]:.1f}, copy of the kernel's elimination {copy[-1]:.1f}")
    assert max(lu) / min(lu) >= 4 and max(max(chol), max(copy)) >= 4 and max(max(chol), max(copy)) <= 32


# ---------------------------------------------------------------- the Python layer on stand-ins
@pytest.fixture
def on_oracle(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "resampled_counter", boot.Counter)
    monkeypatch.setattr(evaluate, "batched_reversible_sweeper", boot.Sweeper)
    monkeypatch.setattr(evaluate, "dirichlet_solver", po.Solver)
    po.Solver.calls = po.Solver.problems = 0


def model_of(T, lag=1, scale=1e7, **kw):
    """a MarkovStateModel fitted on counts pi_i T_ij scale of a reversible T: the estimator returns T"""
    w, v = np.linalg.eig(T.T)
    pi = np.abs(np.real(v[:, np.argmax(np.real(w))]))
    return evaluate.MarkovStateModel(lag, device="cpu", **kw).fit_counts(pi[:, None] / pi.sum() * T * scale)


LINE = np.array([[0.9, 0.1, 0.0], [0.2, 0.7, 0.1], [0.0, 0.3, 0.7]])


def test_flux_matrix_is_set_with_the_transition_matrix(on_oracle):
    m = model_of(LINE)
    X = m.flux_matrix
    assert X.shape == (3, 3) and np.array_equal(X, X.T) and abs(X.sum() - 1) < 1e-15
    assert np.allclose(X, m.stationary_distribution[:, None] * m.transition_matrix, rtol=1e-10)
    assert np.allclose(X / X.sum(axis=1, keepdims=True), LINE, atol=1e-12)
    one = evaluate.MarkovStateModel(1, device="cpu").fit_counts(np.array([[5.0, 0.0], [1.0, 0.0]]))
    assert one.active_set.tolist() == [0] and one.flux_matrix.tolist() == [[1.0]]
    nonrev = evaluate.MarkovStateModel(1, reversible=False, device="cpu").fit_counts(LINE * 100)
    assert nonrev.flux_matrix is None and nonrev.transition_matrix is not None
    assert evaluate.MarkovStateModel(1, device="cpu").flux_matrix is None
    labels, lengths, w = boot.five_state_case()                     # and by the batched route of the bootstrap
    plan = evaluate._BootstrapPlan("t", labels, 2, lengths, 5, None, None, 0, w[:2], 1e-12, 100000, 16, None, "cpu")
    for b0, models in plan.batches():
        for mm in models:
            ref = evaluate.MarkovStateModel(2, steps_per_sync=16, max_iter=100000, device="cpu").fit_counts(mm.count_matrix)
            assert mm.flux_matrix.tobytes() == ref.flux_matrix.tobytes()


def test_hand_cases_through_the_injected_solver(on_oracle):
    a, b = 0.03, 0.07
    two = model_of(np.array([[1 - a, a], [b, 1 - b]]))
    assert abs(evaluate.mfpt(two, [1])[0] - 1 / a) <= 2 * np.spacing(1 / a) and evaluate.mfpt(two, [1])[1] == 0.0
    assert abs(evaluate.mfpt(two, [0], [1]) - 1 / b) <= 2 * np.spacing(1 / b)
    m = model_of(LINE, lag=2)
    assert np.allclose(evaluate.mfpt(m, [2]), [80.0, 60.0, 0.0], rtol=1e-11)
    assert np.allclose(evaluate.mfpt(m, [0]), [0.0, 40.0 / 3.0, 20.0], rtol=1e-11)
    pi = m.stationary_distribution
    assert np.isclose(evaluate.mfpt(m, [2], source=[0, 1]), (pi[0] * 80 + pi[1] * 60) / (pi[0] + pi[1]), rtol=1e-11)
    q = evaluate.committor(m, [0], [2])
    assert q[0] == 0.0 and q[2] == 1.0 and np.isclose(q[1], 1.0 / 3.0, rtol=1e-12)
    assert np.allclose(evaluate.committor(m, [2], [0]), 1.0 - q, atol=1e-15)                       # the backward committor
    rf = evaluate.reactive_flux(m, [0], [2])
    X = m.flux_matrix
    assert isinstance(rf, evaluate.ReactiveFlux) and np.array_equal(rf.committor, q)
    assert np.isclose(rf.total_flux, X[0, 1] * q[1], rtol=1e-14) and np.isclose(rf.total_flux, 0.02, rtol=1e-10)   # pi_0 T_01 q_1 = .6 .1 / 3
    assert np.isclose(rf.rate, 0.02 / (2 * np.dot(pi, 1 - q)), rtol=1e-10)
    want = np.zeros((3, 3))
    want[0, 1], want[1, 2] = X[0, 1] * q[1], X[1, 2] * (1 - q[1])
    assert np.allclose(rf.net_flux, want, atol=1e-16) and np.isclose(want[0, 1], want[1, 2], rtol=1e-10)   # what enters leaves
    assert po.Solver.calls > 0


def test_sets_are_validated_and_inactive_states_dropped(on_oracle):
    C = np.zeros((5, 5))
    C[:3, :3] = LINE * 1000
    C[4, 4] = 7.0                                                    # state 3 never seen, state 4 disconnected
    m = evaluate.MarkovStateModel(1, device="cpu").fit_counts(C)
    assert m.active_set.tolist() == [0, 1, 2]
    assert np.allclose(evaluate.mfpt(m, [2, 3, 4]), evaluate.mfpt(m, [2]))
    for call, what in ((lambda: evaluate.mfpt(m, [3, 4]), "target has no state in the active set"),
                       (lambda: evaluate.mfpt(m, [2], [4]), "source has no state in the active set"),
                       (lambda: evaluate.mfpt(m, [2], [1, 2]), "source and target overlap"),
                       (lambda: evaluate.mfpt(m, [5]), "outside 0 .. 4"), (lambda: evaluate.mfpt(m, [-1]), "outside 0 .. 4"),
                       (lambda: evaluate.committor(m, [0], [4]), "B has no state in the active set"),
                       (lambda: evaluate.committor(m, [0, 1], [1, 2]), "A and B overlap"),
                       (lambda: evaluate.reactive_flux(m, [], [2]), "A has no state"),
                       (lambda: evaluate.mfpt(evaluate.MarkovStateModel(1, device="cpu"), [0]), "not fitted")):
        with pytest.raises(ValueError, match=what):
            call()

    class Failing:
        def __init__(self, device):
            pass

        def __call__(self, flux, flux_of, ks, role, g, s):
            return np.full(role.shape, np.nan), np.full(len(ks), 3, np.int32)
    evaluate.dirichlet_solver = Failing                              # (monkeypatched by the fixture: restored after the test)
    with pytest.raises(ValueError, match="status 3"):
        evaluate.mfpt(m, [2])


def test_nonreversible_models_take_the_host_fallback(on_oracle):
    T = np.array([[0.8, 0.2, 0.0], [0.0, 0.7, 0.3], [0.4, 0.0, 0.6]])                             # a cycle: no detailed balance
    m = evaluate.MarkovStateModel(3, reversible=False, device="cpu").fit_counts(T * 1000)
    assert m.flux_matrix is None
    got = evaluate.mfpt(m, [2])
    m1 = 3 / 0.3
    assert np.allclose(got, [3 / 0.2 + m1, m1, 0.0], rtol=1e-13) and po.Solver.calls == 0          # no device call
    q = evaluate.committor(m, [0], [2])
    assert np.allclose(q, [0.0, 1.0, 1.0]) and po.Solver.calls == 0                                # from 1 the cycle reaches 2 first
    with pytest.raises(ValueError, match="needs a reversible model"):
        evaluate.reactive_flux(m, [0], [2])


def test_bootstrap_passage_on_stand_ins_equals_fit_counts_resample_by_resample(on_oracle):
    labels, lengths, w = boot.five_state_case()
    lag, K, A, Bs = 2, 5, [0], [3, 4]
    settings = dict(tol=1e-12, max_iter=100000, steps_per_sync=16)
    bs = evaluate.bootstrap_passage(labels, lag, A, Bs, lengths, K, weights=w, device="cpu", **settings)
    assert isinstance(bs, evaluate.PassageBootstrap) and bs.committor.shape == (len(w), K) and np.array_equal(bs.weights, w)
    n_batches = po.Solver.calls - 1                                  # one call for the point model, one per batch
    assert n_batches == 1
    solved = 0
    for b, Cb in enumerate(boot.weighted_counts(labels, lengths, lengths, lag, K, w)):
        m = evaluate.MarkovStateModel(lag, device="cpu", **settings).fit_counts(Cb)
        if not all(np.isin(m.active_set, st).any() for st in (A, Bs)):
            assert np.isnan([bs.mfpt_ab[b], bs.mfpt_ba[b], bs.rate_ab[b], bs.rate_ba[b]]).all() and np.isnan(bs.committor[b]).all()
            continue
        solved += 1
        assert evaluate.mfpt(m, Bs, A) == bs.mfpt_ab[b] and evaluate.mfpt(m, A, Bs) == bs.mfpt_ba[b], b
        assert evaluate.reactive_flux(m, A, Bs).rate == bs.rate_ab[b], b
        assert np.isclose(evaluate.reactive_flux(m, Bs, A).rate, bs.rate_ba[b], rtol=1e-12), b      # from 1 - q of the same solve
        full = np.full(K, np.nan)
        full[m.active_set] = evaluate.committor(m, A, Bs)
        assert full.tobytes() == bs.committor[b].tobytes(), b
        assert bs.converged[b] == m.converged
    assert 2 <= solved < len(w) and bs.n_failed == len(w) - solved
    assert bs.point["mfpt_ab"] == bs.mfpt_ab[0] and bs.point["model"].n_iter > 0                   # resample 0 is all ones
    one = evaluate.bootstrap_passage(labels, lag, A, Bs, lengths, K, weights=w, resample_batch=1, device="cpu", **settings)
    assert one.mfpt_ab.tobytes() == bs.mfpt_ab.tobytes() and one.committor.tobytes() == bs.committor.tobytes()
    for kw, what in ((dict(A=[0], B=[0, 3]), "overlap"), (dict(A=[], B=[3]), "A must hold states"), (dict(A=[0], B=[5]), "B must hold states"),
                     (dict(A=[0], B=[3], n_states=0), "n_states"), (dict(A=[0], B=[3], resample_batch=0), "resample_batch")):
        args = dict(n_states=K, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            evaluate.bootstrap_passage(labels, lag, args.pop("A"), args.pop("B"), lengths, **args)


def test_passage_bootstrap_statistics():
    rng = np.random.default_rng(0)
    cols = [rng.lognormal(2.0, 0.3, 41) for _ in range(4)]
    cols[0][[3, 17]] = np.nan
    cols[3][5] = np.inf
    conv = np.ones(41, bool)
    conv[7] = False
    bs = evaluate.PassageBootstrap(*cols, np.zeros((41, 2)), conv, None, None, {})
    assert bs.n_failed == 4
    table = np.stack(cols, axis=1)
    for conf in (0.95, 0.5):
        lo, hi = boot.interval(table, conf)
        got = bs.interval(conf)
        for j, f in enumerate(evaluate.PassageBootstrap.FIELDS):
            assert np.allclose(got[f], (lo[j], hi[j]), rtol=1e-14) and got[f][0] < got[f][1]
    assert np.allclose([bs.std()[f] for f in evaluate.PassageBootstrap.FIELDS], boot.std(table), rtol=1e-13)
    with pytest.raises(ValueError, match="confidence"):
        bs.interval(1.0)


def test_states_by_cv():
    labels = np.array([0, 0, 1, 1, 2, 2, 4, 4, -1, 7, 1])
    cv = np.array([0.1, 0.3, 0.95, 0.9, 0.5, 0.5, 0.0, np.nan, 0.0, 0.0, 0.85])
    A, Bs = evaluate.states_by_cv(labels, cv, 0.2, 0.9, 6)
    assert A.dtype == Bs.dtype == np.int64 and A.tolist() == [0, 4] and Bs.tolist() == [1]         # 3 and 5 have no frames; 7 >= n_states
    A, Bs = evaluate.states_by_cv(torch.from_numpy(labels), torch.from_numpy(cv).float(), 0.25, 0.85, 6)
    assert A.tolist() == [0, 4] and Bs.tolist() == [1]
    for args, what in (((labels, cv, 0.9, 0.2, 6), "lo < hi"), ((labels, cv, 0.2, 0.9, 0), "n_states"), ((labels[:3], cv, 0.2, 0.9, 6), "labels for")):
        with pytest.raises(ValueError, match=what):
            evaluate.states_by_cv(*args)


def test_the_evaluators_reductions(on_oracle):
    m = model_of(LINE, lag=2)
    rows, comm = evaluate._passage_batch([m], [0], [2], 4, "cpu")
    assert np.isclose(rows[0, 0], 80.0, rtol=1e-11) and np.isclose(rows[0, 1], 20.0, rtol=1e-11) and np.isnan(comm[0, 3])
    res = evaluate.MsmPassageEvaluator.summarize(m, rows[0], comm[0], [2, 3], [0], frame_time=0.5, samples_nonfinite=4)
    assert tuple(res) == evaluate.MsmPassageEvaluator.KEYS
    assert np.isclose(res["mfpt_folding"], 40.0, rtol=1e-11) and np.isclose(res["mfpt_unfolding"], 10.0, rtol=1e-11)
    assert np.isclose(res["rate_folding"], 2 * evaluate.reactive_flux(m, [0], [2]).rate) and res["samples_nonfinite"] == 4.0
    assert res["n_folded_states"] == 1.0 and res["n_unfolded_states"] == 1.0 and res["committor_mid_share"] == 0.0   # q_1 = 1 / 3
    sym = model_of(np.array([[0.9, 0.1, 0.0], [0.1, 0.8, 0.1], [0.0, 0.1, 0.9]]))
    rows, comm = evaluate._passage_batch([sym], [0], [2], 3, "cpu")
    res = evaluate.MsmPassageEvaluator.summarize(sym, rows[0], comm[0], [2], [0])
    assert np.isclose(res["committor_mid_share"], 1.0 / 3.0, rtol=1e-9)                             # q_1 = 1 / 2, pi uniform
    rows, comm = evaluate._passage_batch([sym], [0], [7], 8, "cpu")                                 # a set without an active state
    assert np.isnan(rows).all() and np.isnan(comm).all()
    assert np.isnan(evaluate.MsmPassageEvaluator.summarize(sym, rows[0], comm[0], [7], [0])["committor_mid_share"])
    for kw in (dict(lagtime=0), dict(lagtime=2, n_microstates=2000), dict(lagtime=2, cv="x"), dict(lagtime=2, lo=0.9, hi=0.2),
               dict(lagtime=2, n_bootstrap=-1)):
        F = binding.DFF_MAX_BEADS
        with pytest.raises(ValueError):
            evaluate.MsmPassageEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), np.zeros((10, 3)), device="cpu", **kw)


def test_the_passage_evaluator_builds_no_other_evaluator(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    built = []
    for cls in (evaluate.MsmEvaluator, evaluate.FoldingKineticsEvaluator):
        def counted(self, *a, _init=cls.__init__, _name=cls.__name__, **k):
            built.append(_name)
            _init(self, *a, **k)
        monkeypatch.setattr(cls, "__init__", counted)
    F = binding.DFF_MAX_BEADS
    tica = (np.zeros(F), np.zeros((F, 1)))
    e = evaluate.MsmPassageEvaluator("chignolin", tica, np.zeros((10, 3)), n_microstates=3, lagtime=2, centers=np.zeros((3, 1)), device="cpu")
    assert built == [] and e.centers.shape == (3, 1) and e.kmeans is None and (e.lo, e.hi, e.cv) == (0.2, 0.9, "q")
    assert not hasattr(e, "discretiser") and not hasattr(e, "order")
    evaluate.MsmEvaluator("chignolin", tica, lagtime=2, device="cpu")
    evaluate.FoldingKineticsEvaluator("chignolin", np.zeros((10, 3)), lo=0.2, hi=0.9, device="cpu")
    assert built == ["MsmEvaluator", "FoldingKineticsEvaluator"]                                   # the count does count


# ---------------------------------------------------------------- the tool
def test_passage_arguments_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    a = ap.parse_args(base)
    assert a.passage is None and tool.passage_arguments(a) is None
    full = base + ["--folded-pdb", "f.pdb", "--parallel-sim", "4", "--passage", "--passage-states", "50", "--passage-lag", "3"]
    assert tool.passage_arguments(ap.parse_args(full)) == (50, 3, "q", (0.2, 0.9))
    a = ap.parse_args(full[:8] + ["h.pt"] + full[8:] + ["--passage-cv", "rmsd", "--passage-cores", "2,6", "--passage-bootstrap", "20"])
    assert a.passage == "h.pt" and a.passage_bootstrap == 20 and tool.passage_arguments(a) == (50, 3, "rmsd", (2.0, 6.0))
    for cut, what in (("--folded-pdb", "needs --folded-pdb"), ("--parallel-sim", "needs --parallel-sim"),
                      ("--passage-states", "--passage-states K and --passage-lag L"), ("--passage-lag", "--passage-states K and --passage-lag L")):
        i = full.index(cut)
        with pytest.raises(SystemExit, match=what):
            tool.passage_arguments(ap.parse_args(full[:i] + full[i + 2:]))
    with pytest.raises(SystemExit, match="--passage-cv rmsd needs --passage-cores"):
        tool.passage_arguments(ap.parse_args(full + ["--passage-cv", "rmsd"]))
    for alone in (["--passage-states", "5"], ["--passage-lag", "2"], ["--passage-cv", "q"], ["--passage-cores", "0.1,0.8"], ["--passage-bootstrap", "9"]):
        with pytest.raises(SystemExit, match="need --passage"):
            tool.passage_arguments(ap.parse_args(base + alone))
    for bad in (["--passage-states", "0"], ["--passage-states", "1025"], ["--passage-lag", "0"], ["--passage-cv", "z"],
                ["--passage-cores", "0.9,0.2"], ["--passage-bootstrap", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(full + bad)
    assert tool.msm_arguments(ap.parse_args(base + ["--msm", "--msm-states", "9", "--msm-lag", "2"])) == (9, 2)   # the old ones stand
