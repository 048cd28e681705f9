"""Host side of the hidden-Markov-model E-step: the symbols, the plan and the refusals of dff_hmm_estep (refused on the host,
before any device call), the chunked formulation in numpy against the long-double truth on every case of tests/hmm_cases.py,
and initial_hmm / HiddenMarkovModel / HmmEvaluator on a numpy stand-in behind evaluate.hmm_estep_solver
(hmm_cases.host_estep: the chunked formulation with the call's status rules), the re-exports and the tool's arguments.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import hmm_cases as hc
import propagate_cases as pc
from dff_amd import binding, evaluate
from oracle import kinetics as kin
from oracle import msm as oracle
from standins import HostEstep, HostSpectral, OracleSweeps
from support import hmm_chunk, owning_unit, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_hmm_chunk", "dff_hmm_plan", "dff_hmm_workspace_bytes", "dff_hmm_estep")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used


# ---------------------------------------------------------------- symbols, plan and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_hmm_estep"][1]) == 18 and len(binding.SYMBOLS["dff_hmm_workspace_bytes"][1]) == 6
    assert "#define DFF_HMM_MAXM 8" in header and binding.HMM_MAX_HIDDEN == evaluate.HMM_MAX_HIDDEN == 8
    assert hmm_chunk() in (64, 128, 256, 512)
    text = owning_unit("dff_hmm.hip")
    assert '#include "dff_hmm.hip"' in text
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "dff_hmm.hip" in build and "dff_hmm.hip" not in re.sub(r"(?m)^#.*$", "", build)      # named in the comments only


def test_the_plan_counts_chains_and_chunks():
    Cn = hmm_chunk()
    cases = [([], 1), ([0], 1), ([0, 0], 5), ([1], 1), ([1], 7), ([5, 3], 7),                       # a lag longer than every trajectory
             ([Cn], 1), ([2 * Cn], 1), ([2 * Cn], 2), ([3 * Cn, 0, 3 * Cn + 1, 3 * Cn - 1], 3),   # exact multiples of the chunk
             (hc.lengths_for(1, Cn), 1), (hc.lengths_for(3, Cn), 3), (hc.lengths_for(7, Cn), 7), ([Cn + 1] * 80, 10)]
    for lengths, lag in cases:
        assert binding.hmm_plan(lengths, lag) == hc.plan(lengths, lag, Cn), (lengths, lag)
    assert binding.hmm_plan([10, 0, 4], 4)[0] == 12                 # empty chains are counted
    for lengths, lag, text in (([4], 0, "lag must be >= 1"), ([4, -1], 1, "trajectory 1 has negative length"),
                               ([1] * 1025, 1024, "1049600 chains, at most 1048576")):
        with pytest.raises(ValueError, match=text):
            binding.hmm_plan(lengths, lag)


def test_workspace_bytes_and_refusals_before_any_device_call():
    lib = binding.load_library()
    Cn = hmm_chunk()
    L = np.array([3 * Cn + 5, 0, 7], np.int64)
    n = int(L.sum())

    def need(n, lengths, lag, m, K):
        """the sections of the header's comment, each rounded up to 16 bytes"""
        n_chains, n_chunks = hc.plan(lengths, lag, Cn)
        MP = 2 if m <= 2 else (4 if m <= 4 else 8)
        r16 = lambda b: (b + 15) // 16 * 16     # noqa: E731
        return sum(r16(b) for b in (16 * (len(lengths) + 1), 16, 8 * MP * MP, 8 * MP, 8 * K * MP, 8 * n_chunks * MP * MP, 4 * n_chunks * MP,
                                    8 * n_chunks * MP, 8 * n_chunks * MP, 8 * n_chains, 8 * n * m, 8 * ((n + 1023) // 1024) * K * m))
    for lag, m, K in ((1, 1, 1), (3, 3, 5), (7, 8, 1024), (2, 5, 200)):
        assert binding.hmm_workspace_bytes(n, L, lag, m, K) == need(n, L.tolist(), lag, m, K), (lag, m, K)
    assert binding.hmm_workspace_bytes(0, [], 1, 2, 3) == need(0, [], 1, 2, 3)
    for bad, text in (((n, L, 1, 0, 4), "hidden states must be 1..8"), ((n, L, 1, 9, 4), "hidden states must be 1..8"),
                      ((n, L, 1, 2, 0), "symbols must be 1..1024"), ((n, L, 1, 2, 1025), "symbols must be 1..1024"),
                      ((n, L, 0, 2, 4), "lag must be >= 1"), ((n + 1, L, 1, 2, 4), "trajectory lengths sum to"),
                      ((-1, L, 1, 2, 4), "negative frame count"), (((1 << 31) + 1, [(1 << 31) + 1], 1, 2, 4), "more than 2^31 frames")):
        with pytest.raises(ValueError, match=re.escape(text)):
            binding.hmm_workspace_bytes(*bad)

    def call(n=n, lengths=L, lag=1, m=2, K=4, labels=FAKE, trans=FAKE, emit=FAKE, init=FAKE, stats=FAKE, status=FAKE, ws=FAKE,
             wsb=1 << 30):
        lengths = np.asarray(lengths, np.int64)
        return lib.dff_hmm_estep(0, labels, n, p(lengths), len(lengths), lag, trans, emit, init, m, K, stats, None, None, status, ws,
                                 wsb, None)
    refused(lib, call(m=0), "hidden states must be 1..8")
    refused(lib, call(m=9), "hidden states must be 1..8")
    refused(lib, call(K=0), "symbols must be 1..1024")
    refused(lib, call(K=1025), "symbols must be 1..1024")
    refused(lib, call(lag=0), "lag must be >= 1")
    refused(lib, call(n=n + 1), "trajectory lengths sum to")
    refused(lib, call(lengths=[n + 1, -1]), "trajectory 1 has negative length")
    refused(lib, call(lengths=[0] * 2049, n=0, lag=512), "1049088 chains, at most 1048576")
    refused(lib, call(labels=None), "null labels")
    for null in ("trans", "emit", "init", "stats", "status"):
        refused(lib, call(**{null: None}), "null transition matrix")
    want = need(n, L.tolist(), 1, 2, 4)
    refused(lib, call(wsb=want - 1), f"workspace of {want - 1} bytes, {want} needed")
    refused(lib, call(ws=None), f"{want} needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)     # noqa: E731
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensors"):
        binding.hmm_estep(torch.zeros(4, dtype=torch.int32), [4], 1, z(2, 2), z(2, 3), z(2))


def test_every_entry_point_names_itself_and_refuses_the_shape_first():
    """the six hidden-Markov-model entry points share their first checks: each refusal starts with the name of the entry point
    that gave it, and of two faults (m = 0 and lag = 0) the shape is the one that is told"""
    lib = binding.load_library()
    L = np.array([5, 0, 7], np.int64)
    n, K, big = int(L.sum()), 4, 1 << 30

    def sizes(name):
        return lambda lag, m: getattr(lib, "dff_" + name)(n, p(L), len(L), lag, m, K)
    calls = {
        "hmm_workspace_bytes": sizes("hmm_workspace_bytes"),
        "hmm_estep": lambda lag, m: lib.dff_hmm_estep(0, FAKE, n, p(L), len(L), lag, FAKE, FAKE, FAKE, m, K, FAKE, None, None, FAKE, FAKE,
                                                      big, None),
        "hmm_fit_workspace_bytes": sizes("hmm_fit_workspace_bytes"),
        "hmm_fit_steps": lambda lag, m: lib.dff_hmm_fit_steps(0, FAKE, n, p(L), len(L), lag, FAKE, FAKE, FAKE, m, K, 0, 1, 1e-3, 1e-12, 100,
                                                              FAKE, None, FAKE, FAKE, big, None),
        "hmm_viterbi_workspace_bytes": sizes("hmm_viterbi_workspace_bytes"),
        "hmm_viterbi": lambda lag, m: lib.dff_hmm_viterbi(0, FAKE, n, p(L), len(L), lag, FAKE, FAKE, FAKE, m, K, FAKE, 0, None, FAKE, FAKE,
                                                          big, None),
    }
    for name, call in calls.items():
        refusal = -1 if name.endswith("_workspace_bytes") else 1
        for (lag, m), text in (((0, 2), "lag must be >= 1"), ((0, 0), "the number of hidden states must be 1..8")):
            assert call(lag, m) == refusal, (name, lag, m)
            assert lib.dff_last_error().decode() == f"{name}: {text}", (name, lag, m, lib.dff_last_error().decode())


def test_package_reexports():
    for name in ("hmm_estep_solver", "initial_hmm", "HiddenMarkovModel", "HmmEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("hmm_estep", "hmm_plan", "hmm_chunk", "hmm_workspace_bytes"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the chunked formulation against the truth
@pytest.mark.parametrize("case", hc.CASES, ids=lambda c: "m%d-K%d-lag%d%s" % (c[0], c[1], c[2], "-disjoint" if c[3] else ""))
def test_the_chunked_formulation_is_as_close_to_the_truth_as_the_sequential_one(case):
    ref = hc.reference(*case, hmm_chunk())
    for k in hc.OUTPUTS:
        assert ref["e_chunked"][k] <= hc.FACTOR * max(ref["e_seq"][k], 1.0), (k, ref["e_chunked"][k], ref["e_seq"][k])
    truth = ref["truth"]
    n = len(ref["labels"])
    assert abs(float(truth["post"].sum()) - n) < 1e-9 * max(n, 1)
    assert abs(float(truth["gamma_sym"].sum()) - n) < 1e-9 * max(n, 1)          # no label is missing here
    n_chains = sum(1 for c in hc.chains(ref["lengths"], ref["lag"]) if len(c))
    assert abs(float(truth["gamma0"].sum()) - n_chains) < 1e-9 * n_chains and abs(float(truth["xi"].sum()) - (n - n_chains)) < 1e-9 * n


def test_missing_observations_and_the_status_rules_of_the_stand_in():
    m, K, lag, Cn = 3, 5, 3, hmm_chunk()
    labels, lengths, A, B, p0 = hc.case_inputs(m, K, lag, False, Cn)
    lab = hc.with_missing(labels, lengths, lag, Cn)
    ref = hc.reference_of(lab, lengths, lag, A, B, p0, Cn)
    for k in hc.OUTPUTS:
        assert ref["e_chunked"][k] <= hc.FACTOR * max(ref["e_seq"][k], 1.0), (k, ref["e_chunked"][k], ref["e_seq"][k])
    assert abs(float(ref["truth"]["gamma_sym"].sum()) - int((lab >= 0).sum())) < 1e-9 * len(lab)     # a missing label counts nowhere
    whole = [c for c in hc.chains(lengths, lag) if len(c) and (lab[c] < 0).all()]
    assert whole                                                    # a chain of missing labels only: its posterior is the prior's
    prior = p0 / p0.sum()
    for t, f in enumerate(whole[0]):
        assert np.allclose(np.asarray(ref["truth"]["post"][f], np.float64), prior, rtol=1e-12)
        prior = prior @ A
    stats, cl, post, status = hc.host_estep(lab, lengths, lag, A, B, p0, Cn)
    assert status == 0 and not np.isnan(stats).any() and stats.shape == (1 + m * m + m + m * K,)
    for bad in (np.nan, -0.5, np.inf):
        for which in range(3):
            par = [A.copy(), B.copy(), p0.copy()]
            par[which].flat[0] = bad
            out = hc.host_estep(lab, lengths, lag, *par, Cn)
            assert out[3] == 1 and all(np.isnan(x).all() for x in out[:3])
    over = lab.copy()
    over[5] = K
    assert hc.host_estep(over, lengths, lag, A, B, p0, Cn)[3] == 3
    Ad, Bd, pd = hc.model(2, 4, disjoint=True)
    out = hc.host_estep(np.array([0, 2, 1, 1, 0, 2], np.int32), [3, 3], 1, np.eye(2), Bd, pd, Cn)   # 0 -> 1 under A = 1: impossible
    assert out[3] == 2 and all(np.isnan(x).all() for x in out[:3])


# ---------------------------------------------------------------- the Python layer on a stand-in
@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "spectral_solver", HostSpectral)
    monkeypatch.setattr(evaluate, "hmm_estep_solver", HostEstep)
    monkeypatch.setattr(binding, "micro_transition_counts",
                        lambda lab, lengths, lags, K: torch.from_numpy(oracle.transition_counts(lab.numpy(), lengths, lags, K)))
    HostEstep.calls = 0


def test_initial_hmm_on_a_block_model(on_host):
    labels, lengths = pc.three_well_trajectories()
    A, B, p0 = evaluate.initial_hmm(labels, 2, 3, lengths, 10, device="cpu")                       # symbol 9 is never observed
    assert A.shape == (3, 3) and B.shape == (3, 10) and p0.shape == (3,)
    assert np.allclose(A.sum(axis=1), 1.0) and np.allclose(B.sum(axis=1), 1.0) and np.isclose(p0.sum(), 1.0)
    assert (A >= 0).all() and (B >= 0).all() and (np.diag(A) > 0.9).all() and (B[:, 9] == 0).all()
    well = np.argmax(B[:, :9], axis=0)
    assert len(set(well[:3])) == len(set(well[3:6])) == len(set(well[6:])) == 1 and len(set(well)) == 3   # a hidden state per well
    for i in range(3):
        assert B[i, :9][well == i].sum() > 0.9                          # the border microstates share their membership
    model = evaluate.MarkovStateModel(2, device="cpu").fit(torch.from_numpy(labels), lengths, 10)
    flux = model.stationary_distribution[:, None] * model.transition_matrix
    M = evaluate.pcca_memberships(model, 3).clip(0)
    M /= M.sum(axis=1)[:, None]
    X = M.T @ flux @ M
    assert np.allclose(X, X.T, atol=1e-12) and np.allclose(A, X / X.sum(axis=1)[:, None], rtol=1e-12)
    # an observed symbol outside the active set keeps an emission probability: state 9, visited once at a trajectory's end
    lab2 = labels.copy()
    lab2[lengths[0] - 1] = 9
    B2 = evaluate.initial_hmm(lab2, 2, 3, lengths, 10, device="cpu")[1]
    assert (B2[:, 9] > 0).all()
    with pytest.raises(ValueError, match="fewer than n_hidden"):
        evaluate.initial_hmm(np.array([0, 1, 0, 1, 0, 1], np.int32), 1, 3, device="cpu")
    with pytest.raises(ValueError, match="n_hidden must be"):
        evaluate.initial_hmm(labels, 2, 9, lengths, device="cpu")


def em_case():
    A, B, p0 = hc.model(2, 6, seed=3)
    lengths = [150, 90, 0, 160]
    return hc.simulate(A, B, p0 / p0.sum(), lengths, seed=5), lengths, (A, B, p0 / p0.sum())


def start_of(K=6):
    return (np.array([[0.7, 0.3], [0.4, 0.6]]), np.array([[3.0, 2, 1, 1, 1, 1], [1, 1, 1, 1, 2, 3.0]]) / 9.0, np.array([0.5, 0.5]))


def test_the_em_loop_through_the_seam(on_host):
    labels, lengths, _ = em_case()
    for lag in (1, 2):
        h = evaluate.HiddenMarkovModel(2, lag, reversible=False, accuracy=1e-3, max_iter=200, device="cpu")
        h.fit(labels, lengths, 6, initial=start_of())
        ll = np.array(h.log_likelihoods)
        assert h.converged and h.n_iter == len(ll) == HostEstep.calls and not h.degenerate and h.message == ""
        assert (np.diff(ll) >= -1e-9 * np.abs(ll[:-1])).all()                                     # EM never loses likelihood
        assert abs(ll[-1] - ll[-2]) < 1e-3 and (np.abs(np.diff(ll))[:-1] >= 1e-3).all()          # stopped at the first small step
        A, B, p0, pi = h.transition_matrix, h.observation_probabilities, h.initial_distribution, h.stationary_distribution
        assert np.allclose(A.sum(axis=1), 1) and np.allclose(B.sum(axis=1), 1) and np.isclose(p0.sum(), 1) and np.isclose(pi.sum(), 1)
        assert np.allclose(pi @ A, pi, atol=1e-12) and pi[0] >= pi[1]                             # renumbered: largest first
        assert np.isclose(h.log_likelihood(labels, lengths), ll[-1], rtol=1e-12)                  # the parameters of the last E-step
        mm = h.metastable_memberships()
        assert mm.shape == (6, 2) and np.allclose(mm.sum(axis=1), 1.0)
        assert h.timescales().shape == (1,) and h.lifetimes().shape == (2,) and (h.lifetimes() > 0).all()
        post = h.hidden_probabilities(labels, lengths)
        assert post.shape == (len(labels), 2) and torch.allclose(post.sum(dim=1), torch.ones(len(labels), dtype=torch.float64))
        assert h.hidden_states(labels, lengths).dtype == torch.int32
        # the same fit from the start with its hidden states swapped: the same model after the renumbering
        a0, b0, q0 = start_of()
        g = evaluate.HiddenMarkovModel(2, lag, reversible=False, accuracy=1e-3, max_iter=200, device="cpu")
        g.fit(labels, lengths, 6, initial=(a0[::-1, ::-1], b0[::-1], q0[::-1]))
        assert np.allclose(g.transition_matrix, A, rtol=1e-9) and np.allclose(g.observation_probabilities, B, rtol=1e-9, atol=1e-15)
        HostEstep.calls = 0
    few = evaluate.HiddenMarkovModel(2, 1, reversible=False, accuracy=1e-12, max_iter=3, device="cpu").fit(labels, lengths, 6, initial=start_of())
    assert not few.converged and few.n_iter == 3 and len(few.log_likelihoods) == 3


def test_reversible_fit_degenerate_states_and_failures(on_host):
    labels, lengths, _ = em_case()
    h = evaluate.HiddenMarkovModel(2, 1, accuracy=1e-3, max_iter=200, device="cpu").fit(labels, lengths, 6, initial=start_of())
    assert h.converged and h.reversible
    flux = h.stationary_distribution[:, None] * h.transition_matrix
    assert np.allclose(flux, flux.T, atol=1e-10) and h.stationary_distribution[0] >= h.stationary_distribution[1]
    # the default start comes from initial_hmm
    d = evaluate.HiddenMarkovModel(2, 1, max_iter=5, device="cpu").fit(labels, lengths, 6)
    assert d.n_iter >= 2 and np.isfinite(d.log_likelihoods).all()
    # a hidden state that is never occupied keeps its rows
    a0, b0 = np.array([[1.0, 0.0], [0.5, 0.5]]), start_of()[1]
    g = evaluate.HiddenMarkovModel(2, 1, reversible=False, max_iter=4, device="cpu").fit(labels, lengths, 6, initial=(a0, b0, np.array([1.0, 0.0])))
    assert g.degenerate and np.array_equal(g.observation_probabilities[1], b0[1]) and np.array_equal(g.transition_matrix[1], a0[1])
    assert np.allclose(g.stationary_distribution, [1.0, 0.0])
    r = evaluate.HiddenMarkovModel(2, 1, max_iter=4, device="cpu").fit(labels, lengths, 6, initial=(a0, b0, np.array([1.0, 0.0])))
    assert not r.converged and "lost a hidden state" in r.message
    # a model that cannot emit the labels: status 2 ends the fit
    bad = evaluate.HiddenMarkovModel(2, 1, reversible=False, device="cpu").fit(np.array([0, 1, 0], np.int32), None, 2,
                                                                               initial=(np.eye(2), np.eye(2), np.array([0.5, 0.5])))
    assert not bad.converged and "likelihood zero" in bad.message and bad.log_likelihoods == []
    for kw, text in ((dict(n_hidden=0), "n_hidden"), (dict(n_hidden=9), "n_hidden"), (dict(lagtime=0), "lagtime"), (dict(accuracy=0.0), "accuracy"),
                     (dict(max_iter=0), "max_iter")):
        args = dict(n_hidden=2, lagtime=1, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            evaluate.HiddenMarkovModel(**args)
    with pytest.raises(ValueError, match="initial must be"):
        evaluate.HiddenMarkovModel(2, 1, device="cpu").fit(labels, lengths, 6, initial=(np.eye(3), b0, np.ones(2)))
    with pytest.raises(ValueError, match="not fitted"):
        evaluate.HiddenMarkovModel(2, 1, device="cpu").timescales()


# ---------------------------------------------------------------- the evaluator
def test_the_evaluator_checks_its_arguments_and_fills_its_keys(on_host, monkeypatch):
    Cn = hmm_chunk()
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(binding, "hmm_chunk", lambda: Cn)
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.HmmEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None:
                        {"labels": torch.where(torch.isfinite(proj[:, 0]), proj[:, 0].nan_to_num().round(), -torch.ones(len(proj), dtype=proj.dtype)).to(torch.int32)})
    monkeypatch.setattr(evaluate, "label_runs", lambda labels, traj_lengths=None, device=None: kin.label_runs(np.asarray(labels), traj_lengths))

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        args = dict(n_microstates=6, n_hidden=2, lagtime=1, frame_time=0.5, centers=np.arange(6.0).reshape(6, 1), max_iter=30, device="cpu")
        args.update(kw)
        return evaluate.HmmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), **args)
    labels, lengths, _ = em_case()
    frames = labels.astype(np.float64).reshape(-1, 1, 1)
    frames[7] = np.nan                                              # a non-finite frame is a missing observation
    e = make()
    res = e.eval(frames, lengths)
    assert set(res) == set(evaluate.HmmEvaluator.KEYS)
    assert len(res["timescales"]) == 1 and len(res["hidden_populations"]) == len(res["lifetimes"]) == 2
    assert np.isclose(sum(res["hidden_populations"]), 1.0) and res["hidden_populations"][0] >= res["hidden_populations"][1]
    assert res["samples_nonfinite"] == 1.0 and res["n_iter"] >= 2.0 and np.isfinite(res["loglik_per_frame"])
    m = e.models["samples"]
    assert res["lifetimes"] == [float(v) * 0.5 for v in m.lifetimes()] and res["timescales"] == [float(v) * 0.5 for v in m.timescales()]
    assert e.hidden["samples"].shape == (len(labels),) and e.dwell["samples"]["total_frames"] == len(labels)
    assert set(e.dwell["samples"]["labels"]) <= {0, 1}
    with_ref = make(ref_data=frames, ref_traj_lengths=lengths).eval(frames, lengths)
    keys = set(evaluate.HmmEvaluator.KEYS)
    assert set(with_ref) == keys | {k + "_ref" for k in keys} | {"log10_timescale_ratio", "log10_lifetime_ratio", "population_js"}
    assert with_ref["log10_timescale_ratio"] == [0.0] and with_ref["log10_lifetime_ratio"] == [0.0, 0.0] and with_ref["population_js"] == 0.0
    for bad, text in ((dict(lagtime=None), "lagtime"), (dict(lagtime=0), "lagtime"), (dict(n_hidden=0), "n_hidden"), (dict(n_hidden=9), "n_hidden"),
                      (dict(n_microstates=0), "n_microstates"), (dict(frame_time=0.0), "frame_time"), (dict(accuracy=-1.0), "accuracy"),
                      (dict(max_iter=0), "max_iter")):
        with pytest.raises(ValueError, match=text):
            make(**bad)


# ---------------------------------------------------------------- the tools
def test_hmm_arguments_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    full = base + ["--parallel-sim", "4", "--hmm", "--hmm-states", "50", "--hmm-hidden", "3", "--hmm-lag", "5"]
    assert tool.hmm_arguments(ap.parse_args(base)) is None
    assert tool.hmm_arguments(ap.parse_args(full)) == (50, 3, 5)
    assert ap.parse_args(base + ["--parallel-sim", "4", "--hmm", "held.pt", "--hmm-states", "9", "--hmm-hidden", "2", "--hmm-lag", "2"]).hmm == "held.pt"
    assert ap.parse_args(full + ["--frame-time", "0.2"]).frame_time == 0.2
    for alone in (["--hmm-states", "9"], ["--hmm-hidden", "2"], ["--hmm-lag", "2"]):
        with pytest.raises(SystemExit, match="need --hmm"):
            tool.hmm_arguments(ap.parse_args(base + alone))
    with pytest.raises(SystemExit, match="--hmm needs --parallel-sim"):
        tool.hmm_arguments(ap.parse_args(base + ["--hmm", "--hmm-states", "9", "--hmm-hidden", "2", "--hmm-lag", "2"]))
    with pytest.raises(SystemExit, match="--hmm needs --hmm-states K, --hmm-hidden M and --hmm-lag L"):
        tool.hmm_arguments(ap.parse_args(base + ["--parallel-sim", "4", "--hmm", "--hmm-states", "9", "--hmm-lag", "2"]))
    for bad in (["--hmm-hidden", "0"], ["--hmm-hidden", "9"], ["--hmm-states", "0"], ["--hmm-lag", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(full + bad)


def test_the_benchmark_lists_its_rows():
    import tools_bench_hmm as bench
    rows = bench.rows()
    assert len(rows) == 2 * 3 * 2 * 3 and {r["n"] for r in rows} == {100_000, 819_200}
    assert {(r["n_traj"], r["lag"]) for r in rows} == {(80, 1), (80, 10), (1, 1)}
    assert {r["m"] for r in rows} == {2, 4, 8} and {r["K"] for r in rows} == {64, 1024}
    a = bench.build_parser().parse_args(["--rows", "0,5", "--windows", "3"])
    assert a.rows == [0, 5] and a.windows == 3
