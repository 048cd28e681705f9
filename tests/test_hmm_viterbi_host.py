"""Host side of the Viterbi call: the symbols, the workspace and the refusals of dff_hmm_viterbi (refused on the host, before any
device call), the chunked statement in numpy against the sequential recursion and the long-double truth on every case of
tests/hmm_cases.py, the status rules of the stand-in, hmm_chain_lengths, HiddenMarkovModel.viterbi and HmmEvaluator(path=...) on
the stand-in behind evaluate.hmm_viterbi_solver (viterbi_cases.host_viterbi), the re-exports and the tools' arguments.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import hmm_cases as hc
import viterbi_cases as vc
from dff_amd import binding, evaluate
from oracle import kinetics as kin
from standins import HostEstep, HostViterbi
from support import hmm_chunk, owning_unit, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_hmm_viterbi_workspace_bytes", "dff_hmm_viterbi", "dff_debug_hmm_viterbi_stages")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used
ids = lambda c: "m%d-K%d-lag%d%s" % (c[0], c[1], c[2], "-disjoint" if c[3] else "")     # noqa: E731


# ---------------------------------------------------------------- symbols, workspace and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_hmm_viterbi"][1]) == 18 and len(binding.SYMBOLS["dff_hmm_viterbi_workspace_bytes"][1]) == 6
    assert binding.SYMBOLS["dff_debug_hmm_viterbi_stages"] == (C.c_int, [C.c_int])
    text = owning_unit("dff_hmm_viterbi.hip")
    assert '#include "dff_hmm_viterbi.hip"' in text
    kernels = open(os.path.join(ROOT, "two-for-one-diffusion_amd", "csrc", "dff_hmm_viterbi.hip")).read()
    assert '#include "dff_hmm.hip"' in kernels and "#define DFF_HMM_CHUNK" not in kernels          # the plan and the chunk are the E-step's
    code = re.sub(r"(?m)//.*$", "", kernels)
    for word in ("log(", "exp(", "fma(", "atomic"):
        assert word not in code, word                               # additions, comparisons and selects only
    for stages in (-1, 7):
        with pytest.raises(ValueError, match="debug_hmm_viterbi_stages"):
            binding.debug_hmm_viterbi_stages(stages)
    binding.debug_hmm_viterbi_stages(0)


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
        return sum(r16(b) for b in (16 * (len(lengths) + 1), 16, 8 * MP * MP, 8 * MP, 8 * K * MP, 8 * n_chunks * MP * MP, 8 * n_chunks * MP,
                                    4 * n, 4 * n_chunks, 4 * n_chunks, 4 * n_chains, 8 * n_chains))
    for lag, m, K in ((1, 1, 1), (3, 3, 5), (7, 8, 1024), (2, 5, 200)):
        assert binding.hmm_viterbi_workspace_bytes(n, L, lag, m, K) == need(n, L.tolist(), lag, m, K), (lag, m, K)
    assert binding.hmm_viterbi_workspace_bytes(0, [], 1, 2, 3) == need(0, [], 1, 2, 3)
    for bad, text in (((n, L, 1, 0, 4), "hidden states must be 1..8"), ((n, L, 1, 9, 4), "hidden states must be 1..8"),
                      ((n, L, 1, 2, 0), "symbols must be 1..1024"), ((n, L, 1, 2, 1025), "symbols must be 1..1024"),
                      ((n, L, 0, 2, 4), "lag must be >= 1"), ((n + 1, L, 1, 2, 4), "trajectory lengths sum to"),
                      ((-1, L, 1, 2, 4), "negative frame count"), (((1 << 31) + 1, [(1 << 31) + 1], 1, 2, 4), "more than 2^31 frames")):
        with pytest.raises(ValueError, match=re.escape(text)):
            binding.hmm_viterbi_workspace_bytes(*bad)

    def call(n=n, lengths=L, lag=1, m=2, K=4, labels=FAKE, trans=FAKE, emit=FAKE, init=FAKE, path=FAKE, order=0, status=FAKE, ws=FAKE,
             wsb=1 << 30):
        lengths = np.asarray(lengths, np.int64)
        return lib.dff_hmm_viterbi(0, labels, n, p(lengths), len(lengths), lag, trans, emit, init, m, K, path, order, None, status, ws,
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
    for null in ("trans", "emit", "init", "path", "status"):
        refused(lib, call(**{null: None}), "null log transition matrix")
    for order in (-1, 2):
        refused(lib, call(order=order), "chain_order must be 0")
    want = need(n, L.tolist(), 1, 2, 4)
    refused(lib, call(wsb=want - 1), f"workspace of {want - 1} bytes, {want} needed")
    refused(lib, call(ws=None), f"{want} needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)     # noqa: E731
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensors"):
        binding.hmm_viterbi(torch.zeros(4, dtype=torch.int32), [4], 1, z(2, 2), z(2, 3), z(2))


def test_package_reexports():
    for name in ("hmm_viterbi_solver", "hmm_chain_lengths"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("hmm_viterbi", "hmm_viterbi_workspace_bytes", "debug_hmm_viterbi_stages"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the chunked statement against the sequential recursion
@pytest.mark.parametrize("case", hc.CASES, ids=ids)
def test_the_chunked_statement_is_the_sequential_recursion_on_exact_inputs(case):
    ref = vc.exact_reference(*case, hmm_chunk())
    assert (ref["labels"] < 0).any()
    full = np.array([len(c) > 0 for c in hc.chains(ref["lengths"], ref["lag"])])
    assert np.isfinite(ref["sequential"][1][full]).all()            # no chain is impossible
    assert np.array_equal(ref["chunked"][0], ref["sequential"][0]) and ref["chunked"][1].tobytes() == ref["sequential"][1].tobytes()
    assert ref["e_seq"] == ref["e_chunked"] == {"path": 0.0, "chain_logprob": 0.0}       # exact sums: fp64 is the truth


def test_ties_decide_frames_on_the_exact_inputs():
    """with the states renumbered backwards the lowest-index rule picks other paths: the exact inputs do pin the tie rule"""
    decided = 0
    for case in ((8, 5, 1, False), (3, 5, 7, False), (2, 5, 3, False)):
        ref = vc.exact_reference(*case, hmm_chunk())
        la, lb, lp = ref["la"], ref["lb"], ref["lp"]
        flipped = vc.sequential_all(ref["labels"], ref["lengths"], ref["lag"], la[::-1, ::-1], lb[::-1], lp[::-1], np.float64)
        decided += int((case[0] - 1 - flipped[0] != ref["sequential"][0]).sum())
        assert flipped[1].tobytes() == ref["sequential"][1].tobytes()       # the same optimum either way
    assert decided > 0


@pytest.mark.parametrize("case", hc.CASES, ids=ids)
def test_the_chunked_statement_is_as_close_to_the_truth_as_the_sequential_one(case):
    ref = vc.reference(*case, hmm_chunk())
    for k in vc.OUTPUTS:
        assert ref["e_chunked"][k] <= vc.FACTOR * max(ref["e_seq"][k], 1.0), (k, ref["e_chunked"][k], ref["e_seq"][k])
    assert ref["e_seq"]["path"] >= 0.0 and ref["e_chunked"]["path"] >= 0.0        # no path beats the truth's
    n_chains = len(ref["lengths"]) * ref["lag"]
    assert ref["chunked"][1].shape == ref["optimum"].shape == (n_chains,)
    m = case[0]
    assert ref["chunked"][0].min(initial=0) >= 0 and ref["chunked"][0].max(initial=0) < m


def test_missing_observations_and_the_status_rules_of_the_stand_in():
    m, K, lag, Cn = 3, 5, 3, hmm_chunk()
    ref = vc.reference(m, K, lag, False, Cn, missing=True)
    lab, lengths, la, lb, lp = ref["labels"], ref["lengths"], ref["la"], ref["lb"], ref["lp"]
    for k in vc.OUTPUTS:
        assert ref["e_chunked"][k] <= vc.FACTOR * max(ref["e_seq"][k], 1.0)
    whole = [c for c in hc.chains(lengths, lag) if len(c) and (lab[c] < 0).all()]
    assert whole                                                    # a chain of missing labels only: the best path of the bare chain
    path, cl, status = vc.host_viterbi(lab, lengths, lag, la, lb, lp, Cn)
    assert status == 0 and path.dtype == np.int32 and path.shape == lab.shape and (path >= 0).all() and (path < m).all()
    bare = vc.sequential(np.full(len(whole[0]), -1), la, np.zeros_like(lb), lp, np.float64)
    assert np.array_equal(path[whole[0]], bare[0])
    by_chain = vc.host_viterbi(lab, lengths, lag, la, lb, lp, Cn, True)
    assert by_chain[2] == 0 and np.array_equal(by_chain[0], path[vc.chain_order(lengths, lag)]) and np.array_equal(by_chain[1], cl)
    order = vc.chain_order(lengths, lag)
    assert np.array_equal(np.sort(order), np.arange(len(lab)))

    def failed(out, status):
        return out[2] == status and (out[0] == -1).all() and np.isnan(out[1]).all() and len(out[0]) == len(lab)
    over = lab.copy()
    over[5] = K
    for bad in (np.nan, np.inf):
        for which in range(3):
            par = [la.copy(), lb.copy(), lp.copy()]
            par[which].flat[0] = bad
            assert failed(vc.host_viterbi(lab, lengths, lag, *par, Cn), 1)
            assert failed(vc.host_viterbi(over, lengths, lag, *par, Cn), 1)                        # 1 wins over 3
    assert failed(vc.host_viterbi(over, lengths, lag, la, lb, lp, Cn), 3)
    dead = lb.copy()
    dead[:, 2] = -np.inf
    hit = lab.copy()
    hit[3] = 2
    assert failed(vc.host_viterbi(hit, lengths, lag, la, dead, lp, Cn), 2)
    both = hit.copy()
    both[9] = K
    assert failed(vc.host_viterbi(both, lengths, lag, la, dead, lp, Cn), 3)                        # 3 wins over 2
    holes = la.copy()
    holes[0, 1] = -np.inf
    assert vc.host_viterbi(lab, lengths, lag, holes, lb, lp, Cn)[2] == 0                           # -inf alone is no failure
    empty = vc.host_viterbi(np.zeros(0, np.int32), [0, 0], 2, la, lb, lp, Cn)
    assert empty[2] == 0 and empty[0].shape == (0,) and (empty[1] == 0.0).all() and empty[1].shape == (4,)


def test_chain_lengths_are_those_of_the_chains():
    Cn = hmm_chunk()
    for lengths, lag in (([], 1), ([0], 3), ([5, 3], 7), ([10, 0, 4], 4), (hc.lengths_for(1, Cn), 1), (hc.lengths_for(3, Cn), 3),
                         (hc.lengths_for(7, Cn), 7)):
        got = evaluate.hmm_chain_lengths(lengths, lag)
        assert got.dtype == np.int64 and got.tolist() == [len(c) for c in hc.chains(lengths, lag)], (lengths, lag)
        assert int(got.sum()) == sum(lengths)
    with pytest.raises(ValueError, match="lag must be"):
        evaluate.hmm_chain_lengths([4], 0)


# ---------------------------------------------------------------- the Python layer on the stand-in
@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(evaluate, "hmm_estep_solver", HostEstep)
    monkeypatch.setattr(evaluate, "hmm_viterbi_solver", HostViterbi)
    HostViterbi.calls = []


def metastable_case():
    A = np.array([[0.96, 0.03, 0.01], [0.02, 0.95, 0.03], [0.01, 0.04, 0.95]])
    B = hc.model(3, 12, seed=1, disjoint=True)[1]
    B = 0.9 * B + 0.1 / 12                                           # mostly, not only, its own symbols
    lengths = [260, 0, 131, 90]
    p0 = np.array([0.5, 0.3, 0.2])
    return hc.simulate(A, B, p0, lengths, seed=5), lengths, (A, B, p0)


def fitted(lag, labels, lengths, start):
    return evaluate.HiddenMarkovModel(3, lag, reversible=False, accuracy=1e-3, max_iter=3, device="cpu").fit(labels, lengths, 12, initial=start)


def test_the_model_decodes_through_the_seam(on_host):
    labels, lengths, start = metastable_case()
    for lag in (1, 2):
        h = fitted(lag, labels, lengths, start)
        path = h.viterbi(labels, lengths)
        assert isinstance(path, torch.Tensor) and path.dtype == torch.int32 and path.shape == (len(labels),)
        used_lag, order, la, lb, lp = HostViterbi.calls[-1]
        with np.errstate(divide="ignore"):                           # the logarithms of the fitted parameters, taken on the host
            assert used_lag == lag and not order and np.array_equal(la, np.log(h.transition_matrix))
            assert np.array_equal(lb, np.log(h.observation_probabilities)) and np.array_equal(lp, np.log(h.initial_distribution))
        want, cl, status = vc.host_viterbi(labels, lengths, lag, la, lb, lp, binding.hmm_chunk())
        assert status == 0 and np.array_equal(path.numpy(), want)
        by_chain, logprob = h.viterbi(labels, lengths, order="chain", return_log_probabilities=True)
        assert HostViterbi.calls[-1][1] and np.array_equal(by_chain.numpy(), want[vc.chain_order(lengths, lag)])
        assert np.array_equal(logprob, cl) and logprob.shape == (len(lengths) * lag,)
        # the most probable PATH against the most probable STATES: mostly the same frames, never a better score
        states = h.hidden_states(labels, lengths).numpy()
        assert (states == want).mean() > 0.9
        assert (vc.scores(want, labels, lengths, lag, la, lb, lp) >= vc.scores(states, labels, lengths, lag, la, lb, lp) - 1e-9).all()
    with pytest.raises(ValueError, match='order must be "frame" or "chain"'):
        h.viterbi(labels, lengths, order="time")
    with pytest.raises(ValueError, match="not fitted"):
        evaluate.HiddenMarkovModel(2, 1, device="cpu").viterbi(labels, lengths)
    # a model that cannot emit the labels: status 2 raises, as _posterior does
    g = evaluate.HiddenMarkovModel(2, 1, device="cpu")
    g.transition_matrix, g.observation_probabilities, g.initial_distribution = np.eye(2), np.eye(2), np.array([0.5, 0.5])
    with pytest.raises(ValueError, match=r"Viterbi pass failed on these labels \(status 2\)"):
        g.viterbi(np.array([0, 1, 0], np.int32))
    assert g.viterbi(np.array([1, 1, 1], np.int32)).tolist() == [1, 1, 1]      # zeros became -inf: impossible steps, no failure


def test_the_evaluator_takes_dwells_inside_the_chains(on_host, monkeypatch):
    Cn = hmm_chunk()
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(binding, "hmm_chunk", lambda: Cn)
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.HmmEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None:
                        {"labels": torch.where(torch.isfinite(proj[:, 0]), proj[:, 0].nan_to_num().round(), -torch.ones(len(proj), dtype=proj.dtype)).to(torch.int32)})
    monkeypatch.setattr(evaluate, "label_runs", lambda labels, traj_lengths=None, device=None: kin.label_runs(np.asarray(labels), traj_lengths))
    labels, lengths, start = metastable_case()
    monkeypatch.setattr(evaluate, "initial_hmm", lambda *a, **k: start)

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        args = dict(n_microstates=12, n_hidden=3, lagtime=2, frame_time=0.5, centers=np.arange(12.0).reshape(12, 1), max_iter=3,
                    reversible=False, device="cpu")
        args.update(kw)
        return evaluate.HmmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), **args)
    frames = labels.astype(np.float64).reshape(-1, 1, 1)
    frames[7] = np.nan                                              # a non-finite frame is a missing observation: it still gets a state
    v = make(path="viterbi")
    assert v.path == "viterbi" and make().path == "posterior"
    res = v.eval(frames, lengths)
    assert set(res) == set(evaluate.HmmEvaluator.KEYS)
    model = v.models["samples"]
    lab = v.labels["samples"]
    assert lab[7] == -1
    hidden = v.hidden["samples"]
    assert hidden.shape == (len(labels),) and hidden.dtype == np.int32 and hidden[7] >= 0
    assert np.array_equal(hidden, model.viterbi(lab, lengths).numpy())
    chain_path = model.viterbi(lab, lengths, order="chain").numpy()
    want = evaluate.dwell_summary(kin.label_runs(chain_path, evaluate.hmm_chain_lengths(lengths, 2)), 0.5 * 2)
    np.testing.assert_equal(v.dwell["samples"], want)
    assert want["total_frames"] == len(labels) and set(want["labels"]) <= {0, 1, 2}
    # path="posterior" and the default are the evaluator as it was
    a, b = make(), make(path="posterior")
    ra, rb = a.eval(frames, lengths), b.eval(frames, lengths)
    np.testing.assert_equal(ra, rb)
    np.testing.assert_equal(ra, res)
    assert np.array_equal(a.hidden["samples"], b.hidden["samples"])
    assert np.array_equal(a.hidden["samples"], a.models["samples"].hidden_states(lab, lengths).numpy())
    np.testing.assert_equal(a.dwell["samples"], evaluate.dwell_summary(kin.label_runs(a.hidden["samples"], lengths), 0.5))
    np.testing.assert_equal(a.dwell["samples"], b.dwell["samples"])
    with pytest.raises(ValueError, match='path must be "posterior" or "viterbi"'):
        make(path="map")


# ---------------------------------------------------------------- the tools
def test_hmm_path_argument_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    full = base + ["--parallel-sim", "4", "--hmm", "--hmm-states", "50", "--hmm-hidden", "3", "--hmm-lag", "5"]
    assert ap.parse_args(full).hmm_path is None and ap.parse_args(base).hmm_path is None
    for choice in ("posterior", "viterbi"):
        a = ap.parse_args(full + ["--hmm-path", choice])
        assert a.hmm_path == choice and tool.hmm_arguments(a) == (50, 3, 5)
    with pytest.raises(SystemExit, match="--hmm-path needs --hmm"):
        tool.hmm_arguments(ap.parse_args(base + ["--hmm-path", "viterbi"]))
    with pytest.raises(SystemExit):
        ap.parse_args(full + ["--hmm-path", "map"])
    dwell = {"mean_dwell": {0: 4.0, 2: float("nan")}, "events": {(0, 2): 3, (2, 0): 2}}
    assert tool.hmm_dwell(dwell, 3, "viterbi", "_ref") == {"mean_dwell_ref": [4.0, None, None], "n_transitions_ref": 5.0,
                                                           "hidden_path_ref": "viterbi"}


def test_the_benchmark_lists_its_rows():
    import tools_bench_hmm
    import tools_bench_hmm_viterbi as bench
    rows = bench.rows()
    assert rows == tools_bench_hmm.rows() and len(rows) == 2 * 3 * 2 * 3 and {r["n"] for r in rows} == {100_000, 819_200}
    assert {(r["n_traj"], r["lag"]) for r in rows} == {(80, 1), (80, 10), (1, 1)}
    assert {r["m"] for r in rows} == {2, 4, 8} and {r["K"] for r in rows} == {64, 1024}
    assert len(bench.STAGES) == 7
    a = bench.build_parser().parse_args(["--rows", "0,5", "--windows", "3", "--no-baselines"])
    assert a.rows == [0, 5] and a.windows == 3 and a.no_baselines
    # the host baseline is the textbook recursion
    la, lb, lp = vc.exact_parameters(3, 5)
    obs = np.random.default_rng(0).integers(0, 5, 300)
    path, logprob = bench.numpy_viterbi(obs, la, lb, lp)
    want = vc.sequential(obs, la, lb, lp, np.float64)
    assert np.array_equal(path, want[0]) and logprob == want[1]
