"""dff_hmm_viterbi on the GPU (csrc/dff_hmm_viterbi.hip) and HiddenMarkovModel.viterbi / HmmEvaluator(path="viterbi") on top of
it.  tests/viterbi_cases.py holds the log-parameters, the long-double truth (the textbook recursion, every chain on its own),
the score of a path, the measure E (how far a path's score falls short of the optimum, and how far chain_logprob is from it, in
units of 2^-52 |optimum|) and its bar: 8 x the larger of the two numpy E's on the same case (the sequential recursion in fp64, the
chunked statement in fp64), floored at 8 units.  The kernel is never its own reference.

The shapes are those of tests/test_hmm.py, the smallest at which the kernels can go wrong: with C = dff_hmm_chunk(), chains of 0,
1, 2, C - 1, C, C + 1, 2 C + 1 and 20 C frames in one call, empty trajectories among them, lags 1, 3 and 7 (one trajectory shorter
than the lag), m in {1, 2, 3, 8} (every padded width), K in {1, 5, 1024}.  Every case prints its E per output.

MEASURED on the MI355X, worst E over the cases of tests 1 and 2, kernel (worst of the sequential fp64 recursion / of the chunked
numpy statement), in units -- every bar is 8 x the larger numpy E of its own case, 8 units or more:
  path          0.00 (0.00 / 0.00)    every decoded path scores the long-double optimum, on all 17 + 4 cases
  chain_logprob 50.3 (316 / 50.3)     a sum of up to 2 560 rounded terms; the kernel has the chunked statement's bits
On integer log-parameters (test 1) path and chain_logprob equal the sequential recursion bit for bit.  m = 1 with general
parameters: a chain of 257 frames 8.63 (numpy's sequential sum 31.1), of 2 560 frames 3.65 (4.89); chains of one chunk and all
chains with dyadic parameters equal numpy's sum bit for bit.  The file takes 7 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hmm_cases as hc
import viterbi_cases as vc
from oracle import msm as oracle
from oracle.frames import synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from standins import HostViterbi
from support import B, dev, ev, hmm_chunk, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

ids = lambda c: "m%d-K%d-lag%d%s" % (c[0], c[1], c[2], "-disjoint" if c[3] else "")     # noqa: E731


def viterbi(labels, lengths, lag, la, lb, lp, chain_order=False, chain_logprob=True, ws_fill=0xFF):
    """one call -> host dict: path, chain_logprob, status"""
    lab = to_dev(np.array(labels, np.int32))
    m, K = lb.shape
    ws = torch.full((max(B().hmm_viterbi_workspace_bytes(len(labels), lengths, lag, m, K), 8),), ws_fill, dtype=torch.uint8, device="cuda")
    res = B().hmm_viterbi(lab, lengths, lag, to_dev(la), to_dev(lb), to_dev(lp), chain_order=chain_order, chain_logprob=chain_logprob,
                          workspace=ws)
    return {"path": res["path"].cpu().numpy(), "status": int(res["status"].cpu()),
            "chain_logprob": res["chain_logprob"].cpu().numpy() if chain_logprob else None}


def call_ref(ref, **kw):
    return viterbi(ref["labels"], ref["lengths"], ref["lag"], ref["la"], ref["lb"], ref["lp"], **kw)


def assert_within_bars(got, ref, what):
    bars = vc.bars(ref)
    worst = {"path": vc.measure_path(got["path"], ref), "chain_logprob": vc.measure_logprob(got["chain_logprob"], ref)}
    print(f"[viterbi] {what}: " + ", ".join(f"{k} E {worst[k]:.2f} (seq {ref['e_seq'][k]:.2f}, chunked {ref['e_chunked'][k]:.2f})"
                                             for k in vc.OUTPUTS))
    for k in vc.OUTPUTS:
        assert worst[k] <= bars[k], (what, k, worst[k], bars[k])


# ---------------------------------------------------------------- 1. exact inputs: the textbook recursion, bit for bit
@pytest.mark.parametrize("case", hc.CASES, ids=ids)
def test_integer_log_parameters_give_the_sequential_path_bit_for_bit(case, dev):
    ref = vc.exact_reference(*case, hmm_chunk())
    assert (ref["labels"] < 0).any() and np.isfinite(ref["sequential"][1]).all()        # missing observations; no impossible chain
    got = call_ref(ref)
    assert got["status"] == 0 and got["path"].dtype == np.int32
    wrong = np.flatnonzero(got["path"] != ref["sequential"][0])
    assert wrong.size == 0, (ids(case), wrong[:10])
    assert same_bits(got["chain_logprob"], ref["sequential"][1])
    empty = [i for i, c in enumerate(hc.chains(ref["lengths"], ref["lag"])) if len(c) == 0]
    assert (got["chain_logprob"][empty] == 0.0).all()               # a chain without a frame: log-probability 0


# ---------------------------------------------------------------- 2. general inputs: the chunked statement's bits, under the bar
@pytest.mark.parametrize("case", list(hc.CASES) + [(3, 5, 3, False, True), (8, 1024, 1, False, True), (2, 5, 1, True, True),
                                                   (8, 1024, 7, True, True)],
                         ids=lambda c: ids(c) + ("-missing" if len(c) > 4 else ""))
def test_general_inputs_sit_on_the_chunked_statement_and_under_the_bar(case, dev):
    ref = vc.reference(*case[:4], hmm_chunk(), missing=len(case) > 4)
    got = call_ref(ref)
    assert got["status"] == 0 and got["path"].min(initial=0) >= 0 and got["path"].max(initial=0) < case[0]
    assert not np.isnan(got["chain_logprob"]).any()
    assert_within_bars(got, ref, ids(case) + (" missing" if len(case) > 4 else ""))
    wrong = np.flatnonzero(got["path"] != ref["chunked"][0])
    assert wrong.size == 0, (ids(case), wrong[:10])                 # additions and compares in a stated order: the bits are determined
    assert same_bits(got["chain_logprob"], ref["chunked"][1])


# ---------------------------------------------------------------- 3. status and precedence
def test_status_and_precedence(dev):
    m, K, lag, Cn = 2, 5, 1, hmm_chunk()
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, False, Cn)
    la, lb, lp = vc.log_model(A, B_, p0)
    assert viterbi(labels, lengths, lag, la, lb, lp)["status"] == 0

    def refused(r, status):
        return r["status"] == status and (r["path"] == -1).all() and np.isnan(r["chain_logprob"]).all()
    over = labels.copy()
    over[len(over) // 2] = K
    for bad in (np.nan, np.inf):
        for which in range(3):
            par = [la.copy(), lb.copy(), lp.copy()]
            par[which].flat[-1] = bad
            assert refused(viterbi(labels, lengths, lag, *par), 1), (bad, which)
            assert refused(viterbi(over, lengths, lag, *par), 1), (bad, which)                     # 1 wins over 3
    assert refused(viterbi(over, lengths, lag, la, lb, lp), 3)
    # a label whose lb column is all -inf: no state emits it
    dead = lb.copy()
    dead[:, 3] = -np.inf
    with3 = labels.copy()
    with3[7] = 3
    assert refused(viterbi(with3, lengths, lag, la, dead, lp), 2)
    both = with3.copy()
    both[len(both) // 2] = K
    assert refused(viterbi(both, lengths, lag, la, dead, lp), 3)                                   # 3 wins over 2
    # -inf parameters alone are no failure: an impossible transition and an impossible emission that the path avoids
    la2, lb2 = la.copy(), lb.copy()
    la2[0, 1] = -np.inf
    lb2[1, 2] = -np.inf
    r = viterbi(labels, lengths, lag, la2, lb2, lp)
    assert r["status"] == 0 and (r["path"] >= 0).all() and np.isfinite(r["chain_logprob"][[len(c) > 0 for c in hc.chains(lengths, lag)]]).all()
    traj = np.repeat(np.arange(len(lengths)), lengths)
    assert not ((r["path"][:-1] == 0) & (r["path"][1:] == 1) & (traj[:-1] == traj[1:])).any()     # no 0 -> 1 step inside a trajectory
    assert not ((r["path"] == 1) & (labels == 2)).any()
    empty = viterbi(np.zeros(0, np.int32), [0, 0], 2, la, lb, lp)
    assert empty["status"] == 0 and empty["path"].shape == (0,) and (empty["chain_logprob"] == 0.0).all()


# ---------------------------------------------------------------- 4. bit identities
def test_the_call_repeats_itself_on_any_workspace(dev):
    ref = vc.reference(3, 5, 7, False, hmm_chunk())
    a, b, c = call_ref(ref), call_ref(ref), call_ref(ref, ws_fill=0x00)
    for k in ("path", "chain_logprob"):
        assert same_bits(a[k], b[k]) and same_bits(a[k], c[k]), k
    d = call_ref(ref, chain_logprob=False)
    assert d["status"] == 0 and same_bits(a["path"], d["path"])     # the log-probabilities in the workspace: the same path


def test_chain_order_is_the_stated_permutation(dev):
    for case in ((3, 5, 7, False), (8, 1024, 3, True), (2, 5, 1, False)):
        ref = vc.reference(*case, hmm_chunk())
        frame, chain = call_ref(ref), call_ref(ref, chain_order=True)
        assert same_bits(chain["path"], frame["path"][vc.chain_order(ref["lengths"], ref["lag"])])
        assert same_bits(chain["chain_logprob"], frame["chain_logprob"])


def test_a_chain_does_not_depend_on_the_other_chains(dev):
    m, K, lag, Cn = 3, 5, 3, hmm_chunk()
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, False, Cn)
    par = vc.log_model(A, B_, p0)
    base = viterbi(labels, lengths, lag, *par)
    perm = np.random.default_rng(2).permutation(len(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    lab2 = np.concatenate([labels[starts[r]:starts[r + 1]] for r in perm] + [np.zeros(0, np.int32)])
    got = viterbi(lab2, [lengths[r] for r in perm], lag, *par)
    o = 0
    for i, r in enumerate(perm):
        assert same_bits(got["chain_logprob"][i * lag:(i + 1) * lag], base["chain_logprob"][r * lag:(r + 1) * lag]), r
        assert same_bits(got["path"][o:o + lengths[r]], base["path"][starts[r]:starts[r + 1]]), r
        o += lengths[r]


def test_lag_tau_is_lag_one_on_the_strided_sub_trajectories(dev):
    m, K, lag, Cn = 8, 5, 7, hmm_chunk()
    par = vc.log_model(*hc.model(m, K))
    n = lag * (2 * Cn + 1) + 3
    labels = np.random.default_rng(9).integers(0, K, n).astype(np.int32)
    whole = viterbi(labels, [n], lag, *par)
    subs = [labels[f::lag] for f in range(lag)]
    split = viterbi(np.concatenate(subs), [len(s) for s in subs], 1, *par)
    assert whole["status"] == split["status"] == 0 and same_bits(whole["chain_logprob"], split["chain_logprob"])
    o = 0
    for f, s in enumerate(subs):
        assert same_bits(whole["path"][f::lag], split["path"][o:o + len(s)]), f
        o += len(s)


# ---------------------------------------------------------------- 5. closed forms
def sequential_sum(lab, lengths, la, lb, lp, dtype=np.float64):
    """m = 1: every chain's log-probability as the plain sum, in the recursion's order of additions"""
    la, lb, lp = (np.asarray(x, dtype) for x in (la, lb, lp))
    want, o = [], 0
    for n in lengths:
        v = dtype(0)
        for t in range(n):
            le = lb[0, lab[o + t]] if lab[o + t] >= 0 else dtype(0)
            v = lp[0] + le if t == 0 else (v + la[0, 0]) + le
        want.append(v)
        o += n
    return np.array(want, dtype)


def test_one_hidden_state_has_a_closed_form(dev):
    """m = 1: the path is all 0 and the log-probability is numpy's sequential sum, bit for bit -- wherever the call adds in that
    order or the order cannot matter: chains of at most one chunk with any parameters, and chains of any length with dyadic
    parameters (every partial sum exact).  A longer chain with general parameters enters its later chunks with the carried
    delta, (lp + le_0) + P_0 + P_1 ..., the same terms in another association: there the value is held to the long-double sum
    under the rule of the other tests, and its distance to numpy's sum is printed."""
    Cn = hmm_chunk()
    lengths = [2 * Cn + 1, 0, 1, Cn, 20 * Cn]
    K = 7
    rng = np.random.default_rng(3)
    lab = rng.integers(0, K, sum(lengths)).astype(np.int32)
    lab[5] = -1
    one = np.array([len_ <= Cn for len_ in lengths])
    # general parameters
    lb = np.log(rng.uniform(0.05, 1.0, (1, K)))
    la, lp = np.array([[np.log(0.9)]]), np.array([np.log(0.7)])
    got = viterbi(lab, lengths, 1, la, lb, lp)
    assert got["status"] == 0 and (got["path"] == 0).all()
    want, truth = sequential_sum(lab, lengths, la, lb, lp), sequential_sum(lab, lengths, la, lb, lp, np.longdouble)
    assert same_bits(got["chain_logprob"][one], want[one])
    for i in np.flatnonzero(~one):
        unit = vc.EPS * abs(truth[i])
        e, e_np = float(abs(got["chain_logprob"][i] - truth[i]) / unit), float(abs(want[i] - truth[i]) / unit)
        print(f"[viterbi] m = 1, chain of {lengths[i]} frames: chain_logprob E {e:.2f} (numpy's sequential sum {e_np:.2f}), "
              f"{abs(got['chain_logprob'][i] - want[i]) / unit:.2f} units from numpy's sum")
        assert e <= vc.FACTOR * max(e_np, 1.0)
    # dyadic parameters: multiples of 1 / 8, every partial sum exact
    lb = -rng.integers(1, 40, (1, K)) / 8.0
    la, lp = np.array([[-0.125]]), np.array([-0.75])
    got = viterbi(lab, lengths, 1, la, lb, lp)
    assert got["status"] == 0 and (got["path"] == 0).all()
    assert same_bits(got["chain_logprob"], sequential_sum(lab, lengths, la, lb, lp))


@pytest.mark.parametrize("case", [(3, 5, 1), (8, 1024, 3), (2, 5, 7)], ids=lambda c: "m%d-K%d-lag%d" % c)
def test_disjoint_emissions_name_the_hidden_state(case, dev):
    m, K, lag = case
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, True, hmm_chunk())
    lab = hc.with_missing(labels, lengths, lag, hmm_chunk(), seed=1)
    got = viterbi(lab, lengths, lag, *vc.log_model(A, B_, p0))
    assert got["status"] == 0
    seen = lab >= 0
    assert (got["path"][seen] == lab[seen] % m).all() and (got["path"] >= 0).all() and (got["path"] < m).all()


def test_the_debug_stages_stop_where_they_say(dev):
    """dff_debug_hmm_viterbi_stages(s) stops the call after the parameters, the chunk products, the forward carries, the apply
    pass, the backward carries, the backtrack (s = 1 .. 6) and skips the finish launch.  Seen from outside: the forward carries
    write the chain_logprob of the chains without a frame, the apply pass that of the others, the backtrack writes the path, and
    only the finish launch writes the status.  The outputs hold a sentinel that no result equals (a log-probability is <= 0, a
    state < 8).  After the reset the call is the whole call again."""
    m, K, lag, Cn = 3, 5, 2, hmm_chunk()
    lengths = np.array([3 * Cn + 5, 0, 7], np.int64)
    n = int(lengths.sum())
    A, B_, p0 = hc.model(m, K)
    labels = hc.simulate(A, B_, p0, lengths, seed=6)
    la, lb, lp = vc.log_model(A, B_, p0)
    before = viterbi(labels, lengths, lag, la, lb, lp)
    par = [to_dev(x) for x in (la, lb, lp)]
    lab = to_dev(labels)
    ws = torch.empty(B().hmm_viterbi_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    empty = np.array([len(c) == 0 for c in hc.chains(lengths.tolist(), lag)])
    assert empty.tolist() == [False, False, True, True, False, False]
    try:
        for s in range(1, 7):
            out = {"path": torch.full((n,), 0x7b7b7b7b, dtype=torch.int32, device="cuda"),
                   "chain": torch.full((3 * lag,), 123.0, dtype=torch.float64, device="cuda"),
                   "status": torch.full((1,), 0x7b7b7b7b, dtype=torch.int32, device="cuda")}
            B().debug_hmm_viterbi_stages(s)
            raw("dff_hmm_viterbi", 0, ptr(lab), n, lengths.ctypes.data_as(C.c_void_p), 3, lag, ptr(par[0]), ptr(par[1]), ptr(par[2]), m, K,
                ptr(out["path"]), 0, ptr(out["chain"]), ptr(out["status"]), ptr(ws), ws.numel(), stream_of(lab))
            kept = {k: (v == (123.0 if k == "chain" else 0x7b7b7b7b)).cpu().numpy() for k, v in out.items()}
            assert kept["status"].all(), s
            assert kept["chain"][empty].all() if s < 3 else not kept["chain"][empty].any(), s
            assert kept["chain"][~empty].all() if s < 4 else not kept["chain"][~empty].any(), s
            assert kept["path"].all() if s < 6 else not kept["path"].any(), s
    finally:
        B().debug_hmm_viterbi_stages(0)
    after = viterbi(labels, lengths, lag, la, lb, lp)
    assert after["status"] == before["status"] == 0
    assert same_bits(after["path"], before["path"]) and same_bits(after["chain_logprob"], before["chain_logprob"])


# ---------------------------------------------------------------- 6. stream order
def viterbi_spec():
    """three trajectories (one empty) at lag 2, every output written; poison: constant labels and NaN parameters"""
    m, K, lag, Cn = 3, 5, 2, hmm_chunk()
    la, lb, lp = vc.log_model(*hc.model(m, K))
    lengths = np.array([2 * Cn + 5, 0, 3 * Cn], np.int64)
    n = int(lengths.sum())
    labels = np.random.default_rng(4).integers(0, K, n).astype(np.int32)
    ws = torch.empty(B().hmm_viterbi_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    return Spec("dff_hmm_viterbi", {"labels": (to_dev(labels), 0), "trans": (to_dev(la), nan), "emit": (to_dev(lb), nan), "init": (to_dev(lp), nan)},
                {"path": ((n,), torch.int32), "chain": ((3 * lag,), torch.float64), "status": ((1,), torch.int32)},
                lambda _, b: raw("dff_hmm_viterbi", 0, ptr(b["labels"]), n, lengths.ctypes.data_as(C.c_void_p), 3, lag, ptr(b["trans"]),
                                 ptr(b["emit"]), ptr(b["init"]), m, K, ptr(b["path"]), 0, ptr(b["chain"]), ptr(b["status"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["labels"])),
                work={"ws": ws})


def test_the_call_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(viterbi_spec(), gate, side)
    assert int(ref["status"][0]) == 0 and int(ref["path"].min()) >= 0 and int(ref["path"].max()) < 3
    assert bool(torch.isfinite(ref["chain"][[0, 1, 4, 5]]).all()) and bool((ref["chain"][[2, 3]] == 0).all())


def test_fence():
    """The memory contract (tests/fence.py): all eight buffers in one arena; the sections of the workspace (trajectory table,
    padded log-parameters, chunk products, entering deltas, back maps, end states, back-pointer words, chain results) end at
    exactly dff_hmm_viterbi_workspace_bytes."""
    spec = viterbi_spec()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


# ---------------------------------------------------------------- 7. the Python layer
def test_the_model_decodes_what_the_stand_in_decodes(dev, monkeypatch):
    A = np.array([[0.96, 0.03, 0.01], [0.02, 0.95, 0.03], [0.01, 0.04, 0.95]])
    B_ = hc.model(3, 30, seed=1)[1]
    p0 = np.array([0.5, 0.3, 0.2])
    lengths = [700, 0, 333, 500]
    labels = hc.simulate(A, B_, p0, lengths, seed=8)
    model = ev().HiddenMarkovModel(3, 2, reversible=False, accuracy=1e-12, max_iter=3).fit(labels, lengths, 30, initial=(A, B_, p0))
    got = {o: model.viterbi(labels, lengths, order=o, return_log_probabilities=True) for o in ("frame", "chain")}
    monkeypatch.setattr(ev(), "hmm_viterbi_solver", HostViterbi)
    for o in ("frame", "chain"):
        path, cl = model.viterbi(labels, lengths, order=o, return_log_probabilities=True)
        assert got[o][0].dtype == torch.int32 and got[o][0].is_cuda and same_bits(got[o][0].cpu().numpy(), path.numpy()), o
        assert same_bits(np.asarray(got[o][1]), np.asarray(cl)), o
    assert same_bits(got["chain"][0].cpu().numpy(), got["frame"][0].cpu().numpy()[vc.chain_order(lengths, 2)])
    assert same_bits(np.asarray(ev().hmm_chain_lengths(lengths, 2)), np.array([len(c) for c in hc.chains(lengths, 2)], np.int64))


def test_the_evaluator_with_viterbi_paths(dev):
    beads, wells = 10, np.array([[0.97, 0.03], [0.05, 0.95]])
    base = synth_chain_frames(2, beads, 91).astype(np.float64)
    paths = oracle.jump_process(wells, 8, 600, 11)
    x = (base[paths.reshape(-1)] + 0.05 * np.random.default_rng(12).standard_normal((paths.size, beads, 3))).astype(np.float32)
    F = B().struct_tic_num_features(beads)
    rng = np.random.default_rng(17)
    tica = (rng.uniform(0.0, 10.0, F), rng.uniform(-0.1, 0.1, (F, 2)))
    lengths = [600] * 8

    def make(**kw):
        return ev().HmmEvaluator("chignolin", tica, n_microstates=8, n_hidden=2, lagtime=2, frame_time=0.5, **kw)
    v = make(path="viterbi")
    res = v.eval(x, lengths)
    assert set(res) == set(ev().HmmEvaluator.KEYS)
    hidden = v.hidden["samples"]
    assert hidden.shape == (4800,) and hidden.dtype == np.int32 and set(np.unique(hidden)) <= {0, 1}
    model = v.models["samples"]
    assert same_bits(hidden, model.viterbi(v.labels["samples"], lengths).cpu().numpy())
    # dwells are taken inside the chains: 16 chains of 300 frames, times in units of frame_time * lagtime
    chain_path = model.viterbi(v.labels["samples"], lengths, order="chain")
    want = ev().dwell_summary(ev().label_runs(chain_path, ev().hmm_chain_lengths(lengths, 2)), 0.5 * 2)
    np.testing.assert_equal(v.dwell["samples"], want)
    assert want["total_frames"] == 4800
    # the default and path="posterior" are the evaluator as it was
    a, b = make(), make(path="posterior")
    ra, rb = a.eval(x, lengths), b.eval(x, lengths)
    np.testing.assert_equal(ra, rb)
    np.testing.assert_equal(ra, res)                                # the same fit: only .hidden and .dwell differ
    np.testing.assert_equal(a.dwell["samples"], b.dwell["samples"])
    assert same_bits(a.hidden["samples"], b.hidden["samples"])
    assert same_bits(a.hidden["samples"], a.models["samples"].hidden_states(a.labels["samples"], lengths).cpu().numpy())
    print(f"[viterbi] evaluator: {int((hidden != a.hidden['samples']).sum())} of 4800 frames differ between the Viterbi path and the posterior "
          f"argmax; events {sum(want['events'].values())} (inside chains) against {sum(a.dwell['samples']['events'].values())} (interleaved)")
