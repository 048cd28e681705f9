"""dff_hmm_estep on the GPU (csrc/dff_hmm.hip) and HiddenMarkovModel / HmmEvaluator on top of it.  tests/hmm_cases.py holds the
models, the labels, the long-double truth (a sequential forward-backward), the measure E (distance to the truth in units of
2^-52 x the truth's largest magnitude; 2^-52 |l| for the log-likelihoods) and its bar: 8 x the larger of the two numpy E's on the
same case (the sequential recursion in fp64, the chunked formulation in fp64), floored at 8 units.  The kernel is never its own
reference.

The shapes are the smallest at which the kernels can go wrong: with C = dff_hmm_chunk(), chains of 0, 1, 2, C - 1, C, C + 1,
2 C + 1 and 20 C frames in one call, empty trajectories among them, lags 1, 3 and 7 (one trajectory shorter than the lag), m in
{1, 2, 3, 8} (every padded width), K in {1, 5, 1024}.  Every case prints its E per output.

MEASURED on the MI355X, worst E over the cases of tests 1 and 2, kernel (worst of the sequential fp64 recursion / of the chunked
numpy statement), in units -- every bar is 8 x the larger numpy E of its own case, 8 units or more:
  loglik        1.49 (94.8 / 1.03)
  chain_loglik  7.17 (122 / 7.17)
  xi            8.42 (74.9 / 8.42)
  gamma0        3.42 (3.42 / 3.42)
  gamma_sym     51.5 (114 / 51.5)     K = 1: one accumulator takes every frame
  post          3.33 (1.65 / 3.33)
m = 1, loglik against the closed form: 0.31 (numpy's sum of logs 0.31).  Five iterations of Baum-Welch against the loop with a
long-double E-step: log-likelihoods 0.82 (the numpy loop 0.82), A 0.54 (0.54), B 2.31 (1.85), p0 2.85 (2.28).  The kernel sits
on the chunked numpy statement.  The file takes 7 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hmm_cases as hc
from oracle import msm as oracle
from oracle.frames import synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, hmm_chunk, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

ids = lambda c: "m%d-K%d-lag%d%s" % (c[0], c[1], c[2], "-disjoint" if c[3] else "")     # noqa: E731


def estep(labels, lengths, lag, A, B_, p0, post=True, chain_loglik=True, ws_fill=0xFF):
    """one call -> host dict: stats (packed), its parts, chain_loglik, post, status"""
    lab = to_dev(np.array(labels, np.int32))
    m, K = B_.shape
    ws = torch.full((max(B().hmm_workspace_bytes(len(labels), lengths, lag, m, K), 8),), ws_fill, dtype=torch.uint8, device="cuda")
    res = B().hmm_estep(lab, lengths, lag, to_dev(A), to_dev(B_), to_dev(p0), chain_loglik=chain_loglik, post=post, workspace=ws)
    out = {"stats": res["stats"].cpu().numpy(), "status": int(res["status"].cpu()),
           "chain_loglik": res["chain_loglik"].cpu().numpy() if chain_loglik else None,
           "post": res["post"].cpu().numpy() if post else None}
    out.update(hc.unpack(out["stats"], m, K))
    return out


def assert_within_bars(got, ref, what):
    bars = hc.bars(ref)
    worst = {}
    for k in hc.OUTPUTS:
        worst[k] = hc.measure(got[k], ref["truth"][k], k)
    print(f"[hmm] {what}: " + ", ".join(f"{k} E {worst[k]:.2f} (seq {ref['e_seq'][k]:.2f}, chunked {ref['e_chunked'][k]:.2f})"
                                         for k in hc.OUTPUTS))
    for k in hc.OUTPUTS:
        assert worst[k] <= bars[k], (what, k, worst[k], bars[k])
    return worst


# ---------------------------------------------------------------- 1. every output under its bar
@pytest.mark.parametrize("case", hc.CASES, ids=ids)
def test_every_output_is_as_close_to_the_truth_as_numpy(case, dev):
    ref = hc.reference(*case, hmm_chunk())
    got = estep(ref["labels"], ref["lengths"], ref["lag"], ref["A"], ref["B"], ref["p0"])
    assert got["status"] == 0 and not np.isnan(got["stats"]).any() and not np.isnan(got["post"]).any()
    assert not np.isnan(got["chain_loglik"]).any()
    assert_within_bars(got, ref, ids(case))
    empty = [i for i, c in enumerate(hc.chains(ref["lengths"], ref["lag"])) if len(c) == 0]
    assert (got["chain_loglik"][empty] == 0.0).all()                # a chain without a frame contributes nothing


# ---------------------------------------------------------------- 2. missing observations, exact zeros
@pytest.mark.parametrize("case", [(3, 5, 3, False), (8, 1024, 1, False), (2, 5, 1, True), (8, 1024, 7, True)], ids=ids)
def test_missing_observations_follow_the_oracles_rule(case, dev):
    m, K, lag, disjoint = case
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, disjoint, hmm_chunk())
    lab = hc.with_missing(labels, lengths, lag, hmm_chunk(), seed=m)
    ref = hc.reference_of(lab, lengths, lag, A, B_, p0, hmm_chunk())
    got = estep(lab, lengths, lag, A, B_, p0)
    assert got["status"] == 0 and not np.isnan(got["stats"]).any() and not np.isnan(got["post"]).any()
    assert_within_bars(got, ref, "missing " + ids(case))
    assert abs(got["gamma_sym"].sum() - int((lab >= 0).sum())) < 1e-9 * len(lab)


# ---------------------------------------------------------------- 3. closed forms
def test_one_hidden_state_has_a_closed_form(dev):
    Cn = hmm_chunk()
    lengths = [2 * Cn + 1, 0, 1, Cn]
    K = 7
    rng = np.random.default_rng(3)
    lab = rng.integers(0, K, sum(lengths)).astype(np.int32)
    B_ = rng.uniform(0.05, 1.0, (1, K))
    got = estep(lab, lengths, 1, np.ones((1, 1)), B_, np.ones(1))
    assert got["status"] == 0
    assert (got["post"] == 1.0).all() and same_bits(got["gamma_sym"][0], np.bincount(lab, minlength=K).astype(np.float64))
    assert got["gamma0"][0] == 3.0 and abs(got["xi"][0, 0] - (sum(lengths) - 3)) < 1e-12 * sum(lengths)
    logs = np.log(np.asarray(B_[0], np.longdouble))[lab]
    truth, host = logs.sum(), float(np.log(B_[0])[lab].sum())
    e, e_np = hc.measure(got["loglik"], truth, "loglik"), hc.measure(host, truth, "loglik")
    print(f"[hmm] m = 1: loglik E {e:.2f} (numpy's sum of logs {e_np:.2f})")
    assert e <= hc.FACTOR * max(e_np, 1.0)


def test_identical_emission_rows_give_back_the_propagated_prior(dev):
    Cn = hmm_chunk()
    A = np.array([[0.875, 0.125], [0.25, 0.75]])                    # dyadic: the rows sum to 1 exactly, also in long double
    p0 = np.array([0.25, 0.75])
    B_ = np.tile(np.random.default_rng(5).uniform(0.1, 1.0, (1, 6)), (2, 1))
    lengths = [2 * Cn + 3]
    lab = np.random.default_rng(6).integers(0, 6, lengths[0]).astype(np.int32)
    ref = hc.reference_of(lab, lengths, 1, A, B_, p0, Cn)
    prior = np.empty((lengths[0], 2), np.longdouble)
    v = np.asarray(p0, np.longdouble)
    for t in range(lengths[0]):
        prior[t] = v
        v = v @ np.asarray(A, np.longdouble)
    assert np.abs(ref["truth"]["post"] - prior).max() < 1e-16        # the observations say nothing about the hidden state
    got = estep(lab, lengths, 1, A, B_, p0)
    assert got["status"] == 0
    assert_within_bars(got, ref, "identical rows")


# ---------------------------------------------------------------- 4. bit identities
def test_the_call_repeats_itself_on_any_workspace(dev):
    ref = hc.reference(3, 5, 7, False, hmm_chunk())
    args = (ref["labels"], ref["lengths"], ref["lag"], ref["A"], ref["B"], ref["p0"])
    a, b, c = estep(*args), estep(*args), estep(*args, ws_fill=0x00)
    for k in ("stats", "chain_loglik", "post"):
        assert same_bits(a[k], b[k]) and same_bits(a[k], c[k]), k    # 0xFF bytes are NaNs: the workspace's contents are irrelevant
    d = estep(*args, post=False, chain_loglik=False)
    assert d["status"] == 0 and same_bits(a["stats"], d["stats"])    # the posteriors in the workspace: the same stats


def test_a_chain_does_not_depend_on_the_other_chains(dev):
    m, K, lag, Cn = 3, 5, 3, hmm_chunk()
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, False, Cn)
    base = estep(labels, lengths, lag, A, B_, p0)
    perm = np.random.default_rng(2).permutation(len(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    lab2 = np.concatenate([labels[starts[r]:starts[r + 1]] for r in perm] + [np.zeros(0, np.int32)])
    got = estep(lab2, [lengths[r] for r in perm], lag, A, B_, p0)
    o = 0
    for i, r in enumerate(perm):
        assert same_bits(got["chain_loglik"][i * lag:(i + 1) * lag], base["chain_loglik"][r * lag:(r + 1) * lag]), r
        assert same_bits(got["post"][o:o + lengths[r]], base["post"][starts[r]:starts[r + 1]]), r
        o += lengths[r]


def test_lag_tau_is_lag_one_on_the_strided_sub_trajectories(dev):
    m, K, lag, Cn = 8, 5, 7, hmm_chunk()
    A, B_, p0 = hc.model(m, K)
    n = lag * (2 * Cn + 1) + 3
    labels = np.random.default_rng(9).integers(0, K, n).astype(np.int32)
    whole = estep(labels, [n], lag, A, B_, p0)
    subs = [labels[f::lag] for f in range(lag)]
    split = estep(np.concatenate(subs), [len(s) for s in subs], 1, A, B_, p0)
    assert same_bits(whole["chain_loglik"], split["chain_loglik"])
    o = 0
    for f, s in enumerate(subs):
        assert same_bits(whole["post"][f::lag], split["post"][o:o + len(s)]), f
        o += len(s)


# ---------------------------------------------------------------- 5. status
def test_status_and_nan_outputs(dev):
    m, K, lag, Cn = 2, 5, 1, hmm_chunk()
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, False, Cn)
    assert estep(labels, lengths, lag, A, B_, p0)["status"] == 0

    def all_nan(r):
        return np.isnan(r["stats"]).all() and np.isnan(r["chain_loglik"]).all() and np.isnan(r["post"]).all()
    for bad in (np.nan, -0.25):
        for which in range(3):
            par = [A.copy(), B_.copy(), p0.copy()]
            par[which].flat[-1] = bad
            r = estep(labels, lengths, lag, *par)
            assert r["status"] == 1 and all_nan(r), (bad, which)
    over = labels.copy()
    over[len(over) // 2] = K
    r = estep(over, lengths, lag, A, B_, p0)
    assert r["status"] == 3 and all_nan(r)
    # a sequence the model cannot emit: only the chain of the second trajectory is impossible (0 -> 1 under A = 1)
    Bd = np.array([[0.5, 0.0, 0.5, 0.0], [0.0, 0.5, 0.0, 0.5]])
    good = np.array([0, 2, 0, 2, 2], np.int32)
    r = estep(np.concatenate([good, [0, 1, 0], good]), [5, 3, 5], 1, np.eye(2), Bd, np.array([0.5, 0.5]))
    assert r["status"] == 2 and all_nan(r)
    r = estep(np.concatenate([good, good]), [5, 5], 1, np.eye(2), Bd, np.array([0.5, 0.5]))
    assert r["status"] == 0 and not np.isnan(r["stats"]).any() and not np.isnan(r["post"]).any()
    assert np.abs(r["post"][:, 0] - 1.0).max() < 1e-15 and abs(r["xi"][0, 0] - 8.0) < 1e-14 and r["xi"][1, 1] == 0.0
    empty = estep(np.zeros(0, np.int32), [0, 0], 2, A, B_, p0)
    assert empty["status"] == 0 and (empty["stats"] == 0.0).all() and (empty["chain_loglik"] == 0.0).all()


def test_the_debug_stages_stop_where_they_say(dev):
    """dff_debug_hmm_stages(s) stops the call after the parameters, the chunk products, the carries, the apply pass, the emission
    counts (s = 1 .. 5) and skips the finish launch.  Seen from outside: the carries write chain_loglik, the apply pass writes
    post, and only the last two launches write stats and status.  The outputs hold a sentinel that no result equals (a
    log-likelihood is <= 0, a posterior <= 1).  After the reset the call is the whole call again."""
    m, K, lag, Cn = 3, 5, 2, hmm_chunk()
    lengths = np.array([3 * Cn + 5, 0, 7], np.int64)
    n = int(lengths.sum())
    A, B_, p0 = hc.model(m, K)
    labels = hc.simulate(A, B_, p0, lengths, seed=6)
    before = estep(labels, lengths, lag, A, B_, p0)
    par = [to_dev(x) for x in (A, B_, p0)]
    lab = to_dev(labels)
    ws = torch.empty(B().hmm_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    try:
        for s in range(1, 6):
            out = {"stats": torch.full((1 + m * m + m + m * K,), 123.0, dtype=torch.float64, device="cuda"),
                   "chain": torch.full((3 * lag,), 123.0, dtype=torch.float64, device="cuda"),
                   "post": torch.full((n, m), 123.0, dtype=torch.float64, device="cuda"),
                   "status": torch.full((1,), 0x7b7b7b7b, dtype=torch.int32, device="cuda")}
            B().debug_hmm_stages(s)
            raw("dff_hmm_estep", 0, ptr(lab), n, lengths.ctypes.data_as(C.c_void_p), 3, lag, ptr(par[0]), ptr(par[1]), ptr(par[2]), m, K,
                ptr(out["stats"]), ptr(out["chain"]), ptr(out["post"]), ptr(out["status"]), ptr(ws), ws.numel(), stream_of(lab))
            kept = {k: (v == (0x7b7b7b7b if k == "status" else 123.0)).cpu().numpy() for k, v in out.items()}
            assert kept["stats"].all() and kept["status"].all(), s
            assert kept["chain"].all() if s < 3 else not kept["chain"].any(), s
            assert kept["post"].all() if s < 4 else not kept["post"].any(), s
    finally:
        B().debug_hmm_stages(0)
    after = estep(labels, lengths, lag, A, B_, p0)
    assert after["status"] == before["status"] == 0
    for k in ("stats", "chain_loglik", "post"):
        assert same_bits(after[k], before[k]), k


# ---------------------------------------------------------------- 6. stream order
def estep_spec():
    """three trajectories (one empty) at lag 2, every output written; poison: constant labels and NaN parameters"""
    m, K, lag, Cn = 3, 5, 2, hmm_chunk()
    A, B_, p0 = hc.model(m, K)
    lengths = np.array([2 * Cn + 5, 0, 3 * Cn], np.int64)
    n = int(lengths.sum())
    labels = np.random.default_rng(4).integers(0, K, n).astype(np.int32)
    ws = torch.empty(B().hmm_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    return Spec("dff_hmm_estep", {"labels": (to_dev(labels), 0), "trans": (to_dev(A), nan), "emit": (to_dev(B_), nan), "init": (to_dev(p0), nan)},
                {"stats": ((1 + m * m + m + m * K,), torch.float64), "chain": ((3 * lag,), torch.float64), "post": ((n, m), torch.float64),
                 "status": ((1,), torch.int32)},
                lambda _, b: raw("dff_hmm_estep", 0, ptr(b["labels"]), n, lengths.ctypes.data_as(C.c_void_p), 3, lag, ptr(b["trans"]),
                                 ptr(b["emit"]), ptr(b["init"]), m, K, ptr(b["stats"]), ptr(b["chain"]), ptr(b["post"]), ptr(b["status"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["labels"])),
                work={"ws": ws})


def test_the_call_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(estep_spec(), gate, side)
    assert int(ref["status"][0]) == 0 and bool(torch.isfinite(ref["stats"]).all()) and bool(torch.isfinite(ref["post"]).all())
    assert float((ref["post"].sum(dim=1) - 1.0).abs().max()) < 1e-12


def test_fence():
    """The memory contract (tests/fence.py): all nine buffers in one arena; the sections of the workspace (trajectory table,
    parameters, chunk products and carries, chain log-likelihoods, posteriors, emission counts) end at exactly
    dff_hmm_workspace_bytes."""
    spec = estep_spec()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


# ---------------------------------------------------------------- 7. the Python layer
class NumpyEstep:
    """the E-step behind evaluate.hmm_estep_solver on the host: the chunked formulation in fp64, or the sequential one in long double"""
    dtype = None

    def __init__(self, device):
        pass

    def __call__(self, labels, lengths, lag, A, B_, p0, want_post=False):
        lab = np.asarray(labels.cpu())
        if self.dtype is None:
            stats, cl, post, status = hc.host_estep(lab, lengths, lag, A, B_, p0, hmm_chunk())
        else:
            res = hc.sequential(lab, lengths, lag, A, B_, p0, self.dtype)
            stats, cl, post, status = hc.pack(res), np.asarray(res["chain_loglik"], np.float64), np.asarray(res["post"], np.float64), 0
        return stats, (cl if want_post else None), (torch.from_numpy(post) if want_post else None), status


class TruthEstep(NumpyEstep):
    dtype = np.longdouble


def test_five_iterations_of_baum_welch_against_the_same_loop_on_numpy(dev, monkeypatch):
    A, B_, p0 = hc.model(3, 30, seed=1)
    lengths = [500] * 12
    labels = hc.simulate(A, B_, p0, lengths, seed=8)
    rng = np.random.default_rng(12)
    start = (A, B_ * rng.uniform(0.5, 1.5, B_.shape), np.full(3, 1.0 / 3.0))
    start = (start[0], start[1] / start[1].sum(axis=1)[:, None], start[2])

    def fit():
        return ev().HiddenMarkovModel(3, 2, reversible=False, accuracy=1e-12, max_iter=5).fit(labels, lengths, 30, initial=start)
    device = fit()
    monkeypatch.setattr(ev(), "hmm_estep_solver", NumpyEstep)
    host = fit()
    monkeypatch.setattr(ev(), "hmm_estep_solver", TruthEstep)
    truth = fit()
    assert device.n_iter == host.n_iter == truth.n_iter == 5 and len(device.log_likelihoods) == 5
    assert (np.diff(device.log_likelihoods) >= 0).all()
    for name in ("log_likelihoods", "transition_matrix", "observation_probabilities", "initial_distribution"):
        t = np.asarray(getattr(truth, name), np.float64)
        unit = hc.EPS * (np.abs(t) if name == "log_likelihoods" else np.abs(t).max())
        e_dev = float((np.abs(np.asarray(getattr(device, name)) - t) / unit).max())
        e_host = float((np.abs(np.asarray(getattr(host, name)) - t) / unit).max())
        print(f"[hmm] five iterations, {name}: E {e_dev:.2f} (the numpy loop {e_host:.2f})")
        assert e_dev <= hc.FACTOR * max(e_host, 1.0), (name, e_dev, e_host)


def test_the_evaluator_on_a_two_well_jump_process(dev):
    beads, wells = 10, np.array([[0.97, 0.03], [0.05, 0.95]])
    base = synth_chain_frames(2, beads, 91).astype(np.float64)

    def frames(seed):
        paths = oracle.jump_process(wells, 20, 1500, seed)
        return (base[paths.reshape(-1)] + 0.05 * np.random.default_rng(seed + 1).standard_normal((paths.size, beads, 3))).astype(np.float32)
    F = B().struct_tic_num_features(beads)
    rng = np.random.default_rng(17)
    tica = (rng.uniform(0.0, 10.0, F), rng.uniform(-0.1, 0.1, (F, 2)))
    lengths = [1500] * 20
    e = ev().HmmEvaluator("chignolin", tica, n_microstates=8, n_hidden=2, lagtime=2, frame_time=0.5, ref_data=frames(31),
                          ref_traj_lengths=lengths)
    res = e.eval(frames(11), lengths)
    keys = set(ev().HmmEvaluator.KEYS)
    assert set(res) == keys | {k + "_ref" for k in keys} | {"log10_timescale_ratio", "log10_lifetime_ratio", "population_js"}
    flat = [v for k in res for v in (res[k] if isinstance(res[k], list) else [res[k]])]
    assert np.isfinite(flat).all()
    for suffix in ("", "_ref"):
        pops = res["hidden_populations" + suffix]
        assert len(pops) == 2 and abs(sum(pops) - 1.0) < 1e-12 and pops[0] >= pops[1]
        assert res["converged" + suffix] == 1.0 and res["samples_nonfinite" + suffix] == 0.0
    # the jump process has the stationary distribution (5 / 8, 3 / 8) and, at every lag, the timescale -1 / ln(0.92) = 12 frames
    assert abs(res["hidden_populations"][0] - 0.625) < 0.05 and abs(res["timescales"][0] / 0.5 + 1.0 / np.log(0.92)) < 3.0
    assert e.hidden["samples"].shape == (30000,) and e.dwell["samples"]["total_frames"] == 30000
    print(f"[hmm] evaluator: populations {res['hidden_populations']}, timescale {res['timescales'][0]:.2f}, lifetimes {res['lifetimes']}, "
          f"{int(res['n_iter'])} E-steps")
