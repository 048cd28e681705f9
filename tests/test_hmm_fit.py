"""dff_hmm_fit_steps on the GPU (csrc/dff_hmm_mstep.hip) and HiddenMarkovModel(m_step="device") / bootstrap_hmm on top of it.

The reference is tests/hmm_fit_cases.py: replay(), the step loop of the call, over the EXISTING dff_hmm_estep on the device plus
mstep(), the numpy statement of the M-step with every sum in the stated order.  The call must give the same BITS: the
log-likelihoods, A, B, p0, the stationary distribution and every field of the state.  The kernel is never its own reference,
and nothing here has a tolerance.

Shapes: (m, K, lag) over every padded width (2 / 4 / 8) and K in {1, 5, 64, 1024}; weakly metastable models (diagonal <= 0.9: a
reversible M-step is a few hundred sweeps at the most); chains of 0, 1, 2, C - 1, C, C + 1 and 2 C + 1 frames (hmm_cases.lengths_for)
with missing observations (hmm_cases.with_missing).

MEASURED on the MI355X: every comparison holds bit for bit; four reversible steps take 452 - 1 025 sweeps over the shapes; the
two-well fit converges after 14 E-steps and 2 955 sweeps to populations (0.612, 0.388) and a timescale of 12.5 frames, and six
resamples of it give 12.5 +- 1.0 frames after 7 - 11 E-steps each.  The file takes 3 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import hmm_cases as hc
import hmm_fit_cases as fc
from oracle import msm as oracle
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, hmm_chunk, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (2, 5, 1), (3, 5, 3), (4, 64, 1), (5, 1024, 3), (8, 1024, 7), (8, 5, 1))
STATE_FIELDS = ("n_estep", "stop", "estep_status", "flags", "last_loglik", "rev_sweeps")
TINY = 1e-300                                                       # an accuracy no pair of log-likelihoods meets


def weak(A):
    """the model's transition matrix pulled towards uniform: a diagonal of 0.86 at the most"""
    return 0.8 * A + 0.2 / len(A) if len(A) > 1 else A


def case(m, K, lag):
    labels, lengths, A, B_, p0 = hc.case_inputs(m, K, lag, False, hmm_chunk())
    return hc.with_missing(labels, lengths, lag, hmm_chunk(), seed=m), lengths, weak(A), B_, p0


def fit_steps(labels, lengths, lag, A, B_, p0, reversible, n_steps, accuracy, state=None, ws_fill=0xFF, stationary=True, pi=None,
              rev_tol=1e-12, rev_max_sweeps=1_000_000):
    """one call -> host dict: A, B, p0, loglik, pi (NaN where never written; None without the buffer), state (dict)"""
    lab = to_dev(np.array(labels, np.int32))
    m, K = B_.shape
    ws = torch.full((B().hmm_fit_workspace_bytes(len(labels), lengths, lag, m, K),), ws_fill, dtype=torch.uint8, device="cuda")
    par = [to_dev(np.array(x, np.float64)) for x in (A, B_, p0)]
    st = None
    if state is not None:
        rec = np.zeros(1, B().HMM_FIT_STATE)
        for k in STATE_FIELDS:
            rec[k] = state[k]
        st = to_dev(rec.view(np.int32).copy())
    if stationary:
        stationary = to_dev(np.full(m, np.nan) if pi is None else np.array(pi, np.float64))
    res = B().hmm_fit_steps(lab, lengths, lag, *par, reversible, n_steps, accuracy, rev_tol, rev_max_sweeps, state=st,
                            stationary=stationary, workspace=ws)
    return {"A": par[0].cpu().numpy(), "B": par[1].cpu().numpy(), "p0": par[2].cpu().numpy(), "loglik": res["loglik"].cpu().numpy(),
            "pi": res["stationary"].cpu().numpy() if res["stationary"] is not None else None,
            "state": B().hmm_fit_state_dict(res["state"].cpu().numpy())}


class DeviceEstep:
    """the existing dff_hmm_estep behind replay(): (stats, status), the labels uploaded once"""

    def __init__(self, labels):
        self.lab = to_dev(np.array(labels, np.int32))

    def __call__(self, labels, lengths, lag, A, B_, p0):
        res = B().hmm_estep(self.lab, lengths, lag, to_dev(A), to_dev(B_), to_dev(p0), chain_loglik=False, post=False)
        return res["stats"].cpu().numpy(), int(res["status"].cpu())


def replayed(labels, lengths, lag, A, B_, p0, reversible, n_steps, accuracy, state=None, pi=None, **kw):
    a, b, q, ll, pi, st = fc.replay(DeviceEstep(labels), labels, lengths, lag, A, B_, p0, reversible, n_steps, accuracy, state, pi=pi, **kw)
    return {"A": a, "B": b, "p0": q, "loglik": ll, "pi": np.full(len(q), np.nan) if pi is None else pi, "state": st}


def assert_same(got, want, what, pi=True):
    for k in ("loglik", "A", "B", "p0") + (("pi",) if pi else ()):
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])
    for k in STATE_FIELDS:
        a, b = got["state"][k], want["state"][k]
        assert same_bits(np.float64(a), np.float64(b)) if k == "last_loglik" else a == b, (what, k, a, b)


# ---------------------------------------------------------------- 1. the replay, bit for bit
@pytest.mark.parametrize("reversible", (False, True), ids=("plain", "reversible"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d-K%d-lag%d" % s)
def test_four_steps_equal_the_replay_bit_for_bit(shape, reversible, dev):
    m, K, lag = shape
    args = case(m, K, lag)
    got = fit_steps(args[0], args[1], lag, *args[2:], reversible, 4, TINY)
    want = replayed(args[0], args[1], lag, *args[2:], reversible, 4, TINY)
    print(f"[hmm-fit] m {m} K {K} lag {lag} reversible {reversible}: loglik {got['loglik']}, sweeps {got['state']['rev_sweeps']}")
    if K > 1:
        assert got["state"]["n_estep"] == 4 and got["state"]["stop"] == 0 and np.isfinite(got["loglik"]).all()
    else:                                                           # m = K = 1: the model is fitted after one M-step, log-likelihood exactly 0
        assert got["state"]["n_estep"] == 3 and got["state"]["stop"] == 1 and np.isnan(got["loglik"][3]) and got["loglik"][2] == 0.0
    ll = got["loglik"][np.isfinite(got["loglik"])]
    assert (np.diff(ll) >= -1e-9 * np.abs(ll[:-1])).all()           # EM never loses likelihood
    assert (got["state"]["rev_sweeps"] > 0) == (reversible and m > 1)
    assert_same(got, want, shape)
    assert np.isnan(got["pi"]).all() if not reversible else np.isclose(got["pi"].sum(), 1.0)


# ---------------------------------------------------------------- 2. splits and the workspace
@pytest.mark.parametrize("reversible", (False, True), ids=("plain", "reversible"))
def test_split_calls_any_workspace_and_no_stationary_buffer(reversible, dev):
    m, K, lag = 3, 5, 3
    labels, lengths, A, B_, p0 = case(m, K, lag)
    whole = fit_steps(labels, lengths, lag, A, B_, p0, reversible, 6, TINY)
    first = fit_steps(labels, lengths, lag, A, B_, p0, reversible, 2, TINY)
    second = fit_steps(labels, lengths, lag, first["A"], first["B"], first["p0"], reversible, 4, TINY, state=first["state"], pi=first["pi"])
    assert same_bits(whole["loglik"], np.concatenate([first["loglik"], second["loglik"]]))
    assert_same(dict(second, loglik=whole["loglik"]), whole, "2 + 4 steps")
    zeros = fit_steps(labels, lengths, lag, A, B_, p0, reversible, 6, TINY, ws_fill=0x00)
    assert_same(zeros, whole, "a zeroed workspace")                  # 0xFF bytes are NaNs: the workspace's contents are irrelevant
    bare = fit_steps(labels, lengths, lag, A, B_, p0, reversible, 6, TINY, stationary=None)
    assert bare["pi"] is None
    assert_same(bare, whole, "stationary_dev = NULL", pi=False)


# ---------------------------------------------------------------- 3. the convergence freeze
def test_a_converged_fit_is_frozen(dev):
    m, K, lag = 4, 64, 1
    labels, lengths, A, B_, p0 = case(m, K, lag)
    one = fit_steps(labels, lengths, lag, A, B_, p0, True, 1, 1e300)
    got = fit_steps(labels, lengths, lag, A, B_, p0, True, 5, 1e300)
    st = got["state"]
    assert st["n_estep"] == 2 and st["stop"] == 1 and st["estep_status"] == 0
    assert np.isfinite(got["loglik"][:2]).all() and np.isnan(got["loglik"][2:]).all() and st["last_loglik"] == got["loglik"][1]
    for k in ("A", "B", "p0", "pi"):
        assert same_bits(got[k], one[k]), k                          # the parameters after ONE M-step: those loglik[1] was computed with
    assert st["rev_sweeps"] == one["state"]["rev_sweeps"]
    assert_same(got, replayed(labels, lengths, lag, A, B_, p0, True, 5, 1e300), "freeze")
    more = fit_steps(labels, lengths, lag, got["A"], got["B"], got["p0"], True, 3, 1e300, state=st, pi=got["pi"])
    assert np.isnan(more["loglik"]).all() and more["state"] == st
    for k in ("A", "B", "p0", "pi"):
        assert same_bits(more[k], got[k]), k


# ---------------------------------------------------------------- 4. kept rows, a lost state
def test_a_state_that_emits_nothing_observed(dev):
    rng = np.random.default_rng(2)
    lengths = [hmm_chunk() + 3, 0, 40]
    labels = rng.integers(0, 3, sum(lengths)).astype(np.int32)       # symbol 3 is never observed ...
    A = np.array([[0.8, 0.2], [0.3, 0.7]])
    B_ = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.0, 0.0, 1.0]])    # ... and it is all hidden state 1 emits
    p0 = np.array([0.9, 0.1])
    got = fit_steps(labels, lengths, 1, A, B_, p0, False, 2, TINY)
    assert got["state"]["stop"] == 0 and got["state"]["flags"] & 1 and got["state"]["n_estep"] == 2
    assert same_bits(got["B"][1], B_[1]) and same_bits(got["A"][1], A[1]) and same_bits(got["A"][0], np.array([1.0, 0.0]))
    assert same_bits(got["p0"], np.array([1.0, 0.0])) and abs(got["B"][0].sum() - 1.0) < 1e-15
    assert_same(got, replayed(labels, lengths, 1, A, B_, p0, False, 2, TINY), "kept rows")
    lost = fit_steps(labels, lengths, 1, A, B_, p0, True, 3, TINY)
    st = lost["state"]
    assert st["stop"] == 3 and st["n_estep"] == 1 and st["flags"] & 1 and st["rev_sweeps"] == 0
    assert same_bits(lost["A"], A) and same_bits(lost["B"], B_) and same_bits(lost["p0"], p0) and np.isnan(lost["pi"]).all()
    assert np.isfinite(lost["loglik"][0]) and np.isnan(lost["loglik"][1:]).all() and st["last_loglik"] == lost["loglik"][0]
    assert_same(lost, replayed(labels, lengths, 1, A, B_, p0, True, 3, TINY), "lost state")


# ---------------------------------------------------------------- 5. a failed E-step
def test_a_failed_e_step_stops_the_fit(dev):
    m, K, lag = 2, 5, 1
    labels, lengths, A, B_, p0 = case(m, K, lag)
    neg = A.copy()
    neg[1, 0] = -0.25
    over = labels.copy()
    over[len(over) // 2] = K
    Bd = np.array([[0.5, 0.0, 0.5, 0.0], [0.0, 0.5, 0.0, 0.5]])
    good = np.array([0, 2, 0, 2, 2], np.int32)
    impossible = (np.concatenate([good, [0, 1, 0], good]), [5, 3, 5], 1, np.eye(2), Bd, np.array([0.5, 0.5]))   # 0 -> 1 under A = 1
    for status, args in ((1, (labels, lengths, lag, neg, B_, p0)), (3, (over, lengths, lag, A, B_, p0)), (2, impossible)):
        for reversible in (False, True):
            got = fit_steps(*args, reversible, 3, 1e-3)
            st = got["state"]
            assert (st["stop"], st["estep_status"], st["n_estep"], st["flags"]) == (2, status, 1, 0), (status, st)
            assert np.isnan(got["loglik"]).all() and np.isnan(got["pi"]).all()
            assert same_bits(got["A"], args[3]) and same_bits(got["B"], args[4]) and same_bits(got["p0"], args[5])
    # the failure may come later: one good step, then the parameters are poisoned between two calls
    ok = fit_steps(labels, lengths, lag, A, B_, p0, False, 1, 1e-3)
    bad = ok["B"].copy()
    bad[0, 0] = np.nan
    got = fit_steps(labels, lengths, lag, ok["A"], bad, ok["p0"], False, 2, 1e-3, state=ok["state"])
    assert (got["state"]["stop"], got["state"]["estep_status"], got["state"]["n_estep"]) == (2, 1, 2)
    assert got["state"]["last_loglik"] == ok["loglik"][0] and same_bits(got["B"], bad)


# ---------------------------------------------------------------- 6. the sweep cap
def test_the_sweep_cap_sets_its_flag_and_counts(dev):
    m, K, lag = 5, 1024, 3
    labels, lengths, A, B_, p0 = case(m, K, lag)
    got = fit_steps(labels, lengths, lag, A, B_, p0, True, 3, TINY, rev_max_sweeps=3)
    assert got["state"]["flags"] == 2 and got["state"]["rev_sweeps"] == 9 and got["state"]["stop"] == 0
    assert_same(got, replayed(labels, lengths, lag, A, B_, p0, True, 3, TINY, rev_max_sweeps=3), "cap 3")
    free = fit_steps(labels, lengths, lag, A, B_, p0, True, 3, TINY)
    assert free["state"]["flags"] == 0 and free["state"]["rev_sweeps"] > 9 and not same_bits(free["A"], got["A"])
    loose = fit_steps(labels, lengths, lag, A, B_, p0, True, 3, TINY, rev_tol=1e-3)
    assert loose["state"]["flags"] == 0 and 3 <= loose["state"]["rev_sweeps"] < free["state"]["rev_sweeps"]
    assert_same(loose, replayed(labels, lengths, lag, A, B_, p0, True, 3, TINY, rev_tol=1e-3), "rev_tol 1e-3")


# ---------------------------------------------------------------- 7. stream order
def fit_spec():
    """three trajectories (one empty) at lag 2, three reversible steps; poison: constant labels, NaN parameters and a state
    that says the fit has stopped"""
    m, K, lag, Cn, steps = 3, 5, 2, hmm_chunk(), 3
    A, B_, p0 = hc.model(m, K)
    lengths = np.array([2 * Cn + 5, 0, 3 * Cn], np.int64)
    n = int(lengths.sum())
    labels = np.random.default_rng(4).integers(0, K, n).astype(np.int32)
    ws = torch.empty(B().hmm_fit_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    ins = {"labels": (to_dev(labels), 0), "trans": (to_dev(weak(A)), nan), "emit": (to_dev(B_), nan), "init": (to_dev(p0), nan),
           "state": (torch.zeros(8, dtype=torch.int32, device="cuda"), 1)}
    return Spec("dff_hmm_fit_steps", ins, {"loglik": ((steps,), torch.float64), "pi": ((m,), torch.float64)},
                lambda _, b: raw("dff_hmm_fit_steps", 0, ptr(b["labels"]), n, lengths.ctypes.data_as(C.c_void_p), 3, lag, ptr(b["trans"]),
                                 ptr(b["emit"]), ptr(b["init"]), m, K, 1, steps, C.c_double(TINY), C.c_double(1e-12), C.c_longlong(100000),
                                 ptr(b["loglik"]), ptr(b["pi"]), ptr(b["state"]), ptr(b["ws"]), b["ws"].numel(), stream_of(b["labels"])),
                inout=("trans", "emit", "init", "state"), work={"ws": ws})


def test_the_call_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(fit_spec(), gate, side)
    st = B().hmm_fit_state_dict(ref["state"].cpu().numpy())
    assert st["n_estep"] == 3 and st["stop"] == 0 and bool(torch.isfinite(ref["loglik"]).all())
    assert abs(float(ref["pi"].sum()) - 1.0) < 1e-12 and float((ref["trans"].sum(dim=1) - 1.0).abs().max()) < 1e-12


def test_fence():
    """The memory contract (tests/fence.py): all nine buffers in one arena, the E-step's sections plus the packed statistics and
    the status word at exactly dff_hmm_fit_workspace_bytes.  The state travels as eight int32 words; the header documents it as
    8-byte aligned (it holds a double), so "tight" puts it at 8 mod 16."""
    spec = fit_spec()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref, align={"state": 8})


# ---------------------------------------------------------------- 8. end to end: a two-well jump process
def two_wells(seed=11, n_traj=20, length=500):
    """labels of a two-state jump process seen through 6 symbols, three per well, one in ten frames showing the other well's"""
    paths = oracle.jump_process(np.array([[0.97, 0.03], [0.05, 0.95]]), n_traj, length, seed).reshape(-1)
    rng = np.random.default_rng(seed + 1)
    seen = np.where(rng.random(paths.size) < 0.1, 1 - paths, paths)
    return (3 * seen + rng.integers(0, 3, paths.size)).astype(np.int32), [length] * n_traj


START = (np.array([[0.8, 0.2], [0.2, 0.8]]), np.array([[2.0, 2, 2, 1, 1, 1], [1, 1, 1, 2, 2, 2.0]]) / 9.0, np.array([0.5, 0.5]))


@pytest.fixture(scope="module")
def point(dev):
    labels, lengths = two_wells()
    model = ev().HiddenMarkovModel(2, 2, m_step="device", steps_per_sync=7).fit(labels, lengths, 6, initial=START)
    return labels, lengths, model


def test_the_device_fit_equals_the_replay_run_to_convergence(point):
    labels, lengths, model = point
    assert model.converged and model.message == "" and not model.degenerate and not model.rev_unconverged and model.rev_sweeps > 0
    want = replayed(labels, lengths, 2, *START, True, 200, 1e-3)
    ll = want["loglik"][np.isfinite(want["loglik"])]
    assert want["state"]["stop"] == 1 and model.n_iter == want["state"]["n_estep"] == len(ll) and model.rev_sweeps == want["state"]["rev_sweeps"]
    assert same_bits(np.array(model.log_likelihoods), ll)
    order = np.argsort(-want["pi"], kind="stable")
    assert same_bits(model.transition_matrix, want["A"][np.ix_(order, order)]) and same_bits(model.observation_probabilities, want["B"][order])
    assert same_bits(model.initial_distribution, want["p0"][order]) and same_bits(model.stationary_distribution, want["pi"][order])
    other = ev().HiddenMarkovModel(2, 2, m_step="device", steps_per_sync=32).fit(labels, lengths, 6, initial=START)
    assert other.n_iter == model.n_iter and same_bits(other.transition_matrix, model.transition_matrix)
    # the jump process: stationary (5 / 8, 3 / 8), timescale -1 / ln(0.92) = 12 frames; the host path finds the same model
    assert abs(model.stationary_distribution[0] - 0.625) < 0.08 and abs(model.timescales()[0] + 1.0 / np.log(0.92)) < 4.0
    host = ev().HiddenMarkovModel(2, 2).fit(labels, lengths, 6, initial=START)
    assert host.n_iter == model.n_iter and np.allclose(host.transition_matrix, model.transition_matrix, rtol=1e-8)
    print(f"[hmm-fit] two wells: {model.n_iter} E-steps, {model.rev_sweeps} sweeps, populations {model.stationary_distribution}, "
          f"timescale {model.timescales()[0]:.2f}")


def test_every_resample_is_a_warm_started_device_fit_of_its_labels(point):
    labels, lengths, model = point
    start = (model.transition_matrix, model.observation_probabilities, model.initial_distribution)
    bs = ev().bootstrap_hmm(labels, 2, 2, lengths, 6, n_resamples=6, seed=0, point=model)
    assert bs.n_failed == 0 and bs.converged.all() and same_bits(bs.weights, ev().bootstrap_weights(20, 6, 0)) and bs.point is model
    lab = to_dev(labels)
    for b in range(6):
        own = ev().HiddenMarkovModel(2, 2, m_step="device").fit(*ev().resampled_labels(lab, bs.unit_lengths, bs.weights[b]), 6,
                                                                  initial=start, renumber=False)
        assert same_bits(bs.transition_matrices[b], own.transition_matrix) and same_bits(bs.stationary[b], own.stationary_distribution), b
        assert same_bits(bs.timescales[b], own.timescales()) and same_bits(bs.lifetimes[b], own.lifetimes()), b
        assert bs.n_iter[b] == own.n_iter and bs.log_likelihood[b] == own.log_likelihoods[-1], b
    ones = ev().bootstrap_hmm(labels, 2, 2, lengths, 6, weights=np.ones((1, 20)), point=model)
    warm = ev().HiddenMarkovModel(2, 2, m_step="device").fit(labels, lengths, 6, initial=start, renumber=False)
    assert same_bits(ones.transition_matrices[0], warm.transition_matrix) and ones.n_iter[0] == warm.n_iter
    assert same_bits(ones.stationary[0], warm.stationary_distribution)
    print(f"[hmm-fit] bootstrap of 6: timescale {model.timescales()[0]:.2f} +- {bs.std()[0]:.2f}, populations +- {bs.std('stationary')}, "
          f"E-steps per resample {bs.n_iter.tolist()}")
