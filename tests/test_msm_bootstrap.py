"""The bootstrap calls on the GPU (csrc/dff_msm_batch.hip) and evaluate.bootstrap_msm on top of them.

What is compared how:
- counts      integer and exact: equal to the oracle's explicit loop over the pairs (oracle/msm_bootstrap.py); with all
              weights 1 every slice is dff_micro_transition_counts' matrix; the same from a workspace of 0xFF and of 0x00.
- estimator   bit-identical to dff_msm_reversible_steps, problem by problem, x and err, on both forced drivers and the default:
              the single call is the reference (tests/test_msm.py holds IT to the oracle), computed once per problem.
- bootstrap   resample b of bootstrap_msm equals MarkovStateModel.fit_counts of the oracle's weighted counts bit for bit.
- error bars  one dataset of the two-state chain of the host calibration test: the bootstrap std of t2 within [0.6, 1.5] x the
              std of the point estimate across 100 datasets, measured by the oracle on the CPU (closed form for two states).
              The per-dataset ratio stayed within 0.75 .. 1.15 in a numpy run of 200 datasets; the bars leave room around it.
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from oracle import msm_bootstrap as boot
from oracle import msm as oracle
from oracle.frames import synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. resampled counts
LENGTHS = [700, 0, 1, 64, 65, 0, 2000, 3, 1500, 667]         # unequal, two empty, 1 and 3 shorter than the lag
N = sum(LENGTHS)                                             # 5000
LAG = 7
UNITS = {"misaligned": [333, 1, 0, 1000, 650, 16, 3000],     # cut through trajectories; a unit of one frame; an empty unit
         "one": [N], "trajectories": LENGTHS, "blocks": boot.units(LENGTHS, 100).tolist()}


def sticky_labels(n, K, seed, stay=0.9):
    """a metastable path (stays with probability `stay`), some -1 among the labels"""
    rng = np.random.default_rng(seed)
    jump = rng.random(n) > stay
    lab = np.where(jump, rng.integers(0, K, n), 0)
    last = np.maximum.accumulate(np.where(jump, np.arange(n), 0))
    lab = lab[last]
    lab[rng.random(n) < 0.01] = -1
    return lab.astype(np.int32)


def some_weights(Bn, n_units, seed):
    """multiplicities 0 .. 3 with 0 and 2^32 - 1 placed in every row"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, (Bn, n_units)).astype(np.uint32)
    w[:, rng.integers(0, n_units)] = 0
    w[np.arange(Bn), rng.integers(0, n_units, Bn)] = 2 ** 32 - 1
    return w


def resampled(labels, lengths, units, lag, K, w, fill=0xFF):
    need = B().micro_resampled_counts_workspace_bytes(len(lengths), len(units))
    ws = torch.full((max(need, 8),), fill, dtype=torch.uint8, device="cuda")
    out = B().micro_resampled_counts(to_dev(labels), lengths, units, lag, K, to_dev(w), workspace=ws)
    assert out.dtype == torch.uint64 and tuple(out.shape) == (len(w), K, K)
    return out.cpu().numpy()


@pytest.mark.parametrize("Bn", [1, 3, 65])
@pytest.mark.parametrize("K", [2, 64, 65, 300])
def test_resampled_counts_equal_the_oracle(dev, K, Bn):
    labels = sticky_labels(N, K, 7 * K + Bn)
    assert (labels == -1).any()
    for name, units in UNITS.items():
        w = some_weights(Bn, len(units), K + Bn)
        got = resampled(labels, LENGTHS, units, LAG, K, w)
        want = boot.weighted_counts(labels, LENGTHS, units, LAG, K, w)
        assert got.dtype == want.dtype == np.uint64 and np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
        assert int(got.sum()) > 0 and same_bits(got, resampled(labels, LENGTHS, units, LAG, K, w, fill=0x00)), name
    # all weights 1: every slice is the plain count matrix, whatever the units
    plain = B().micro_transition_counts(to_dev(labels), LENGTHS, [LAG], K)[0].cpu().numpy()
    for name in ("misaligned", "one"):
        ones = resampled(labels, LENGTHS, UNITS[name], LAG, K, np.ones((Bn, len(UNITS[name])), np.uint32))
        for b in range(Bn):
            assert same_bits(ones[b].view(np.int64), plain), (name, b)


def test_resampled_counts_edges(dev):
    K = 70
    labels = sticky_labels(N, K, 5)
    w = some_weights(3, 1, 2)
    long_lag = resampled(labels, LENGTHS, [N], 2000, K, w)                    # longer than every trajectory
    assert not long_lag.any()
    one = np.full(N, K - 1, np.int32)                                          # every pair on ONE counter, one frame per unit
    w1 = np.arange(1, N + 1, dtype=np.uint32)[None, :]
    got = resampled(one, [N], [1] * N, 1, K, w1)
    assert got[0, K - 1, K - 1] == (N - 1) * N // 2 and got.sum() == (N - 1) * N // 2
    big = resampled(one, [N], [N], 1, K, np.full((2, 1), 2 ** 32 - 1, np.uint32))
    assert (big[:, K - 1, K - 1] == (N - 1) * (2 ** 32 - 1)).all()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    empty = B().micro_resampled_counts(to_dev(np.zeros(0, np.int32)), [], [0], 1, K, to_dev(w), workspace=ws)
    assert tuple(empty.shape) == (3, K, K) and not empty.cpu().numpy().any()  # n == 0 zeroes the output


def test_resampled_counts_refusals(dev):
    lab, w = to_dev(sticky_labels(100, 4, 1)), to_dev(np.ones((2, 1), np.uint32))
    for args, what in (((lab, [100], [100], 1, 0, w), "states must be 1..1024"), ((lab, [100], [100], 1, 1025, w), "states must be 1..1024"),
                       ((lab, [100], [100], 0, 4, w), "must be >= 1"), ((lab, [60, 30], [100], 1, 4, w), "sum to 90, not n = 100"),
                       ((lab, [100], [100], 1, 1024, to_dev(np.ones((257, 1), np.uint32))), "must not exceed 2\\^28"),
                       ((lab, [100], [100], 1, 4, to_dev(np.ones((4097, 1), np.uint32))), "resamples must be 1..4096")):
        with pytest.raises(ValueError, match=what):
            B().micro_resampled_counts(*args)
    with pytest.raises(ValueError, match="unit lengths sum to 90"):
        B().micro_resampled_counts(lab, [100], [60, 30], 1, 4, to_dev(np.ones((2, 2), np.uint32)))
    with pytest.raises(ValueError, match="uint32"):
        B().micro_resampled_counts(lab, [100], [100], 1, 4, w.to(torch.int64))
    with pytest.raises(ValueError, match="uint32"):
        B().micro_resampled_counts(lab, [100], [60, 40], 1, 4, w)            # (B, 1) weights for two units
    with pytest.raises(ValueError, match="workspace of 8 bytes"):
        B().micro_resampled_counts(lab, [100], [100], 1, 4, w, workspace=torch.empty(8, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- 2. the batched estimator
MIX = [1, 2, 3, 5, 32, 33, 64, 65, 300]
KMAX = 300
M_SWEEPS = 50


@functools.lru_cache(maxsize=None)
def problem(K, seed):
    """(S, c, x0) of a strongly connected problem with K states, and the single call's (x, err) after M_SWEEPS sweeps"""
    Cm = oracle.connected_counts(K, 11 * K + seed) + np.eye(K)              # + I: no empty row, also at K = 1
    S, c = Cm + Cm.T, Cm.sum(axis=1)
    x0 = oracle.start(S)
    return S, c, x0, single(S, c, x0, M_SWEEPS)


def single(S, c, x, n):
    xd = to_dev(x)
    err = B().msm_reversible_steps(to_dev(S), to_dev(c), xd, n)
    return xd.cpu().numpy(), err.cpu().numpy()


def batch_of(Bn):
    return [(MIX[(2 * i + Bn) % len(MIX)] if Bn > 1 else 65, i) for i in range(Bn)] if Bn != 9 else [(K, 0) for K in MIX]


def packed(probs, x=None):
    """slots of KMAX^2 / KMAX doubles, NaN wherever a problem does not reach"""
    P = len(probs)
    S, c, xs = np.full((P, KMAX * KMAX), np.nan), np.full((P, KMAX), np.nan), np.full((P, KMAX), np.nan)
    for p, (K, seed) in enumerate(probs):
        Sp, cp, x0, _ = problem(K, seed)
        S[p, :K * K], c[p, :K], xs[p, :K] = Sp.reshape(-1), cp, x0 if x is None else x[p, :K]
    return S.reshape(P, KMAX, KMAX), c, xs, np.array([K for K, _ in probs], np.int32)


def batched(S, c, ks, x, n, driver=0, skip=None, fill=0xFF):
    B().debug_msm_driver(driver)
    try:
        xd = to_dev(x)
        ws = torch.full((B().msm_batched_workspace_bytes(len(ks), KMAX),), fill, dtype=torch.uint8, device="cuda")
        err = B().msm_reversible_steps_batched(to_dev(S), to_dev(c), ks, xd, n, skip=skip, workspace=ws)
        assert tuple(err.shape) == (n, len(ks))
        return xd.cpu().numpy(), err.cpu().numpy()
    finally:
        B().debug_msm_driver(0)


@pytest.mark.parametrize("Bn", [1, 9, 70])
def test_batched_sweeps_are_the_single_calls_bits(dev, Bn):
    probs = batch_of(Bn)
    assert Bn != 70 or {K for K, _ in probs} == set(MIX)
    S, c, x0, ks = packed(probs)
    runs = {drv: batched(S, c, ks, x0, M_SWEEPS, drv) for drv in (0, 1, 2)}
    runs["zeros"] = batched(S, c, ks, x0, M_SWEEPS, 0, fill=0x00)
    for name, (x, err) in runs.items():
        for p, (K, seed) in enumerate(probs):
            want_x, want_err = problem(K, seed)[3]
            assert same_bits(x[p, :K], want_x), (name, p, K)
            assert same_bits(err[:, p], want_err), (name, p, K)
            assert np.isnan(x[p, K:]).all(), (name, p, K)                   # nothing is written beyond K_b
            assert np.isfinite(want_x).all() and np.isfinite(want_err).all() and (K == 1 or (want_err > 0).all())
    half, e1 = batched(S, c, ks, x0, 20)                                    # 20 + 30 sweeps are the 50
    rest, e2 = batched(S, c, ks, half, 30)
    assert same_bits(rest, runs[0][0]) and same_bits(np.concatenate([e1, e2]), runs[0][1])
    kept, none = batched(S, c, ks, x0, 0)
    assert same_bits(kept, x0) and none.shape == (0, Bn)


def test_skipped_problems_and_a_zero_row_count(dev):
    probs = batch_of(9)
    S, c, x0, ks = packed(probs)
    skip = np.zeros(9, bool)
    skip[[1, 4, 8]] = True
    for drv in (1, 2):
        x, err = batched(S, c, ks, x0, 12, drv, skip=skip)
        for p, (K, seed) in enumerate(probs):
            if skip[p]:
                assert same_bits(x[p], x0[p]) and not err[:, p].any(), (drv, p)
            else:
                Sp, cp, xp, _ = problem(K, seed)
                want_x, want_err = single(Sp, cp, xp, 12)
                assert same_bits(x[p, :K], want_x) and same_bits(err[:, p], want_err), (drv, p)
        everything = batched(S, c, ks, x0, 12, drv, skip=np.ones(9, bool))
        assert same_bits(everything[0], x0) and not everything[1].any()
    c2 = c.copy()
    c2[3, 2] = 0.0                                                          # problem 3 (K = 5): a row without counts
    for drv in (1, 2):
        x, err = batched(S, c2, ks, x0, 3, drv)
        assert np.isnan(x[3, 2]) and np.isnan(err[:, 3]).all()
        others = [p for p in range(9) if p != 3]
        assert np.isfinite(err[:, others]).all() and all(np.isfinite(x[p, :ks[p]]).all() for p in others)
        Sp, cp, xp, _ = problem(5, 0)
        cp = cp.copy()
        cp[2] = 0.0
        want_x, want_err = single(Sp, cp, xp, 3)
        assert same_bits(x[3, :5], want_x) and same_bits(err[:, 3], want_err)


def test_sweeps_stay_inside_their_workspace(dev):
    """A workspace 64 bytes longer than asked for, all 0xA5: the 64 bytes stay, and x and err are those of the exact-size run.
    Single call at K = 2 (one workgroup) and K = 33 (the smallest K with a launch per sweep); batched call at B = 2,
    Kmax = 33 on both forced drivers."""
    CANARY, n = 64, 3

    def run(call, need, extra):
        ws = torch.full((need + extra,), 0xA5, dtype=torch.uint8, device="cuda")
        x, err = call(ws)
        assert bool((ws[need:] == 0xA5).all())
        return x.cpu().numpy(), err.cpu().numpy()

    assert B().msm_driver_for(2) == 2 and B().msm_driver_for(33) == 1
    for K in (2, 33):
        S, c, x0, _ = problem(K, 0)

        def one(ws):
            xd = to_dev(x0)
            return xd, B().msm_reversible_steps(to_dev(S), to_dev(c), xd, n, workspace=ws)
        need = B().msm_workspace_bytes(K)
        exact, padded = run(one, need, 0), run(one, need, CANARY)
        assert same_bits(padded[0], exact[0]) and same_bits(padded[1], exact[1]), K
        assert np.isfinite(exact[0]).all() and (exact[1] > 0).all(), K

    ks, Kmax = np.array([33, 5], np.int32), 33
    Sb, cb, xb = np.full((2, Kmax * Kmax), np.nan), np.full((2, Kmax), np.nan), np.full((2, Kmax), np.nan)
    for p, K in enumerate(ks):
        Sp, cp, xp, _ = problem(int(K), 0)
        Sb[p, :K * K], cb[p, :K], xb[p, :K] = Sp.reshape(-1), cp, xp
    Sb = Sb.reshape(2, Kmax, Kmax)

    def many(ws):
        xd = to_dev(xb)
        return xd, B().msm_reversible_steps_batched(to_dev(Sb), to_dev(cb), ks, xd, n, workspace=ws)
    need = B().msm_batched_workspace_bytes(2, Kmax)
    for drv in (1, 2):
        B().debug_msm_driver(drv)
        try:
            exact, padded = run(many, need, 0), run(many, need, CANARY)
        finally:
            B().debug_msm_driver(0)
        assert same_bits(padded[0], exact[0]) and same_bits(padded[1], exact[1]), drv
        for p, K in enumerate(ks):
            want_x, want_err = single(*problem(int(K), 0)[:3], n)
            assert same_bits(exact[0][p, :K], want_x) and same_bits(exact[1][:, p], want_err), (drv, p)


def test_batched_refusals(dev):
    f64 = dict(dtype=torch.float64, device="cuda")
    S, c, x = torch.ones((2, 4, 4), **f64), torch.ones((2, 4), **f64), torch.ones((2, 4), **f64)
    for ks, what in (([4, 5], "problem 1 has 5 states"), ([0, 4], "problem 0 has 0 states")):
        with pytest.raises(ValueError, match=what):
            B().msm_reversible_steps_batched(S, c, ks, x, 1)
    with pytest.raises(ValueError, match="negative n_steps"):
        B().msm_reversible_steps_batched(S, c, [4, 4], x, -1)
    with pytest.raises(ValueError, match="one state count per problem"):
        B().msm_reversible_steps_batched(S, c, [4], x, 1)
    with pytest.raises(ValueError, match="one flag per problem"):
        B().msm_reversible_steps_batched(S, c, [4, 4], x, 1, skip=[True])
    with pytest.raises(ValueError, match="contiguous float64"):
        B().msm_reversible_steps_batched(S.float(), c, [4, 4], x, 1)
    with pytest.raises(ValueError, match="workspace of 143 bytes, 144 needed"):
        B().msm_reversible_steps_batched(S, c, [4, 4], x, 1, workspace=torch.empty(143, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="states must be 1..1024"):
        B().msm_reversible_steps_batched(torch.ones((1, 1025, 1025), **f64), torch.ones((1, 1025), **f64), [4],
                                         torch.ones((1, 1025), **f64), 1)


# ---------------------------------------------------------------- 3. stream order
def resampled_counts_spec():
    """weights and counts travel as int32 / int64 tensors of the same bits: the gate fills and compares them"""
    K, Bn, units = 70, 5, np.array(UNITS["misaligned"], np.int64)
    lengths = np.array(LENGTHS, np.int64)
    labels = sticky_labels(N, K, 3, stay=0.5)
    w = np.random.default_rng(1).integers(1, 4, (Bn, len(units))).astype(np.int32)
    ws = torch.empty(B().micro_resampled_counts_workspace_bytes(len(lengths), len(units)), dtype=torch.uint8, device="cuda")
    return Spec("dff_micro_resampled_counts", {"labels": (to_dev(labels), 0), "weights": (to_dev(w), 0)},
                {"counts": ((Bn, K, K), torch.int64)},
                lambda _, b: raw("dff_micro_resampled_counts", 0, ptr(b["labels"]), N, lengths.ctypes.data_as(C.c_void_p), len(lengths),
                                 units.ctypes.data_as(C.c_void_p), len(units), LAG, K, ptr(b["weights"]), Bn, ptr(b["counts"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["labels"])),
                work={"ws": ws},
                wrap=lambda _, b: {"counts": B().micro_resampled_counts(b["labels"], lengths, units, LAG, K,
                                                                        b["weights"].view(torch.uint32)).view(torch.int64)})


def batched_spec():
    """x is in/out (real: the start vectors; poison NaN); 12 sweeps of the nine problems"""
    S, c, x0, ks = packed(batch_of(9))
    S, c, x0 = np.nan_to_num(S, nan=1.0), np.nan_to_num(c, nan=1.0), np.nan_to_num(x0, nan=1.0)
    ws = torch.empty(B().msm_batched_workspace_bytes(9, KMAX), dtype=torch.uint8, device="cuda")
    return Spec("dff_msm_reversible_steps_batched",
                {"S": (to_dev(S), float("nan")), "c": (to_dev(c), float("nan")), "x": (to_dev(x0), float("nan"))},
                {"err": ((12, 9), torch.float64)},
                lambda _, b: raw("dff_msm_reversible_steps_batched", 0, ptr(b["S"]), ptr(b["c"]), ks.ctypes.data_as(C.c_void_p), None, 9,
                                 KMAX, ptr(b["x"]), 12, ptr(b["err"]), ptr(b["ws"]), b["ws"].numel(), stream_of(b["x"])),
                inout=("x",), work={"ws": ws})


def test_resampled_counts_are_ordered_on_their_stream(gate, side):
    ref = analysis_call(resampled_counts_spec(), gate, side)
    assert int(ref["counts"].sum()) > N


@pytest.mark.parametrize("forced", [0, 1, 2], ids=["default", "launch-per-sweep", "one-workgroup-per-problem"])
def test_batched_sweeps_are_ordered_on_their_stream(forced, gate, side):
    B().debug_msm_driver(forced)
    try:
        ref = analysis_call(batched_spec(), gate, side)
    finally:
        B().debug_msm_driver(0)
    assert bool(torch.isfinite(ref["x"]).all()) and bool((ref["err"][:, 1:] > 0).all())     # (problem 0 has one state: err = 0)


def _fence(spec):
    """The memory contract (tests/fence.py): both patterns at both placements against one reference."""
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


def test_fence_resampled_counts():
    """the trajectory and unit start tables at exactly dff_micro_resampled_counts_workspace_bytes"""
    _fence(resampled_counts_spec())


@pytest.mark.parametrize("forced", [0, 1, 2], ids=["default", "launch-per-sweep", "one-workgroup-per-problem"])
def test_fence_batched_sweeps(forced):
    """two vectors of B Kmax doubles and B descriptors at exactly dff_msm_batched_workspace_bytes, under either driver; what
    lies beyond K_b in a problem's slot of x is neither read nor written: x is a result, compared whole"""
    B().debug_msm_driver(forced)
    try:
        _fence(batched_spec())
    finally:
        B().debug_msm_driver(0)


# ---------------------------------------------------------------- 4. bootstrap_msm
def test_bootstrap_msm_equals_fit_counts_of_the_oracles_counts(dev):
    labels, lengths, w = boot.five_state_case()
    lag, K, k = 2, 5, 3
    settings = dict(tol=1e-12, max_iter=100000, steps_per_sync=16)
    bs = ev().bootstrap_msm(labels, lag, lengths, K, weights=w, k=k, **settings)
    counts = boot.weighted_counts(labels, lengths, lengths, lag, K, w)
    assert sorted(set(bs.n_active.tolist())) == [1, 4, 5] and bs.n_failed == int(np.isnan(bs.timescales[:, -1]).sum())
    for b, Cb in enumerate(counts):
        m = ev().MarkovStateModel(lag, **settings).fit_counts(Cb)
        assert m.n_iter == bs.n_iter[b] and m.converged == bs.converged[b] and len(m.active_set) == bs.n_active[b], b
        assert same_bits(m.timescales(k), bs.timescales[b]) and m.active_count_share == bs.active_count_share[b], b
        full = np.zeros(K)
        full[m.active_set] = m.stationary_distribution
        assert same_bits(full, bs.stationary[b]), b
    plain = ev().MarkovStateModel(lag, **settings).fit(labels, lengths, K)
    assert same_bits(plain.transition_matrix, bs.point.transition_matrix) and plain.n_iter == bs.point.n_iter
    one = ev().bootstrap_msm(labels, lag, lengths, K, weights=w, k=k, resample_batch=1, **settings)
    for name in ("timescales", "stationary", "n_iter", "converged", "n_active", "active_count_share"):
        assert same_bits(getattr(one, name), getattr(bs, name)), name
    want = boot.bootstrap(labels, lengths, lengths, lag, K, w, k=k, **settings)                 # and the oracle's own estimator
    ok = ~np.isnan(want["timescales"])
    assert np.array_equal(~np.isnan(bs.timescales), ok) and np.allclose(bs.timescales[ok], want["timescales"][ok], rtol=1e-8)
    drawn = ev().bootstrap_msm(labels, lag, lengths, K, n_resamples=5, block_frames=150, seed=4, k=k, **settings)
    assert np.array_equal(drawn.weights, boot.weights(12, 5, 4)) and drawn.timescales.shape == (5, 3)


def test_error_bar_of_one_two_state_dataset(dev):
    across = boot.across_dataset_std(100, 7000)
    labels, lengths = boot.two_state_dataset(424242)
    bs = ev().bootstrap_msm(labels, 1, lengths, 2, n_resamples=200, seed=1, k=1)
    std, (lo, hi) = bs.std()[0], bs.interval(0.90)
    print(f"two-state chain: t2 {bs.point.timescales(1)[0]:.4f} (true {boot.TRUE_T2:.4f}), bootstrap std {std:.4f}, std across 100 "
          f"datasets (oracle, CPU) {across:.4f}, ratio {std / across:.3f}, 90 % interval [{lo[0]:.3f}, {hi[0]:.3f}]")
    assert bs.n_failed == 0 and bs.converged.all()
    closed = boot.two_state_t2(boot.FastCounter(labels, lengths, lengths, 1, 2, None)(bs.weights))
    assert np.allclose(bs.timescales[:, 0], closed, rtol=1e-8)
    assert 0.6 * across <= std <= 1.5 * across, (std, across)


# ---------------------------------------------------------------- 5. the evaluator and the tool
BEADS, STATES, LAGTIME, FRAME_TIME, N_BOOT = 10, 12, 5, 0.5, 6
M_SAMPLES = np.array([[0.98, 0.015, 0.005], [0.02, 0.97, 0.01], [0.004, 0.016, 0.98]])
M_REFS = np.array([[0.97, 0.02, 0.01], [0.02, 0.96, 0.02], [0.01, 0.02, 0.97]])


def conformer_frames(M, n_traj, n_frames, seed):
    """float32 frames: three fixed chain conformations visited by the jump process of M, plus 0.05 A of noise"""
    paths = oracle.jump_process(M, n_traj, n_frames, seed)
    base = synth_chain_frames(3, BEADS, 91).astype(np.float64)
    noise = np.random.default_rng(seed + 1).standard_normal((paths.size, BEADS, 3))
    return (base[paths.reshape(-1)] + 0.05 * noise).astype(np.float32)


def evaluator_inputs():
    F = B().struct_tic_num_features(BEADS)
    rng = np.random.default_rng(17)
    tica = (rng.uniform(0.0, 10.0, F), rng.uniform(-0.1, 0.1, (F, 2)))
    return conformer_frames(M_SAMPLES, 10, 1000, 5), [1000] * 10, conformer_frames(M_REFS, 6, 1200, 6), [1200, 2400, 0, 3600], tica


def oracle_bars(labels, lengths, block, seed, conf):
    units = boot.units(lengths, block)
    res = boot.bootstrap(labels, lengths, units, LAGTIME, STATES, boot.weights(len(units), N_BOOT, seed), k=2)
    return res["timescales"], boot.interval(res["timescales"], conf), boot.std(res["timescales"])


def test_evaluator_and_tool_against_the_oracle_pipeline(dev, tmp_path):
    import tools_eval_samples as tool
    x, lengths, refs, ref_lengths, tica = evaluator_inputs()
    plain = ev().MsmEvaluator("chignolin", tica, n_microstates=STATES, lagtime=LAGTIME, n_timescales=2, frame_time=FRAME_TIME,
                              ref_data=refs, ref_traj_lengths=ref_lengths)
    old = plain.eval(x, lengths)
    e = ev().MsmEvaluator("chignolin", tica, n_microstates=STATES, lagtime=LAGTIME, n_timescales=2, frame_time=FRAME_TIME,
                          ref_data=refs, ref_traj_lengths=ref_lengths, centers=plain.centers, n_bootstrap=N_BOOT, block_frames=400,
                          confidence=0.8, bootstrap_seed=3)
    got = e.eval(x, lengths)
    new = {"timescales_lo", "timescales_hi", "timescales_std", "bootstrap_failed"}
    assert set(got) == set(old) | new | {k + "_ref" for k in new} | {"log10_timescale_ratio_lo", "log10_timescale_ratio_hi"}
    assert {k: got[k] for k in old} == old                                   # the point estimates do not move
    ts = {}
    for name, suffix, ln, seed in (("samples", "", lengths, 3), ("refs", "_ref", ref_lengths, 4)):
        ts[name], (lo, hi), sd = oracle_bars(e.labels[name], ln, 400, seed, 0.8)
        assert np.isfinite(ts[name]).all()
        for key, want in (("timescales_lo", lo), ("timescales_hi", hi), ("timescales_std", sd)):
            assert np.allclose(got[key + suffix], FRAME_TIME * want, rtol=1e-6), (key + suffix, got[key + suffix], want)
        assert got["bootstrap_failed" + suffix] == 0.0
    rlo, rhi = boot.interval(np.log10(ts["samples"] / ts["refs"]), 0.8)
    assert np.allclose(got["log10_timescale_ratio_lo"], rlo, atol=1e-6) and np.allclose(got["log10_timescale_ratio_hi"], rhi, atol=1e-6)
    # the tool: the evaluator's dict, cleaned for JSON, the settings, the implied-timescale table with its bars
    np.savez(tmp_path / "saved_TICA_CHIGNOLIN_testset.npz", mean=tica[0], coeff=tica[1])
    bounds = np.cumsum([0] + ref_lengths)
    torch.save([torch.from_numpy(refs[a:b]) for a, b in zip(bounds[:-1], bounds[1:])], tmp_path / "heldout.pt")
    a = tool.build_parser().parse_args(["s.pt", "chignolin", str(tmp_path), "--parallel-sim", "10", "--msm", str(tmp_path / "heldout.pt"),
                                        "--msm-states", str(STATES), "--msm-lag", str(LAGTIME), "--msm-lagtimes", "1,5",
                                        "--frame-time", str(FRAME_TIME), "--msm-bootstrap", str(N_BOOT), "--msm-block-frames", "400",
                                        "--msm-confidence", "0.8"])
    res = tool.msm(a, torch.from_numpy(x))
    assert json.loads(json.dumps(res)) == res
    assert (res["n_bootstrap"], res["block_frames"], res["confidence"]) == (N_BOOT, 400, 0.8)
    direct = ev().MsmEvaluator("chignolin", tica, n_microstates=STATES, lagtime=LAGTIME, frame_time=FRAME_TIME, ref_data=refs,
                               ref_traj_lengths=ref_lengths, n_bootstrap=N_BOOT, block_frames=400, confidence=0.8).eval(x, lengths)
    clean = lambda v: None if not np.isfinite(v) else float(v)     # noqa: E731
    for k, v in direct.items():
        assert res[k] == ([clean(u) for u in v] if isinstance(v, list) else clean(v)), k
    its = res["implied_timescales"]
    assert its["lagtimes"] == [1, 5] and set(its) == {"lagtimes", "timescales", "timescales_lo", "timescales_hi"}
    assert its["timescales"][1][:2] == pytest.approx(res["timescales"][:2], rel=1e-9)
    assert its["timescales_lo"][1] == pytest.approx(res["timescales_lo"], rel=1e-9)          # seed 0, the same blocks and draws
    assert all(lo <= hi for lo, hi in zip(its["timescales_lo"][0][:2], its["timescales_hi"][0][:2]))
