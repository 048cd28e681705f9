"""The Markov-state-model calls on the GPU (csrc/dff_msm.hip) against the fp64 numpy oracle of oracle/msm.py, and the
classes of evaluate.py on top of them.  C = binding.MICRO_CHUNK is the number of points one workgroup of
dff_micro_kmeans_step takes: the point counts below sit on its boundaries.

What is compared how:
- K <= 64     labels and dist2 of dff_micro_kmeans_step are dff_kmeans_step's bits; dff_micro_transition_counts' counts are
              dff_transition_counts'.
- grid        coordinates and centres k 2^-10, |k| < 2^12 (a few far ones: whole numbers up to 2^9).  Every difference is a
              multiple of 2^-10 below 2^10, every square a multiple of 2^-20 below 2^20, a d2 stays below 2^23 and the sum of
              all of them below 2^33: every operation is exact in fp64, fused or not, in any order -> torch.equal with the
              oracle on labels, dist2, sums, counts and inertia.
- Gaussian    labels equal the oracle's where the oracle's best and second-best d2 differ by more than 2^-40 relative (the
              kernel fuses, numpy does not: a few 2^-53 relative); counts exact; |sum - fsum| <= (m - 1) 2^-53 sum |x| for a
              cluster of m members, the a-priori bound of ANY order of summation; the same for the inertia.
- estimator   the map x -> x' is monotone and homogeneous of degree 1, hence non-expansive in the sup-norm of log-ratios; a
              sweep's row sum of K positive terms, each with a division and two additions, is off by at most (K + 4) 2^-53
              relative in any order, on either side: after m sweeps |x_gpu / x_oracle - 1| <= 2 m (K + 4) 2^-53 =: b.
              err_s = max_i |x_i' / x_i - 1| then differs by at most 2 b (1 + err_s) (both x and x' carry b) plus the two
              roundings of the expression itself.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import msm as oracle
from oracle.frames import synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DS = [1, 2, 8]
KS = [1, 2, 64, 65, 257, 1024]


def point_counts():
    c = B().MICRO_CHUNK
    return [0, 1, 63, 64, 65, 1000, c - 1, c, c + 1, 2 * c + 1]


def micro(pts, centers, accumulate=True, fill=0xFF):
    """binding.micro_kmeans_step on a workspace of `fill` bytes -> dict of host arrays"""
    pd, cd = to_dev(np.asarray(pts, np.float64)), to_dev(np.asarray(centers, np.float64))
    ws = None
    if accumulate:
        need = B().micro_kmeans_workspace_bytes(pd.shape[0], pd.shape[1], cd.shape[0])
        ws = torch.full((max(need, 8),), fill, dtype=torch.uint8, device="cuda")
    return {k: v.cpu().numpy() for k, v in B().micro_kmeans_step(pd, cd, accumulate=accumulate, workspace=ws).items()}


def spoil(pts):
    """NaN, +inf and -inf into three rows (where there are that many)"""
    pts = pts.copy()
    n, d = pts.shape
    for row, v in ((2, np.nan), (n // 2, np.inf), (n - 1, -np.inf)):
        if n > 5:
            pts[row, row % d] = v
    return pts


# ---------------------------------------------------------------- 1. assignment
def gaussian(n, d, K, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal((K, d))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", [1, 2, 64])
def test_assignment_is_kmeans_step_bit_for_bit(dev, d, K):
    for n in point_counts():
        pts, cen = gaussian(n, d, K, 1000 * n + 10 * d + K)
        pts = spoil(pts)
        got = micro(pts, cen, accumulate=False)
        old = B().kmeans_step(to_dev(pts), to_dev(cen), accumulate=False)
        assert same_bits(got["labels"], old["labels"].cpu().numpy()), (n, d, K)
        assert same_bits(got["dist2"], old["dist2"].cpu().numpy()), (n, d, K)
        if n > 5:
            assert (got["labels"] == -1).sum() == 3 and np.isnan(got["dist2"]).sum() == 3


def grid_case(n, d, K, seed):
    """Points and centres on the dyadic grid with the ties the rule has to break: the last centre duplicates centre 0, point 0
    sits on a centre, point 1 is equidistant from centres 0 and 1 (K >= 2), four points and one centre are far away."""
    rng = np.random.default_rng(seed)
    g = lambda *shape: rng.integers(-2 ** 12, 2 ** 12, shape) * 2.0 ** -10          # noqa: E731
    pts, cen = g(n, d), g(K, d)
    if K >= 3:
        cen[K - 1] = cen[0]
        cen[K // 2] = rng.integers(-2 ** 9, 2 ** 9, d).astype(np.float64)
    if K >= 2:
        cen[1] = cen[0]
        cen[1, 0] += 2.0 ** -9
    if n >= 1:
        pts[0] = cen[K // 3]
    if n >= 2:
        pts[1] = cen[0]
        pts[1, 0] += 2.0 ** -10
    for i in range(4):
        if n > 20 + i:
            pts[10 + i] = rng.integers(-2 ** 9, 2 ** 9, d).astype(np.float64)
    return spoil(pts), cen


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", KS)
def test_grid_inputs_are_exact(dev, d, K):
    """labels, dist2, sums, counts and inertia equal the oracle's bit for bit at every point count; the assignment-only call
    gives the same labels and dist2."""
    for n in point_counts():
        pts, cen = grid_case(n, d, K, 77 * n + 5 * d + K)
        lab, d2, _ = oracle.assign(pts, cen)
        want = oracle.accumulate(pts, lab, d2, K)
        got = micro(pts, cen)
        what = f"n = {n}, d = {d}, K = {K}"
        assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], lab), what
        assert same_bits(got["dist2"], d2), what
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want["counts"]), what
        assert same_bits(got["sums"] + 0.0, want["sums"] + 0.0), (what, np.argwhere(got["sums"] != want["sums"])[:4])
        assert got["inertia"][0] == want["inertia"], (what, got["inertia"][0], want["inertia"])
        only = micro(pts, cen, accumulate=False)
        assert same_bits(only["labels"], got["labels"]) and same_bits(only["dist2"], got["dist2"]), what
        if K >= 3:
            assert (lab != K - 1).all()                              # a duplicate of centre 0 never wins


def gaussian_checked(n, d, K, seed):
    """Gaussian inputs, the oracle's labels and the mask of points it decides by more than 2^-40 (at most 1 % may be left out:
    asserted on the oracle alone)."""
    pts, cen = gaussian(n, d, K, seed)
    lab, d2, gap = oracle.assign(pts, cen)
    clear = gap > 2.0 ** -40
    assert n == 0 or (~clear).mean() <= 0.01, f"seed {seed}: the oracle leaves {(~clear).sum()} of {n} points undecided"
    return pts, cen, lab, d2, clear


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", KS)
def test_gaussian_assignment_and_sums(dev, d, K):
    for n in point_counts():
        pts, cen, lab, d2, clear = gaussian_checked(n, d, K, 31 * n + 7 * d + K)
        got = micro(pts, cen)
        what = f"n = {n}, d = {d}, K = {K}"
        assert np.array_equal(got["labels"][clear], lab[clear]), what
        ok = np.abs(got["dist2"] - d2) <= 4 * d * U * d2                    # d fused terms against d rounded ones
        assert ok.all(), (what, np.abs(got["dist2"] - d2).max())
        want = oracle.accumulate(pts, got["labels"], got["dist2"], K)      # sums over the GPU's own assignment
        assert np.array_equal(got["counts"], want["counts"]) and got["counts"].sum() == n, what
        bound = np.maximum(want["counts"] - 1, 0)[:, None] * U * want["abs_sums"]
        err = np.abs(got["sums"] - want["sums"])
        print(f"{what}: worst sum error / bound {np.max(err / np.where(bound > 0, bound, np.inf), initial=0.0):.3f}")
        assert (err <= bound).all(), (what, np.argwhere(err > bound)[:4])
        ib = max(want["members"] - 1, 0) * U * want["abs_inertia"]
        assert abs(got["inertia"][0] - want["inertia"]) <= ib, (what, got["inertia"][0], want["inertia"], ib)
        again = micro(pts, cen, fill=0x00)
        for k in ("labels", "dist2", "sums", "counts", "inertia"):
            assert same_bits(got[k], again[k]), (what, k, "differs between two calls / two workspaces")


def test_empty_clusters_one_full_cluster_and_non_finite_points(dev):
    c = B().MICRO_CHUNK
    n, d, K = c + 37, 2, 257
    rng = np.random.default_rng(9)
    pts = spoil(rng.standard_normal((n, d)))
    cen = 100.0 + rng.standard_normal((K, d))
    cen[K - 1] = 0.0                                                     # every finite point is nearest to the LAST centre
    got = micro(pts, cen)
    fin = np.isfinite(pts).all(axis=1)
    assert fin.sum() == n - 3 and (got["labels"][fin] == K - 1).all() and (got["labels"][~fin] == -1).all()
    assert got["counts"][K - 1] == n - 3 and got["counts"][:K - 1].sum() == 0
    assert not got["sums"][:K - 1].any() and np.isfinite(got["sums"]).all() and np.isfinite(got["inertia"]).all()
    want = oracle.accumulate(pts, got["labels"], got["dist2"], K)
    assert (np.abs(got["sums"] - want["sums"]) <= (n - 4) * U * want["abs_sums"]).all()
    empty = micro(np.zeros((0, d)), cen)
    assert not empty["sums"].any() and not empty["counts"].any() and empty["inertia"][0] == 0.0 and empty["labels"].size == 0


def test_microstate_kmeans_draws_and_fits_like_kmeans(dev):
    rng = np.random.default_rng(4)
    pts = rng.integers(-2 ** 12, 2 ** 12, (1000, 2)) * 2.0 ** -10
    pts[::2] += 3.0
    a = ev().MicrostateKMeans(8, seed=3).fit(pts)
    b = ev().KMeans(8, seed=3).fit(pts)
    assert same_bits(a.cluster_centers, b.cluster_centers) and a.n_iter == b.n_iter > 1
    assert a.inertia == pytest.approx(b.inertia, rel=1e-13)
    assert same_bits(a.transform(pts), b.transform(pts))
    seeded = ev().MicrostateKMeans(8, seed=3, max_iter=0)
    assert same_bits(seeded._seed_centers(to_dev(pts)), b._seed_centers(to_dev(pts)))


def test_inertia_does_not_increase_at_300_centres(dev):
    rng = np.random.default_rng(12)
    blobs = np.array([[0.0, 0.0], [40.0, 5.0], [-10.0, 60.0]])
    pts = blobs[rng.integers(0, 3, 3000)] + rng.standard_normal((3000, 2))
    centers = pts[rng.choice(3000, 300, replace=False)]
    pd = to_dev(pts)
    inertias = []
    for _ in range(8):
        r = B().micro_kmeans_step(pd, to_dev(centers))
        sums, counts = r["sums"].cpu().numpy(), r["counts"].cpu().numpy()
        inertias.append(float(r["inertia"][0]))
        has = counts > 0
        centers = centers.copy()
        centers[has] = sums[has] / counts[has, None]
    assert all(b <= a for a, b in zip(inertias, inertias[1:])), inertias
    assert inertias[-1] < 0.9 * inertias[0]
    km = ev().MicrostateKMeans(300, seed=1, max_iter=5).fit(pts)
    assert km.cluster_centers.shape == (300, 2) and km.inertia > 0 and len(np.unique(km.transform(pts))) > 250


# ---------------------------------------------------------------- 2. counts
def sticky_labels(n, K, seed, stay=0.9):
    """a metastable path (stays with probability `stay`), some -1 among the labels"""
    rng = np.random.default_rng(seed)
    jump = rng.random(n) > stay
    lab = np.where(jump, rng.integers(0, K, n), 0)
    last = np.maximum.accumulate(np.where(jump, np.arange(n), 0))
    lab = lab[last]
    lab[rng.random(n) < 0.01] = -1
    return lab.astype(np.int32)


RAGGED = [700, 0, 1, 64, 65, 0, 2000, 3, 1500]
LAGS = [1, 3, 7, 64]


@pytest.mark.parametrize("K", [1, 2, 64])
def test_counts_equal_transition_counts(dev, K):
    """K <= 64: the call launches dff_transition_counts' own LDS kernel (measured faster there), so equality with that call
    pins the routing and the argument plumbing; the oracle is what both are held to.  The global-atomic kernel is the
    K > 64 test below."""
    n = sum(RAGGED)
    for lengths in (RAGGED, [n], [619] * 7):
        for stay in (0.0, 0.95):
            lab = to_dev(sticky_labels(n, K, K + int(100 * stay)))
            got = B().micro_transition_counts(lab, lengths, LAGS, K)
            old = B().transition_counts(lab, lengths, LAGS, K)
            assert got.dtype == torch.int64 and torch.equal(got, old), (K, lengths[:3], stay)
            assert np.array_equal(got.cpu().numpy(), oracle.transition_counts(lab.cpu().numpy(), lengths, LAGS, K))
            assert int(got[0].sum()) > 0
    short = B().micro_transition_counts(to_dev(sticky_labels(150, K, 5)), [50, 50, 50], [50, 64], K)
    assert short.shape == (2, K, K) and not short.any()                    # lags longer than every trajectory


@pytest.mark.parametrize("K", [65, 1024])
def test_counts_equal_the_oracle(dev, K):
    n = sum(RAGGED)
    for lengths in (RAGGED, [619] * 7):
        for stay in (0.0, 0.95):
            lab = sticky_labels(n, K, K + int(100 * stay))
            lags = LAGS + [2, 5, 11, 5000]
            got = B().micro_transition_counts(to_dev(lab), lengths, lags, K).cpu().numpy()
            assert np.array_equal(got, oracle.transition_counts(lab, lengths, lags, K)), (K, lengths[:3], stay)
            again = B().micro_transition_counts(to_dev(lab), lengths, lags, K).cpu().numpy()
            assert np.array_equal(got, again)
    one = np.full(5000, K - 1, np.int32)
    got = B().micro_transition_counts(to_dev(one), [2500, 2500], [1, 10], K).cpu().numpy()
    assert got[0, K - 1, K - 1] == 4998 and got[1, K - 1, K - 1] == 4980 and got.sum() == 4998 + 4980
    empty = B().micro_transition_counts(to_dev(np.zeros(0, np.int32)), [], [1], K)
    assert empty.shape == (1, K, K) and not empty.any()


def test_counts_refusals(dev):
    lab = to_dev(sticky_labels(100, 4, 1))
    for args, what in (((lab, [100], [1], 0), "states must be 1..1024"), ((lab, [100], [1], 1025), "states must be 1..1024"),
                       ((lab, [100], [0], 4), "must be >= 1"), ((lab, [100], list(range(1, 10)), 4), "lag times must be 1..8"),
                       ((lab, [60, 30], [1], 4), "sum to 90, not n = 100")):
        with pytest.raises(ValueError, match=what):
            B().micro_transition_counts(*args)
    with pytest.raises(ValueError, match="int32"):
        B().micro_transition_counts(lab.long(), [100], [1], 4)


# ---------------------------------------------------------------- 3. the estimator
EST_KS = [2, 3, 5, 64, 65, 300]
M_SWEEPS = 50


def est_inputs(K):
    Cm = oracle.connected_counts(K, 11 * K + 1)
    assert len(oracle.largest_connected_set(Cm)) == K
    S, c = Cm + Cm.T, Cm.sum(axis=1)
    return Cm, S, c, oracle.start(S)


def gpu_sweeps(S, c, x, n, driver=0, fill=0xFF):
    B().debug_msm_driver(driver)
    try:
        xd = to_dev(x)
        ws = torch.full((B().msm_workspace_bytes(len(c)),), fill, dtype=torch.uint8, device="cuda")
        err = B().msm_reversible_steps(to_dev(S), to_dev(c), xd, n, workspace=ws)
        return xd.cpu().numpy(), err.cpu().numpy()
    finally:
        B().debug_msm_driver(0)


@pytest.mark.parametrize("K", EST_KS)
def test_fifty_sweeps_against_the_oracle(dev, K):
    _, S, c, x0 = est_inputs(K)
    want_x, want_err = oracle.sweeps(S, c, x0, M_SWEEPS)
    b = 2 * M_SWEEPS * (K + 4) * U
    runs = {drv: gpu_sweeps(S, c, x0, M_SWEEPS, drv) for drv in (0, 1, 2)}
    x, err = runs[0]
    rel = np.abs(x / want_x - 1).max()
    derr = np.abs(err - want_err)
    print(f"K = {K}: |x / oracle - 1| {rel:.2e} (bound {b:.2e}), err off by {derr.max():.2e}")
    assert rel <= b, (K, rel, b)
    assert (derr <= 2 * b * (1 + want_err) + 4 * U).all(), (K, derr.max())
    for drv in (1, 2):                                       # one launch per sweep, one workgroup for all: the same bits
        assert same_bits(runs[drv][0], x) and same_bits(runs[drv][1], err), (K, drv)
    again = gpu_sweeps(S, c, x0, M_SWEEPS, 0, fill=0x00)
    assert same_bits(again[0], x) and same_bits(again[1], err), K
    kept, none = gpu_sweeps(S, c, x0, 0)
    assert same_bits(kept, x0) and none.shape == (0,)
    half, e1 = gpu_sweeps(S, c, x0, 20)                      # 20 + 30 sweeps are the 50
    rest, e2 = gpu_sweeps(S, c, half, 30)
    assert same_bits(rest, x) and same_bits(np.concatenate([e1, e2]), err), K


@pytest.mark.parametrize("K", EST_KS)
def test_symmetric_counts_are_a_fixed_point(dev, K):
    Cm = oracle.connected_counts(K, 13 * K + 2)
    Cm = Cm + Cm.T
    S, c = Cm + Cm.T, Cm.sum(axis=1)
    for drv in (1, 2):
        x, err = gpu_sweeps(S, c, oracle.start(S), 1, drv)
        assert err[0] <= (K + 4) * U, (K, drv, err[0])


@pytest.mark.parametrize("K", EST_KS)
def test_converged_model_has_the_estimators_properties(dev, K):
    Cm, _, _, _ = est_inputs(K)
    m = ev().MarkovStateModel(1, tol=1e-12, max_iter=8_000_000, steps_per_sync=16384).fit_counts(Cm)
    assert m.converged and m.n_iter > 1 and m.active_set.tolist() == list(range(K))
    print(f"K = {K}: {m.n_iter} sweeps")
    oracle.check_reversible(Cm, m.transition_matrix, m.stationary_distribution, f"K = {K}")
    if K == 2:
        assert np.abs(m.transition_matrix - Cm / Cm.sum(axis=1, keepdims=True)).max() < 1e-10


def test_a_row_without_counts_gives_nan(dev):
    _, S, c, x0 = est_inputs(5)
    c = c.copy()
    c[3] = 0.0
    x, err = gpu_sweeps(S, c, x0, 2)
    assert np.isnan(x[3]) and np.isnan(err).all()


def test_estimator_refusals(dev):
    f64 = dict(dtype=torch.float64, device="cuda")
    for K in (0, 1025):
        with pytest.raises(ValueError, match="states must be 1..1024"):
            B().msm_reversible_steps(torch.zeros((K, K), **f64), torch.zeros(K, **f64), torch.zeros(K, **f64), 1)
    S, c, x = torch.ones((4, 4), **f64), torch.ones(4, **f64), torch.ones(4, **f64)
    with pytest.raises(ValueError, match="workspace of 63 bytes, 64 needed"):
        B().msm_reversible_steps(S, c, x, 1, workspace=torch.empty(63, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="negative n_steps"):
        B().msm_reversible_steps(S, c, x, -1)
    with pytest.raises(ValueError, match="contiguous float64"):
        B().msm_reversible_steps(S.float(), c, x, 1)
    with pytest.raises(ValueError, match="centres must be 1..1024"):
        B().micro_kmeans_step(torch.zeros((5, 2), **f64), torch.zeros((1025, 2), **f64))
    with pytest.raises(ValueError, match="d must be 1..8"):
        B().micro_kmeans_step(torch.zeros((5, 9), **f64), torch.zeros((3, 9), **f64))
    with pytest.raises(ValueError, match="workspace of 8 bytes"):
        B().micro_kmeans_step(torch.zeros((5, 2), **f64), torch.zeros((3, 2), **f64),
                              workspace=torch.empty(8, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- 4. stream order
N_PTS = 2500


def micro_kmeans_step_spec():
    n, d, K = N_PTS, 2, 70
    rng = np.random.default_rng(21)
    pts = rng.standard_normal((n, d)) + np.array([[3.0, -2.0]]) * (np.arange(n) % 5)[:, None]
    centers = pts[:K].copy()
    ws = torch.empty(B().micro_kmeans_workspace_bytes(n, d, K), dtype=torch.uint8, device="cuda")
    return Spec("dff_micro_kmeans_step", {"pts": (to_dev(pts), float("nan")), "centers": (to_dev(centers), 0.5)},
                {"labels": ((n,), torch.int32), "dist2": ((n,), torch.float64), "sums": ((K, d), torch.float64),
                 "counts": ((K,), torch.int64), "inertia": ((1,), torch.float64)},
                lambda _, b: raw("dff_micro_kmeans_step", 0, ptr(b["pts"]), n, d, ptr(b["centers"]), K, ptr(b["labels"]),
                                 ptr(b["dist2"]), ptr(b["sums"]), ptr(b["counts"]), ptr(b["inertia"]), ptr(b["ws"]),
                                 b["ws"].numel(), stream_of(b["pts"])),
                work={"ws": ws}, wrap=lambda _, b: B().micro_kmeans_step(b["pts"], b["centers"]))


def micro_transition_counts_spec():
    K, lags, lengths = 70, np.array([1, 7], np.int32), np.array([1000, 600, 900], np.int64)
    labels = sticky_labels(N_PTS, K, 3, stay=0.5)
    return Spec("dff_micro_transition_counts", {"labels": (to_dev(labels), 0)}, {"counts": ((2, K, K), torch.int64)},
                lambda _, b: raw("dff_micro_transition_counts", 0, ptr(b["labels"]), N_PTS, lengths.ctypes.data_as(C.c_void_p), 3,
                                 lags.ctypes.data_as(C.c_void_p), 2, K, ptr(b["counts"]), stream_of(b["labels"])),
                wrap=lambda _, b: {"counts": B().micro_transition_counts(b["labels"], lengths, lags, K)})


def msm_reversible_steps_spec(K):
    """x is in/out (real: the start vector; poison NaN); 12 sweeps."""
    _, S, c, x0 = est_inputs(K)
    ws = torch.empty(B().msm_workspace_bytes(K), dtype=torch.uint8, device="cuda")
    return Spec("dff_msm_reversible_steps", {"S": (to_dev(S), float("nan")), "c": (to_dev(c), float("nan")), "x": (to_dev(x0), float("nan"))},
                {"err": ((12,), torch.float64)},
                lambda _, b: raw("dff_msm_reversible_steps", 0, ptr(b["S"]), ptr(b["c"]), K, ptr(b["x"]), 12, ptr(b["err"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["x"])),
                inout=("x",), work={"ws": ws})


def test_micro_kmeans_step_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(micro_kmeans_step_spec(), gate, side)
    assert int(ref["counts"].sum()) == N_PTS


def test_micro_transition_counts_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(micro_transition_counts_spec(), gate, side)
    assert 0 < int(ref["counts"][0].sum()) <= N_PTS - 3


LAUNCH_PER_SWEEP, ONE_WORKGROUP = 1, 2


@pytest.mark.parametrize("K,forced,runs", [
    (5, 0, ONE_WORKGROUP), (32, 0, ONE_WORKGROUP), (33, 0, LAUNCH_PER_SWEEP), (300, 0, LAUNCH_PER_SWEEP),
    (65, ONE_WORKGROUP, ONE_WORKGROUP), (16, LAUNCH_PER_SWEEP, LAUNCH_PER_SWEEP),
], ids=["one-workgroup-5", "one-workgroup-32", "launch-per-sweep-33", "launch-per-sweep-300", "one-workgroup-forced-65",
        "launch-per-sweep-forced-16"])
def test_msm_reversible_steps_is_ordered_on_its_stream(K, forced, runs, gate, side):
    """Both drivers behind the gate: the library's own choice on either side of its threshold, and each one forced.  Which
    driver a case runs is asked of the library (dff_msm_driver_for), not assumed."""
    B().debug_msm_driver(forced)
    try:
        assert B().msm_driver_for(K) == runs
        ref = analysis_call(msm_reversible_steps_spec(K), gate, side)
        assert B().msm_driver_for(K) == runs
    finally:
        B().debug_msm_driver(0)
    assert bool(torch.isfinite(ref["x"]).all()) and bool((ref["err"] > 0).all())


def _fence(spec):
    """The memory contract (tests/fence.py): both patterns at both placements against one reference."""
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


def test_fence_micro_kmeans_step():
    """ceil(n / chunk) rows of K (d + 1) + 1 doubles, at exactly dff_micro_kmeans_workspace_bytes"""
    _fence(micro_kmeans_step_spec())


def test_fence_micro_transition_counts():
    _fence(micro_transition_counts_spec())


@pytest.mark.parametrize("forced", [0, LAUNCH_PER_SWEEP, ONE_WORKGROUP], ids=["default", "launch-per-sweep", "one-workgroup"])
@pytest.mark.parametrize("K", [5, 33, 71])
def test_fence_msm_reversible_steps(K, forced):
    """two vectors of K doubles, under either driver; K = 71: a partial last stride of the 64 lanes of a row sum"""
    B().debug_msm_driver(forced)
    try:
        _fence(msm_reversible_steps_spec(K))
    finally:
        B().debug_msm_driver(0)


# ---------------------------------------------------------------- 5. end to end
def test_three_well_jump_process(dev):
    """40 trajectories x 2 000 frames of a 3-state chain with known M, seen as noisy points in the plane; 60 microstates."""
    M = np.array([[0.98, 0.015, 0.005], [0.02, 0.97, 0.01], [0.004, 0.016, 0.98]])
    paths = oracle.jump_process(M, 40, 2000, seed=8)
    wells = np.array([[0.0, 0.0], [6.0, 1.0], [2.0, 7.0]])
    rng = np.random.default_rng(80)
    pts = wells[paths.reshape(-1)] + rng.standard_normal((paths.size, 2))
    lengths = [2000] * 40
    km = ev().MicrostateKMeans(60, seed=2, max_iter=20).fit(pts)
    labels = km.transform(pts)
    assert labels.min() >= 0 and labels.max() < 60
    lag, k = 10, 2
    m = ev().MarkovStateModel(lag, tol=1e-13, steps_per_sync=128).fit(labels, lengths, 60)
    act, want, T, pi = oracle.pipeline(labels, lengths, lag, 60, k)
    assert m.converged and np.array_equal(m.active_set, act)
    got = m.timescales(k)
    print(f"timescales {got} (oracle {want}), {m.n_iter} sweeps, active share {m.active_count_share:.4f}")
    assert np.isfinite(want).all() and np.abs(got / want - 1).max() <= 1e-8, (got, want)
    exact = np.sort(-1.0 / np.log(np.sort(np.abs(np.linalg.eigvals(M)))[::-1][1:]))[::-1]     # of M itself, lag 1
    assert np.abs(got / exact - 1).max() < 0.5                     # the two slow processes of the chain, at the right scale
    its = ev().implied_timescales(labels, [1, 2, 5, 10, 20, 30, 40, 50, 60], lengths, 60, k=2)
    assert its.shape == (9, 2) and np.abs(its[3] / got - 1).max() < 1e-6 and np.isfinite(its).all()


# ---------------------------------------------------------------- 6. the evaluator and the tool
MSM_BEADS, MSM_STATES, MSM_LAG, MSM_FRAME_TIME = 10, 12, 5, 0.5
M_SAMPLES = np.array([[0.98, 0.015, 0.005], [0.02, 0.97, 0.01], [0.004, 0.016, 0.98]])
M_REFS = np.array([[0.97, 0.02, 0.01], [0.02, 0.96, 0.02], [0.01, 0.02, 0.97]])


def conformer_frames(M, n_traj, n_frames, seed):
    """float32 frames (n_traj n_frames, 10, 3): three fixed chain conformations visited by the jump process of M, plus 0.05 A
    of noise"""
    paths = oracle.jump_process(M, n_traj, n_frames, seed)
    base = synth_chain_frames(3, MSM_BEADS, 91).astype(np.float64)
    noise = np.random.default_rng(seed + 1).standard_normal((paths.size, MSM_BEADS, 3))
    return (base[paths.reshape(-1)] + 0.05 * noise).astype(np.float32)


def tic_pair():
    F = B().struct_tic_num_features(MSM_BEADS)
    rng = np.random.default_rng(17)
    return rng.uniform(0.0, 10.0, F), rng.uniform(-0.1, 0.1, (F, 2))


def evaluator_inputs():
    x = conformer_frames(M_SAMPLES, 10, 1000, 5)
    x[4321, 3, 1] = np.nan
    return x, [1000] * 10, conformer_frames(M_REFS, 6, 1200, 6), [1200, 2400, 0, 3600]


def js(h1, h2):
    """evaluate.js_divergence restated: both normalised, 1e-10 added, the mean of the two KL divergences to the mixture"""
    p1, p2 = h1 / h1.sum() + 1e-10, h2 / h2.sum() + 1e-10
    m = 0.5 * (p1 + p2)
    return 0.5 * (np.sum(p1 * np.log(p1 / m)) + np.sum(p2 * np.log(p2 / m)))


def oracle_side(x, lengths, mean, coeff, centers, got_labels):
    """the oracle's dict of one ensemble from the projection of the (separately tested) dff_struct_tic call"""
    proj = B().struct_tic(to_dev(x), mean, coeff).cpu().numpy()
    lab, _, gap = oracle.assign(proj, centers)
    assert np.nanmin(gap) > 2.0 ** -40                               # no frame sits on a microstate boundary
    assert np.array_equal(got_labels, lab)
    Cm = oracle.transition_counts(lab, lengths, [MSM_LAG], MSM_STATES)[0].astype(np.float64)
    act, ts, T, pi = oracle.pipeline(lab, lengths, MSM_LAG, MSM_STATES, 2)
    res = {"timescales": ts * MSM_FRAME_TIME, "n_active": float(len(act)),
           "active_count_share": Cm[np.ix_(act, act)].sum() / Cm.sum(), "converged": 1.0,
           "samples_nonfinite": float((lab < 0).sum())}
    return res, act, pi


def test_msm_evaluator_against_the_oracle_pipeline(dev):
    """Frames -> TIC projection -> microstates fitted on the reference -> both ensembles on the same centres -> models: every
    key of eval()'s dict against the oracle.  Timescales to 1e-6: both estimates stop at a per-sweep change below 1e-12 /
    1e-13, the iteration contracts geometrically on these dense counts (about 200 sweeps for 13 digits: rate ~0.87, so x is
    within ~1e-11), and d ln t / d lambda = 1 / (lambda |ln lambda|) is below 10^3 for timescales under 100 lags."""
    x, lengths, refs, ref_lengths = evaluator_inputs()
    mean, coeff = tic_pair()
    e = ev().MsmEvaluator("chignolin", (mean, coeff), n_microstates=MSM_STATES, lagtime=MSM_LAG, n_timescales=2,
                          frame_time=MSM_FRAME_TIME, ref_data=refs, ref_traj_lengths=ref_lengths)
    assert e.kmeans is not None and e.centers.shape == (MSM_STATES, 2) and set(e.models) == {"refs"}
    got = e.eval(x, lengths)
    want_s, act_s, pi_s = oracle_side(x, lengths, mean, coeff, e.centers, e.labels["samples"])
    want_r, act_r, pi_r = oracle_side(refs, ref_lengths, mean, coeff, e.centers, e.labels["refs"])
    keys = set(ev().MsmEvaluator.KEYS)
    assert set(got) == keys | {k + "_ref" for k in keys} | {"log10_timescale_ratio", "stationary_js"}
    for want, suffix in ((want_s, ""), (want_r, "_ref")):
        for k in ("n_active", "converged", "samples_nonfinite"):
            assert got[k + suffix] == want[k], (k + suffix, got[k + suffix], want[k])
        assert got["active_count_share" + suffix] == pytest.approx(want["active_count_share"], rel=1e-14)
        ts = np.array(got["timescales" + suffix])
        print(f"timescales{suffix} {ts} (oracle {want['timescales']})")
        assert np.isfinite(want["timescales"]).all() and np.abs(ts / want["timescales"] - 1).max() <= 1e-6
    assert got["samples_nonfinite"] == 1.0 and got["samples_nonfinite_ref"] == 0.0
    ratio = np.log10(want_s["timescales"] / want_r["timescales"])
    assert np.abs(np.array(got["log10_timescale_ratio"]) - ratio).max() <= 1e-6
    union = np.union1d(act_s, act_r)
    p = np.zeros((2, len(union)))
    p[0, np.searchsorted(union, act_s)], p[1, np.searchsorted(union, act_r)] = pi_s, pi_r
    assert got["stationary_js"] == pytest.approx(js(p[0], p[1]), abs=1e-9) and got["stationary_js"] > 0
    assert np.array_equal(e.models["samples"].active_set, act_s) and np.array_equal(e.models["refs"].active_set, act_r)
    again = ev().MsmEvaluator("chignolin", (mean, coeff), n_microstates=MSM_STATES, lagtime=MSM_LAG, n_timescales=2,
                              frame_time=MSM_FRAME_TIME, centers=e.centers).eval(x, lengths)
    assert set(again) == keys and again["timescales"] == got["timescales"]          # given centres, no reference


def test_msm_of_tools_eval_samples(dev, tmp_path):
    """tools_eval_samples.msm() on a saved TICA model and a held-out file of trajectories: the evaluator's dict, cleaned for
    JSON, the settings, and the implied-timescale table."""
    import json

    import tools_eval_samples as tool
    x, lengths, refs, ref_lengths = evaluator_inputs()
    mean, coeff = tic_pair()
    np.savez(tmp_path / "saved_TICA_CHIGNOLIN_testset.npz", mean=mean, coeff=coeff)
    bounds = np.cumsum([0] + ref_lengths)
    torch.save([torch.from_numpy(refs[a:b]) for a, b in zip(bounds[:-1], bounds[1:])], tmp_path / "heldout.pt")
    a = tool.build_parser().parse_args(["s.pt", "chignolin", str(tmp_path), "--parallel-sim", "10", "--msm", str(tmp_path / "heldout.pt"),
                                        "--msm-states", str(MSM_STATES), "--msm-lag", str(MSM_LAG), "--msm-lagtimes", "1,5,20",
                                        "--frame-time", str(MSM_FRAME_TIME)])
    res = tool.msm(a, torch.from_numpy(x))
    assert json.loads(json.dumps(res)) == res
    direct = ev().MsmEvaluator("chignolin", (mean, coeff), n_microstates=MSM_STATES, lagtime=MSM_LAG, frame_time=MSM_FRAME_TIME,
                               ref_data=refs, ref_traj_lengths=ref_lengths).eval(x, lengths)
    clean = lambda v: None if not np.isfinite(v) else float(v)     # noqa: E731
    for k, v in direct.items():
        assert res[k] == ([clean(u) for u in v] if isinstance(v, list) else clean(v)), k
    assert (res["n_microstates"], res["lagtime"], res["frame_time"]) == (MSM_STATES, MSM_LAG, MSM_FRAME_TIME)
    its = res["implied_timescales"]
    assert its["lagtimes"] == [1, 5, 20] and np.array(its["timescales"], dtype=float).shape == (3, 3)
    assert its["timescales"][1][:2] == pytest.approx(res["timescales"][:2], rel=1e-9)      # the same model, fitted again
    assert res["samples_nonfinite"] == 1.0 and len(res["log10_timescale_ratio"]) == 3
