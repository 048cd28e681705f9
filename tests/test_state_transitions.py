"""States in TIC space and the transitions between them (csrc/dff_states.hip, evaluate.KMeans /
StateTransitionEvaluator): the dynamics analysis of the reference's evaluate_fastfolders.ipynb, cells 20-24.

Every oracle is float64 numpy (oracle/states.py: deeptime is not installed, so MiniBatchKMeans and
TransitionCountEstimator are restated there from their documented semantics).

Labels are compared with the argmin of float64 distances computed from dff_struct_tic's projections.  A frame whose
best and second-best squared distance differ by less than 1e-9 relative is a legitimate disagreement of summation
order (the kernel's FMA chain against numpy's products and sums: a few ulps, 1e-16 relative, of d2); such frames are
left out, and at most 1e-5 of the frames of any case may be.

Sums and inertia of the k-means step are compared at rtol 1e-12: the test's points have positive coordinates (no
cancellation), the kernel adds a few dozen terms one after another per accumulator between its fixed trees and numpy
sums pairwise, so the two differ by summation order only -- some tens of ulps (1.1e-16 each) at the very worst."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.frames import blobs, chain_frames, two_state_trajectories
from oracle.states import counts64, dist2_64, lloyd64
from support import dev, ev, on_device  # noqa: F401  (dev: fixture)

AMBIGUOUS_REL = 1e-9
AMBIGUOUS_CAP = 1e-5


# ================================================================ the label rule
def check_labels(labels, p, centers):
    """labels == argmin of the float64 distances, but for the (capped) frames whose two best distances nearly tie;
    returns the oracle's labels with those frames taken from `labels`."""
    labels = np.asarray(labels)
    d2 = dist2_64(p, centers)
    n, K = d2.shape
    assert labels.shape == (n,)
    if n == 0:
        return labels.astype(np.int64)
    finite = np.isfinite(np.asarray(p, np.float64)).all(1)
    want = np.where(finite, np.argmin(np.where(np.isfinite(d2), d2, np.inf), axis=1), -1)
    amb = np.zeros(n, bool)
    if K > 1:
        s = np.sort(d2, axis=1)
        with np.errstate(invalid="ignore"):
            amb = finite & ((s[:, 1] - s[:, 0]) < AMBIGUOUS_REL * s[:, 1])
    print(f"labels: n {n} K {K} left out {int(amb.sum())} mismatches {int((labels != want)[~amb].sum())}")
    assert amb.sum() <= AMBIGUOUS_CAP * n, (int(amb.sum()), n)
    assert np.array_equal(labels[~amb], want[~amb])
    assert np.all((labels[amb] >= 0) & (labels[amb] < K))
    return np.where(amb, labels, want).astype(np.int64)


# ================================================================ CPU
def test_transition_matrix_rows():
    e = ev()
    rng = np.random.default_rng(0)
    c = rng.integers(0, 50, (3, 5, 5))
    c[1, 2] = 0
    c[2] = 0
    T = e.transition_matrix(c)
    assert T.shape == c.shape and T.dtype == np.float64
    rows = T.sum(-1)
    assert np.allclose(rows[c.sum(-1) > 0], 1.0, rtol=0, atol=1e-15)
    assert np.all(T[1, 2] == 0) and np.all(T[2] == 0)
    assert np.array_equal(e.transition_matrix(c[0]), c[0] / c[0].sum(1, keepdims=True))
    try:
        from sklearn.preprocessing import normalize
    except ImportError:                                  # scikit-learn is optional: the checks above stand alone
        return
    for m in c:
        assert np.array_equal(e.transition_matrix(m), normalize(m.astype(np.float64), axis=1, norm="l1"))


def test_msm_timescales_two_state():
    e = ev()
    a, b = 0.03, 0.12                                    # T = [[1 - a, a], [b, 1 - b]]: eigenvalues 1 and 1 - a - b
    T = np.array([[1 - a, a], [b, 1 - b]])
    ts = e.msm_timescales(T, 10)
    assert ts.shape == (1,) and abs(ts[0] - (-10.0 / np.log(1 - a - b))) <= 1e-12 * abs(ts[0])
    T3 = np.diag([1.0, 0.5, -0.8])                       # sorted by magnitude: 1, -0.8, 0.5
    assert np.allclose(e.msm_timescales(T3, 2), [-2 / np.log(0.8), -2 / np.log(0.5)], rtol=1e-14)


def test_state_presets_shapes():
    e = ev()
    assert set(e.STATE_CENTERS) == set(e.STATE_COUNTS) == {"chignolin", "trp_cage", "bba", "villin"}
    for mol, K in e.STATE_COUNTS.items():
        c = np.asarray(e.STATE_CENTERS[mol], np.float64)
        assert c.shape == (K, 2) and np.all(np.isfinite(c))
    assert e.STATE_COUNTS["bba"] == 4 and e.STATE_COUNTS["chignolin"] == 3


def test_refusals_without_device():
    e = ev()
    F = 7 + 45
    tica = (np.zeros(F), np.ones((F, 2)))
    with pytest.raises(ValueError):
        e.StateTransitionEvaluator("protein_g", tica)                         # no preset, no centres
    with pytest.raises(ValueError):
        e.StateTransitionEvaluator("chignolin", tica, n_clusters=3)           # n_clusters without fit_data
    with pytest.raises(ValueError):
        e.StateTransitionEvaluator("chignolin", tica, np.zeros((3, 3)))       # centres of the wrong width
    with pytest.raises(ValueError):
        e.StateTransitionEvaluator("chignolin", object())
    s = e.StateTransitionEvaluator("chignolin", tica)
    assert s.n_states == 3 and np.array_equal(s.centers, np.asarray(e.STATE_CENTERS["chignolin"]))
    x = np.zeros((10, 10, 3), np.float32)
    with pytest.raises(ValueError):
        s.eval(x, traj_lengths=[3, 3])                                        # 6 != 10
    with pytest.raises(ValueError):
        s.eval(x, traj_lengths=[12, -2])
    with pytest.raises(NotImplementedError):
        s.eval(x, plot_transitions=True)
    with pytest.raises(ValueError):
        e.KMeans(0)
    with pytest.raises(ValueError):
        e.KMeans(3, init="random")
    with pytest.raises(ValueError):
        e.KMeans(3, initial_centers=np.zeros((2, 2)))


# ================================================================ GPU
def tic_model(N, k, seed, x):
    """a random projection whose coordinates are O(1) on the frames x, and K centres among the projected frames"""
    from dff_amd import binding
    rng = np.random.default_rng(seed)
    F = binding.struct_tic_num_features(N)
    f = binding.struct_tic_features(x[:256]).cpu().numpy().astype(np.float64) if len(x) else np.zeros((1, F))
    mean = f.mean(0)
    coeff = rng.standard_normal((F, k)) / (np.sqrt(F) * (f.std(0).mean() + 1.0))
    return mean, coeff


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 35, 56, 61])
def test_assign_projection_and_labels(dev, N):
    from dff_amd import binding
    for i, n in enumerate((0, 1, 63, 64, 65, 1000)):
        for vec4 in (True, False):
            k, K = (2, 4) if i % 2 == 0 else (3, 5)
            x = on_device(chain_frames(n, N, 100 * N + n), dev, vec4)
            mean, coeff = tic_model(N, k, N + i, x)
            ref = binding.struct_tic(x, mean, coeff)
            rng = np.random.default_rng(n)
            centers = (ref.cpu().numpy()[rng.choice(n, K, replace=False)] if n >= K else rng.standard_normal((K, k)))
            labels, proj, d2 = binding.struct_tic_assign(x, mean, coeff, centers, return_proj=True, return_dist2=True)
            assert labels.dtype == torch.int32 and labels.shape == (n,) and proj.shape == (n, k)
            assert torch.equal(proj, ref)                                        # bit-identical to dff_struct_tic
            assert torch.equal(binding.struct_tic_assign(x, mean, coeff, centers), labels)   # proj / dist2 NULL
            p = ref.cpu().numpy()
            want = check_labels(labels.cpu().numpy(), p, centers)
            if n:
                best = dist2_64(p, centers)[np.arange(n), want]
                assert np.allclose(d2.cpu().numpy(), best, rtol=1e-12, atol=1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("N,n,vec4", [(10, 200_003, True), (35, 200_001, False), (61, 200_000, True)])
def test_assign_large(dev, N, n, vec4):
    from dff_amd import binding
    x = on_device(chain_frames(n, N, N), dev, vec4)
    mean, coeff = tic_model(N, 2, N, x)
    ref = binding.struct_tic(x, mean, coeff)
    p = ref.cpu().numpy()
    centers = p[np.random.default_rng(N).choice(n, 4, replace=False)]
    labels, proj = binding.struct_tic_assign(x, mean, coeff, centers, return_proj=True)
    assert torch.equal(proj, ref)
    want = check_labels(labels.cpu().numpy(), p, centers)
    assert len(np.unique(want)) == 4


@pytest.mark.gpu
def test_assign_ties_and_nan(dev):
    from dff_amd import binding
    N, n = 10, 5000
    xh = chain_frames(n, N, 7)
    mean, coeff = tic_model(N, 2, 3, torch.from_numpy(xh).to(dev))        # from the clean frames
    xh[17, 3, 1] = np.nan
    xh[4000, 0, 0] = np.inf
    x = torch.from_numpy(xh).to(dev)
    p = binding.struct_tic(x, mean, coeff).cpu().numpy()
    c0, c1 = p[5], p[77]
    centers = np.stack([c0, c1, c0, c1])                      # 2 repeats 0, 3 repeats 1: the lower index must win
    labels, d2 = binding.struct_tic_assign(x, mean, coeff, centers, return_dist2=True)
    labels, d2 = labels.cpu().numpy(), d2.cpu().numpy()
    bad = ~np.isfinite(p).all(1)
    assert bad[17] and bad[4000] and bad.sum() == 2
    assert np.all(labels[bad] == -1) and np.all(np.isnan(d2[bad]))
    assert set(np.unique(labels[~bad])) == {0, 1}
    check_labels(labels[~bad], p[~bad], centers[:2])
    # the same rule in the k-means step
    r = binding.kmeans_step(torch.from_numpy(p).to(dev), centers, accumulate=True)
    assert np.array_equal(r["labels"].cpu().numpy(), labels)
    assert int(r["counts"].sum()) == n - 2 and int(r["counts"][2]) == 0 and int(r["counts"][3]) == 0
    assert np.allclose(float(r["inertia"][0]), d2[~bad].sum(), rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("d,K", [(1, 1), (2, 4), (3, 3), (8, 64), (2, 64)])
def test_kmeans_step(dev, d, K):
    from dff_amd import binding
    for n in (0, 1, 255, 256, 257, 200_001):
        rng = np.random.default_rng(1000 * d + K + n)
        true = rng.uniform(1.0, 10.0, (K, d))
        p = true[rng.integers(0, K, n)] + rng.uniform(0.0, 0.5, (n, d))          # positive coordinates
        centers = np.vstack([true, np.full((1, d), 1e6)]) if K < 64 else true    # + a centre nobody is near
        Kc = len(centers)
        pd = torch.from_numpy(p).to(dev)
        r = binding.kmeans_step(pd, centers)
        r2 = binding.kmeans_step(pd, centers)
        for key in ("labels", "dist2", "sums", "counts", "inertia"):
            assert torch.equal(r[key], r2[key]), key                             # bit-identical from call to call
        want = check_labels(r["labels"].cpu().numpy(), p, centers)
        counts = np.bincount(want, minlength=Kc)
        sums = np.stack([p[want == c].sum(0) for c in range(Kc)]) if n else np.zeros((Kc, d))
        inertia = dist2_64(p, centers)[np.arange(n), want].sum() if n else 0.0
        got_s, got_i = r["sums"].cpu().numpy(), float(r["inertia"][0])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.nanmax(np.abs(got_s - sums) / np.abs(sums), initial=0.0)
        print(f"kmeans_step d {d} K {K} n {n}: sums max rel err {rel:.3e}, inertia rel err "
              f"{abs(got_i - inertia) / max(inertia, 1e-300):.3e}")
        assert np.array_equal(r["counts"].cpu().numpy(), counts)                 # exact
        assert np.allclose(got_s, sums, rtol=1e-12, atol=0)
        assert np.isclose(got_i, inertia, rtol=1e-12, atol=0)
        if K < 64:
            assert counts[-1] == 0 and np.all(got_s[-1] == 0.0)                  # the empty cluster
        a = binding.kmeans_step(pd, centers, accumulate=False)                   # plain assignment
        assert torch.equal(a["labels"], r["labels"]) and torch.equal(a["dist2"], r["dist2"]) and "sums" not in a


@pytest.mark.gpu
@pytest.mark.parametrize("K,d", [(3, 2), (4, 2), (3, 3), (4, 3)])
def test_kmeans_fit(dev, K, d):
    e = ev()
    true, p, _ = blobs(K, d, 3000, seed=10 * K + d)
    rng = np.random.default_rng(K + d)
    init = true + rng.standard_normal((K, d)) * 3.0
    km = e.KMeans(K, max_iter=100, tolerance=1e-5, initial_centers=init).fit(p)
    c64, it64, in64 = lloyd64(p, init, 100, 1e-5)
    print(f"kmeans fit K {K} d {d}: n_iter {km.n_iter} / {it64}, centres max rel err "
          f"{np.abs(km.cluster_centers / c64 - 1).max():.3e}")
    assert km.n_iter == it64
    assert np.allclose(km.cluster_centers, c64, rtol=1e-10, atol=0)
    assert np.isclose(km.inertia, in64, rtol=1e-10)
    assert np.array_equal(km.transform(p), dist2_64(p, c64).argmin(1))
    # max_iter = 0: the notebook's call, the centres untouched
    k0 = e.KMeans(K, max_iter=0, initial_centers=init)
    lab0 = k0.fit_transform(p)
    assert k0.n_iter == 0 and np.array_equal(k0.cluster_centers, init)
    check_labels(lab0, p, init)
    # k-means++: reproducible, and one centre per blob
    a = e.KMeans(K, seed=5).fit(p)
    b = e.KMeans(K, seed=5).fit(p)
    assert np.array_equal(a.cluster_centers, b.cluster_centers) and a.n_iter == b.n_iter and a.inertia == b.inertia
    owner = dist2_64(a.cluster_centers, true).argmin(1)
    assert sorted(owner) == list(range(K)), owner
    assert np.allclose(a.cluster_centers[np.argsort(owner)], c64[np.argsort(dist2_64(c64, true).argmin(1))], rtol=1e-8)


@pytest.mark.gpu
def test_kmeans_inertias_non_increasing(dev):
    e = ev()
    _, p, _ = blobs(3, 2, 4000, seed=2)
    ks = (1, 2, 3, 4, 5)
    inert = e.kmeans_inertias(p, ks, seed=1)
    print("inertias", inert)
    assert inert.shape == (5,) and np.all(np.isfinite(inert)) and np.all(np.diff(inert) <= 0)
    assert inert[2] < 0.01 * inert[1]                                            # the elbow at the true k = 3


TRANSITION_LENGTHS = [
    [5000],
    [0, 1, 100, 101, 5000, 0, 7, 8, 1, 30000, 2, 0],
    [1000] * 50,                                              # equal lengths: the sampler's output
    [0, 640, 640, 0, 640],                                    # equal but for empty ones
]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 4, 64])
@pytest.mark.parametrize("lags", [(1,), (1, 7, 100)])
def test_transition_counts(dev, K, lags):
    from dff_amd import binding
    rng = np.random.default_rng(K + len(lags))
    many = [int(v) for v in rng.integers(0, 300, 150)]                           # more trajectories than one launch takes
    big = [200_000, 37, 100_001]
    for lengths in TRANSITION_LENGTHS + [many, big]:
        n = sum(lengths)
        lab = rng.integers(0, K, n).astype(np.int32)
        lab[rng.random(n) < 0.02] = -1
        ld = torch.from_numpy(lab).to(dev)
        got = binding.transition_counts(ld, lengths, lags, K)
        assert got.dtype == torch.int64 and got.shape == (len(lags), K, K)
        want, skipped = counts64(lab, lengths, lags, K)
        assert np.array_equal(got.cpu().numpy(), want)
        for li, lag in enumerate(lags):
            assert int(got[li].sum()) == sum(max(L - lag, 0) for L in lengths) - skipped[li]
        assert torch.equal(binding.transition_counts(ld, lengths, lags, K), got)
        # one trajectory of n frames: the notebook's single dtraj; it differs by exactly the pairs across boundaries
        single = binding.transition_counts(ld, [n], lags, K).cpu().numpy()
        assert np.array_equal(single, counts64(lab, [n], lags, K)[0])
        tid = np.repeat(np.arange(len(lengths)), lengths)
        for li, lag in enumerate(lags):
            a, b = lab[:-lag].astype(np.int64), lab[lag:].astype(np.int64)
            cross = (tid[:-lag] != tid[lag:]) & (a >= 0) & (b >= 0)
            D = np.zeros((K, K), np.int64)
            np.add.at(D, (a[cross], b[cross]), 1)
            assert np.array_equal(single[li] - want[li], D)
    # no frames at all
    z = binding.transition_counts(torch.empty(0, dtype=torch.int32, device=dev), [], lags, K)
    assert z.shape == (len(lags), K, K) and not z.any()


@pytest.mark.gpu
def test_end_to_end_two_state(dev, golden):
    e = ev()
    folded = golden("struct_folded.npz")["chignolin"]
    lengths = [4000, 2500, 3500]
    x = np.concatenate(two_state_trajectories(folded, lengths, seed=11))
    tica = e.TICA(10, dim=2).fit(x, traj_lengths=lengths)
    st = e.StateTransitionEvaluator("toy", tica, n_clusters=2, fit_data=x)
    res = st.eval(x, traj_lengths=lengths, lagtimes=(1, 10))
    # the float64 pipeline on tica.transform's projections
    p = tica.transform(x)
    init = np.stack([p[np.argmin(p[:, 0])], p[np.argmax(p[:, 0])]])
    c64, _, _ = lloyd64(p, init, 100, 1e-5)
    order = dist2_64(c64, st.centers).argmin(1)                  # the oracle's centre i is the evaluator's order[i]
    assert sorted(order) == [0, 1]
    assert np.allclose(st.centers[order], c64, rtol=1e-8, atol=1e-10)
    lab = res["assignments"]
    assert lab.dtype == np.int32 and np.array_equal(lab, st.assign(x))
    check_labels(lab, p, st.centers)
    want, _ = counts64(lab, lengths, (1, 10), 2)
    assert np.array_equal(res["count_matrices"], want)
    assert want[0].sum() == sum(L - 1 for L in lengths) and want[1].sum() == sum(L - 10 for L in lengths)
    T = want / want.sum(-1, keepdims=True)
    assert np.allclose(res["transition_matrices"], T, rtol=1e-15)
    assert np.allclose(res["populations"], np.bincount(lab, minlength=2) / len(lab), rtol=1e-15)
    for i, lag in enumerate((1, 10)):
        lam2 = np.linalg.det(T[i])                                # 2 x 2 stochastic matrix: eigenvalues 1 and det
        assert np.allclose(res["timescales"][i], [-lag / np.log(abs(lam2))], rtol=1e-10)
    assert min(res["populations"]) > 0.1 and T[0, 0, 0] > 0.9 and T[0, 1, 1] > 0.9     # two metastable states
    # as one trajectory (the notebook): the two boundary pairs per lag come on top
    one = st.eval(x, lagtimes=(1,))["count_matrices"]
    assert one.sum() == len(x) - 1 and np.all(one[0] >= want[0])
    # the constructor's traj_lengths is eval's default
    st2 = e.StateTransitionEvaluator("toy", (tica.mean, tica.coeff), st.centers, traj_lengths=lengths)
    assert np.array_equal(st2.eval(x, lagtimes=(1, 10))["count_matrices"], want)


@pytest.mark.gpu
def test_chignolin_presets_assign(dev, golden):
    e = ev()
    path = os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle")
    folded = golden("struct_folded.npz")["chignolin"]
    x = np.concatenate(two_state_trajectories(folded, [700, 300], seed=3, amp=1.0, sigma=1.0))
    st = e.StateTransitionEvaluator("chignolin", path)
    assert st.n_states == 3 and np.array_equal(st.centers, np.asarray(e.STATE_CENTERS["chignolin"]))
    lab = st.assign(x)
    assert lab.shape == (1000,) and lab.dtype == np.int32 and lab.min() >= 0 and lab.max() <= 2
    ref = e.load_tica_reference(path)
    from dff_amd import binding
    p = binding.struct_tic(torch.from_numpy(x).to(dev), ref["mean"], ref["coeff"]).cpu().numpy()
    check_labels(lab, p, st.centers)
    res = st.eval(x, traj_lengths=[700, 300])
    assert res["count_matrices"].shape == (1, 3, 3) and res["count_matrices"].sum() == 998
    assert np.array_equal(res["assignments"], lab)


@pytest.mark.gpu
def test_states_abi_refuses_bad_arguments(dev):
    from dff_amd import binding
    lib = binding.load_library()

    def refused(fn, *a, **kw):
        with pytest.raises(ValueError) as info:
            fn(*a, **kw)
        assert len(str(info.value)) > 20                                         # dff_last_error's message came along

    for N in (3, 65):
        F = max(binding.struct_tic_num_features(N), 1) if N > 3 else 1
        # the binding checks mean / coeff against F itself: go to the ABI for the bead count
        x = torch.zeros((8, N, 3), device=dev)
        m, A = torch.zeros(F, dtype=torch.float64, device=dev), torch.zeros((F, 2), dtype=torch.float64, device=dev)
        c, lab = torch.zeros((2, 2), dtype=torch.float64, device=dev), torch.full((8,), 7, dtype=torch.int32, device=dev)
        rc = lib.dff_struct_tic_assign(0, x.data_ptr(), 8, N, m.data_ptr(), A.data_ptr(), 2, c.data_ptr(), 2,
                                       lab.data_ptr(), None, None, None)
        assert rc == 1 and b"n_beads" in lib.dff_last_error()
        torch.cuda.synchronize()
        assert bool((lab == 7).all())                                            # nothing launched
    N = 10
    F = binding.struct_tic_num_features(N)
    x = torch.zeros((8, N, 3), device=dev)
    mean = np.zeros(F)
    refused(binding.struct_tic_assign, x, mean, np.zeros((F, 0)), np.zeros((2, 0)))          # k = 0
    refused(binding.struct_tic_assign, x, mean, np.zeros((F, 9)), np.zeros((2, 9)))          # k = 9
    refused(binding.struct_tic_assign, x, mean, np.zeros((F, 2)), np.zeros((0, 2)))          # K = 0
    refused(binding.struct_tic_assign, x, mean, np.zeros((F, 2)), np.zeros((65, 2)))         # K = 65
    p = torch.zeros((300, 2), dtype=torch.float64, device=dev)
    refused(binding.kmeans_step, p, np.zeros((0, 2)))
    refused(binding.kmeans_step, p, np.zeros((65, 2)))
    refused(binding.kmeans_step, torch.zeros((300, 9), dtype=torch.float64, device=dev), np.zeros((2, 9)))   # d = 9
    refused(binding.kmeans_workspace_bytes, 300, 0, 2)
    refused(binding.kmeans_workspace_bytes, 300, 2, 65)
    need = binding.kmeans_workspace_bytes(300, 2, 4)
    assert need > 0
    small = torch.empty(need - 8, dtype=torch.uint8, device=dev)
    refused(binding.kmeans_step, p, np.zeros((4, 2)), workspace=small)                       # workspace too small
    with pytest.raises(ValueError, match="kmeans_step: the workspace must be 8-byte aligned"):  # the partials are doubles
        binding.kmeans_step(p, np.zeros((4, 2)), workspace=torch.empty(need + 4, dtype=torch.uint8, device=dev)[4:])
    binding.kmeans_step(p, np.zeros((4, 2)), workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    lab = torch.zeros(300, dtype=torch.int32, device=dev)
    refused(binding.transition_counts, lab, [300], (0,), 3)                                  # lag = 0
    refused(binding.transition_counts, lab, [300], (1, -1), 3)
    refused(binding.transition_counts, lab, [300], tuple(range(1, 10)), 3)                   # n_lags = 9
    refused(binding.transition_counts, lab, [300], (), 3)                                    # n_lags = 0
    refused(binding.transition_counts, lab, [100, 150], (1,), 3)                             # lengths sum to 250
    refused(binding.transition_counts, lab, [301, -1], (1,), 3)
    refused(binding.transition_counts, lab, [300], (1,), 0)                                  # K = 0
    refused(binding.transition_counts, lab, [300], (1,), 65)                                 # K = 65
    got = binding.transition_counts(lab, [300], (1,), 3)                                     # the same call, valid
    assert int(got[0, 0, 0]) == 299 and int(got.sum()) == 299
