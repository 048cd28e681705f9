"""Fitting TICA models: evaluate.TICA, the host algebra (tica_covariances, tica_from_covariances) and the HIP kernels
dff_struct_tic_features / dff_tica_moments (csrc/dff_tica.hip).

CPU part: the decomposition against the reference's saved chignolin model (its pickle) and trp-cage model
(tests/golden/tica_trp_cage_cov.npz, recorded by tests/golden/make_golden_tica_fit.py), the sums -> covariances algebra
against direct centred formulas, rank truncation, refusals and the .npz round trip.
GPU part (-m gpu): features and moments against float64 numpy (oracle/struct_metric.py, oracle/tica_fit.py), determinism and
streaming, fits of seeded Ornstein-Uhlenbeck trajectories against a float64 pipeline, the evaluators' fit path, and the ABI's refusals.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.frames import ou_trajectories
from oracle.struct_metric import tic_features64
from oracle.tica_fit import mirror, moments64, sign_aligned_rel
from support import dev, ev  # noqa: F401  (dev: fixture)


def fit64(f, lengths, lag, dim=2):
    """the whole fit in float64 numpy on given features f (n, F): shift = f[0].  (Not in oracle/tica_fit.py: it runs the
    product's own host algebra on the oracle's moments, and oracle/ does not import dff_amd.)"""
    s = np.asarray(f[0], np.float64)
    sx, sy, m0, mt, w = moments64(np.asarray(f, np.float64) - s, lengths, lag)
    mean, c00, c0t = ev().tica_covariances(sx, sy, m0, mt, w, s)
    return ev().tica_from_covariances(c00, c0t, mean, dim)


# ================================================================ CPU
def test_decomposition_matches_chignolin_pickle():
    t = ev().restricted_load(os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))[0]
    cov, model = t._model._cov, t._model
    m = ev().tica_from_covariances(cov._cov_00, cov._cov_0t, cov._mean_0, dim=2, epsilon=t._epsilon)
    assert m["rank"] == 52
    np.testing.assert_allclose(m["singular_values"], model._singular_values, rtol=0, atol=1e-10)
    rel = sign_aligned_rel(m["full_coeff"], np.asarray(model._whitening_instantaneous.sqrt_inv_cov))
    assert rel[:8].max() <= 1e-9 and rel.max() <= 1e-7, rel
    assert np.array_equal(m["coeff"], m["full_coeff"][:, :2]) and np.array_equal(m["mean"], cov._mean_0)
    big = np.abs(m["full_coeff"]).argmax(0)
    assert np.all(m["full_coeff"][big, np.arange(52)] > 0)          # the documented sign convention


def test_decomposition_matches_trp_cage_model(golden):
    z = golden("tica_trp_cage_cov.npz")
    F = len(z["mean"])
    m = ev().tica_from_covariances(mirror(z["cov_00_triu"], F), mirror(z["cov_0t_triu"], F), z["mean"], dim=2,
                                   epsilon=float(z["epsilon"]))
    assert m["rank"] == F == 207
    np.testing.assert_allclose(m["singular_values"], z["singular_values"], rtol=0, atol=1e-10)
    R = z["sqrt_inv_cov_lead"]
    rel = sign_aligned_rel(m["full_coeff"][:, :R.shape[1]], R)
    assert rel.max() <= 1e-9, rel
    ts = ev().tica_timescales(m["singular_values"][:2], int(z["lagtime"]))
    np.testing.assert_allclose(ts, -100.0 / np.log(np.abs(z["singular_values"][:2])), rtol=1e-12)


@pytest.mark.parametrize("lag", [1, 3])
def test_sums_to_covariances(lag):
    """tica_covariances on the kernel's sums (upper triangles only) = deeptime's symmetrised centred formulas."""
    rng = np.random.default_rng(lag)
    F = 7
    lengths = [1, lag, lag + 1, 9, 0, 23, 2]                    # L <= tau contributes nothing
    n = sum(lengths)
    f = rng.standard_normal((n, F)) * rng.uniform(0.5, 3, F) + rng.uniform(-10, 10, F)
    s = f[0]
    sx, sy, m0, mt, w = moments64(f - s, lengths, lag)
    mean, c00, c0t = ev().tica_covariances(sx, sy, np.triu(m0), np.triu(mt), w, s)
    X, Y, o = [], [], 0
    for L in lengths:
        if L > lag:
            X.append(f[o:o + L - lag])
            Y.append(f[o + lag:o + L])
        o += L
    X, Y = np.concatenate(X), np.concatenate(Y)
    mu = (X.sum(0) + Y.sum(0)) / (2 * len(X))
    Xc, Yc = X - mu, Y - mu
    np.testing.assert_allclose(mean, mu, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(c00, (Xc.T @ Xc + Yc.T @ Yc) / (2 * len(X)), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(c0t, (Xc.T @ Yc + Yc.T @ Xc) / (2 * len(X)), rtol=1e-11, atol=1e-11)
    assert w == sum(max(L - lag, 0) for L in lengths)


def test_epsilon_truncates_rank():
    rng = np.random.default_rng(5)
    F, r = 12, 7
    A = rng.standard_normal((F, r))
    c00 = A @ A.T + 1e-9 * np.eye(F)                                # 5 eigenvalues at 1e-9 < epsilon
    B = rng.standard_normal((F, r))
    c0t = 0.5 * (A @ B.T + B @ A.T) * 0.1
    m = ev().tica_from_covariances(c00, c0t, np.zeros(F), dim=2, epsilon=1e-6)
    assert m["rank"] == r and m["full_coeff"].shape == (F, r) and len(m["singular_values"]) == r
    assert np.all(np.diff(np.abs(m["singular_values"])) <= 0)
    W = m["full_coeff"]
    np.testing.assert_allclose(W.T @ c00 @ W, np.diag(m["singular_values"] ** 2), atol=1e-8)
    assert ev().tica_from_covariances(c00, c0t, np.zeros(F), dim=2, epsilon=1e-12)["rank"] == F


def test_refusals():
    e = ev()
    F = 6
    with pytest.raises(ValueError):
        e.tica_covariances(np.zeros(F), np.zeros(F), np.zeros((F, F)), np.zeros((F, F)), 0, np.zeros(F))   # w = 0
    c = np.diag([1.0, 1.0, 1e-9, 1e-9, 1e-9, 1e-9])
    with pytest.raises(ValueError):
        e.tica_from_covariances(c, 0.5 * c, np.zeros(F), dim=3)                    # dim > rank 2
    with pytest.raises(ValueError):
        e.tica_from_covariances(np.eye(12), 0.5 * np.eye(12), np.zeros(12), dim=9)  # dim > 8
    with pytest.raises(ValueError):
        e.tica_from_covariances(np.eye(F), 0.5 * np.eye(F), np.zeros(F), scaling="commute_map")


def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    F = 9
    A = rng.standard_normal((F, 40))
    c00 = A @ A.T / 40
    c0t = 0.3 * c00 + 0.01 * np.eye(F)
    m = ev().tica_from_covariances(c00, c0t, rng.standard_normal(F), dim=3)
    m["cov_00"], m["cov_0t"] = c00, c0t
    p = str(tmp_path / "model.npz")
    ev().save_tica_model(p, m, 25, gt_prob=np.ones((4, 4)), bin_edges_x=np.arange(5.0), bin_edges_y=np.arange(5.0))
    t = ev().load_tica_reference(p, dim=3)
    assert np.array_equal(t["mean"], m["mean"]) and np.array_equal(t["coeff"], m["coeff"])
    assert np.array_equal(t["singular_values"], m["singular_values"]) and int(t["lagtime"]) == 25
    assert np.array_equal(ev().load_tica_reference(p)["coeff"], m["coeff"][:, :2])


def check_plan(plan, lengths, lag, C):
    """every valid pair start (t, t + lag in one trajectory) exactly once, runs of > 0 pairs, chunks within their limits"""
    starts = np.concatenate([np.arange(o, o + L - lag) for o, L in zip(np.cumsum([0] + list(lengths[:-1])), lengths)
                             if L > lag] or [np.zeros(0, np.int64)])
    got = []
    for chunk in np.unique(plan[:, 0]):
        runs = plan[plan[:, 0] == chunk]
        f0, rows, pairs = runs[0, 1:4]
        assert np.all(runs[:, 1:4] == runs[0, 1:4]) and len(runs) <= 64
        assert np.all(runs[:, 5] > 0) and runs[:, 5].sum() == pairs and 0 < pairs <= C
        assert rows <= C + lag and runs[0, 4] == 0
        t = np.concatenate([f0 + r + np.arange(k) for r, k in runs[:, 4:6]])
        assert t.max() < f0 + C and t.max() + lag == f0 + rows - 1
        got.append(t)
    got = np.concatenate(got) if got else np.zeros(0, np.int64)
    assert np.array_equal(got, starts)       # in order, each once: no pair crosses a trajectory


def test_chunk_plan_covers_every_pair_once():
    """The chunking of dff_tica_moments (host code, no GPU): trajectory tails and short trajectories across the chunk
    limit, splits inside a trajectory, more runs than one launch holds, at the real chunk sizes and small ones."""
    from dff_amd import binding
    lag = 100
    layouts = [[4500] * 64, [18250] * 64, [32350, 700], [32350, 700, 40000], [1000] + [50] * 1000 + [1000],
               [7] * 150, [101] * 200, [0, 100, 101, 0], [100], [250_000]]
    for L in range(1000, 60001, 1700):
        layouts.append([L] * 64)
    for N in (10, 28, 35, 56, 64):
        for lengths in layouts:
            plan = binding.tica_debug_plan(N, lengths, lag)
            C = (1 << 28) // (4 * binding.struct_tic_num_features(N)) // 32 * 32
            check_plan(plan, lengths, lag, C)
    rng = np.random.default_rng(0)
    for trial in range(300):                 # small chunk sizes: every boundary case many times over
        lag = int(rng.integers(1, 12))
        lengths = [int(v) for v in rng.integers(0, 40, int(rng.integers(1, 90)))]
        C = int(rng.integers(1, 60))
        check_plan(binding.tica_debug_plan(10, lengths, lag, C), lengths, lag, C)


# ================================================================ GPU
def gpu_moments(x, lengths, lag, shift, workspace=None):
    from dff_amd import binding
    F = binding.struct_tic_num_features(x.shape[1])
    acc = [torch.zeros(s, dtype=torch.float64, device=x.device) for s in ((F,), (F,), (F, F), (F, F))]
    sh = torch.as_tensor(shift, dtype=torch.float64).to(x.device).contiguous()
    binding.tica_moments(x, lengths, lag, sh, *acc, workspace=workspace)
    return [a.cpu().numpy() for a in acc]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 20, 64])
def test_features_match_float64_and_projection(dev, N):
    from dff_amd import binding
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((333, N, 3)) * 4 + np.arange(N)[None, :, None] * 3.0).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    f = binding.struct_tic_features(xd).cpu().numpy()
    nd = N - 3
    assert f.shape == (333, binding.struct_tic_num_features(N)) and f.dtype == np.float32
    assert np.array_equal(f[:, :nd], binding.struct_dihedrals(xd).cpu().numpy())
    ref = tic_features64(x)
    assert np.all(np.abs(f[:, nd:] - ref[:, nd:]) <= 1e-6 * ref[:, nd:])          # distances: fp32 rounding
    # dihedrals of non-degenerate quadruples (neither bond angle within ~6 degrees of 0 or 180): fp32 rounding
    b = np.diff(x.astype(np.float64), axis=1)
    sin = np.linalg.norm(np.cross(b[:, :-1], b[:, 1:]), axis=-1) / (
        np.linalg.norm(b[:, :-1], axis=-1) * np.linalg.norm(b[:, 1:], axis=-1))
    good = (sin[:, :-1] > 0.1) & (sin[:, 1:] > 0.1)
    err = np.abs(np.angle(np.exp(1j * (f[:, :nd] - ref[:, :nd]))))
    assert good.mean() > 0.8 and err[good].max() <= 2e-5, err[good].max()
    # the same features dff_struct_tic projects
    F = f.shape[1]
    mean, A = rng.standard_normal(F), rng.standard_normal((F, 8))
    got = binding.struct_tic(xd, mean, A).cpu().numpy()
    want = (f.astype(np.float64) - mean) @ A
    bound = np.abs(f.astype(np.float64) - mean) @ np.abs(A)
    assert np.all(np.abs(got - want) <= 1e-12 * bound)


MOMENT_CASES = [  # (N, lag, lengths)
    (4, 1, [200]),
    (5, 7, [3, 7, 8, 150, 1, 64, 65, 33]),
    (10, 100, [1000, 50, 100, 101, 333]),
    (20, 7, [517]),
    (35, 1, [2, 1, 97, 211]),
    (56, 100, [1111, 99]),
    (64, 7, [300, 8, 129]),
    (10, 1, [7] * 150),                         # more runs than one launch holds (64)
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,lag,lengths", MOMENT_CASES)
def test_moments_match_float64(dev, N, lag, lengths):
    from dff_amd import binding
    rng = np.random.default_rng(N * 1000 + lag)
    n = sum(lengths)
    x = torch.from_numpy((rng.standard_normal((n, N, 3)) * 3 + np.arange(N)[None, :, None] * 2.5).astype(np.float32)).to(dev)
    f = binding.struct_tic_features(x).cpu().numpy().astype(np.float64)
    s = f[0] + rng.standard_normal(f.shape[1]) * 0.1
    got = gpu_moments(x, lengths, lag, s)
    ref = moments64(f - s, lengths, lag)
    iu = np.triu_indices(f.shape[1])
    for k, (a, b) in enumerate(zip(got, ref[:4])):
        if k >= 2:
            assert np.all(np.tril(a, -1) == 0), "the lower triangle is not touched"
            a, b = a[iu], b[iu]
        assert np.abs(a - b).max() <= 1e-11 * max(np.abs(b).max(), 1e-300), (k, np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.gpu
def test_moments_large_n_and_protein_g_width(dev):
    from dff_amd import binding
    rng = np.random.default_rng(17)
    for N, lengths, lag in ((5, [310_001, 12_345], 100), (56, [20_011], 100)):      # > 300 k frames; F = 1 593
        n = sum(lengths)
        x = torch.from_numpy((rng.standard_normal((n, N, 3)) * 3 + np.arange(N)[None, :, None] * 2.0)
                             .astype(np.float32)).to(dev)
        f = binding.struct_tic_features(x).cpu().numpy().astype(np.float64)
        assert f.shape[1] == (1593 if N == 56 else 12)
        s = f[0]
        got = gpu_moments(x, lengths, lag, s)
        ref = moments64(f - s, lengths, lag)
        iu = np.triu_indices(f.shape[1])
        for k, (a, b) in enumerate(zip(got, ref[:4])):
            if k >= 2:
                a, b = a[iu], b[iu]
            assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), (N, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N,lengths", [
    (64, [32_350, 700, 33_000]),            # C = 32 288: a tail across the chunk limit, then a split inside a trajectory
    (56, [1000] + [50] * 1000 + [1000]),    # C = 42 112: a thousand trajectories of <= lag frames across the limit
])
def test_moments_across_chunks(dev, N, lengths):
    from dff_amd import binding
    rng = np.random.default_rng(N)
    lag = 100
    n = sum(lengths)
    C = (1 << 28) // (4 * binding.struct_tic_num_features(N)) // 32 * 32
    assert n > C and len(np.unique(binding.tica_debug_plan(N, lengths, lag)[:, 0])) >= 2
    x = torch.from_numpy((rng.standard_normal((n, N, 3)) * 3 + np.arange(N)[None, :, None] * 2.0)
                         .astype(np.float32)).to(dev)
    f = binding.struct_tic_features(x).cpu().numpy().astype(np.float64)
    s = f[0]
    got = gpu_moments(x, lengths, lag, s)
    ref = moments64(f - s, lengths, lag)
    iu = np.triu_indices(f.shape[1])
    for k, (a, b) in enumerate(zip(got, ref[:4])):
        if k >= 2:
            a, b = a[iu], b[iu]
        assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), (N, k)


@pytest.mark.gpu
def test_moments_deterministic_and_streaming(dev, golden):
    e = ev()
    folded = golden("struct_folded.npz")["trp_cage"]
    A, B = ou_trajectories(folded, [3000, 2500], seed=2)
    xa, xb = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    s = np.linspace(-1.0, 1.0, 207)
    r1 = gpu_moments(xa, [1700, 1300], 100, s)
    r2 = gpu_moments(xa, [1700, 1300], 100, s)
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2))
    t1 = e.TICA(100).partial_fit(A).partial_fit(B)
    t2 = e.TICA(100).fit(np.concatenate([A, B]), traj_lengths=[len(A), len(B)])
    t3 = e.TICA(100).fit([B, A])               # other order: other shift (B's first frame), other summation order
    for t in (t2, t3):
        for name in ("mean", "cov_00", "cov_0t"):
            a, b = getattr(t1, name), getattr(t, name)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
    assert t1.n_pairs == len(A) + len(B) - 200


@pytest.mark.gpu
@pytest.mark.parametrize("mol", ["chignolin", "trp_cage"])
def test_fit_end_to_end_float32_band(dev, golden, mol):
    """GPU fit vs a float64 pipeline on float64 features: no further than 2x that pipeline on the kernel's fp32 features."""
    from dff_amd import binding
    e = ev()
    folded = golden("struct_folded.npz")[mol]
    lengths, lag = [6000, 4000], 100
    trajs = ou_trajectories(folded, lengths, seed=1 if mol == "chignolin" else 3)
    x = np.concatenate(trajs)
    tica = e.TICA(lag, dim=2).fit(trajs)
    f32 = binding.struct_tic_features(torch.from_numpy(x).to(dev)).cpu().numpy()
    m64 = fit64(tic_features64(x), lengths, lag)            # full fp64 pipeline
    m32 = fit64(f32, lengths, lag)                          # fp64 pipeline on the kernel's fp32 features
    fx = tic_features64(x)

    def dists(sv, mean, coeff):
        p = (fx - mean) @ coeff
        q = (fx - m64["mean"]) @ m64["coeff"]
        p = p * np.sign((p * q).sum(0))
        return (np.abs(sv[:2] - m64["singular_values"][:2]).max(),
                (np.linalg.norm(p - q, axis=0) / np.linalg.norm(q, axis=0)).max(),
                np.abs(e.tica_timescales(sv[:2], lag) / e.tica_timescales(m64["singular_values"][:2], lag) - 1).max())

    d_gpu = dists(tica.singular_values, tica.mean, tica.coeff)
    d_32 = dists(m32["singular_values"], m32["mean"], m32["coeff"])
    for a, b in zip(d_gpu, d_32):
        assert a <= 2 * b + 1e-13, (d_gpu, d_32)
    assert abs(tica.singular_values[0]) > 0.5 and np.all(np.isfinite(tica.timescales()))
    proj = tica.transform(x)
    assert proj.shape == (len(x), 2) and np.allclose(proj, (f32.astype(np.float64) - tica.mean) @ tica.coeff,
                                                     rtol=0, atol=1e-9 * np.abs(proj).max())


@pytest.mark.gpu
def test_evaluators_fit_when_no_saved_model(dev, golden, tmp_path):
    e = ev()
    folded = golden("struct_folded.npz")
    # BBA: TicEvaluator with fit_data
    fit = ou_trajectories(folded["bba"], [1500, 1200], seed=4)
    val, samp = ou_trajectories(folded["bba"], [800, 600], seed=5)
    ref_path = str(tmp_path / "saved_TICA_BBA_testset.pickle")
    with pytest.raises(NotImplementedError):
        e.TicEvaluator(val, "bba", saved_ref=ref_path)
    t1 = e.TicEvaluator(val, "bba", saved_ref=ref_path, fit_data=fit, lagtime=20)
    js1 = t1.eval(samp)[0]
    assert np.isfinite(js1) and os.path.exists(str(tmp_path / "saved_TICA_BBA_testset.npz"))
    assert not os.path.exists(ref_path)
    npz_path = str(tmp_path / "saved_TICA_BBA_testset.npz")
    mtime = os.path.getmtime(npz_path)
    t2 = e.TicEvaluator(val, "bba", saved_ref=npz_path)
    assert t2.eval(samp)[0] == js1
    t3 = e.TicEvaluator(val, "bba", saved_ref=ref_path, fit_data=fit, lagtime=20)    # loads the .npz, no refit
    assert t3.eval(samp)[0] == js1 and os.path.getmtime(npz_path) == mtime
    with pytest.raises(NotImplementedError):                                         # no fit_data: as before
        e.TicEvaluator(val, "bba", saved_ref=ref_path)
    assert t1.gt_prob.shape == (101, 101) and abs(t1.gt_prob.sum() * np.prod([np.diff(t1.bin_edges_x)[0],
                                                                               np.diff(t1.bin_edges_y)[0]]) - 1) < 1e-9
    # villin: Evaluator with tica_fit_data
    fit = ou_trajectories(folded["villin"], [1500], seed=6)
    val, samp = ou_trajectories(folded["villin"], [700, 500], seed=7)
    vt = torch.from_numpy(val)
    r1 = e.Evaluator(vt, None, "villin", saved_ref_dir=str(tmp_path), tica_fit_data=fit, tica_lagtime=20).eval(samp, 0)
    assert np.isfinite(r1["TIC JS"]) and np.isfinite(r1["PWD JS"])
    assert os.path.exists(str(tmp_path / "saved_TICA_VILLIN_testset.npz"))
    r2 = e.Evaluator(vt, None, "villin", saved_ref_dir=str(tmp_path)).eval(samp, 0)
    assert r2["TIC JS"] == r1["TIC JS"]


@pytest.mark.gpu
def test_tica_abi_refuses_bad_arguments(dev):
    from dff_amd import binding

    def acc(F):
        return [torch.zeros(s, dtype=torch.float64, device=dev) for s in ((F,), (F,), (F,), (F, F), (F, F))]

    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    for N in (3, 65):
        F = binding.struct_tic_num_features(N)
        with pytest.raises(ValueError):
            binding.tica_moments(torch.zeros((300, N, 3), device=dev), [300], 10, *acc(F), workspace=ws)
        with pytest.raises(ValueError):
            binding.tica_workspace_bytes(N, 300, 10)
    x = torch.zeros((300, 10, 3), device=dev)
    F = binding.struct_tic_num_features(10)
    big = torch.empty(binding.tica_workspace_bytes(10, 300, 10), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        binding.tica_moments(x, [100, 150], 10, *acc(F), workspace=big)          # lengths sum to 250, not 300
    with pytest.raises(ValueError):
        binding.tica_moments(x, [300], 0, *acc(F), workspace=big)                # lagtime 0
    with pytest.raises(ValueError):
        binding.tica_moments(x, [300], 10, *acc(F), workspace=big[:4096])        # workspace too small
    odd = torch.empty(big.numel() + 4, dtype=torch.uint8, device=dev)[4:]        # room enough, at 4 mod 8: the partial sums are doubles
    with pytest.raises(ValueError, match="tica_moments: the workspace must be 8-byte aligned"):
        binding.tica_moments(x, [300], 10, *acc(F), workspace=odd)
    a = acc(F)
    binding.tica_moments(x, [300], 10, *a, workspace=big)                        # the same call with room: accepted
    assert all(bool((t == 0).all()) for t in a)                                  # zero frames -> zero moments
