"""dff_sym_eig_topk on the GPU (csrc/dff_sym_eig.hip) and evaluate.msm_spectrum / MarkovStateModel.eigenvectors /
eigensolver="device" on top of it.  tests/eig_cases.py holds the matrices, the measures rho / omega / delta and their bars
(8 x LAPACK's own value on the same case, capped by max(K, 32) units); the kernel is never its own reference.

Every size runs all kinds of eig_cases.kinds in one call with k = 8, on each path that takes the size; the figures are printed
per case.

MEASURED on the MI355X, worst over the kinds of a size, in units (u = 2^-52 |A|_2 for rho and delta, 2^-52 for omega), the kernel's
value and in brackets LAPACK's on the same cases (the full table is DESIGN.md section 21):
  K      rho LDS / workspace (LAPACK)   omega LDS / workspace (LAPACK)   delta
  2      0.71 / 0.71 (0.61)             1.92 / 1.92 (0.99)               0.88
  3      2.06 / 2.06 (1.51)             1.70 / 1.70 (3.77)               1.00
  5      1.56 / 1.56 (1.91)             1.87 / 1.87 (4.14)               2.00
  16     3.54 / 4.33 (5.72)             1.86 / 2.24 (6.58)               4.71
  17     2.54 / 2.44 (5.68)             2.14 / 2.34 (9.99)               3.50
  21 W+  0.83 / 0.83 (1.11)             1.79 / 2.07 (2.90)               1.49
  33     3.39 / 2.93 (4.44)             1.78 / 2.26 (9.89)               3.00
  64     3.68 / 3.99 (5.11)             1.68 / 2.12 (9.11)               5.00
  65     5.29 / 4.10 (8.74)             2.75 / 2.75 (8.14)               4.00
  128    3.58 / 3.45 (5.49)             1.31 / 2.14 (10.88)              3.50
  257       - / 2.91 (4.37)                - / 2.17 (15.0)               3.07
  1024      - / 5.12 (2.77)                - / 2.04 (5.35)               3.00
Every bar is 8 x LAPACK's value (floored at one unit), capped by max(K, 32): no case uses more than a fifth of its bar except
K = 1024, whose rho is 1.8 x LAPACK's (bar 22).  Before every vector was orthogonalised against all earlier ones (dstein does so
inside clusters only) omega was 72 units at K = 5 on the negative-dominant matrix, bar 20.6: the code was changed, not the bar.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import eig_cases as ec
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

BY_SIZE, LDS, WORKSPACE = 0, 1, 2
K_TOP = 8


def limit():
    return B().sym_eig_lds_limit()


def paths_of(K):
    return [LDS, WORKSPACE] if K <= limit() else [WORKSPACE]


def pack(mats, Kmax=None):
    """compact slots, NaN wherever a problem does not reach"""
    ks = np.array([len(M) for M in mats], np.int32)
    Kmax = Kmax or int(ks.max())
    a = np.full((len(mats), Kmax * Kmax), np.nan)
    for p, M in enumerate(mats):
        a[p, :M.size] = np.asarray(M).reshape(-1)
    return a.reshape(len(mats), Kmax, Kmax), ks


def topk(mats, k=K_TOP, vectors=True, path=BY_SIZE, Kmax=None, fill=0xFF, extra=0):
    """-> (w (P, k), v (P, k, Kmax) | None, status (P,), the workspace's bytes after the call)"""
    a, ks = pack(mats, Kmax)
    need = B().sym_eig_workspace_bytes(len(mats), a.shape[1])
    ws = torch.full((need + extra,), fill, dtype=torch.uint8, device="cuda")
    B().debug_sym_eig_path(path)
    try:
        w, v, status = B().sym_eig_topk(to_dev(a), ks, k, vectors=vectors, workspace=ws)
    finally:
        B().debug_sym_eig_path(BY_SIZE)
    w, status = w.cpu().numpy(), status.cpu().numpy()
    v = v.cpu().numpy() if v is not None else None
    for p, K in enumerate(ks):
        assert np.isnan(w[p, K:]).all(), f"problem {p}: w must be NaN from K_p = {K} on"
        assert status[p] == 1 or not np.isnan(w[p, :min(K, k)]).any(), f"problem {p}: NaN eigenvalue with status {status[p]}"
        if v is not None:
            assert np.isnan(v[p, :, K:]).all(), f"problem {p}: v is written beyond K_p = {K}"
            assert np.isnan(v[p, K:, :K]).all(), f"problem {p}: rows from K_p = {K} on must be NaN"
    return w, v, status, ws.cpu().numpy()


# ---------------------------------------------------------------- 1. accuracy over sizes, kinds and paths
def check_size(K, names=None, k=K_TOP):
    kinds = ec.kinds(K)
    names = names or list(kinds)
    for path in paths_of(K):
        w, v, status, _ = topk([kinds[n] for n in names], k, path=path)
        wn, _, sn, _ = topk([kinds[n] for n in names], k, vectors=False, path=path)
        assert same_bits(w, wn) and same_bits(status, sn), f"K = {K}, path {path}: eigenvalues differ without vectors"
        kk = min(k, K)
        for p, n in enumerate(names):
            assert status[p] == 0, (K, n, path, status[p])
            lam, V = w[p, :kk], v[p, :kk, :K]
            assert np.isfinite(lam).all() and np.isfinite(V).all(), (K, n, path)
            assert (np.diff(lam) <= 0).all(), f"K = {K} {n}: eigenvalues not descending"
            r, o, d = ec.measure(K, n, k, lam, V)
            rb, ob, db = ec.bars(K, n, k)
            _, _, rl, ol = ec.lapack(K, n, k)
            print(f"[eig] K {K:4d} path {path} {n:18s} rho {r:6.2f} (lapack {rl:5.2f}, bar {rb:5.1f})  omega {o:6.2f} "
                  f"(lapack {ol:5.2f}, bar {ob:5.1f})  delta {d:6.2f} (bar {db:5.1f})")
            assert r <= rb and o <= ob and d <= db, (K, n, path, (r, rb), (o, ob), (d, db))
            nrm = np.sqrt((V * V).sum(axis=1))
            assert np.abs(nrm - 1.0).max() <= 4 * ec.EPS, (K, n, "unit norm", nrm)
            for j in range(kk):
                top = int(np.argmax(np.abs(V[j])))
                assert V[j, top] > 0, f"K = {K} {n} vector {j}: the largest component {V[j, top]} at {top} is not positive"


@pytest.mark.parametrize("K", ec.SIZES)
def test_measures_under_their_bars(K, dev):
    check_size(K)


def test_measures_around_the_lds_limit_and_above(dev):
    L = limit()
    for K in (L, L + 1, 257):
        check_size(K)


def test_wilkinson(dev):
    check_size(21, ["wilkinson"])


def test_one_problem_of_1024_states(dev):
    check_size(1024, ["metastable"])


# ---------------------------------------------------------------- 2. padding, canaries, batches, determinism
def test_k_at_and_above_the_size_and_canaries(dev):
    mats = [ec.kinds(3)["metastable"], ec.kinds(5)["negative_dominant"], ec.kinds(1)["metastable"], ec.kinds(16)["tridiagonal"]]
    for path in (LDS, WORKSPACE):
        for k in (3, 5, 8):
            w, v, status, ws = topk(mats, k, path=path, Kmax=20, fill=0xAB, extra=4096)
            assert not status.any()
            assert (ws[-4096:] == 0xAB).all(), "the call wrote beyond the workspace it asked for"
            for p, M in enumerate(mats):
                K, kk = len(M), min(k, len(M))
                ref = np.linalg.eigvalsh(M)[::-1][:kk]
                assert np.abs(w[p, :kk] - ref).max() <= 32 * ec.EPS * ec.norm2(M), (p, k, path)
                assert np.isnan(w[p, kk:]).all() and np.isfinite(v[p, :kk, :K]).all()


def mixed():
    L = limit()
    sizes = (3, L + 1, 1, 64, 17)
    return [ec.kinds(K)["metastable" if i % 2 == 0 else "negative_dominant"] for i, K in enumerate(sizes)]


def test_a_problem_alone_in_a_batch_and_permuted_has_the_same_bits(dev):
    mats = mixed()
    Kmax = max(len(M) for M in mats)
    w, v, status, _ = topk(mats, 4, Kmax=Kmax, fill=0xFF)
    w2, v2, status2, _ = topk(mats, 4, Kmax=Kmax, fill=0xFF)
    assert same_bits(w, w2) and same_bits(v, v2) and same_bits(status, status2), "two calls differ"
    order = [3, 0, 4, 2, 1]
    wp, vp, sp, _ = topk([mats[i] for i in order], 4, Kmax=Kmax, fill=0x00)
    for at, i in enumerate(order):
        assert same_bits(w[i], wp[at]) and same_bits(v[i], vp[at]) and status[i] == sp[at], f"problem {i} permuted"
    for i, M in enumerate(mats):
        wa, va, sa, _ = topk([M], 4, Kmax=Kmax, fill=0x7F)
        assert same_bits(w[i], wa[0]) and same_bits(v[i], va[0]) and status[i] == sa[0], f"problem {i} alone"


def test_non_finite_entries_fail_their_problem_alone(dev):
    mats = [np.array(M) for M in mixed()]
    clean = topk(mats, 4)
    dirty = [M.copy() for M in mats]
    dirty[1][5, 2] = np.nan                    # lower triangle
    dirty[3][63, 63] = np.inf
    dirty[0][0, 2] = np.nan                    # strict upper triangle: never read
    dirty[4][3, 9] = np.inf
    w, v, status, _ = topk(dirty, 4)
    assert list(status) == [0, 1, 0, 1, 0]
    for p in (1, 3):
        K = len(mats[p])
        assert np.isnan(w[p]).all() and np.isnan(v[p, :, :K]).all()
    for p in (0, 2, 4):
        assert same_bits(w[p], clean[0][p]) and same_bits(v[p], clean[1][p])


# ---------------------------------------------------------------- 3. stream order
def eig_spec():
    """five problems of 40 states, every entry written (K_p = Kmax, k < K); poison: the all-ones matrix"""
    K, k = 40, 4
    a, ks = pack([ec.metastable(K, seed=s) for s in range(5)])
    ws = torch.empty(B().sym_eig_workspace_bytes(5, K), dtype=torch.uint8, device="cuda")
    return Spec("dff_sym_eig_topk", {"a": (to_dev(a), 1.0)},
                {"w": ((5, k), torch.float64), "v": ((5, k, K), torch.float64), "status": ((5,), torch.int32)},
                lambda _, b: raw("dff_sym_eig_topk", 0, ptr(b["a"]), ks.ctypes.data_as(C.c_void_p), 5, K, k, ptr(b["w"]), ptr(b["v"]),
                                 ptr(b["status"]), ptr(b["ws"]), b["ws"].numel(), stream_of(b["a"])),
                work={"ws": ws})


@pytest.mark.parametrize("forced", [LDS, WORKSPACE], ids=["lds", "workspace"])
def test_the_call_is_ordered_on_its_stream(forced, gate, side):
    B().debug_sym_eig_path(forced)
    try:
        ref = analysis_call(eig_spec(), gate, side)
    finally:
        B().debug_sym_eig_path(BY_SIZE)
    assert not bool(ref["status"].any()) and bool(torch.isfinite(ref["v"]).all())
    assert float((ref["w"][:, 0] - 1.0).abs().max()) < 1e-12


@pytest.mark.parametrize("forced", [LDS, WORKSPACE], ids=["lds", "workspace"])
def test_fence(forced):
    """The memory contract (tests/fence.py) on both paths: the state counts and the P slices of 4 + Kmax^2 doubles at exactly
    dff_sym_eig_workspace_bytes -- the workspace path reduces inside them."""
    B().debug_sym_eig_path(forced)
    try:
        spec = eig_spec()
        ref = reference(spec)
        for pattern, placement in COMBINATIONS:
            fenced(spec, pattern=pattern, placement=placement, ref=ref)
    finally:
        B().debug_sym_eig_path(BY_SIZE)


# ---------------------------------------------------------------- 4. the Python layer
SETTINGS = dict(tol=1e-12, max_iter=100000, steps_per_sync=64)


def chain_model(skip_state=None, lag=2):
    labels = ec.three_well_labels(skip_state=skip_state)
    return ev().MarkovStateModel(lag, **SETTINGS).fit(labels, n_states=12), labels


@pytest.mark.parametrize("skip_state", [None, 5], ids=["all-active", "one-inactive"])
def test_model_eigenvectors(skip_state, dev):
    m, _ = chain_model(skip_state)
    n = len(m.active_set)
    assert n == (12 if skip_state is None else 11)
    T, pi = m.transition_matrix.astype(np.longdouble), m.stationary_distribution
    psi, phi = m.eigenvectors(3), m.eigenvectors(3, side="left")
    assert psi.shape == phi.shape == (4, n)
    M = m.symmetrized()
    assert same_bits(M, M.T)
    unit = ec.EPS * ec.norm2(M)
    w, V = np.linalg.eigh(M)
    rl = ec.rho(M, w[::-1][:4], V[:, ::-1][:, :4].T, unit)
    rb = min(ec.FACTOR * max(rl, 1.0), 32.0)
    bar = (rb + 4.0) * ec.EPS / np.sqrt(pi.min())                    # + 4: T and M differ by roundings
    # ... and by the estimator's tolerance: T_ij = flow_ij / x_i has row sums x'_i / x_i = 1 + O(tol), while M is normalised by
    # the flow's total, so T psi = (lambda / c) psi with |c - 1| <= tol exactly where M v = lambda v: a term tol |lambda| |psi|
    # that is no error of the eigensolver (measured: c - 1 = -1.4e-14 at tol = 1e-12; m.eigenvalues()[0] = 1 + 1.4e-14).
    tol = SETTINGS["tol"]
    spec = ev().msm_spectrum(m, k=3, vectors=True)
    for j in range(4):
        lj = np.longdouble(spec.eigenvalues[0, j])
        assert abs(float(lj) - w[::-1][j]) <= (rb + rl) * unit, (j, float(lj), w[::-1][j])       # delta's bar, the same matrix
        assert abs(float(lj) - m.eigenvalues()[j]) <= (rb + rl + 4.0) * unit + tol * abs(float(lj))
        r = float(np.sqrt(((T @ psi[j] - lj * psi[j]) ** 2).sum())), float(np.sqrt(((phi[j] @ T - lj * phi[j]) ** 2).sum()))
        print(f"[eig] model n {n} pair {j}: |T psi - l psi| {r[0]:.2e}  |phi T - l phi| {r[1]:.2e}  bar {bar:.2e}")
        slack = tol * abs(float(lj))
        assert r[0] <= bar * np.sqrt(n) + slack * np.linalg.norm(psi[j]) and r[1] <= bar + slack * np.linalg.norm(phi[j]), (j, r, bar)
    # psi_1 = 1 and phi_1 = pi up to the estimator's tolerance over the spectral gap: (M sqrt(pi))_i = sqrt(pi_i) (1 + e_i) with
    # |e_i| <= 2 tol (the flux's row sums against x / sum x), so sqrt(pi) is an eigenvector of M to a residual of 2 tol and lies
    # within 2 tol / (1 - lambda_2) of the true one (Davis-Kahan).  Measured: 2.3e-10 at tol = 1e-12, gap 4e-3 (bound 1.8e-9).
    drift = 2.0 * tol / (1.0 - float(spec.eigenvalues[0, 1]))
    print(f"[eig] model n {n}: |psi_1 - 1| {np.abs(psi[0] - 1.0).max():.2e}  |phi_1 - pi| {np.abs(phi[0] - pi).max():.2e}  drift {drift:.2e}")
    assert np.abs(psi[0] - 1.0).max() <= (16 * ec.EPS + drift) / np.sqrt(pi.min()) and np.abs(phi[0] - pi).max() <= 16 * ec.EPS + drift
    gram = (psi * pi) @ psi.T
    assert np.abs(gram - np.eye(4)).max() <= 32 * 8 * ec.EPS


def test_msm_spectrum_over_models_equals_single_calls(dev):
    models = [chain_model()[0], chain_model(5)[0], chain_model(0, lag=3)[0]]
    both = ev().msm_spectrum(models, k=3, vectors=True)
    assert both.eigenvalues.shape == (3, 4) and both.right.shape == (3, 4, 12) and both.timescales.shape == (3, 3)
    for p, m in enumerate(models):
        one = ev().msm_spectrum(m, k=3, vectors=True)
        for name in ("eigenvalues", "timescales", "right", "left", "status"):
            assert same_bits(getattr(one, name)[0], getattr(both, name)[p]), (p, name)
        inactive = np.setdiff1d(np.arange(12), m.active_set)
        assert (both.right[p][:, inactive] == 0).all() and (both.left[p][:, inactive] == 0).all()


def test_bootstrap_with_the_device_eigensolver(dev):
    labels = ec.three_well_labels(n=20000)
    lengths = [5000] * 4
    w = np.random.default_rng(5).multinomial(4, [0.25] * 4, size=6).astype(np.uint32)
    kw = dict(traj_lengths=lengths, n_states=12, weights=w, k=3, **SETTINGS)
    host = ev().bootstrap_msm(labels, 2, eigensolver="host", **kw)
    devi = ev().bootstrap_msm(labels, 2, eigensolver="device", **kw)
    for name in ("stationary", "n_active", "active_count_share", "converged", "n_iter", "weights", "unit_lengths"):
        assert same_bits(getattr(host, name), getattr(devi, name)), name
    assert np.array_equal(np.isnan(host.timescales), np.isnan(devi.timescales))
    # t = -tau / ln(lambda): |dt| / t <= (t / tau) |dlambda| / lambda, |dlambda| <= (delta's bar + 4) u, u = 2^-52 (lambda_1 = 1).
    # delta's bar is rho's bar, at most its cap of 32 units at K = 12, plus LAPACK's rho, at most 8 units (6.1 is the largest
    # the issue lists); + 4: the two routes build M from T and from the flux matrix, a few roundings per entry apart
    # The two routes also differ by the estimator's tolerance, which is no error of either eigensolver: the host route takes the
    # eigenvalues of T_ij = flow_ij / x_i, whose rows sum to x'_i / x_i = 1 + O(tol), the device route those of the flux matrix
    # normalised by the flow's total, so lambda_device = c lambda_host with |c - 1| <= tol exactly (measured: 1.4e-14 at 1e-12).
    dl = (32.0 + 8.0 + 4.0) * ec.EPS
    ok = ~np.isnan(host.timescales)
    t = host.timescales[ok]
    lam = np.exp(-2.0 / t)
    rel = np.abs(devi.timescales[ok] - t) / t
    bar = (t / 2.0) * (dl / lam + SETTINGS["tol"])
    print(f"[eig] bootstrap timescales: worst relative difference {rel.max():.2e}, its bar {bar[np.argmax(rel)]:.2e}")
    assert (rel <= bar).all(), (rel, bar)
