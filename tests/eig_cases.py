"""Seeded symmetric matrices and the three measures that tests/test_sym_eig.py and tests/test_sym_eig_host.py hold
dff_sym_eig_topk and its Python layer to (not a test).

Units: u = 2^-52 |A|_2, |A|_2 = max |eigvalsh(A)| from numpy; the matrix products run in np.longdouble.
  rho    max_j |A v_j - lambda_j v_j|_2 / u.  For a symmetric A this bounds each lambda_j's distance to a true eigenvalue,
         so no high-precision truth is needed.
  omega  max |V^T V - I| / 2^-52.
  delta  max_j |lambda_j - lambda_j^LAPACK| / u against np.linalg.eigvalsh's k largest: with rho and omega it shows that the
         eigenvalues are the TOP k and that none was skipped.
Bars: 8 x LAPACK's own value (np.linalg.eigh on the same matrix, recomputed per case), capped by max(K, 32) units.  LAPACK's
value is floored at one unit before the factor: lambda and v are themselves rounded to fp64, which moves rho by up to about
one unit, and LAPACK's exact 0 on a diagonal input says that it special-cases such input, not that rounding is absent.  delta
is bounded by the triangle inequality: both eigenvalues lie within their rho of a true one, so its bar is the bar of rho plus
LAPACK's rho."""
import functools

import numpy as np

EPS = 2.0 ** -52
FACTOR = 8.0
SIZES = (1, 2, 3, 5, 16, 17, 33, 64, 65)          # + L, L + 1, 257 and one problem of 1024 (test_sym_eig.py)


# ---------------------------------------------------------------- matrices
def metastable(K, seed=0, blocks=4, coupling=1e-4, scale=1.0):
    """(a) pi^(1/2) T pi^(-1/2) of a reversible chain with `blocks` metastable blocks: a symmetric non-negative flux X, dense
    inside a block and `coupling` between them -> M_ij = X_ij / sqrt(pi_i pi_j).  Eigenvalues 1, then blocks - 1 close to 1."""
    rng = np.random.default_rng(1000 * K + seed)
    nb = min(blocks, K)
    of = np.arange(K) * nb // K
    X = rng.uniform(0.5, 1.5, (K, K))
    X = 0.5 * (X + X.T)
    X *= np.where(of[:, None] == of[None, :], 1.0, coupling)
    X += np.diag(rng.uniform(2.0, 4.0, K) * X.sum(axis=1))           # a lazy chain: every eigenvalue positive
    X /= X.sum()
    r = np.sqrt(X.sum(axis=1))
    M = X / r[:, None] / r[None, :]
    return 0.5 * (M + M.T) * scale


def twin_blocks(K, seed=0):
    """(b) two identical disconnected blocks (and a 1 x 1 block of 0.25 when K is odd): every eigenvalue of a block twice"""
    h = K // 2
    M = np.zeros((K, K))
    if h:
        Bk = metastable(h, seed + 7)
        M[:h, :h] = Bk
        M[h:2 * h, h:2 * h] = Bk
    if K % 2:
        M[-1, -1] = 0.25
    return M


def diagonal(K, seed=0):
    """(c) a diagonal matrix with distinct entries in no order"""
    return np.diag(np.random.default_rng(2000 * K + seed).permutation(np.linspace(-1.0, 2.0, K)))


def tridiagonal(K, seed=0):
    """(c) already tridiagonal"""
    rng = np.random.default_rng(3000 * K + seed)
    M = np.diag(rng.normal(size=K))
    if K > 1:
        e = rng.normal(size=K - 1)
        M += np.diag(e, 1) + np.diag(e, -1)
    return M


def all_equal(K):
    """(d) rank one"""
    return np.full((K, K), 1.0 / K)


def wilkinson21():
    """(e) W21+: pairs about 1e-14 apart"""
    return np.diag(np.abs(np.arange(21) - 10.0)) + np.diag(np.ones(20), 1) + np.diag(np.ones(20), -1)


def negative_dominant(K, seed=0):
    """(f) the eigenvalue of largest magnitude is negative: the k LARGEST are asked for, not the largest by magnitude"""
    rng = np.random.default_rng(4000 * K + seed)
    Q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    lam = rng.uniform(-1.0, 1.0, K)
    lam[0] = -10.0
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)


@functools.lru_cache(maxsize=None)
def kinds(K):
    """name -> matrix of size K, every kind of the issue (W21+ at K = 21 only)"""
    out = {"metastable": metastable(K), "twin_blocks": twin_blocks(K), "diagonal": diagonal(K), "identity": np.eye(K),
           "tridiagonal": tridiagonal(K), "all_equal": all_equal(K), "negative_dominant": negative_dominant(K),
           "scaled_down": metastable(K, scale=2.0 ** -30), "scaled_up": metastable(K, scale=2.0 ** 30)}
    if K == 21:
        out["wilkinson"] = wilkinson21()
    for M in out.values():
        M.setflags(write=False)
    return out


# ---------------------------------------------------------------- measures
def norm2(A):
    return float(np.abs(np.linalg.eigvalsh(A)).max())


def rho(A, lam, V, unit):
    """V (k, K): eigenvector j in row j"""
    Al, Vl = np.asarray(A, np.longdouble), np.asarray(V, np.longdouble)
    R = Vl @ Al - np.asarray(lam, np.longdouble)[:, None] * Vl          # A symmetric: rows of V A^T = V A
    return float(np.sqrt((R * R).sum(axis=1)).max() / unit)


def omega(V):
    Vl = np.asarray(V, np.longdouble)
    return float(np.abs(Vl @ Vl.T - np.eye(len(Vl))).max() / EPS)


def delta(lam, lam_ref, unit):
    return float(np.abs(np.asarray(lam) - np.asarray(lam_ref)).max() / unit)


@functools.lru_cache(maxsize=None)
def lapack(K, name, k):
    """the reference of one case: (unit, the kk largest eigenvalues descending, LAPACK's rho, LAPACK's omega)"""
    A = kinds(K)[name]
    w, V = np.linalg.eigh(A)
    kk = min(k, K)
    lam, Vt = w[::-1][:kk], V[:, ::-1][:, :kk].T
    unit = EPS * float(np.abs(w).max())
    return unit, lam, rho(A, lam, Vt, unit), omega(Vt)


def bars(K, name, k):
    """(rho's bar, omega's bar, delta's bar) in units, from LAPACK on the same case"""
    _, _, r, o = lapack(K, name, k)
    cap = float(max(K, 32))
    rb, ob = min(FACTOR * max(r, 1.0), cap), min(FACTOR * max(o, 1.0), cap)
    return rb, ob, rb + r


def measure(K, name, k, lam, V):
    """(rho, omega, delta) of computed pairs lam (kk,), V (kk, K) -- V None: (None, None, delta)"""
    unit, ref, _, _ = lapack(K, name, k)
    d = delta(lam, ref, unit)
    if V is None:
        return None, None, d
    return rho(kinds(K)[name], lam, V, unit), omega(V), d


# ---------------------------------------------------------------- the call's conventions on the host (the tests' stand-in)
def fix_sign(v):
    """the component of largest magnitude positive, the lowest index winning a tie"""
    v = np.asarray(v, np.float64)
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def host_topk(a, ks, k, vectors):
    """dff_sym_eig_topk's contract on np.linalg.eigh: a (P, Kmax, Kmax) compact slots -> (w (P, k), v (P, k, Kmax) | None,
    status (P,)), NaN padding and the sign rule included"""
    P, Kmax = a.shape[0], a.shape[1]
    w = np.full((P, k), np.nan)
    v = np.full((P, k, Kmax), np.nan) if vectors else None
    status = np.zeros(P, np.int32)
    for p in range(P):
        K = int(ks[p])
        A = a[p].reshape(-1)[:K * K].reshape(K, K)
        L = np.tril(A)
        if not np.isfinite(L).all():
            status[p] = 1
            if vectors:
                v[p, :, :K] = np.nan
            continue
        lam, V = np.linalg.eigh(L + np.tril(A, -1).T)
        kk = min(k, K)
        w[p, :kk] = lam[::-1][:kk]
        if vectors:
            for j in range(kk):
                v[p, j, :K] = fix_sign(V[:, K - 1 - j])
    return w, v, status


# ---------------------------------------------------------------- chains for the Python layer
def three_well_labels(n=60000, K=12, seed=3, skip_state=None):
    """a trajectory of a three-well chain on K states (wells of K / 3 states, rare hops between neighbouring wells);
    skip_state: a state that is never visited (an inactive state for the model)"""
    rng = np.random.default_rng(seed)
    T = np.zeros((K, K))
    w = K // 3
    for i in range(K):
        for j in range(K):
            if i != j and i // w == j // w:
                T[i, j] = 0.2 / w
        if (i + 1) % w == 0 and i + 1 < K:
            T[i, i + 1] = 0.01
        if i % w == 0 and i > 0:
            T[i, i - 1] = 0.01
    if skip_state is not None:
        T[:, skip_state] = 0.0
        T[skip_state, :] = 0.0
    T += np.diag(1.0 - T.sum(axis=1))
    cdf = np.cumsum(T, axis=1)
    x = np.empty(n, np.int32)
    s = 0 if skip_state != 0 else 1
    r = rng.random(n)
    for t in range(n):
        x[t] = s
        s = min(int(np.searchsorted(cdf[s], r[t])), K - 1)
    return x
