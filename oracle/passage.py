"""Helper of test_msm_passage.py / test_msm_passage_host.py (not a test): the Dirichlet problem of dff_msm_dirichlet_solve in
numpy, from scratch.

- system / dirichlet   the fp64 formulation of include/dff.h: compact interior, W = diag(d) - offdiag(X_II) with d summed
                        directly, b = (sum_j X_ij) s_i + sum_{j boundary} X_ij g_j, np.linalg.solve.
- truth                np.linalg.solve refined eight times with residuals in np.longdouble.
- lapack_error         np.linalg.solve(W, b) against truth: what a good fp64 solver loses on this system.
- backward_error       eta = |b - W u|_inf / (|W|_inf |u|_inf + |b|_inf) in longdouble.
- ldlt_solve / Solver  the kernel's elimination (square-root-free Cholesky with b carried as the last row, running-sum back
                        substitution) in numpy: the stand-in behind evaluate.dirichlet_solver in the host tests.
- ring, two_well       input generators; case(...) the (X, role, g, s) of a named problem.
"""
import numpy as np

from oracle import msm as oracle

U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------- the formulation
def row_sums(off):
    """sum_j off_ij in the order include/dff.h fixes for d_i: 64 partial sums, partial l over j = l, l + 64, ... in order, then
    the butterfly v_l += v_(l xor m), m = 32 .. 1.  The order is part of the contract because it matters: on two_well K = 300
    (cond 6e9) the EXACT solutions of the systems whose d_i are summed in two valid orders (this one, np.sum's, a longdouble
    sum rounded once) differ by 7e-8 .. 1.2e-7 relative, 18 .. 31 times np.linalg.solve's own error -- a 2-ulp change of a
    diagonal entry times cond(W).  With d_i summed as the call sums it, `truth` measures the elimination alone."""
    K = off.shape[1]
    pad = np.zeros((off.shape[0], -(-K // 64) * 64))
    pad[:, :K] = off
    acc = np.zeros((off.shape[0], 64))
    for c in range(pad.shape[1] // 64):
        acc = acc + pad[:, 64 * c:64 * c + 64]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ m]
    return acc[:, 0]


def system(X, role, g, s, plain=False):
    """(W, b, interior indices) of one problem; X (K, K), role / g / s (K,).  plain=True: d_i by np.sum, the formulation without
    any knowledge of the call's order (the tests hold the kernel to both)."""
    X = np.asarray(X, np.float64)
    role = np.asarray(role)
    I, Bd = np.flatnonzero(role == 0), np.flatnonzero(role == 1)
    off = X.copy()
    np.fill_diagonal(off, 0.0)
    d = off.sum(axis=1) if plain else row_sums(off)
    W = -X[np.ix_(I, I)]
    W[np.arange(len(I)), np.arange(len(I))] = d[I]
    b = (d[I] + np.diag(X)[I]) * np.asarray(s, np.float64)[I] + X[np.ix_(I, Bd)] @ np.asarray(g, np.float64)[Bd]
    return W, b, I


def status_of(X, role):
    role = np.asarray(role)
    if ((role != 0) & (role != 1)).any():
        return -2
    if not (role == 1).any():
        return -1
    return 0


def scatter(role, g, I, ui):
    u = np.where(np.asarray(role) == 1, np.asarray(g, np.float64), np.nan)
    u[I] = ui
    return u


def dirichlet(X, role, g, s):
    """u (K,) by np.linalg.solve; NaN where the call reports a failure (no boundary, a bad role)."""
    if status_of(X, role):
        return np.full(len(role), np.nan)
    W, b, I = system(X, role, g, s)
    return scatter(role, g, I, np.linalg.solve(W, b) if len(I) else np.zeros(0))


def truth(W, b, rounds=8):
    """the solution of W x = b to working precision of longdouble residuals: iterative refinement on LAPACK's LU"""
    x = np.linalg.solve(W, b).astype(LD)
    Wl, bl = W.astype(LD), b.astype(LD)
    for _ in range(rounds):
        r = (bl - Wl @ x).astype(np.float64)
        x = x + np.linalg.solve(W, r).astype(LD)
    return x


def forward_error(u, t):
    """max |u - truth| / max |truth|"""
    t = np.asarray(t, LD)
    return float(np.max(np.abs(np.asarray(u, LD) - t)) / np.max(np.abs(t)))


def lapack_error(W, b, t=None):
    t = truth(W, b) if t is None else t
    return forward_error(np.linalg.solve(W, b), t)


def backward_error(W, b, u):
    Wl, bl, ul = W.astype(LD), b.astype(LD), np.asarray(u).astype(LD)
    r = np.max(np.abs(bl - Wl @ ul))
    return float(r / (np.max(np.sum(np.abs(Wl), axis=1)) * np.max(np.abs(ul)) + np.max(np.abs(bl))))


def eta_bar(n):
    """Higham's bound of a Cholesky solve, gamma_(3n+1) |L||L^T|, with the factor n of the norm equivalence"""
    return n * (3 * n + 1) * U


# ---------------------------------------------------------------- the kernel's elimination in numpy
def ldlt_solve(W, b):
    """(x, failed column or -1): W = L D L^T without pivoting or square roots, b carried as row n, then L^T x = D^-1 L^-1 b by
    running sums.  A pivot that is not a finite positive number stops it."""
    n = len(b)
    A = np.vstack([np.tril(W), np.asarray(b, np.float64)[None, :]])
    d0 = np.diag(W).copy()
    A[np.arange(n), np.arange(n)] = np.where(np.isfinite(A[n]), d0, np.nan)     # a b_i that is not finite fails its state
    w = np.zeros(n)
    for j in range(n):
        p = A[j, j]
        if not (p > n * 2.0 ** -52 * d0[j] and np.isfinite(p)):    # the call's guard: finite and above n 2^-52 d_j
            return np.full(n, np.nan), j
        l = A[j + 1:, j] / p
        w[j] = l[-1]
        A[j + 1:, j + 1:] -= np.tril(np.outer(l, A[j + 1:n, j]), 0) if j + 1 < n else 0.0
    x, t = np.zeros(n), np.zeros(n)
    for j in range(n - 1, -1, -1):
        x[j] = w[j] - t[j] / A[j, j]
        t[:j] += A[j, :j] * x[j]
    return x, -1


def cholesky_solve(W, b):
    """LAPACK's own Cholesky (np.linalg.cholesky: potrf) and two substitutions written out in numpy: the yardstick for what a
    backward-stable symmetric elimination loses against np.linalg.solve's LU on one system"""
    L = np.linalg.cholesky(W)
    n = len(b)
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_one(X, role, g, s):
    """(u (K,), status) as the call defines them, by ldlt_solve"""
    K = len(role)
    st = status_of(X, role)
    if st:
        return np.full(K, np.nan), st
    W, b, I = system(X, role, g, s)
    if not len(I):
        return np.asarray(g, np.float64).copy(), 0
    x, failed = ldlt_solve(W, b)
    if failed >= 0:
        return np.full(K, np.nan), 1 + int(I[failed])
    return scatter(role, g, I, x), 0


class Solver:
    """numpy stand-in of evaluate.dirichlet_solver(device): solve(flux, flux_of, ks, role, g, s) -> (u (P, Kmax), status (P,))"""
    calls = 0
    problems = 0

    def __init__(self, device=None):
        pass

    def __call__(self, flux, flux_of, ks, role, g, s):
        P, Kmax = np.shape(role)
        u, status = np.full((P, Kmax), np.nan), np.zeros(P, np.int32)
        for p in range(P):
            K = int(ks[p])
            X = np.asarray(flux[int(flux_of[p])]).reshape(-1)[:K * K].reshape(K, K)
            u[p, :K], status[p] = solve_one(X, role[p, :K], g[p, :K], s[p, :K])
        Solver.calls += 1
        Solver.problems += P
        return u, status


# ---------------------------------------------------------------- inputs
def ring(K, seed):
    """X = C + C^T of seeded strongly connected counts (a ring, sparse extras, heavy diagonals), scaled to sum 1"""
    C = oracle.connected_counts(K, seed)
    X = C + C.T
    return X / X.sum()


def two_well(K, bridge=1e-6, seed=0, diag=1e4):
    """two 30 %-dense blocks with a ring each, joined by ONE bridge entry; diagonals up to `diag` x the off-diagonals"""
    rng = np.random.default_rng(seed)
    h = K // 2
    X = np.zeros((K, K))
    for lo, hi in ((0, h), (h, K)):
        m = hi - lo
        blk = (rng.random((m, m)) < 0.3) * rng.uniform(0.1, 1.0, (m, m))
        idx = np.arange(m)
        blk[idx, (idx + 1) % m] += rng.uniform(0.5, 1.0, m)
        blk = np.triu(blk, 1)
        X[lo:hi, lo:hi] = blk + blk.T
    X[h - 1, h] = X[h, h - 1] = bridge
    X[np.arange(K), np.arange(K)] = rng.uniform(1.0, diag, K) * rng.random(K)
    return X / X.sum()


def boundary_at(K, n_boundary, where):
    """roles with n_boundary boundary states at the start, middle or end of the index range, or interleaved"""
    role = np.zeros(K, np.int32)
    if where == "start":
        role[:n_boundary] = 1
    elif where == "end":
        role[K - n_boundary:] = 1
    elif where == "middle":
        a = (K - n_boundary) // 2
        role[a:a + n_boundary] = 1
    else:                                                            # interleaved: spread evenly
        role[(np.arange(n_boundary) * K) // max(n_boundary, 1)] = 1
    return role


def mfpt_problem(X, role, lagtime=1.0):
    K = len(role)
    return X, role, np.zeros(K), np.full(K, float(lagtime))


def committor_problem(X, role, seed=0):
    """the boundary states alternate between A (g = 0) and B (g = 1)"""
    K = len(role)
    g = np.zeros(K)
    bd = np.flatnonzero(role == 1)
    g[bd[1::2]] = 1.0
    return X, role, g, np.zeros(K)
