"""From-scratch fp64 numpy oracle of the Markov-state-model calls (csrc/dff_msm.hip, evaluate.py): nearest-centre assignment,
per-cluster sums, sliding-window transition counts, the largest strongly connected set, the reversible maximum-likelihood
estimator and the implied timescales.  Nothing here is taken from the code under test; scipy is not used either."""
import math

import numpy as np


# ---------------------------------------------------------------- assignment
def assign(pts, centers):
    """labels int32 (n,), dist2 (n,), gap (n,): d2 summed in coordinate order in fp64 (products rounded, the kernel's are
    fused: equal on inputs where every operation is exact); the lowest index among equal d2; a row with a non-finite
    coordinate -> -1 / NaN.  gap = (second-best d2 - best d2) / second-best d2 (inf with one centre, NaN at label -1)."""
    pts, centers = np.asarray(pts, np.float64), np.asarray(centers, np.float64)
    n, d = pts.shape
    K = len(centers)
    finite = np.isfinite(pts).all(axis=1)
    p = np.where(finite[:, None], pts, 0.0)
    labels = np.zeros(n, np.int32)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    for c in range(K):                                   # index order, strict <
        d2 = np.zeros(n)
        for j in range(d):
            e = p[:, j] - centers[c, j]
            d2 = d2 + e * e
        better = d2 < best
        second = np.where(better, best, np.minimum(second, d2))
        labels[better] = c
        best = np.where(better, d2, best)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(np.isfinite(second), (second - best) / second, np.inf)
        gap = np.where(second == 0, 0.0, gap)            # two centres on the point
    labels[~finite] = -1
    best = np.where(finite, best, np.nan)
    gap = np.where(finite, gap, np.nan)
    return labels, best, gap


def accumulate(pts, labels, dist2, K):
    """math.fsum per cluster and coordinate over the members (label >= 0): a dict of sums (K, d), counts int64 (K,), inertia,
    and the sums of absolute values behind the a-priori error bound: abs_sums (K, d), abs_inertia."""
    pts = np.asarray(pts, np.float64)
    d = pts.shape[1]
    sums, abs_sums = np.zeros((K, d)), np.zeros((K, d))
    counts = np.zeros(K, np.int64)
    for c in range(K):
        m = pts[labels == c]
        counts[c] = len(m)
        for j in range(d):
            sums[c, j] = math.fsum(m[:, j])
            abs_sums[c, j] = math.fsum(np.abs(m[:, j]))
    ok = labels >= 0
    return {"sums": sums, "counts": counts, "inertia": math.fsum(dist2[ok]), "abs_sums": abs_sums,
            "abs_inertia": math.fsum(np.abs(dist2[ok])), "members": int(ok.sum())}


# ---------------------------------------------------------------- counts
def transition_counts(labels, lengths, lags, K):
    """(n_lags, K, K) int64: pairs (t, t + lag) inside one trajectory, both labels in 0 .. K - 1."""
    labels = np.asarray(labels, np.int64)
    out = np.zeros((len(lags), K, K), np.int64)
    o = 0
    for n in lengths:
        seg = labels[o:o + n]
        o += n
        for l, lag in enumerate(lags):
            if lag >= n:
                continue
            a, b = seg[:-lag], seg[lag:]
            ok = (a >= 0) & (a < K) & (b >= 0) & (b < K)
            np.add.at(out[l], (a[ok], b[ok]), 1)
    return out


# ---------------------------------------------------------------- connectivity
def largest_connected_set(counts):
    """Largest strongly connected component by reachability (boolean closure by repeated squaring): the component of i is
    {j : i reaches j and j reaches i}; ties go to the component with the lowest index."""
    A = np.asarray(counts) > 0
    K = len(A)
    R = A | np.eye(K, dtype=bool)
    for _ in range(max(1, int(np.ceil(np.log2(max(K, 2)))))):
        R = R | ((R.astype(np.float64) @ R.astype(np.float64)) > 0)
    both = R & R.T
    sizes = both.sum(axis=1)
    i = int(np.argmax(sizes))                              # the first maximum: the lowest index
    return np.flatnonzero(both[i])


# ---------------------------------------------------------------- the reversible estimator
def sweep(S, c, x):
    """x_i' = sum_j S_ij / (c_i / x_i + c_j / x_j), pairs with S_ij = 0 left out; err = max_i |x_i' - x_i| / x_i."""
    q = c / x
    den = q[:, None] + q[None, :]
    xn = np.divide(S, den, out=np.zeros_like(S), where=S != 0).sum(axis=1)
    return xn, float(np.max(np.abs(xn - x) / x))


def sweeps(S, c, x, n):
    errs = np.zeros(n)
    for s in range(n):
        x, errs[s] = sweep(S, c, x)
    return x, errs


def start(S):
    return 0.5 * S.sum(axis=1)


def reversible_mle(C, tol=1e-13, max_iter=2_000_000):
    """(T, pi, x, n_iter) of the reversible maximum-likelihood estimate on a strongly connected count matrix C."""
    C = np.asarray(C, np.float64)
    S, c = C + C.T, C.sum(axis=1)
    x = start(S)
    for it in range(max_iter):
        x, err = sweep(S, c, x)
        if err < tol:
            break
    else:
        raise AssertionError(f"oracle: not converged after {max_iter} sweeps")
    return transition_matrix_from_x(S, c, x) + (x, it + 1)


def transition_matrix_from_x(S, c, x):
    q = c / x
    den = q[:, None] + q[None, :]
    flow = np.divide(S, den, out=np.zeros_like(S), where=S != 0)
    return flow / x[:, None], x / x.sum()


def row_normalised(C):
    C = np.asarray(C, np.float64)
    return C / C.sum(axis=1, keepdims=True)


def log_likelihood(C, T):
    C = np.asarray(C, np.float64)
    m = C > 0
    return float(np.sum(C[m] * np.log(T[m])))


def timescales(T, pi, lag, k):
    """-lag / ln(lambda_i), i = 2 .. k + 1, of the symmetrised pi^(1/2) T pi^(-1/2); NaN for lambda <= 0 or missing."""
    r = np.sqrt(pi)
    M = r[:, None] * T / r[None, :]
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))[::-1][1:k + 1]
    out = np.full(k, np.nan)
    for i, v in enumerate(lam):
        if v > 0:
            out[i] = -lag / math.log(v)
    return out


def pipeline(labels, lengths, lag, K, k):
    """labels -> counts -> active set -> reversible estimate -> timescales: (active set, timescales, T, pi)."""
    C = transition_counts(labels, lengths, [lag], K)[0].astype(np.float64)
    act = largest_connected_set(C)
    T, pi, _, _ = reversible_mle(C[np.ix_(act, act)])
    return act, timescales(T, pi, lag, k), T, pi


def check_reversible(C, T, pi, what):
    """What a reversible maximum-likelihood estimate (T, pi) of the counts C must satisfy, whoever computed it."""
    K = len(C)
    assert np.all(T >= 0) and np.all(T[C + C.T == 0] == 0), what
    assert np.abs(T.sum(axis=1) - 1).max() < 1e-10, (what, np.abs(T.sum(axis=1) - 1).max())
    assert abs(pi.sum() - 1) < 1e-12 and np.all(pi > 0), what
    flow = pi[:, None] * T
    assert np.abs(flow - flow.T).max() < 1e-12, (what, np.abs(flow - flow.T).max())         # detailed balance
    assert np.abs(pi @ T - pi).max() < 1e-11, what
    ll = log_likelihood(C, T)
    lo, hi = log_likelihood(C, row_normalised(C + C.T)), log_likelihood(C, row_normalised(C))
    slack = 1e-9 * abs(hi)
    assert lo - slack <= ll <= hi + slack, (what, lo, ll, hi)
    if K == 2:
        assert np.abs(T - row_normalised(C)).max() < 1e-10, what


# ---------------------------------------------------------------- inputs
def connected_counts(K, seed, diag=1e4):
    """Strongly connected seeded counts: a ring i -> i + 1, random sparse entries, diagonals up to `diag` x the off-diagonals."""
    rng = np.random.default_rng(seed)
    C = np.zeros((K, K))
    idx = np.arange(K)
    C[idx, (idx + 1) % K] = rng.integers(1, 20, K)
    extra = max(K, K * K // 8)
    C[rng.integers(0, K, extra), rng.integers(0, K, extra)] += rng.integers(1, 20, extra)
    C[idx, idx] = np.floor(rng.uniform(0.0, diag, K) * rng.integers(1, 20, K))
    return C


def jump_process(M, n_traj, n_frames, seed):
    """state paths (n_traj, n_frames) of the Markov chain with transition matrix M, started from its rows' uniform choice."""
    rng = np.random.default_rng(seed)
    cum = np.cumsum(M, axis=1)
    s = rng.integers(0, len(M), n_traj)
    out = np.empty((n_traj, n_frames), np.int64)
    for t in range(n_frames):
        out[:, t] = s
        u = rng.random(n_traj)
        s = np.minimum((u[:, None] >= cum[s]).sum(axis=1), len(M) - 1)
    return out
