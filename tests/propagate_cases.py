"""Seeded transition matrices, start vectors and observables, the truth and the measure that tests/test_msm_propagate.py and
tests/test_msm_propagate_host.py hold dff_msm_propagate and its Python layer to (not a test).

The call: w_0 = w0, w_{s+1} = w_s T (row vector times matrix), out[s][m][r] = sum_j w_s[m][j] obs[r][j].
Truth: the same chain in np.longdouble.
Measure, in units: E(s) = max over (m, r) of |out[s][m][r] - truth| / (2^-52 |w0_m|_1 |T|_inf^s |obs_r|_inf), |T|_inf the largest
absolute row sum: |w T|_1 <= |w|_1 |T|_inf, so the denominator bounds |out| and a unit is one rounding of the largest possible
value.
Bar: per case 8 x the worst E(s) of numpy's own fp64 chain on the same case (`w @ T` repeatedly, then `w @ obs.T`), numpy's
value floored at one unit before the factor (out is itself rounded to fp64, which moves E by up to half a unit, and numpy's
exact 0 on a permutation matrix says that nothing is added there, not that rounding is absent), and capped at step s by
(s + 2) K units, the order of the a-priori bound of s products and one scalar product of length K.  The factor, the floor and
the cap mirror tests/eig_cases.py."""
import functools

import numpy as np

EPS = 2.0 ** -52
FACTOR = 8.0
SIZES = (1, 2, 3, 5, 16, 17, 33, 64, 65)          # + L, L + 1, 257 and one problem of 1024 (test_msm_propagate.py)
M_ROWS, R_OBS, STEPS = 3, 4, 64


# ---------------------------------------------------------------- matrices
def metastable(K, seed=0, blocks=4, coupling=1e-4, scale=1.0):
    """the reversible chain of eig_cases.metastable (a symmetric non-negative flux X, dense inside a block and `coupling` between
    blocks, a lazy diagonal) as its row-stochastic T = X / pi, times `scale`"""
    rng = np.random.default_rng(1000 * K + seed)
    nb = min(blocks, K)
    of = np.arange(K) * nb // K
    X = rng.uniform(0.5, 1.5, (K, K))
    X = 0.5 * (X + X.T)
    X *= np.where(of[:, None] == of[None, :], 1.0, coupling)
    X += np.diag(rng.uniform(2.0, 4.0, K) * X.sum(axis=1))
    return X / X.sum(axis=1)[:, None] * scale


def nonreversible(K, seed=0):
    X = np.random.default_rng(5000 * K + seed).uniform(0.0, 1.0, (K, K))
    return X / X.sum(axis=1)[:, None]


def cyclic(K):
    """T[i][(i + 1) % K] = 1: (w T)[j] = w[j - 1]"""
    T = np.zeros((K, K))
    T[np.arange(K), (np.arange(K) + 1) % K] = 1.0
    return T


def signed(K, seed=0):
    """a signed matrix that is not stochastic, |T|_inf = 1 (up to one rounding)"""
    X = np.random.default_rng(6000 * K + seed).normal(size=(K, K))
    return X / np.abs(X).sum(axis=1).max()


@functools.lru_cache(maxsize=None)
def kinds(K):
    out = {"metastable": metastable(K), "nonreversible": nonreversible(K), "identity": np.eye(K), "cyclic": cyclic(K),
           "all_equal": np.full((K, K), 1.0 / K), "signed": signed(K), "scaled_down": metastable(K, scale=2.0 ** -3),
           "scaled_up": metastable(K, scale=2.0 ** 3)}
    for T in out.values():
        T.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def vectors(K, M=M_ROWS, R=R_OBS, seed=0):
    """(w0 (M, K): non-negative rows of sum 1; obs (R, K): signed)"""
    rng = np.random.default_rng(7000 * K + 16 * M + R + seed)
    w0 = rng.uniform(0.0, 1.0, (M, K))
    w0 /= w0.sum(axis=1)[:, None]
    obs = rng.normal(size=(R, K))
    w0.setflags(write=False)
    obs.setflags(write=False)
    return w0, obs


# ---------------------------------------------------------------- truth, numpy's chain, the measure
def chain(T, w0, obs, S, dtype):
    T, w, o = np.asarray(T, dtype), np.asarray(w0, dtype), np.asarray(obs, dtype)
    out = np.empty((S + 1, w.shape[0], o.shape[0]), dtype)
    for s in range(S + 1):
        out[s] = w @ o.T
        if s < S:
            w = w @ T
    return out, w


def norm_inf(T):
    return float(np.abs(T).sum(axis=1).max())


def units(T, w0, obs, S):
    """(S + 1, M, R): what one unit is at every output"""
    n = np.longdouble(norm_inf(T)) ** np.arange(S + 1)
    return (EPS * n[:, None, None] * np.abs(w0).sum(axis=1)[None, :, None] * np.abs(obs).max(axis=1)[None, None, :]).astype(np.longdouble)


def measure(out, truth, unit):
    """E(s), s = 0 .. S"""
    return np.asarray((np.abs(np.asarray(out, np.longdouble) - truth) / unit).max(axis=(1, 2)), np.float64)


@functools.lru_cache(maxsize=None)
def reference(K, name, S=STEPS, M=M_ROWS, R=R_OBS):
    """(truth (S + 1, M, R) longdouble, units, numpy's E(s)) of one case, computed once"""
    T = kinds(K)[name]
    w0, obs = vectors(K, M, R)
    truth, _ = chain(T, w0, obs, S, np.longdouble)
    unit = units(T, w0, obs, S)
    mine, _ = chain(T, w0, obs, S, np.float64)
    return truth, unit, measure(mine, truth, unit)


def bar_of(e_numpy, K):
    """the bar at every step from numpy's E(s) on the case"""
    s = np.arange(len(e_numpy))
    return np.minimum(FACTOR * max(float(e_numpy.max()), 1.0), (s + 2.0) * K)


# ---------------------------------------------------------------- the call's contract on the host (the tests' stand-in)
def host_propagate(t, mat_of, ks, w0, obs, n_steps, want_last=False):
    """dff_msm_propagate on numpy: t (n_mat, Kmax, Kmax) compact slots -> (out (P, S + 1, M, R), w_last (P, M, Kmax) | None,
    status (P,))"""
    t, w0, obs = np.asarray(t, np.float64), np.asarray(w0, np.float64), np.asarray(obs, np.float64)
    P, M, Kmax = w0.shape
    R, S = obs.shape[1], int(n_steps)
    out = np.full((P, S + 1, M, R), np.nan)
    last = np.full((P, M, Kmax), np.nan) if want_last else None
    status = np.zeros(P, np.int32)
    for p in range(P):
        K = int(ks[p])
        T = t[p if mat_of is None else int(mat_of[p])].reshape(-1)[:K * K].reshape(K, K)
        w, o = w0[p, :, :K], obs[p, :, :K]
        if not (np.isfinite(T).all() and np.isfinite(w).all() and np.isfinite(o).all()):
            status[p] = 1
            continue
        with np.errstate(all="ignore"):
            res, wl = chain(T, w, o, S, np.float64)
        if np.isnan(res).any():
            status[p] = 2
            continue
        out[p] = res
        if want_last:
            last[p, :, :K] = wl
    return out, last, status


# ---------------------------------------------------------------- chains for the Python layer
def three_well_T(K=9, hop=0.02):
    """a jump process on K states in three wells of K / 3: fast inside a well, rare hops between neighbouring wells"""
    w = K // 3
    T = np.zeros((K, K))
    for i in range(K):
        for j in range(K):
            if i != j and i // w == j // w:
                T[i, j] = 0.3 / w
        if (i + 1) % w == 0 and i + 1 < K:
            T[i, i + 1] = hop
        if i % w == 0 and i > 0:
            T[i, i - 1] = hop
    return T + np.diag(1.0 - T.sum(axis=1))


@functools.lru_cache(maxsize=None)
def three_well_trajectories(n_traj=80, length=1000, K=9, seed=11):
    """(labels int32 (n_traj * length,), lengths): seeded trajectories of three_well_T, each from a state drawn uniformly"""
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(three_well_T(K), axis=1)
    x = np.empty((n_traj, length), np.int32)
    for t in range(n_traj):
        s = int(rng.integers(K))
        r = rng.random(length)
        for i in range(length):
            x[t, i] = s
            s = min(int(np.searchsorted(cdf[s], r[i])), K - 1)
    return x.reshape(-1), [length] * n_traj


def three_well_sets(K=9):
    w = K // 3
    return [list(range(a * w, (a + 1) * w)) for a in range(3)]


def four_block_counts(K, seed=0, inside=200.0, between=1.0):
    """a symmetric count matrix of four equal metastable blocks in index order"""
    rng = np.random.default_rng(8000 * K + seed)
    of = np.arange(K) * 4 // K
    C = rng.uniform(0.5, 1.5, (K, K))
    C = 0.5 * (C + C.T) * np.where(of[:, None] == of[None, :], inside, between)
    C += np.diag(C.sum(axis=1))
    return np.round(C), [np.flatnonzero(of == b) for b in range(4)]
