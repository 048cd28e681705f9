"""From-scratch numpy oracle of the Markov-state-model bootstrap (csrc/dff_msm_batch.hip, evaluate.bootstrap_msm): weighted
sliding-window counts by explicit loops over the pairs, the resampling units and weights, and the bootstrap pipeline on top
of the estimator of oracle/msm.py.  Nothing here is taken from the code under test.  Also the numpy stand-ins that
host tests put behind evaluate.resampled_counter / evaluate.batched_reversible_sweeper, and the two-state chain of the
calibration test."""
import numpy as np

from oracle import msm as oracle


# ---------------------------------------------------------------- units, weights, counts
def units(traj_lengths, block_frames=None):
    out = []
    for n in traj_lengths:
        if block_frames is None:
            out.append(int(n))
            continue
        left = int(n)
        while left > 0:
            out.append(min(block_frames, left))
            left -= block_frames
    return np.array(out, np.int64)


def weights(n_units, B, seed):
    return np.random.default_rng(seed).multinomial(n_units, np.full(n_units, 1 / n_units), size=B)


def weighted_counts(labels, lengths, unit_lengths, lag, K, w):
    """(B, K, K) uint64: sum of w[b, unit(t)] over the pairs (t, t + lag) inside one trajectory with both labels in
    0 .. K - 1; the unit of a pair is the unit of frame t.  One pair at a time."""
    labels = np.asarray(labels, np.int64)
    w = np.asarray(w).astype(np.uint64)
    unit_of = np.repeat(np.arange(len(unit_lengths)), np.asarray(unit_lengths, np.int64))
    assert len(unit_of) == len(labels) == int(np.sum(lengths))
    out = np.zeros((w.shape[0], K, K), np.uint64)
    o = 0
    for n in lengths:
        for t in range(o, o + n - lag):
            a, b = labels[t], labels[t + lag]
            if 0 <= a < K and 0 <= b < K:
                out[:, a, b] += w[:, unit_of[t]]
        o += n
    return out


# ---------------------------------------------------------------- one resample: counts -> model
def fit_counts(C, lag, k, tol=1e-12, max_iter=1_000_000, steps_per_sync=256):
    """The estimator of oracle.msm on the largest connected set of C, swept in batches of steps_per_sync and stopped as
    evaluate.MarkovStateModel documents it: converged at the first sweep whose err is below tol, n_iter the sweeps up to
    and including it, x the vector after the whole batch.  -> dict."""
    C = np.asarray(C, np.float64)
    act = oracle.largest_connected_set(C)
    Ca = C[np.ix_(act, act)]
    res = {"active_set": act, "share": Ca.sum() / C.sum() if C.sum() > 0 else 0.0, "n_iter": 0, "converged": True}
    if len(act) == 1:
        res.update(T=np.ones((1, 1)), pi=np.ones(1), timescales=np.full(k, np.nan))
        return res
    S, c = Ca + Ca.T, Ca.sum(axis=1)
    x = oracle.start(S)
    res["converged"] = False
    while res["n_iter"] < max_iter and not res["converged"]:
        n = min(steps_per_sync, max_iter - res["n_iter"])
        x, err = oracle.sweeps(S, c, x, n)
        hit = np.flatnonzero(err < tol)
        res["converged"] = hit.size > 0
        res["n_iter"] += int(hit[0]) + 1 if hit.size else n
        if not np.isfinite(err).all():
            break
    T, pi = oracle.transition_matrix_from_x(S, c, x)
    res.update(T=T, pi=pi, timescales=oracle.timescales(T, pi, lag, k))
    return res


def bootstrap(labels, lengths, unit_lengths, lag, K, w, k=3, **fit):
    """The whole pipeline, one resample at a time -> dict of arrays over the resamples and "fits", the per-resample dicts."""
    counts = weighted_counts(labels, lengths, unit_lengths, lag, K, w)
    fits = [fit_counts(Cb, lag, k, **fit) for Cb in counts]
    stationary = np.zeros((len(fits), K))
    for row, f in zip(stationary, fits):
        row[f["active_set"]] = f["pi"]
    return {"counts": counts, "fits": fits, "stationary": stationary,
            "timescales": np.array([f["timescales"] for f in fits]), "n_active": np.array([len(f["active_set"]) for f in fits]),
            "share": np.array([f["share"] for f in fits]), "converged": np.array([f["converged"] for f in fits]),
            "n_iter": np.array([f["n_iter"] for f in fits])}


def interval(values, confidence):
    """percentile interval per column over the finite entries -> (lo, hi)"""
    lo, hi = [], []
    for col in np.asarray(values).T:
        col = np.sort(col[np.isfinite(col)])
        if col.size == 0:
            lo.append(np.nan), hi.append(np.nan)
            continue
        for q, dst in (((1 - confidence) / 2, lo), ((1 + confidence) / 2, hi)):     # linear interpolation between order statistics
            pos = q * (col.size - 1)
            i = int(np.floor(pos))
            j = min(i + 1, col.size - 1)
            dst.append(col[i] + (col[j] - col[i]) * (pos - i))
    return np.array(lo), np.array(hi)


def std(values):
    out = []
    for col in np.asarray(values).T:
        col = col[np.isfinite(col)]
        out.append(np.sqrt(np.sum((col - col.mean()) ** 2) / (col.size - 1)) if col.size >= 2 else np.nan)
    return np.array(out)


# ---------------------------------------------------------------- numpy stand-ins for the two device seams
class Counter:
    """evaluate.resampled_counter on the host: per-unit count matrices once, then the integer product weights x units."""
    calls = 0

    def __init__(self, labels, lengths, unit_lengths, lag, K, device):
        eye = np.eye(len(unit_lengths), dtype=np.uint64)
        self.per_unit = weighted_counts(np.asarray(labels), lengths, unit_lengths, lag, K, eye).reshape(len(unit_lengths), K * K)
        self.K = K

    def __call__(self, w):
        Counter.calls += 1
        w = np.asarray(w).astype(np.uint64)
        return (w @ self.per_unit).reshape(len(w), self.K, self.K)


class FastCounter(Counter):
    """The same with the per-unit matrices from array operations (labels all valid): what 100 datasets need."""

    def __init__(self, labels, lengths, unit_lengths, lag, K, device):
        labels = np.asarray(labels, np.int64)
        unit_of = np.repeat(np.arange(len(unit_lengths)), np.asarray(unit_lengths, np.int64))
        traj_of = np.repeat(np.arange(len(lengths)), np.asarray(lengths, np.int64))
        t = np.arange(len(labels) - lag)
        t = t[traj_of[t] == traj_of[t + lag]]
        self.per_unit = np.zeros((len(unit_lengths), K * K), np.uint64)
        np.add.at(self.per_unit, (unit_of[t], labels[t] * K + labels[t + lag]), 1)
        self.K = K


class Sweeper:
    """evaluate.batched_reversible_sweeper on the host: the oracle's sweeps, problem by problem, on the compact slots."""
    calls = 0

    def __init__(self, S, c, ks, device):
        self.S, self.c, self.ks = np.array(S), np.array(c), np.array(ks)

    def __call__(self, x, n, skip=None):
        Sweeper.calls += 1
        x = np.array(x)
        err = np.zeros((n, len(self.ks)))
        for p, K in enumerate(self.ks):
            if skip is not None and skip[p]:
                continue
            Sp = self.S[p].reshape(-1)[:K * K].reshape(K, K)
            x[p, :K], err[:, p] = oracle.sweeps(Sp, self.c[p, :K], x[p, :K], n)
        return x, err


class FastSweeper(Sweeper):
    """The same sweep on all problems at once where every problem has Kmax states (else problem by problem)."""

    def __call__(self, x, n, skip=None):
        if not (self.ks == self.c.shape[1]).all():
            return Sweeper.__call__(self, x, n, skip)
        Sweeper.calls += 1
        x = np.array(x)
        live = np.ones(len(self.ks), bool) if skip is None else ~np.asarray(skip, bool)
        S, c, xl = self.S[live], self.c[live], x[live]
        err = np.zeros((n, len(self.ks)))
        for s in range(n):
            q = c / xl
            den = q[:, :, None] + q[:, None, :]
            xn = np.divide(S, den, out=np.zeros_like(S), where=S != 0).sum(axis=2)
            err[s, live] = np.max(np.abs(xn - xl) / xl, axis=1)
            xl = xn
        x[live] = xl
        return x, err


# ---------------------------------------------------------------- inputs
def five_state_case():
    """Four trajectories on 5 states: 0 sits in state 0 throughout, 1 and 2 wander over 0 .. 3, 3 alone visits state 4; some
    labels are -1.  Explicit weights: all ones, one resample that loses state 4, one that collapses to state 0, zeros, draws."""
    rng = np.random.default_rng(3)
    M = np.full((5, 5), 0.05) + 0.75 * np.eye(5)
    wander = oracle.jump_process(M[:4, :4] / M[:4, :4].sum(axis=1, keepdims=True), 2, 400, 4)
    last = oracle.jump_process(M / M.sum(axis=1, keepdims=True), 1, 500, 9)[0]
    assert (last == 4).sum() > 20 and set(np.unique(wander)) == {0, 1, 2, 3}
    labels = np.concatenate([np.zeros(300, np.int64), wander[0], wander[1], last]).astype(np.int32)
    labels[rng.integers(300, len(labels), 12)] = -1
    lengths = [300, 400, 400, 500]
    w = np.array([[1, 1, 1, 1], [1, 2, 1, 0], [4, 0, 0, 0], [0, 3, 0, 1]] + weights(4, 4, 8).tolist())
    return labels, lengths, w


# ---------------------------------------------------------------- the two-state chain of the calibration test
P01, P10 = 0.05, 0.10
TRUE_T2 = -1.0 / np.log(1.0 - P01 - P10)                 # 6.153 frames
CHAIN = np.array([[1 - P01, P01], [P10, 1 - P10]])
N_TRAJ, N_FRAMES = 200, 200


def two_state_dataset(seed):
    """labels (40 000,) int32 and the trajectory lengths of one dataset of the chain"""
    return oracle.jump_process(CHAIN, N_TRAJ, N_FRAMES, seed).reshape(-1).astype(np.int32), [N_FRAMES] * N_TRAJ


def two_state_t2(counts):
    """t2 of the 2 x 2 count matrices (..., 2, 2) in closed form: with two states every chain is reversible, the maximum-
    likelihood T is the row-normalised counts and lambda_2 = 1 - T01 - T10"""
    counts = np.asarray(counts, np.float64)
    T = counts / counts.sum(axis=-1, keepdims=True)
    return -1.0 / np.log(1.0 - T[..., 0, 1] - T[..., 1, 0])


def across_dataset_std(n_datasets, seed0):
    """std (ddof = 1) of the point estimate of t2 (lag 1) over independently generated datasets, in closed form"""
    t2 = []
    for s in range(n_datasets):
        labels, lengths = two_state_dataset(seed0 + s)
        C = oracle.transition_counts(labels, lengths, [1], 2)[0]
        t2.append(two_state_t2(C))
    return float(np.std(t2, ddof=1))
