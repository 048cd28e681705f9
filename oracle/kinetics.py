"""ORACLE (test infrastructure only) of the folding-kinetics calls (dff_struct_native_q, dff_core_states, dff_label_runs):
deliberately naive numpy -- a Python loop per trajectory for the core states, a loop for the runs, float64 numpy for Q.
Nothing here imports dff_amd."""
import numpy as np


def native_q(x, pairs, r0, beta=5.0, lam=1.2):
    """Q_s = (1 / P) sum_p 1 / (1 + exp(beta (r_p(s) - lam r0_p))) in float64 from the float32 coordinates -> float64 (n,);
    NaN for a frame with a non-finite coordinate, and for every frame when a pair is out of range or has i == j."""
    x = np.asarray(x, np.float32).astype(np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    r0 = np.asarray(r0, np.float32).astype(np.float64)
    n, N = x.shape[:2]
    if ((pairs < 0) | (pairs >= N)).any() or (pairs[:, 0] == pairs[:, 1]).any():
        return np.full(n, np.nan)
    q = np.full(n, np.nan)
    fin = np.isfinite(x).all((1, 2))
    d = x[fin][:, pairs[:, 0]] - x[fin][:, pairs[:, 1]]
    r = np.sqrt((d * d).sum(-1))
    with np.errstate(over="ignore"):
        q[fin] = (1.0 / (1.0 + np.exp(beta * (r - lam * r0)))).sum(-1) / len(pairs)
    return q


def starts_of(lengths, n):
    lengths = [int(n)] if lengths is None else [int(v) for v in lengths]
    assert sum(lengths) == n and min(lengths, default=0) >= 0
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def core_states(cv, lo, hi, lengths=None):
    """(labels int32 (n,), core int8 (n,)): the rule of include/dff.h, one frame after the other"""
    cv = np.asarray(cv, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    labels = np.empty(len(cv), np.int32)
    core = np.empty(len(cv), np.int8)
    s = starts_of(lengths, len(cv))
    for a, b in zip(s[:-1], s[1:]):
        state = -1
        for t in range(a, b):
            c = cv[t]
            here = -1
            if not np.isfinite(c):
                state = -1
            elif c <= lo:
                state = here = 0
            elif c >= hi:
                state = here = 1
            labels[t] = state
            core[t] = here
    return labels, core


def core_states_scan(cv, lo, hi, lengths=None):
    """the same labels by the formulation the kernel uses: an inclusive maximum over the index of the latest decisive frame
    (in a core, non-finite, or a trajectory's first), then the kind of that frame"""
    cv = np.asarray(cv, np.float32)
    n = len(cv)
    if n == 0:
        return np.empty(0, np.int32)
    fin = np.isfinite(cv)
    kind = np.where(~fin, -1, np.where(cv <= np.float32(lo), 0, np.where(cv >= np.float32(hi), 1, -1))).astype(np.int32)
    decisive = ~fin | (kind >= 0)
    s = starts_of(lengths, n)
    decisive[s[:-1][s[:-1] < n]] = True
    key = np.where(decisive, np.arange(n), -1)
    return kind[np.maximum.accumulate(key)]


def label_runs(labels, lengths=None):
    """dict of start int64, length int64, label int32, flags uint8 (bit 0: begins at its trajectory's first frame, bit 1: ends
    at its last), one entry per run, in time order"""
    labels = np.asarray(labels, np.int32)
    s = starts_of(lengths, len(labels))
    start, length, label, flags = [], [], [], []
    for a, b in zip(s[:-1], s[1:]):
        t = a
        while t < b:
            e = t
            while e + 1 < b and labels[e + 1] == labels[t]:
                e += 1
            start.append(t)
            length.append(e + 1 - t)
            label.append(labels[t])
            flags.append((1 if t == a else 0) | (2 if e + 1 == b else 0))
            t = e + 1
    return {"start": np.array(start, np.int64), "length": np.array(length, np.int64), "label": np.array(label, np.int32),
            "flags": np.array(flags, np.uint8)}


def helix(N, rise=3.6, radius=2.3, turn=np.deg2rad(100.0)):
    """an extended helical chain: the unfolded end of the scripted folding tests"""
    k = np.arange(N)
    return np.stack([radius * np.cos(turn * k), radius * np.sin(turn * k), rise * k], 1)


def scripted_frames(folded, script, repeat, sigma, seed):
    """frames folded + w (extended - folded) + sigma noise, w following `script`, each value `repeat` times: float32"""
    f = np.asarray(folded, np.float64)
    ext = helix(len(f))
    ext = ext - ext.mean(0) + f.mean(0)
    w = np.repeat(np.asarray(script, np.float64), repeat)
    rng = np.random.default_rng(seed)
    return (f[None] + w[:, None, None] * (ext - f)[None] + sigma * rng.standard_normal((len(w),) + f.shape)).astype(np.float32), w
