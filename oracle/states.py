"""ORACLE (test infrastructure only) -- float64 numpy restatements of the state analysis (csrc/dff_states.hip,
evaluate.KMeans / StateTransitionEvaluator).  deeptime is not installed, so MiniBatchKMeans and TransitionCountEstimator
are restated from their documented semantics: nearest centre, lowest index on a tie; every pair (t, t + lag) inside a
discrete trajectory.  numpy only; nothing here imports dff_amd, and the product path never imports this.
"""
import numpy as np


def dist2_64(p, centers):
    p, c = np.asarray(p, np.float64), np.asarray(centers, np.float64)
    return ((p[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def counts64(labels, lengths, lags, K):
    labels = np.asarray(labels, np.int64)
    C = np.zeros((len(lags), K, K), np.int64)
    skipped = np.zeros(len(lags), np.int64)
    o = 0
    for L in lengths:
        seg = labels[o:o + L]
        o += L
        for li, lag in enumerate(lags):
            if L > lag:
                a, b = seg[:-lag], seg[lag:]
                ok = (a >= 0) & (b >= 0)
                np.add.at(C[li], (a[ok], b[ok]), 1)
                skipped[li] += int((~ok).sum())
    return C, skipped


def lloyd64(p, centers, max_iter, tol):
    """KMeans.fit's documented loop; returns (centres, n_iter, inertia of the final centres)."""
    p, c = np.asarray(p, np.float64), np.array(centers, np.float64)
    prev, n_iter = None, 0
    for _ in range(max_iter):
        d2 = dist2_64(p, c)
        lab = d2.argmin(1)
        inertia = d2[np.arange(len(p)), lab].sum()
        for k in range(len(c)):
            if np.any(lab == k):
                c[k] = p[lab == k].sum(0) / (lab == k).sum()
        n_iter += 1
        if prev is not None and abs(prev - inertia) <= tol * prev:
            break
        prev = inertia
    return c, n_iter, dist2_64(p, c).min(1).sum()
