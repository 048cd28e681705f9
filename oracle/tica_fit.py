"""ORACLE (test infrastructure only) -- float64 numpy statement of the sums dff_tica_moments accumulates, and the two
helpers the TICA tests compare models with.  The features themselves are oracle/struct_metric.py's tic_features64.
numpy only; nothing here imports dff_amd, and the product path never imports this.
"""
import numpy as np


def mirror(triu, F):
    m = np.zeros((F, F))
    m[np.triu_indices(F)] = triu
    return m + np.triu(m, 1).T


def sign_aligned_rel(W, R):
    """per-column relative error of W against R, each column of W flipped to R's sign"""
    W = W * np.sign((W * R).sum(0))
    return np.linalg.norm(W - R, axis=0) / np.linalg.norm(R, axis=0)


def moments64(g, lengths, lag):
    """(S_x, S_y, M_0, M_tau, w) of dff_tica_moments over shifted float64 features g"""
    X, Y, o = [], [], 0
    for L in lengths:
        if L > lag:
            X.append(g[o:o + L - lag])
            Y.append(g[o + lag:o + L])
        o += L
    F = g.shape[1]
    X = np.concatenate(X) if X else np.zeros((0, F))
    Y = np.concatenate(Y) if Y else np.zeros((0, F))
    return X.sum(0), Y.sum(0), X.T @ X + Y.T @ Y, X.T @ Y + Y.T @ X, len(X)
