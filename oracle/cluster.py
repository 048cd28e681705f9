"""ORACLE of the RMSD clustering tests (a helper, not a test): the greedy loop of Daura et al. (`gmx cluster -method
gromos`) in numpy on a boolean neighbour matrix, with the rules of dff_gromos_steps (include/dff.h) --
  the self bit is set by definition for every frame that takes part, and for no other;
  the centre is the alive frame with the most alive neighbours, the LOWEST index among ties;
  when the largest alive degree is 1 the remaining frames become singletons in ascending index order (what the plain
  loop gives anyway; written out so that the cap on the number of clusters is applied the same way);
  a frame that does not take part (non-finite coordinates) keeps -1, as do frames beyond max_clusters --
the seeded ensemble the GPU tests cluster, its float64 distances, and the cutoff picker that keeps every pair clear of
the cutoff.  numpy only; nothing here imports dff_amd."""
import numpy as np

from oracle.frames import noisy_ensemble, walks
from oracle.struct_metric import kabsch_matrix

SIGMA = 0.5                     # Angstrom per coordinate: two copies of a template are ~ SIGMA sqrt(6) apart
COUNTS = (90, 60, 30)           # copies of the three templates
OUTLIERS = 20
BASE = SIGMA * np.sqrt(3.0)     # the scale the cutoff windows are multiples of


# ---------------------------------------------------------------- the greedy loop
def neighbors(D, cutoff, finite=None):
    """boolean (n, n): D <= cutoff off the diagonal, the diagonal = finite, all-zero rows and columns for the others"""
    D = np.asarray(D)
    n = len(D)
    fin = np.ones(n, bool) if finite is None else np.asarray(finite, bool)
    with np.errstate(invalid="ignore"):
        A = D <= cutoff                                         # NaN compares false
    A = A & fin[:, None] & fin[None, :]
    A[np.arange(n), np.arange(n)] = fin
    return A


def gromos(A, max_clusters=None):
    """-> (labels (n,) int64, centers (K,) int64, sizes (K,) int64) of the symmetric boolean matrix A whose diagonal says
    which frames take part"""
    A = np.asarray(A, bool)
    n = len(A)
    assert A.shape == (n, n) and np.array_equal(A, A.T)
    kmax = n if max_clusters is None else int(max_clusters)
    alive = A[np.arange(n), np.arange(n)].copy()
    labels = np.full(n, -1, np.int64)
    centers, sizes = [], []
    while alive.any() and len(centers) < kmax:
        deg = (A & alive[None, :]).sum(1)
        deg[~alive] = 0
        top = int(deg.max())
        if top == 1:
            for s in np.flatnonzero(alive)[:kmax - len(centers)]:
                labels[s] = len(centers)
                centers.append(int(s))
                sizes.append(1)
                alive[s] = False
            break
        c = int(np.argmax(deg))                                 # the first of the maxima: the lowest index
        members = A[c] & alive
        labels[members] = len(centers)
        centers.append(c)
        sizes.append(int(members.sum()))
        alive &= ~members
    return labels, np.asarray(centers, np.int64), np.asarray(sizes, np.int64)


def top_ties(A):
    """how many frames share the largest degree of A (the tie rule is exercised when > 1)"""
    deg = np.asarray(A, bool).sum(1)
    return int((deg == deg.max()).sum())


# ---------------------------------------------------------------- bits
def pack(A):
    """boolean (n, n) -> int64 (n, ceil(n / 64)): bit r & 63 of word [s, r >> 6] = A[s, r]"""
    A = np.asarray(A, bool)
    n = len(A)
    W = (n + 63) // 64
    P = np.zeros((n, 64 * W), bool)
    P[:, :n] = A
    return np.ascontiguousarray(np.packbits(P, axis=1, bitorder="little")).view(np.int64).reshape(n, W)


def unpack(words, n):
    """int64 (n, W) -> boolean (n, 64 W): every bit, the padding included"""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint8).reshape(n, -1)
    return np.unpackbits(w, axis=1, bitorder="little").astype(bool)


# ---------------------------------------------------------------- the seeded ensemble
def ensemble(N, seed):
    """200 frames float32 (200, N, 3): three random-walk templates, 90 / 60 / 30 noisy copies of them (SIGMA per
    coordinate, randomly rotated and moved), 20 random walks that belong to nothing, in a seeded random order"""
    rng = np.random.default_rng(seed)
    templates = walks(rng, len(COUNTS), N).astype(np.float64)
    parts = [noisy_ensemble(rng, t, c, SIGMA) for t, c in zip(templates, COUNTS)]
    parts.append(walks(rng, OUTLIERS, N))
    x = np.concatenate(parts)
    return np.ascontiguousarray(x[rng.permutation(len(x))])


def distances(x):
    """float64 (n, n) minimum RMSD over proper rotations, symmetrised (the two orders of a pair differ by rounding);
    NaN rows and columns for non-finite frames"""
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x).all((1, 2))
    D = kabsch_matrix(x, x)
    D[~fin, :] = np.nan
    D[:, ~fin] = np.nan
    with np.errstate(invalid="ignore"):
        return np.minimum(D, D.T)


def pick_cutoff(D, lo, hi):
    """(cutoff, half_gap): the middle of the widest gap between consecutive sorted pair RMSDs inside [lo, hi], and half
    that gap: no pair is closer to the cutoff.  ValueError when fewer than two pair RMSDs fall inside."""
    D = np.asarray(D)
    v = D[np.triu_indices(len(D), 1)]
    v = np.sort(v[np.isfinite(v) & (v >= lo) & (v <= hi)])
    if len(v) < 2:
        raise ValueError(f"{len(v)} pair RMSDs in [{lo}, {hi}]")
    gaps = np.diff(v)
    i = int(np.argmax(gaps))
    return float((v[i] + v[i + 1]) / 2), float(gaps[i] / 2)


def pick_cutoff_widening(D, factor, step=0.1):
    """pick_cutoff in the window (1 -+ k step) factor BASE, k = 1, 2, ... until pair RMSDs fall inside it"""
    for k in range(1, 10):
        try:
            return pick_cutoff(D, (1 - k * step) * factor * BASE, (1 + k * step) * factor * BASE)
        except ValueError:
            continue
    raise ValueError(f"no pair RMSD near {factor * BASE}")
