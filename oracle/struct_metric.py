"""ORACLE (test infrastructure only) -- float64 numpy statements of what the structure kernels compute (dff_struct_*,
dff_rmsd_matrix / dff_rmsd_nearest, dff_superpose): dihedrals, the TIC features and their projection, contacts by torch's
float32 formula, and ONE Kabsch superposition by SVD with the reflection correction, in four shapes:

  kabsch64        one frame at a time (the plain statement; NaN for a non-finite frame)
  kabsch64_batch  the same RMSD by a batched SVD (tests/test_struct_edges.py holds the two together)
  kabsch_matrix   kabsch64_batch once per candidate: the (n, m) matrix between two ensembles
  superpose64     kabsch64_batch extended to the rotation, the aligned frames and Horn's eigenvalue gap; stats64 on top

numpy and torch-CPU only; nothing here imports dff_amd, and the product path never imports this.
"""
import numpy as np
import torch


# ---------------------------------------------------------------- dihedrals
def dihedrals64(x, ind):
    x = np.asarray(x, np.float64)
    ind = np.asarray(ind)
    b1 = x[:, ind[:, 1]] - x[:, ind[:, 0]]
    b2 = x[:, ind[:, 2]] - x[:, ind[:, 1]]
    b3 = x[:, ind[:, 3]] - x[:, ind[:, 2]]
    c1, c2 = np.cross(b2, b3), np.cross(b1, b2)
    return np.arctan2((b1 * c1).sum(-1) * np.sqrt((b2 * b2).sum(-1)), (c1 * c2).sum(-1))


def consecutive(N):
    i = np.arange(N - 3)
    return np.stack([i, i + 1, i + 2, i + 3], 1)


def dihedral_ok(x, min_sin=0.1):
    """(n, N - 3) mask of well-conditioned dihedrals: the sines of both bond angles above min_sin (0.1, ~6 degrees from
    0 and 180, as in test_struct_metrics.py::test_dihedrals_vs_float64), and the float64 value at least 1e-3 from the
    +-pi branch cut"""
    b = np.diff(np.asarray(x, np.float64), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):       # coincident beads: NaN, masked out
        sin = np.linalg.norm(np.cross(b[:, :-1], b[:, 1:]), axis=-1) / (
            np.linalg.norm(b[:, :-1], axis=-1) * np.linalg.norm(b[:, 1:], axis=-1))
        ref = dihedrals64(x, consecutive(x.shape[1]))
    return (sin[:, :-1] > min_sin) & (sin[:, 1:] > min_sin) & (np.abs(ref) < np.pi - 1e-3)


def tic_rows(x):
    """frames whose dihedral features are all well enough conditioned for the TIC bar (an fp32 dihedral that lands on
    the other side of the branch cut, or at a near-straight bond angle, is off by up to 2 pi)"""
    return dihedral_ok(x, 0.01).all(1)


def wrap_err(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, np.float64) - b))))


# ---------------------------------------------------------------- TIC features and projection
def tic_features64(x):
    x = np.asarray(x, np.float64)
    N = x.shape[1]
    iu = np.triu_indices(N, 1)
    d = np.linalg.norm(x[:, iu[0]] - x[:, iu[1]], axis=-1)
    return np.hstack([dihedrals64(x, consecutive(N)), d])


def tic64_batch(x, mean, A, chunk=1 << 15):
    """(tic_features64(x) - mean) @ A, a chunk of frames at a time"""
    return np.concatenate([(tic_features64(x[i:i + chunk]) - mean) @ A for i in range(0, len(x), chunk)])


# ---------------------------------------------------------------- contacts
def torch_contacts(x, cutoff):
    x = torch.from_numpy(np.asarray(x, np.float32))
    return torch.norm(x[:, :, None, :] - x[:, None, :, :], dim=-1) < cutoff


def triu_mismatch(c, folded, offset):
    N = c.shape[-1]
    iu = torch.triu_indices(N, N, offset=offset)
    return (c[:, iu[0], iu[1]] != torch.as_tensor(folded)[iu[0], iu[1]]).sum(-1).numpy()


def contacts_batch(x, cutoff, folded=None, offset=3, chunk=1 << 13):
    """torch's float32 contact formula, a chunk of frames at a time -> (counts (N, N), mismatches (n,) or None)"""
    N = x.shape[1]
    counts = np.zeros((N, N), np.int64)
    mism = []
    for i in range(0, len(x), chunk):
        c = torch_contacts(x[i:i + chunk], cutoff)
        counts += c.sum(0).numpy()
        if folded is not None:
            mism.append(triu_mismatch(c, folded, offset))
    return counts, (np.concatenate(mism) if folded is not None else None)


# ---------------------------------------------------------------- Kabsch
def kabsch64(x, ref):
    """optimal proper-rotation RMSD, float64 SVD with the reflection correction; NaN for non-finite frames"""
    x = np.asarray(x, np.float64)
    r = np.asarray(ref, np.float64)
    r = r - r.mean(0)
    out = np.full(len(x), np.nan)
    for s, a in enumerate(x):
        if not np.isfinite(a).all():
            continue
        a = a - a.mean(0)
        U, S, Vt = np.linalg.svd(a.T @ r)
        S[-1] *= np.sign(np.linalg.det(U @ Vt))
        out[s] = np.sqrt(max(((a * a).sum() + (r * r).sum() - 2 * S.sum()) / len(a), 0.0))
    return out


def kabsch64_batch(x, ref, chunk=1 << 17):
    """kabsch64 for many frames at once: batched SVD of the (n, 3, 3) correlation matrices with the reflection fix"""
    x = np.asarray(x)
    r = np.asarray(ref, np.float64)
    r = r - r.mean(0)
    Gb = (r * r).sum()
    N = x.shape[1]
    out = np.empty(len(x))
    for i in range(0, len(x), chunk):
        a = np.asarray(x[i:i + chunk], np.float64)
        fin = np.isfinite(a).all((1, 2))
        a = np.where(fin[:, None, None], a, 0.0)
        a = a - a.mean(1, keepdims=True)
        U, S, Vt = np.linalg.svd(np.einsum("nbi,bj->nij", a, r))
        S[:, -1] *= np.sign(np.linalg.det(U @ Vt))
        msd = ((a * a).sum((1, 2)) + Gb - 2 * S.sum(1)) / N
        out[i:i + chunk] = np.where(fin, np.sqrt(np.maximum(msd, 0.0)), np.nan)
    return out


def kabsch_matrix(x, y):
    """(n, m) float64: kabsch64_batch(x, y[r]) for every candidate r; NaN columns for non-finite candidates"""
    out = np.full((len(x), len(y)), np.nan)
    for r, ref in enumerate(y):
        if np.isfinite(ref).all():
            out[:, r] = kabsch64_batch(x, ref)
    return out


# ---------------------------------------------------------------- superposition
def horn_gap(S):
    """relative gap (l1 - l2) / (l1 - l4) of the eigenvalues l1 >= ... >= l4 of Horn's key matrix of the (n, 3, 3)
    correlations S[s, i, j] = sum_b a_bi r_bj; 0 where l1 == l4 (K = 0)"""
    K = np.zeros((len(S), 4, 4))
    K[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    K[:, 0, 1] = S[:, 1, 2] - S[:, 2, 1]
    K[:, 0, 2] = S[:, 2, 0] - S[:, 0, 2]
    K[:, 0, 3] = S[:, 0, 1] - S[:, 1, 0]
    K[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    K[:, 1, 2] = S[:, 0, 1] + S[:, 1, 0]
    K[:, 1, 3] = S[:, 2, 0] + S[:, 0, 2]
    K[:, 2, 2] = -S[:, 0, 0] + S[:, 1, 1] - S[:, 2, 2]
    K[:, 2, 3] = S[:, 1, 2] + S[:, 2, 1]
    K[:, 3, 3] = -S[:, 0, 0] - S[:, 1, 1] + S[:, 2, 2]
    w = np.linalg.eigvalsh(K, UPLO="U")
    span = w[:, 3] - w[:, 0]
    return np.where(span > 0, (w[:, 3] - w[:, 2]) / np.where(span > 0, span, 1.0), 0.0)


def superpose64(x, ref):
    """kabsch64_batch extended to the rotation: for the float32 frames x (n, N, 3) and the float32 reference (N, 3), in
    float64: {"finite" (n,), "R" (n, 3, 3) the proper rotation minimising sum_b |R a_b - r_b|^2, "aligned" (n, N, 3) =
    R a + c_ref, "rmsd" (n,), "gap" (n,)}; NaN rows for non-finite frames."""
    x = np.asarray(x, np.float32).astype(np.float64)
    r = np.asarray(ref, np.float32).astype(np.float64)
    cr = r.mean(0)
    r0 = r - cr
    fin = np.isfinite(x).all((1, 2)) & bool(np.isfinite(r).all())
    a = np.where(fin[:, None, None], x, 0.0)
    a = a - a.mean(1, keepdims=True)
    S = np.einsum("nbi,bj->nij", a, np.where(np.isfinite(r0), r0, 0.0))
    U, sv, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(U @ Vt))
    d[d == 0] = 1.0
    D = np.stack([np.ones_like(d), np.ones_like(d), d], 1)
    R = np.einsum("nji,nj,nkj->nik", Vt, D, U)               # V D U^T
    sv[:, -1] *= d
    msd = ((a * a).sum((1, 2)) + (r0 * r0).sum() - 2 * sv.sum(1)) / x.shape[1]
    nan = np.where(fin, 0.0, np.nan)
    return {"finite": fin, "R": R + nan[:, None, None], "aligned": np.einsum("nij,nbj->nbi", R, a) + cr + nan[:, None, None],
            "rmsd": np.sqrt(np.maximum(msd, 0.0)) + nan, "gap": np.where(fin, horn_gap(S), np.nan)}


def stats64(o, ref):
    """(dsum (N, 3), dsq (N,), count, sum |d| (N, 3)) of the oracle's aligned frames: what dff_superpose accumulates, and
    the sum of the absolute terms its tolerance is relative to"""
    d = o["aligned"][o["finite"]] - np.asarray(ref, np.float32).astype(np.float64)
    return d.sum(0), (d * d).sum((0, 2)), int(o["finite"].sum()), np.abs(d).sum(0)
