"""ORACLE (test infrastructure only) -- the seeded input generators of the analysis tests: rotations, frames, trajectories,
points and labels.  Each takes a numpy Generator (or a seed) and draws from it in a fixed order, so a test's inputs follow
from its seed alone.  Two generators with different formulas are two functions: walks / gaussian, chain_frames /
synth_chain_frames, ou_trajectories / two_state_trajectories.  numpy only; nothing here imports dff_amd.
"""
import numpy as np

from . import synth


# ---------------------------------------------------------------- rotations
def rand_rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def axis_rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [k for k in range(3) if k != axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def half_turn(axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return 2.0 * np.outer(a, a) - np.eye(3)


# ---------------------------------------------------------------- frames
def walks(rng, n, N):
    """random walks with 3.8 A bonds, each at a random place: float32 (n, N, 3)"""
    step = rng.standard_normal((n, N, 3))
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    return (np.cumsum(step, 1) + 20 * rng.standard_normal((n, 1, 3))).astype(np.float32)


def gaussian(rng, n, N):
    return (rng.standard_normal((n, N, 3)) * 5).astype(np.float32), (rng.standard_normal((N, 3)) * 5).astype(np.float32)


def needle(rng, N, width):
    """a straight 3.8 A-spaced chain along x with Gaussian lateral scatter of the given width"""
    t = (np.arange(N) - (N - 1) / 2) * 3.8
    return np.stack([t, width * rng.standard_normal(N), width * rng.standard_normal(N)], 1)


def integer_walks(rng, n, N):
    """integer chains whose consecutive beads are 5, 7 or 9 apart exactly: signed permutations of (3, 4, 0),
    (2, 3, 6) and (1, 4, 8)"""
    steps = np.array([[3, 4, 0], [2, 3, 6], [1, 4, 8]], np.float64)
    perms = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]])
    k = rng.integers(3, size=(n, N - 1))
    v = steps[k[..., None], perms[rng.integers(6, size=(n, N - 1))]] * rng.choice([-1.0, 1.0], size=(n, N - 1, 3))
    x = np.concatenate([np.zeros((n, 1, 3)), np.cumsum(v, 1)], 1) + rng.integers(-20, 20, size=(n, 1, 3))
    return x.astype(np.float32)


def planar_walks(rng, n, N):
    """integer chains in the z = 0 plane, no two consecutive bonds parallel, mapped by 3 x an exact rotation
    [[1, 2, 2], [2, 1, -2], [2, -2, 1]] / 3 into an oblique plane: every dihedral is exactly 0 (cis) or pi (trans)"""
    dirs = np.array([[1, 0], [1, 1], [0, 1], [-1, 1], [-1, 0], [-1, -1], [0, -1], [1, -1]], np.float64)   # k + 4: opposite
    x = np.zeros((n, N, 3))
    for s in range(n):
        k = rng.integers(8)
        for i in range(1, N):
            k = (k + rng.choice([1, 2, 3, 5, 6, 7])) % 8 if i > 1 else k
            x[s, i, :2] = x[s, i - 1, :2] + dirs[k] * rng.integers(1, 4)
    M = np.array([[1, 2, 2], [2, 1, -2], [2, -2, 1]], np.float64)
    return (x @ M.T + rng.integers(-10, 10, size=(n, 1, 3))).astype(np.float32)


def chain_frames(n, N, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, N, 3)) * 4 + np.arange(N)[None, :, None] * 3.0).astype(np.float32)


def synth_chain_frames(n, N, stream):
    """Chain-like frames in Angstrom: beads 2 apart along x plus O(3) noise."""
    return (synth.normal((n, N, 3), 777, stream) * 3 + np.arange(N)[None, :, None] * 2.0).astype(np.float32)


def noisy_ensemble(rng, template, n, sigma):
    """n copies of the template, each with Gaussian noise of width sigma, randomly rotated and translated"""
    N = len(template)
    x = np.empty((n, N, 3), np.float32)
    for s in range(n):
        x[s] = (template + sigma * rng.standard_normal((N, 3))) @ rand_rot(rng).T + 10 * rng.standard_normal(3)
    return x


# ---------------------------------------------------------------- trajectories
def ou_trajectories(folded, lengths, seed, rho_slow=0.999, rho_fast=0.6, sigma=1.5):
    """seeded Ornstein-Uhlenbeck trajectories around a folded structure: 3N modes of a random orthonormal basis, their
    autocorrelations spread from rho_slow to rho_fast per frame"""
    rng = np.random.default_rng(seed)
    f = np.asarray(folded, np.float64).reshape(-1)
    D = f.size
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    rho = np.geomspace(rho_slow, rho_fast, D)
    out = []
    for L in lengths:
        z = np.empty((L, D))
        z[0] = rng.standard_normal(D) * sigma
        eps = rng.standard_normal((L, D)) * sigma * np.sqrt(1 - rho ** 2)
        for t in range(1, L):
            z[t] = rho * z[t - 1] + eps[t]
        out.append((f + z @ Q.T).reshape(L, -1, 3).astype(np.float32))
    return out


def two_state_trajectories(folded, lengths, seed, amp=4.0, sigma=0.4):
    """seeded Ornstein-Uhlenbeck trajectories around a folded structure, as ou_trajectories builds them (3N modes of a
    random orthonormal basis with autocorrelations from 0.995 to 0.6 per frame), the slowest mode driving a two-state
    switch: the structure is displaced by +-amp along that mode according to the sign of its OU coordinate."""
    rng = np.random.default_rng(seed)
    f = np.asarray(folded, np.float64).reshape(-1)
    D = f.size
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    rho = np.geomspace(0.995, 0.6, D)
    out = []
    for L in lengths:
        z = np.empty((L, D))
        z[0] = rng.standard_normal(D) * sigma
        eps = rng.standard_normal((L, D)) * sigma * np.sqrt(1 - rho ** 2)
        for t in range(1, L):
            z[t] = rho * z[t - 1] + eps[t]
        z[:, 0] = np.where(z[:, 0] > 0, amp, -amp) + 0.25 * z[:, 0]
        out.append((f + z @ Q.T).reshape(L, -1, 3).astype(np.float32))
    return out


# ---------------------------------------------------------------- points and labels
def blobs(K, d, per, seed, sep=50.0, sigma=0.5):
    rng = np.random.default_rng(seed)
    true = (rng.permutation(K)[:, None] * sep + rng.uniform(5.0, 15.0, (K, d)))
    which = rng.integers(0, K, K * per)
    return true, true[which] + rng.standard_normal((K * per, d)) * sigma, which


def splitmix_labels(n, K):
    """Labels 0 .. K - 1 with a few -1 (the label of a non-finite frame)."""
    lab = np.floor(synth.uniform((n,), 781, 1, 0.0, float(K))).astype(np.int32)
    lab[::97] = -1
    return lab
