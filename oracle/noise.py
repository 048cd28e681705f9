"""Host reference of the kernels' noise stream (csrc/dff_device.h: philox4x32_10, philox_normal), numpy only.

The draw for (seed; item = traj_offset / sample_offset + i; step; bead; component c) is documented in include/dff.h:
the Philox4x32-10 block (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) of

    key     = (seed low word, seed high word)
    counter = (item low word, item high word ^ (bead << 8), step low word, step high word)

with step = step_offset + s for Langevin, the level t for a reverse DDPM step and 0xFFFFFFFF for the DDPM prior, followed
by a Box-Muller on u(w) = (float32(w) + 0.5) * 2^-32:

    c = 0, 1:  sqrt(-2 ln u(w0)) * cos / sin(2 pi u(w1))          c = 2:  sqrt(-2 ln u(w2)) * cos(2 pi u(w3))

The uniforms are three exactly rounded float32 operations, reproduced here bit for bit; the kernels evaluate the
transcendentals with the hardware instructions, so their draws equal `normals64` up to those instructions' error only.
`normals32_plain` is the same Box-Muller in plain numpy float32: the yardstick that error is measured in.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57     # Philox4x32 round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85     # Weyl increments of the two key words
PRIOR_STEP = 0xFFFFFFFF             # the step the DDPM prior x_T is drawn at
ITEM_LIMIT = 1 << 40                # items (offset + index) must stay below this: bits 40.. would alias the bead field

_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(a):
    """Python ints (up to 2^64 - 1) or integer arrays -> uint64 array, without a detour through float64 or int64."""
    if isinstance(a, np.ndarray) and a.dtype == np.uint64:
        return a
    a = np.asarray(a, dtype=object)
    return np.frompyfunc(lambda v: np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF), 1, 1)(a).astype(np.uint64)


def philox4x32_10(key, ctr):
    """key (..., 2), ctr (..., 4) words -> the (..., 4) output words (uint32) of ten Philox4x32 rounds."""
    key, ctr = _u64(key), _u64(ctr)
    shape = np.broadcast_shapes(key.shape[:-1], ctr.shape[:-1])
    k0, k1 = (np.broadcast_to(key[..., i] & _LO, shape) for i in range(2))
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i] & _LO, shape) for i in range(4))
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + np.uint64(W0)) & _LO
        k1 = (k1 + np.uint64(W1)) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def counters(seed, item, step, bead):
    """(key (..., 2), counter (..., 4)) as uint64 words for the broadcast of item, step, bead (ints or integer arrays)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    item, step, bead = np.broadcast_arrays(_u64(item), _u64(step), _u64(bead))
    if item.size and int(item.max()) >= ITEM_LIMIT:
        raise ValueError("item index >= 2^40: outside the range the counter layout keeps distinct (include/dff.h)")
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), item.shape + (2,))
    ctr = np.stack([item & _LO, ((item >> _S32) ^ (bead << np.uint64(8))) & _LO, step & _LO, (step >> _S32) & _LO], axis=-1)
    return key, ctr


def uniforms(words):
    """uint32 words -> the kernel's float32 uniforms in (0, 1]: float32(w) (round to nearest even), + 0.5f, * 2^-32."""
    w = np.asarray(words)
    assert w.dtype == np.uint32
    return (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def words(seed, items, steps, n_beads):
    """Philox words for every bead: (broadcast(items, steps).shape, n_beads, 4) uint32."""
    items, steps = np.broadcast_arrays(_u64(items), _u64(steps))
    bead = np.arange(n_beads, dtype=np.uint64)
    return philox4x32_10(*counters(seed, items[..., None], steps[..., None], bead))


def _box_muller(w, dtype, two_pi):
    u = uniforms(w).astype(dtype)
    minus2 = dtype(-2.0)
    ra, rb = np.sqrt(minus2 * np.log(u[..., 0])), np.sqrt(minus2 * np.log(u[..., 2]))
    a1, a3 = two_pi * u[..., 1], two_pi * u[..., 3]
    return np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3)], axis=-1)


def normals64(seed, items, steps, n_beads):
    """The draws in float64 on the exact float32 uniforms: (broadcast(items, steps).shape, n_beads, 3)."""
    return _box_muller(words(seed, items, steps, n_beads), np.float64, np.float64(2.0 * np.pi))


def normals32_plain(seed, items, steps, n_beads):
    """The same Box-Muller in plain numpy float32 (log, sqrt, cos / sin of float32(2 pi) * u): the accuracy yardstick."""
    out = _box_muller(words(seed, items, steps, n_beads), np.float32, np.float32(2.0 * np.pi))
    assert out.dtype == np.float32
    return out
