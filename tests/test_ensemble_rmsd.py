"""Nearest-structure RMSD between two ensembles on the GPU (dff_rmsd_matrix, dff_rmsd_nearest; csrc/dff_ensemble.hip).

The reference throughout is the float64 Kabsch / SVD model of oracle/struct_metric.py (kabsch64_batch, with the determinant
correction), applied once per candidate (kabsch_matrix), at the bar of tests/support.py: |err| <= RMSD_ATOL + RMSD_RTOL * rmsd.
Bead counts 4 and 64 are the limits, 5, 10 and 35 need the zero-padded k-steps; frame counts 1, 15, 16, 17, 65, 257 cross the 16-frame MFMA
tile, the 32-candidate workgroup tile, the 64-lane wave and one workgroup.  The value of a pair does not depend on what
else is in the call, so the small shapes are checked bit for bit against blocks of the 257 x 257 matrix, and that matrix
once against Kabsch."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle.frames import needle, rand_rot, walks
from oracle.struct_metric import kabsch_matrix
from support import MIRROR, RMSD_ATOL, RMSD_RTOL, B, assert_close, dev, up, x_rmsd  # noqa: F401  (dev: fixture)

pytestmark = pytest.mark.gpu

BEADS = [4, 5, 10, 35, 64]
COUNTS = [1, 15, 16, 17, 65, 257]


def row_min(M):
    """(min, first argmin) of every row of the float32 matrix M, NaN entries left out; NaN / -1 for an all-NaN row"""
    M = np.asarray(M)
    if M.shape[1] == 0:
        return np.full(len(M), np.nan, np.float32), np.full(len(M), -1, np.int64)
    filled = np.where(np.isnan(M), np.float32(np.inf), M)
    idx = filled.argmin(1)                                   # numpy's argmin is the first minimum
    val = M[np.arange(len(M)), idx]
    none = np.isnan(M).all(1)
    return np.where(none, np.float32(np.nan), val).astype(np.float32), np.where(none, -1, idx)


def matrix(x, y, dev):
    return B().rmsd_matrix(up(x, dev), up(y, dev)).cpu().numpy()


def nearest(x, y, dev, self_first=-1):
    r, i = B().rmsd_nearest(up(x, dev), up(y, dev), self_first)
    return r.cpu().numpy(), i.cpu().numpy()


def assert_nearest_is_row_min(x, y, dev, M=None, what=""):
    M = matrix(x, y, dev) if M is None else M
    r, i = nearest(x, y, dev)
    wr, wi = row_min(M)
    assert r.dtype == np.float32 and i.dtype == np.int64
    assert np.array_equal(r, wr, equal_nan=True), what
    assert np.array_equal(i, wi), what
    return r, i


_sets = {}


@pytest.fixture(scope="module")
def ensembles(golden):
    """per bead count: queries x and candidates y (257 frames each, float32), the float64 Kabsch matrix between them --
    computed once and shared, never modified.  At 10 beads half of each set are golden chignolin frames."""
    def get(N):
        if N not in _sets:
            rng = np.random.default_rng(4000 + N)
            x, y = walks(rng, 257, N), walks(rng, 257, N)
            if N == 10:
                g = golden("struct_ref_chignolin.npz")["x"].astype(np.float32)
                g = g[np.isfinite(g).all((1, 2))]
                x[128:] = g[:129]
                y[128:] = g[1000:1129]
            for a in (x, y):
                a.setflags(write=False)
            _sets[N] = (x, y, kabsch_matrix(x, y))
        return _sets[N]
    return get


# ---------------------------------------------------------------- 1. the matrix vs Kabsch, every pair
@pytest.mark.parametrize("N", BEADS)
def test_matrix_vs_kabsch(dev, ensembles, N):
    x, y, want = ensembles(N)
    M = matrix(x, y, dev)
    assert M.dtype == np.float32 and M.shape == (257, 257)
    assert_close(M, want, f"N={N} 257 x 257")
    for n in COUNTS:
        for m in COUNTS:
            sub = matrix(x[:n], y[:m], dev)
            assert np.array_equal(sub, M[:n, :m]), f"N={N} n={n} m={m}: not the block of the large matrix"
    # a window that starts inside a tile: the same pairs, the same bits
    assert np.array_equal(matrix(x[5:70], y[3:40], dev), M[5:70, 3:40])


@pytest.mark.parametrize("N", BEADS)
def test_matrix_vs_single_reference_kernel(dev, ensembles, N):
    """where the old kernel gives the same quantity: dff_struct_rmsd(x, ref=y[r]), at the same bar"""
    x, y, _ = ensembles(N)
    M = matrix(x, y, dev).astype(np.float64)
    xd = up(x, dev)
    for r in (0, 15, 16, 31, 32, 256):
        old = B().struct_rmsd(xd, torch.tensor(y[r])).cpu().numpy().astype(np.float64)
        assert_close(M[:, r], old, f"N={N} candidate {r} vs dff_struct_rmsd")


# ---------------------------------------------------------------- 2. nearest = row minimum and first argmin, bit for bit
@pytest.mark.parametrize("N", BEADS)
def test_nearest_is_row_minimum(dev, ensembles, N):
    x, y, want = ensembles(N)
    M = matrix(x, y, dev)
    for n in COUNTS:
        for m in COUNTS:
            r, i = assert_nearest_is_row_min(x[:n], y[:m], dev, M[:n, :m], f"N={N} n={n} m={m}")
            assert_close(r, want[:n, :m].min(1), f"N={N} n={n} m={m} nearest vs Kabsch")


@pytest.mark.parametrize("N", [4, 10, 64])
def test_nearest_lowest_index_among_exact_duplicates(dev, ensembles, N):
    x, y, _ = ensembles(N)
    x = x[:65]
    # every candidate three times, in different workgroup tiles (32 candidates each) and different 16-column halves;
    # the queries' own copies too, so that every row's minimum is reached three times
    base = np.concatenate([y[:40], x[:25]])
    cand = np.concatenate([base, base[::-1], base])
    M = matrix(x, cand, dev)
    k = len(base)
    assert np.array_equal(M[:, :k], M[:, 2 * k:]) and np.array_equal(M[:, :k], M[:, k:2 * k][:, ::-1])
    r, i = assert_nearest_is_row_min(x, cand, dev, M, f"N={N} duplicates")
    assert (i < k).all()
    assert np.array_equal(i[:25], 40 + np.arange(25))          # the query's own first copy
    assert (np.sum(M == r[:, None], axis=1) >= 3).all()


# ---------------------------------------------------------------- 3. bit-identical: calls, splits, chunk sizes
@pytest.mark.parametrize("N", [5, 35])
def test_nearest_is_reproducible_and_split_invariant(dev, ensembles, N):
    from dff_amd import evaluate
    x, y, _ = ensembles(N)
    xd, yd = up(x, dev), up(y, dev)
    r0, i0 = B().rmsd_nearest(xd, yd)
    r1, i1 = B().rmsd_nearest(xd, yd)
    assert torch.equal(r0, r1) and torch.equal(i0, i1)
    for chunk in (1, 16, 100):
        r, i = evaluate.nearest_rmsd(torch.tensor(x), torch.tensor(y), chunk=chunk, device=dev)
        assert r.device.type == "cuda" and torch.equal(r, r0) and torch.equal(i, i0), chunk
    # candidates split over calls at an odd place, merged by (value, index): the same answer
    ra, ia = B().rmsd_nearest(xd, yd[:77].contiguous())
    rb, ib = B().rmsd_nearest(xd, yd[77:].contiguous())
    take_b = rb < ra
    assert torch.equal(torch.where(take_b, rb, ra), r0) and torch.equal(torch.where(take_b, ib + 77, ia), i0)


def test_nearest_across_query_passes_and_grid_stride(dev):
    """n = 2^20 + 17 queries: two passes over the key workspace (2^20 queries each), and with 3 candidates (one
    workgroup tile) a grid capped at 4096 workgroups whose waves stride over 65537 query tiles"""
    rng = np.random.default_rng(77)
    N, n = 4, (1 << 20) + 17
    x = torch.from_numpy(walks(rng, 4096, N)).to(dev).repeat(257, 1, 1)[:n].contiguous()
    x[-17:] += 0.25 * torch.randn((17, N, 3), device=dev)
    y = torch.from_numpy(walks(rng, 3, N)).to(dev)
    r, i = B().rmsd_nearest(x, y)
    for sl in (slice(0, 4096), slice(n - 4096, n), slice((1 << 20) - 100, (1 << 20) + 17)):
        M = B().rmsd_matrix(x[sl].contiguous(), y).cpu().numpy()
        wr, wi = row_min(M)
        assert np.array_equal(r[sl].cpu().numpy(), wr) and np.array_equal(i[sl].cpu().numpy(), wi)
    # the 4096 distinct queries repeat with period 4096: so do the results
    assert torch.equal(r[: 255 * 4096].view(255, 4096), r[:4096].expand(255, 4096))
    assert torch.equal(i[: 255 * 4096].view(255, 4096), i[:4096].expand(255, 4096))


# ---------------------------------------------------------------- 4. self_first
@pytest.mark.parametrize("N", BEADS)
def test_self_first(dev, ensembles, N):
    from dff_amd import evaluate
    x, _, _ = ensembles(N)
    M = matrix(x, x, dev)
    r, i = nearest(x, x, dev)
    assert (r <= RMSD_ATOL).all() and np.array_equal(i, np.arange(len(x)))
    masked = M.copy()
    np.fill_diagonal(masked, np.nan)
    wr, wi = row_min(masked)
    r, i = nearest(x, x, dev, self_first=0)
    assert np.array_equal(r, wr) and np.array_equal(i, wi)
    assert (r > 0).all() and (i != np.arange(len(x))).all()
    for chunk in (None, 16, 100):
        xt = torch.tensor(x)
        rt, it = evaluate.nearest_rmsd(xt, xt, exclude_self=True, chunk=chunk, device=dev)
        assert np.array_equal(rt.cpu().numpy(), wr) and np.array_equal(it.cpu().numpy(), wi)
    # a window of the ensemble as queries: query s is candidate 40 + s
    r, i = nearest(x[40:105], x, dev, self_first=40)
    assert np.array_equal(r, wr[40:105]) and np.array_equal(i, wi[40:105])
    # a single structure against itself alone: no candidate is left
    r, i = nearest(x[:1], x[:1], dev, self_first=0)
    assert np.isnan(r).all() and (i == -1).all()


# ---------------------------------------------------------------- 5. rigid motions match, mirror images do not
@pytest.mark.parametrize("N", BEADS)
def test_rigid_copies_match_and_mirror_images_do_not(dev, ensembles, N):
    x = ensembles(N)[0][:65]
    rng = np.random.default_rng(5000 + N)
    x64 = x.astype(np.float64)
    moved = np.stack([a @ rand_rot(rng).T + 30 * rng.standard_normal(3) for a in x64]).astype(np.float32)
    mirrored = np.stack([(a * MIRROR) @ rand_rot(rng).T + 30 * rng.standard_normal(3) for a in x64]).astype(np.float32)
    cand = np.concatenate([mirrored, moved])                 # the mirror images come first: a tie would pick them
    want = kabsch_matrix(x, cand)
    M = matrix(x, cand, dev)
    assert_close(M, want, f"N={N} rigid + mirrored copies")
    own_mirror = want[np.arange(65), np.arange(65)]
    chiral = own_mirror > 0.05               # proper rotations only: a mirror image is far (a near-planar walk aside)
    assert chiral.mean() > 0.8, "the oracle itself: a random walk is chiral"
    assert (M[np.arange(65), np.arange(65)][chiral] > 0.049).all()
    r, i = assert_nearest_is_row_min(x, cand, dev, M, f"N={N} rigid")
    assert (r <= RMSD_ATOL).all() and np.array_equal(i, 65 + np.arange(65))


# ---------------------------------------------------------------- 6. hard spectra, as queries and as candidates
@pytest.mark.parametrize("N", [4, 10, 35, 64])
def test_hard_spectra_both_sides(dev, N):
    """the families test_struct_edges.py found hard for the single-reference kernel -- needles (the two largest
    eigenvalues of the key matrix nearly coincide), planar frames (a mirror image is a rotation away), symmetric tops --
    against one another"""
    rng = np.random.default_rng(6000 + N)
    frames = []
    for w in (0.0, 1e-3, 1e-2, 0.1, 1.0):
        for s in (0.0, 1e-3, 0.1, 1.0):
            a = (needle(rng, N, w) + s * rng.standard_normal((N, 3))) @ rand_rot(rng).T
            frames += [a, a * MIRROR]
    plane = rng.standard_normal((N, 3)) * 5 * np.array([1.0, 1.0, 0.0])
    frames += [plane, plane @ rand_rot(rng).T, plane * MIRROR, (plane * MIRROR) @ rand_rot(rng).T]
    frames += [(plane + 0.1 * rng.standard_normal((N, 3))) @ rand_rot(rng).T for _ in range(3)]
    t = rng.standard_normal((N, 3))
    t -= t.mean(0)
    w, V = np.linalg.eigh(t.T @ t)
    t = t @ V / np.sqrt(w)
    for c in ((9.0, 4.0, 4.0), (6.0, 6.0, 6.0), (30.0, 0.5, 0.5)):
        top = t * np.sqrt(np.array(c) * N)
        frames += [top, top * MIRROR, top * -1.0, (top * MIRROR) @ rand_rot(rng).T, top @ rand_rot(rng).T]
    compact = rng.standard_normal((N, 3)) * 5
    frames += [compact, compact * MIRROR, np.tile(np.array([[1.5, -2.0, 3.25]]), (N, 1))]
    f = np.asarray(frames, np.float32)
    want = kabsch_matrix(f, f)
    M = matrix(f, f, dev)
    assert_close(M, want, f"N={N} hard spectra, {len(f)} x {len(f)}")
    assert_nearest_is_row_min(f, f, dev, M, f"N={N} hard spectra")
    masked = M.copy()
    np.fill_diagonal(masked, np.nan)
    wr, wi = row_min(masked)
    r, i = nearest(f, f, dev, self_first=0)
    assert np.array_equal(r, wr) and np.array_equal(i, wi)


# ---------------------------------------------------------------- 7. non-finite frames, empty sets, refused arguments
@pytest.mark.parametrize("N", [4, 10, 64])
def test_nonfinite_frames(dev, ensembles, N):
    x, y, _ = ensembles(N)
    x, y = x[:70].copy(), y[:70].copy()
    clean = matrix(x, y, dev)
    bad_q = {0: (0, 0, np.inf), 15: (N - 1, 2, -np.inf), 16: (N // 2, 1, np.nan), 69: (0, 2, np.nan)}
    bad_c = {1: (0, 1, np.nan), 31: (N - 1, 0, np.inf), 32: (1, 2, -np.inf), 68: (N // 2, 0, np.nan)}
    for s, (b, c, v) in bad_q.items():
        x[s, b, c] = v
    for s, (b, c, v) in bad_c.items():
        y[s, b, c] = v
    M = matrix(x, y, dev)
    nanq, nanc = np.zeros(70, bool), np.zeros(70, bool)
    nanq[list(bad_q)] = True
    nanc[list(bad_c)] = True
    assert np.array_equal(np.isnan(M), nanq[:, None] | nanc[None, :])
    keep = ~(nanq[:, None] | nanc[None, :])
    assert np.array_equal(M[keep], clean[keep])               # every other pair: the same bits
    assert_close(M, kabsch_matrix(x, y), f"N={N} non-finite")
    r, i = assert_nearest_is_row_min(x, y, dev, M, f"N={N} non-finite")
    assert np.isnan(r[nanq]).all() and (i[nanq] == -1).all()
    assert np.isfinite(r[~nanq]).all() and not np.isin(i, list(bad_c)).any()
    # every candidate bad, no candidate, no query
    r, i = nearest(x, y[list(bad_c)], dev)
    assert np.isnan(r).all() and (i == -1).all()
    r, i = nearest(x, y[:0], dev)
    assert r.shape == (70,) and np.isnan(r).all() and (i == -1).all()
    r, i = nearest(x[:0], y, dev)
    assert r.shape == (0,) and i.shape == (0,)
    assert matrix(x[:0], y, dev).shape == (0, 70) and matrix(x, y[:0], dev).shape == (70, 0)


def test_refused_arguments(dev):
    b = B()
    lib = b.load_library()
    for N in (3, 65):
        x, y = torch.ones((20, N, 3), device=dev), torch.ones((20, N, 3), device=dev)
        with pytest.raises(ValueError, match="n_beads"):
            b.rmsd_nearest(x, y)
        with pytest.raises(ValueError, match="n_beads"):
            b.rmsd_matrix(x, y)
        with pytest.raises(ValueError, match="n_beads"):
            b.rmsd_nearest_workspace_bytes(20, 20, N)
    with pytest.raises(ValueError, match="negative"):
        b.rmsd_nearest_workspace_bytes(-1, 20, 10)
    with pytest.raises(ValueError, match="negative"):
        b.rmsd_nearest_workspace_bytes(20, -1, 10)
    with pytest.raises(ValueError, match="beads"):
        b.rmsd_nearest(torch.ones((5, 10, 3), device=dev), torch.ones((5, 11, 3), device=dev))
    N, n, m = 10, 20, 30
    x, y = torch.randn((n, N, 3), device=dev), torch.randn((m, N, 3), device=dev)
    need = b.rmsd_nearest_workspace_bytes(n, m, N)
    assert 0 < need <= 8 << 20
    assert b.rmsd_nearest_workspace_bytes(1 << 40, 1 << 30, N) <= 8 << 20     # bounded
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((n,), -7.0, device=dev)
    idx = torch.full((n,), -7, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731

    def call(xp, yp, outp, wsp, wsb, n_=n, m_=m, sf=-1):
        return lib.dff_rmsd_nearest(0, xp, n_, yp, m_, N, sf, outp, p(idx), wsp, wsb, None)

    assert call(p(x), p(y), p(out), p(ws), need - 1) == 1 and b"workspace" in lib.dff_last_error()
    assert call(p(x), p(y), p(out), None, need) == 1
    odd = torch.empty(need + 4, dtype=torch.uint8, device=dev)[4:]           # the keys are 64-bit words under an atomic minimum
    assert call(p(x), p(y), p(out), p(odd), need) == 1 and b"the workspace must be 8-byte aligned" in lib.dff_last_error()
    assert call(p(x), p(y), None, p(ws), need) == 1 and b"null output" in lib.dff_last_error()
    assert call(None, p(y), p(out), p(ws), need) == 1
    assert call(p(x), None, p(out), p(ws), need) == 1
    assert call(p(x), p(y), p(out), p(ws), need, n_=-1) == 1
    assert call(p(x), p(y), p(out), p(ws), need, m_=-1) == 1
    assert call(p(x), p(y), p(out), p(ws), need, sf=-2) == 1
    assert lib.dff_rmsd_matrix(0, p(x), n, p(y), m, N, None, None) == 1 and b"null output" in lib.dff_last_error()
    assert lib.dff_rmsd_matrix(0, p(x), 1 << 20, p(y), 1 << 20, N, p(out), None) == 1 and b"2^28" in lib.dff_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (idx == -7).all()          # a refused call writes nothing
    # index_dev may be NULL, and the call still works after the refusals
    assert lib.dff_rmsd_nearest(0, p(x), n, p(y), m, N, -1, p(out), None, p(ws), need, None) == 0
    r, i = b.rmsd_nearest(x, y)
    assert torch.equal(out, r) and (idx == -7).all()


# ---------------------------------------------------------------- 8. the evaluator against numpy on the Kabsch matrix
def np_stats(d, prefix, stats):
    f = d[~np.isnan(d)]
    return {f"{prefix}_rmsd_{s}": float(getattr(np, s)(f)) for s in stats}


def test_coverage_evaluator_vs_kabsch(dev, golden):
    from dff_amd import evaluate
    g = x_rmsd(golden("struct_ref_chignolin.npz")).astype(np.float32)
    bad = np.flatnonzero(~np.isfinite(g).all((1, 2)))
    assert len(bad) >= 1
    pick = np.setdiff1d(np.arange(0, 4096, 8), bad)
    samples = np.concatenate([g[pick[:255]], g[bad[:2]]])                     # 257 frames, two of them non-finite
    refs = np.concatenate([g[np.setdiff1d(np.arange(3, 4096, 20), bad)[:199]], g[bad[:1]]])   # 200, one non-finite
    thresholds = (1.0, 2.0, 4.0)
    ev = evaluate.EnsembleCoverageEvaluator(torch.from_numpy(refs), "chignolin", thresholds, device=dev)
    got = ev.eval(torch.from_numpy(samples))
    assert all(type(v) is float for v in got.values())

    D = kabsch_matrix(samples, refs)
    S = kabsch_matrix(samples, samples)
    np.fill_diagonal(S, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # all-NaN rows: the non-finite frames
        nov, cov, div = np.nanmin(D, 1), np.nanmin(D, 0), np.nanmin(S, 1)
    assert np.isnan(nov).sum() == 2 and np.isnan(cov).sum() == 1 and np.isnan(div).sum() == 2
    want = np_stats(nov, "novelty", ("mean", "median", "min"))
    want.update(np_stats(cov, "coverage", ("mean", "median", "max")))
    want.update(np_stats(div, "diversity", ("mean", "median")))
    for k, v in want.items():
        print(f"{k}: got {got[k]:.7f}, Kabsch {v:.7f}")
        assert abs(got[k] - v) <= RMSD_ATOL + RMSD_RTOL * v, k
    for d in (nov, cov, div):                   # no value sits within the bar of a threshold: the shares are exact
        f = d[~np.isnan(d)]
        assert all((np.abs(f - t) > 2 * (RMSD_ATOL + RMSD_RTOL * t)).all() for t in thresholds)
    for t in thresholds:
        assert got[f"precision@{t:g}"] == np.mean(nov[~np.isnan(nov)] <= t)
        assert got[f"recall@{t:g}"] == np.mean(cov[~np.isnan(cov)] <= t)
    assert got["duplicates@1"] == np.mean(div[~np.isnan(div)] < 1.0)
    assert got["samples_nonfinite"] == 2.0 and got["refs_nonfinite"] == 1.0
    assert set(got) == set(want) | {f"{p}@{t:g}" for p in ("precision", "recall") for t in thresholds} | {
        "duplicates@1", "samples_nonfinite", "refs_nonfinite"}
