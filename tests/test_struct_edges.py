"""Edges of the structure-metric kernels (dff_struct_*) that the golden frames never reach.

- the grid-stride loop (more tiles than workgroups) and ragged tails, with the float64 oracles of oracle/struct_metric.py
  vectorised over frames (held to the per-frame ones here);
- unaligned contiguous views (the scalar tile-load path), bit-equal to an aligned copy;
- the bead-count limits N = 4 and 64, and the rejection of N = 3 and 65;
- RMSD on elongated, planar, degenerate and far-off frames, where the two largest eigenvalues of Horn's key matrix
  nearly coincide;
- non-finite frames, contacts at exactly the cutoff, and dihedrals at exactly 0, pi and atan2(0, 0).
"""
import numpy as np
import pytest
import torch

from oracle.frames import axis_rot, integer_walks, needle, planar_walks, rand_rot
from oracle.struct_metric import (consecutive, contacts_batch, dihedral_ok, dihedrals64, kabsch64, kabsch64_batch, tic64_batch,
                                  tic_features64, tic_rows, torch_contacts, wrap_err)
from support import MIRROR, MOLS, RMSD_ATOL, B, assert_rmsd, dev, x_rmsd  # noqa: F401  (dev: fixture)


# ================================================================ CPU
@pytest.mark.parametrize("mol", MOLS + ["ala2"])
def test_kabsch64_batch_equals_per_frame(golden, mol):
    f = golden("struct_folded.npz")[mol].astype(np.float32)
    x = golden("struct_ref_ala2.npz")["x"] if mol == "ala2" else x_rmsd(golden(f"struct_ref_{mol}.npz"))
    ref = kabsch64(x, f)
    got = kabsch64_batch(x, f, chunk=777)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-12


def test_tic64_batch_equals_unchunked():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((1000, 13, 3)) * 5).astype(np.float32)
    F = (13 - 3) + 13 * 12 // 2
    mean, A = rng.standard_normal(F), rng.standard_normal((F, 3))
    np.testing.assert_allclose(tic64_batch(x, mean, A, chunk=97), (tic_features64(x) - mean) @ A, rtol=0, atol=1e-12)


# ================================================================ GPU
def all_metrics(xd, ref, mean, A, folded):
    """the four metrics of the frames xd (device) -> dict of host arrays"""
    b = B()
    counts, mism = b.struct_contacts(xd, 8.0, folded, 3)
    return {"rmsd": b.struct_rmsd(xd, ref).cpu().numpy(), "dihedrals": b.struct_dihedrals(xd).cpu().numpy(),
            "tic": b.struct_tic(xd, mean, A).cpu().numpy(), "counts": counts.cpu().numpy(),
            "mismatch": mism.cpu().numpy()}


def metric_inputs(rng, N, k=3):
    ref = (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    F = B().struct_tic_num_features(N)
    folded = torch_contacts((rng.standard_normal((1, N, 3)) * 6).astype(np.float32), 8.0)[0].to(torch.uint8)
    return ref, rng.standard_normal(F), rng.standard_normal((F, k)), folded


# ---------------------------------------------------------------- grid stride and ragged tails
@pytest.mark.gpu
def test_grid_stride_rmsd_dihedrals_tic(dev):
    """n = 786469 frames: 12289 tiles on a grid capped at 8192 workgroups, the last tile 37 frames long"""
    b = B()
    rng = np.random.default_rng(2024)
    n, N = 786469, 10
    x = (rng.standard_normal((n, N, 3)) * 5).astype(np.float32)
    ref, mean, A, _ = metric_inputs(rng, N)
    xd = torch.from_numpy(x).to(dev)
    rmsd = b.struct_rmsd(xd, ref).cpu().numpy()
    dih = b.struct_dihedrals(xd).cpu().numpy()
    tic = b.struct_tic(xd, mean, A).cpu().numpy()

    assert_rmsd(rmsd, kabsch64_batch(x, ref), "grid-stride rmsd")
    ok = dihedral_ok(x)
    assert ok.mean() > 0.9
    assert wrap_err(dih, dihedrals64(x, consecutive(N)))[ok].max() <= 2e-5
    ref_tic = tic64_batch(x, mean, A)
    rows = tic_rows(x)
    err = np.abs(tic - ref_tic)[rows]
    assert rows.mean() > 0.99 and err.max() <= 1e-4 * np.abs(ref_tic).max(), err.max()

    # one lane computes one frame: its value does not depend on the workgroup, tile or lane that handles it
    for sl in (slice(0, 64 * 1001 + 13), slice(n - 64 * 1001 - 29, n)):
        sub = xd[sl].clone()
        assert np.array_equal(b.struct_rmsd(sub, ref).cpu().numpy(), rmsd[sl], equal_nan=True)
        assert np.array_equal(b.struct_dihedrals(sub).cpu().numpy(), dih[sl], equal_nan=True)
        assert np.array_equal(b.struct_tic(sub, mean, A).cpu().numpy(), tic[sl], equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 35])
def test_grid_stride_contacts(dev, N):
    """n = 262181 frames: 4097 tiles on a grid capped at 2048 workgroups, whose LDS counters add up across tiles"""
    b = B()
    rng = np.random.default_rng(N + 100)
    n = 262181
    x = (rng.standard_normal((n, N, 3)) * 6).astype(np.float32)
    _, _, _, folded = metric_inputs(rng, N)
    xd = torch.from_numpy(x).to(dev)
    counts, mism = b.struct_contacts(xd, 8.0, folded, 3)
    counts, mism = counts.cpu().numpy(), mism.cpu().numpy()
    rc, rm = contacts_batch(x, 8.0, folded, 3)
    assert np.array_equal(counts, rc) and np.array_equal(mism, rm)
    # the counts add up exactly over a split of the frames, and the per-frame mismatches are those of the parts
    m = 64 * 1500 + 41
    c1, m1 = b.struct_contacts(xd[:m].clone(), 8.0, folded, 3)
    c2, m2 = b.struct_contacts(xd[m:].clone(), 8.0, folded, 3)
    assert np.array_equal((c1 + c2).cpu().numpy(), counts)
    assert np.array_equal(torch.cat([m1, m2]).cpu().numpy(), mism)


# ---------------------------------------------------------------- unaligned views: the scalar tile-load path
@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 13, 64])
def test_unaligned_views_bit_equal(dev, N):
    rng = np.random.default_rng(N)
    ref, mean, A, folded = metric_inputs(rng, N)
    for n in (1, 63, 129, 1000):
        flat = torch.from_numpy((rng.standard_normal(n * 3 * N + 4) * 5).astype(np.float32)).to(dev)
        for k in (1, 2, 3):
            v = flat[k:k + n * 3 * N].view(n, N, 3)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
            al = v.clone()
            assert al.data_ptr() % 16 == 0
            got, want = all_metrics(v, ref, mean, A, folded), all_metrics(al, ref, mean, A, folded)
            for key in want:
                assert np.array_equal(got[key], want[key], equal_nan=True), (n, k, key)


# ---------------------------------------------------------------- bead-count limits
@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 5, 63, 64])
def test_bead_count_limits(dev, N):
    rng = np.random.default_rng(1000 + N)
    n = 300
    x = (rng.standard_normal((n, N, 3)) * 6).astype(np.float32)
    ref, mean, A, folded = metric_inputs(rng, N, k=8)
    got = all_metrics(torch.from_numpy(x).to(dev), ref, mean, A, folded)
    assert_rmsd(got["rmsd"], kabsch64_batch(x, ref), f"N={N}")
    ok = dihedral_ok(x)
    assert ok.mean() > 0.9
    assert wrap_err(got["dihedrals"], dihedrals64(x, consecutive(N)))[ok].max() <= 2e-5
    rows = tic_rows(x)
    ref_tic = tic64_batch(x, mean, A)
    assert rows.mean() > 0.9
    np.testing.assert_allclose(got["tic"][rows], ref_tic[rows], rtol=0, atol=1e-4 * np.abs(ref_tic).max())
    rc, rm = contacts_batch(x, 8.0, folded, 3)
    assert np.array_equal(got["counts"], rc) and np.array_equal(got["mismatch"], rm)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [3, 65])
def test_bead_count_out_of_range_rejected(dev, N):
    b = B()
    x = torch.ones((70, N, 3), device=dev)
    F = b.struct_tic_num_features(N)
    with pytest.raises(ValueError, match="n_beads"):
        b.struct_rmsd(x, np.zeros((N, 3), np.float32))
    with pytest.raises(ValueError, match="n_beads"):
        b.struct_dihedrals(x)
    with pytest.raises(ValueError, match="n_beads"):
        b.struct_tic(x, np.zeros(F), np.zeros((F, 2)))
    with pytest.raises(ValueError, match="n_beads"):
        b.struct_contacts(x, 8.0, torch.zeros((N, N), dtype=torch.uint8), 3)
    torch.cuda.synchronize()
    assert torch.isfinite(b.struct_rmsd(torch.ones((2, 4, 3), device=dev), np.zeros((4, 3)))).all()


# ---------------------------------------------------------------- RMSD geometry family
def rmsd_family_check(ref, frames, what):
    ref = np.asarray(ref, np.float32)
    x = np.asarray(frames, np.float32)
    got = B().struct_rmsd(torch.from_numpy(x).to("cuda"), torch.from_numpy(ref)).cpu().numpy()
    want = kabsch64_batch(x, ref)
    assert_rmsd(got, want, what)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 5, 10, 35, 56, 64])
def test_rmsd_needles(dev, N):
    """extended chains: sigma2 + sigma3 of the correlation matrix is small, and the two largest eigenvalues of
    Horn's key matrix nearly coincide"""
    rng = np.random.default_rng(300 + N)
    widths = (0.0, 1e-3, 1e-2, 0.1, 0.5, 1.0)
    noises = (0.0, 1e-3, 1e-2, 0.1, 0.3, 1.0)
    compact = rng.standard_normal((N, 3)) * 5
    for w in widths:
        ref = needle(rng, N, w)
        frames = []
        for w2 in widths:
            for s in noises:
                a = (needle(rng, N, w2) + s * rng.standard_normal((N, 3))) @ rand_rot(rng).T
                frames += [a, a * MIRROR]
        frames += [ref, ref * MIRROR, ref @ rand_rot(rng).T]
        rmsd_family_check(ref, frames, f"N={N} needle reference, width {w}")
        # an elongated frame against a compact reference, and the other way round
        rmsd_family_check(compact, [f @ rand_rot(rng).T for f in frames], f"N={N} compact reference, width {w}")
        rmsd_family_check(ref, [compact @ rand_rot(rng).T, compact * MIRROR], f"N={N} compact frame, width {w}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 35, 64])
def test_rmsd_planar_and_symmetric_tops(dev, N):
    """planar structures (det S = 0: a mirror image is a proper rotation away) and references whose covariance
    has c2 = c3 or c1 = c2 = c3, against their own mirror images"""
    rng = np.random.default_rng(400 + N)
    for scale in (1.0, 0.1):
        plane = rng.standard_normal((N, 3)) * 5 * np.array([1.0, 1.0, 0.0])
        frames = [plane @ rand_rot(rng).T, plane * MIRROR, (plane * MIRROR) @ rand_rot(rng).T]
        frames += [(plane + scale * rng.standard_normal((N, 3))) @ rand_rot(rng).T for _ in range(4)]
        frames += [f * MIRROR for f in frames]
        got, _ = rmsd_family_check(plane, frames, f"N={N} planar")
        assert got[1] <= RMSD_ATOL
    y = rng.standard_normal((N, 3))
    y -= y.mean(0)
    w, V = np.linalg.eigh(y.T @ y)
    y = y @ V / np.sqrt(w)                         # covariance exactly I (in float64)
    for c in ((9.0, 4.0, 4.0), (4.0, 4.0, 9.0), (6.0, 6.0, 6.0), (30.0, 0.5, 0.5)):
        top = y * np.sqrt(np.array(c) * N)
        frames = [top * MIRROR, top * -1.0, (top * MIRROR) @ rand_rot(rng).T, top @ rand_rot(rng).T,
                  (top + 0.05 * rng.standard_normal((N, 3))) * MIRROR]
        rmsd_family_check(top, frames, f"N={N} symmetric top {c}")
        rmsd_family_check(top * MIRROR, frames, f"N={N} mirrored symmetric top {c}")


@pytest.mark.gpu
@pytest.mark.parametrize("mol", ["chignolin", "villin", "protein_g"])
def test_rmsd_half_turns_offsets_and_scales(dev, golden, mol):
    f = golden("struct_folded.npz")[mol].astype(np.float64)
    N = len(f)
    rng = np.random.default_rng(500 + N)
    frames = [f]
    for axis in range(3):
        for d in (0.0, 1e-7, -1e-7, 1e-6, -1e-6):
            R = axis_rot(axis, np.pi + d)
            frames += [f @ R.T, (f + 0.3 * rng.standard_normal((N, 3))) @ R.T, (f @ R.T) * MIRROR]
    for off in (1e2, 1e3, 1e4):
        o = off * np.array([1.0, -0.5, 0.25])
        frames += [f + o, f @ rand_rot(rng).T - o, (f + rng.standard_normal((N, 3))) @ rand_rot(rng).T + o]
    rmsd_family_check(f, frames, f"{mol} half turns, offsets")
    rmsd_family_check(f + 1e4, frames[:4], f"{mol} reference offset 1e4")
    # scaled structures.  Ga + Gb - 2 lambda cancels to rounding of the order of 1e-16 (Ga + Gb), in the kernel and in
    # the oracle alike: at 1e3 times protein size that alone is ~1e-4 A on a near-zero RMSD, so the frames at scale
    # 1e3 carry noise of their own size.  At 1e-3 every RMSD is within the absolute bar of exact.
    for scale, noises in ((1e-3, (0.0, 0.1, 1.0)), (1e3, (0.1, 1.0))):
        fs = f * scale
        frames = [(fs + scale * s * rng.standard_normal((N, 3))) @ rand_rot(rng).T for s in noises]
        frames += [g * MIRROR for g in frames]
        rmsd_family_check(fs, frames, f"{mol} scale {scale}")


@pytest.mark.gpu
def test_rmsd_coincident_and_self(dev, golden):
    rng = np.random.default_rng(600)
    for N in (4, 10, 56, 64):
        x = rng.standard_normal((70, N, 3)) * 5
        point = np.tile(np.array([[1.5, -2.0, 3.25]]), (N, 1))
        # an all-coincident reference (Gb = 0): the RMSD is the frame's radius of gyration
        got, want = rmsd_family_check(point, x, f"N={N} coincident reference")
        x32 = x.astype(np.float32).astype(np.float64)
        rg = np.sqrt(((x32 - x32.mean(1, keepdims=True)) ** 2).sum((1, 2)) / N)
        assert np.all(np.abs(want - rg) <= 1e-9 * rg)
        # an all-coincident frame, and the reference itself
        ref = rng.standard_normal((N, 3)) * 5
        got, _ = rmsd_family_check(ref, [point, ref, ref * MIRROR], f"N={N} coincident frame")
        assert got[1] <= RMSD_ATOL


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 64])
def test_rmsd_nonfinite_lanes(dev, N):
    """+-inf and NaN at single coordinates in the first and last lane of a tile: NaN there, every other lane exact"""
    rng = np.random.default_rng(700 + N)
    n = 130
    ref = (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    x = (rng.standard_normal((n, N, 3)) * 5).astype(np.float32)
    clean = B().struct_rmsd(torch.from_numpy(x).to(dev), torch.from_numpy(ref)).cpu().numpy()
    bad = {0: (0, 0, np.inf), 63: (N - 1, 2, -np.inf), 64: (N // 2, 1, np.nan), 127: (0, 2, np.nan),
           128: (N - 1, 0, np.inf)}
    for s, (bead, c, v) in bad.items():
        x[s, bead, c] = v
    got, want = rmsd_family_check(ref, x, f"N={N} non-finite")
    assert np.isnan(got[list(bad)]).all()
    keep = np.setdiff1d(np.arange(n), list(bad))
    assert np.array_equal(got[keep], clean[keep])


# ---------------------------------------------------------------- non-finite frames in the other metrics
@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 35])
def test_nonfinite_dihedrals_tic_contacts(dev, N):
    b = B()
    rng = np.random.default_rng(800 + N)
    n = 200
    x = (rng.standard_normal((n, N, 3)) * 6).astype(np.float32)
    _, mean, A, folded = metric_inputs(rng, N)
    clean_tic = b.struct_tic(torch.from_numpy(x).to(dev), mean, A).cpu().numpy()
    bad = [0, 1, 63, 64, 100, 127, 199]
    vals = [np.inf, -np.inf, np.nan]
    for i, s in enumerate(bad):
        x[s, rng.integers(N), rng.integers(3)] = vals[i % 3]
    x[100, :, :] = np.nan
    x[1, 0, :] = np.inf
    xd = torch.from_numpy(x).to(dev)

    dih = b.struct_dihedrals(xd).cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref = dihedrals64(x, consecutive(N))
    assert np.array_equal(np.isnan(dih), np.isnan(ref))
    assert np.isnan(ref).any()
    fin = np.isfinite(x).all(2)
    quad_ok = np.stack([fin[:, i:i + 4].all(1) for i in range(N - 3)], 1) & dihedral_ok(np.where(np.isfinite(x), x, 0))
    assert wrap_err(dih[quad_ok], ref[quad_ok]).max() <= 2e-5

    tic = b.struct_tic(xd, mean, A).cpu().numpy()
    assert not np.isfinite(tic[bad]).any()
    keep = np.setdiff1d(np.arange(n), bad)
    assert np.array_equal(tic[keep], clean_tic[keep])

    counts, mism = b.struct_contacts(xd, 8.0, folded, 3)
    rc, rm = contacts_batch(x, 8.0, folded, 3)
    assert np.array_equal(counts.cpu().numpy(), rc) and np.array_equal(mism.cpu().numpy(), rm)


# ---------------------------------------------------------------- contacts at the cutoff
@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 16, 64])
def test_contacts_exactly_at_cutoff(dev, N):
    b = B()
    rng = np.random.default_rng(900 + N)
    x = integer_walks(rng, 300, N)
    xd = torch.from_numpy(x).to(dev)
    folded = torch_contacts(x[:1], 7.0)[0].to(torch.uint8)
    for c in (5.0, 7.0, 9.0):
        below, above = np.nextafter(np.float32(c), np.float32(0)), np.nextafter(np.float32(c), np.float32(np.inf))
        assert torch_contacts(x, float(above)).sum() > torch_contacts(x, c).sum() == torch_contacts(x, float(below)).sum()
        for cut in (float(below), c, float(above)):
            counts, mism = b.struct_contacts(xd, cut, folded, 3)
            rc, rm = contacts_batch(x, cut, folded, 3)
            assert np.array_equal(counts.cpu().numpy(), rc) and np.array_equal(mism.cpu().numpy(), rm), cut


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 13, 64])
def test_contacts_cutoff_and_offset_edges(dev, N):
    b = B()
    rng = np.random.default_rng(950 + N)
    x = (rng.standard_normal((150, N, 3)) * 6).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    folded = torch_contacts((rng.standard_normal((1, N, 3)) * 6).astype(np.float32), 8.0)[0].to(torch.uint8)
    for cut in (0.0, -0.0, -1.0, -np.inf):
        counts, mism = b.struct_contacts(xd, cut, folded, 0)
        assert not counts.any()                  # not even the diagonal: d_ii = 0 is not < 0
        rc, rm = contacts_batch(x, cut, folded, 0)
        assert np.array_equal(mism.cpu().numpy(), rm)
    counts, mism = b.struct_contacts(xd, np.inf, folded, 0)
    rc, rm = contacts_batch(x, np.inf, folded, 0)
    assert np.array_equal(counts.cpu().numpy(), rc) and (rc == len(x)).all()
    assert np.array_equal(mism.cpu().numpy(), rm)
    for offset in (1, N - 1, N, N + 1, 1000):
        counts, mism = b.struct_contacts(xd, 8.0, folded, offset)
        rc, rm = contacts_batch(x, 8.0, folded, offset)
        assert np.array_equal(counts.cpu().numpy(), rc) and np.array_equal(mism.cpu().numpy(), rm), offset
        if offset >= N:
            assert not rm.any()


# ---------------------------------------------------------------- dihedral special values
@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 10, 64])
def test_dihedral_special_values(dev, N):
    b = B()
    rng = np.random.default_rng(1100 + N)
    x = planar_walks(rng, 200, N)
    got = b.struct_dihedrals(torch.from_numpy(x).to(dev)).cpu().numpy()
    ref = dihedrals64(x, consecutive(N))
    assert np.all(np.isclose(np.abs(ref), 0) | np.isclose(np.abs(ref), np.pi))
    assert (np.abs(ref) < 1).any() and (np.abs(ref) > 3).any()
    assert wrap_err(got, ref).max() <= 2e-5
    # collinear quadruples (c1 = c2 = 0): atan2(+-0, +0) = 0, on lines with either direction of travel
    d = rng.integers(-3, 4, size=(50, 1, 3)).astype(np.float64)
    d[np.all(d == 0, axis=-1)] = 1.0
    line = (np.arange(N)[None, :, None] * d + rng.integers(-10, 10, size=(50, 1, 3))).astype(np.float32)
    got = b.struct_dihedrals(torch.from_numpy(line).to(dev)).cpu().numpy()
    assert np.array_equal(dihedrals64(line, consecutive(N)), np.zeros((50, N - 3)))
    assert np.all(got == 0)
