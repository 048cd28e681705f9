"""Structure metrics of the reference's evaluators: RMSD, dihedrals, TIC projection, contacts.

CPU part: the restricted unpickler on the reference's own chignolin TICA pickle, and the host reductions of
evaluate.py fed the per-frame values of the reference-executed vectors (tests/golden/make_golden_struct.py).
GPU part (-m gpu): the HIP kernels dff_struct_* through the C ABI against the float64 oracles of oracle/struct_metric.py,
exact contact counts against torch's float32 formula, and the evaluators end to end against the reference's numbers.
"""
import io
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.struct_metric import consecutive, dihedrals64, kabsch64, tic_features64, torch_contacts, triu_mismatch
from support import MOLS, N_BEADS, dev, ev, x_rmsd  # noqa: F401  (dev: fixture)


def saved_refs(golden):
    return golden("struct_saved_refs.npz")


# ================================================================ CPU
def test_restricted_unpickler_reads_reference_tica(golden):
    s = saved_refs(golden)
    t = ev().load_tica_reference(os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))
    pre = "tica_chignolin_testset"
    for k in ("mean", "coeff", "singular_values", "gt_prob", "bin_edges_x", "bin_edges_y", "cov_00"):
        assert np.array_equal(t[k], s[f"{pre}_{k}"]), k
    assert t["mean"].shape == (52,) and t["coeff"].shape == (52, 2)


def test_tica_coefficients_whiten_c00(golden):
    """A^T C00 A = diag(s^2), A = sqrt_inv_cov[:, :2] (kinetic-map scaling); the instantaneous coefficients are
    sqrt_inv_cov itself."""
    s = saved_refs(golden)
    pre = "tica_chignolin_testset"
    t = ev().restricted_load(os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))[0]
    full = np.asarray(t._model._whitening_instantaneous.sqrt_inv_cov)
    assert np.array_equal(full, s[f"{pre}_instantaneous_coefficients"])
    A, C00, sv = s[f"{pre}_coeff"], s[f"{pre}_cov_00"], s[f"{pre}_singular_values"]
    np.testing.assert_allclose(A.T @ C00 @ A, np.diag(sv[:2] ** 2), rtol=0, atol=1e-12)


class _Boom:
    def __reduce__(self):
        return (os.system, ("echo should-not-run",))


@pytest.mark.parametrize("payload", [
    pickle.dumps(_Boom()),
    pickle.dumps(print),
    pickle.dumps(io.BytesIO),
    b"\x80\x04\x95\x1f\x00\x00\x00\x00\x00\x00\x00\x8c\x12deeptime.basis._xx\x94\x8c\x03Bar\x94\x93\x94.",
])
def test_restricted_unpickler_refuses_other_globals(payload):
    with pytest.raises(pickle.UnpicklingError):
        ev().RestrictedUnpickler(io.BytesIO(payload)).load()


def test_tica_npz_reference(golden, tmp_path):
    s = saved_refs(golden)
    pre = "tica_trp_cage_valset"
    p = tmp_path / "t.npz"
    np.savez(p, **{k: s[f"{pre}_{k}"] for k in ("mean", "coeff", "gt_prob", "bin_edges_x", "bin_edges_y")})
    t = ev().load_tica_reference(str(p))
    assert t["coeff"].shape == (207, 2) and np.array_equal(t["gt_prob"], s[f"{pre}_gt_prob"])


def test_dihedral_reductions_match_reference(golden):
    g = golden("struct_ref_ala2.npz")
    e = ev()
    probs = e.get_prob(g["torsions"], n_bins=61)
    assert np.array_equal(probs, g["probs"])
    got = e.dihedral_scores(probs, saved_refs(golden)["dih_probs_ala2_testset"])
    for a, k in zip(got, ("dih_mse", "dih_js", "dih_kl_1", "dih_kl_2")):
        assert a == float(g[k]), k


@pytest.mark.parametrize("mol", ["chignolin", "trp_cage"])
def test_tic_js_reduction_matches_reference(golden, mol):
    g, s = golden(f"struct_ref_{mol}.npz"), saved_refs(golden)
    pre = f"tica_{mol}_testset"
    js, _ = ev().tic_js(g["tic_proj"], s[f"{pre}_gt_prob"], s[f"{pre}_bin_edges_x"], s[f"{pre}_bin_edges_y"])
    assert js == float(g["tic_js"])


@pytest.mark.parametrize("mol", MOLS)
def test_rmsd_curve_matches_reference(golden, mol):
    g = golden(f"struct_ref_{mol}.npz")
    e = ev()
    c = e.rmsd_curve(g["rmsd"], 100, float(g["rmsd_cutoff"]))
    assert np.array_equal(c["bin_mids"], g["rmsd_bin_mids"])
    assert np.array_equal(c["energies"], g["rmsd_energies"], equal_nan=True)
    c = e.rmsd_curve(g["rmsd"], 50, None)
    assert np.array_equal(c["bin_mids"], g["rmsd_auto_bin_mids"])
    assert np.array_equal(c["energies"], g["rmsd_auto_energies"], equal_nan=True)
    assert np.isnan(g["rmsd"][np.unique(g["nonfinite_at"][:, 0])]).all()


@pytest.mark.parametrize("mol", MOLS)
def test_contact_bce_matches_reference(golden, mol):
    g = golden(f"struct_ref_{mol}.npz")
    N = N_BEADS[mol]
    folded = torch.from_numpy(g["folded"]).float()
    assert np.array_equal((torch.norm(folded[:, None] - folded[None], dim=-1) < 10).numpy(), g["contacts_folded"])
    c = torch_contacts(g["x"], 10)
    assert np.array_equal(c.sum(0).numpy(), g["contact_counts"])
    mism = triu_mismatch(c, g["contacts_folded"], 3)
    bce, mean = ev().contact_bce_from_mismatch(mism, (N - 3) * (N - 2) // 2)
    ref = g["bce"].astype(np.float32)
    assert np.all(np.abs(bce.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)) <= 1)
    assert abs(float(mean) - float(g["bce_mean"])) <= 1e-6 * abs(float(g["bce_mean"]))


def test_folded_fixture_shapes(golden):
    f = golden("struct_folded.npz")
    for m in MOLS:
        assert f[m].shape == (N_BEADS[m], 3)
        assert np.isfinite(float(f[f"{m}_rmsd_to_cg"]))
    assert f["ala2"].shape == (5, 3)


def test_saved_rmsd_reference_loads(golden, tmp_path):
    """RmsdEvaluator's "Reference" curve comes from the saved pickle through the restricted unpickler."""
    s = saved_refs(golden)
    d = {"bin_mids": s["rmsd_villin_bin_mids"], "energies": s["rmsd_villin_energies"]}
    p = tmp_path / "saved_rmsd_VILLIN_reference_total.pickle"
    p.write_bytes(pickle.dumps(d))
    got = ev().restricted_load(str(p))
    assert np.array_equal(got["energies"], d["energies"], equal_nan=True)


# ================================================================ GPU
def cases(golden):
    out = {m: golden(f"struct_ref_{m}.npz") for m in MOLS}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mol", MOLS + ["ala2"])
def test_rmsd_vs_kabsch(dev, golden, mol):
    from dff_amd import binding
    f = golden("struct_folded.npz")[mol]
    if mol == "ala2":
        x = golden("struct_ref_ala2.npz")["x"]
    else:
        x = x_rmsd(golden(f"struct_ref_{mol}.npz"))
    got = binding.struct_rmsd(torch.from_numpy(x).to(dev), torch.from_numpy(f).float()).cpu().numpy()
    ref = kabsch64(x, f.astype(np.float32))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-5 + 1e-6 * ref[ok]), np.abs(got[ok] - ref[ok]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("mol", MOLS)
def test_rmsd_rigid_copy_and_mirror(dev, golden, mol):
    from dff_amd import binding
    f = golden("struct_folded.npz")[mol].astype(np.float32)
    rng = np.random.default_rng(7)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    rigid = (f @ q.T + np.array([12.5, -3.0, 40.0])).astype(np.float32)
    mirror = (f * np.array([-1.0, 1.0, 1.0])).astype(np.float32)
    x = np.stack([rigid, mirror, f])
    got = binding.struct_rmsd(torch.from_numpy(x).to(dev), torch.from_numpy(f)).cpu().numpy()
    assert got[0] <= 1e-5 and got[2] <= 1e-5
    ref_m = kabsch64(mirror[None], f)[0]
    assert ref_m > 0.1 and abs(got[1] - ref_m) <= 1e-5 + 1e-6 * ref_m


@pytest.mark.gpu
@pytest.mark.parametrize("mol", MOLS + ["ala2"])
def test_dihedrals_vs_float64(dev, golden, mol):
    from dff_amd import binding
    x = golden(f"struct_ref_{mol}.npz")["x"]
    N = x.shape[1]
    got = binding.struct_dihedrals(torch.from_numpy(x).to(dev)).cpu().numpy().astype(np.float64)
    ref = dihedrals64(x, consecutive(N))
    # non-degenerate quadruples: neither bond angle within ~6 degrees of 0 or 180
    xd = x.astype(np.float64)
    b = np.diff(xd, axis=1)
    sin = np.linalg.norm(np.cross(b[:, :-1], b[:, 1:]), axis=-1) / (
        np.linalg.norm(b[:, :-1], axis=-1) * np.linalg.norm(b[:, 1:], axis=-1))
    good = (sin[:, :-1] > 0.1) & (sin[:, 1:] > 0.1)
    err = np.abs(np.angle(np.exp(1j * (got - ref))))
    assert good.mean() > 0.9 and err[good].max() <= 2e-5, err[good].max()
    if mol == "ala2":
        e = ev()
        edges = np.linspace(-np.pi, np.pi, 61)
        near = (np.abs(ref[:, :, None] - edges[None, None]) < 1e-4).any(-1).any(-1)
        pg = e.get_prob(got[~near], 61)
        pr = e.get_prob(ref[~near], 61)
        hg = np.histogram2d(got[~near, 0], got[~near, 1], bins=edges)[0]
        hr = np.histogram2d(ref[~near, 0], ref[~near, 1], bins=edges)[0]
        assert np.array_equal(hg, hr) and np.array_equal(pg, pr)


@pytest.mark.gpu
@pytest.mark.parametrize("mol", ["chignolin", "trp_cage"])
def test_tic_projection_vs_float64(dev, golden, mol):
    from dff_amd import binding
    g, s = golden(f"struct_ref_{mol}.npz"), saved_refs(golden)
    pre = f"tica_{mol}_testset"
    mean, A = s[f"{pre}_mean"], s[f"{pre}_coeff"]
    x = g["x"]
    got = binding.struct_tic(torch.from_numpy(x).to(dev), mean, A).cpu().numpy()
    ref = (tic_features64(x) - mean) @ A
    rng_ = ref.max(0) - ref.min(0)
    assert np.all(np.abs(got - ref) <= 1e-5 * rng_), (np.abs(got - ref) / rng_).max()
    js, _ = ev().tic_js(got, s[f"{pre}_gt_prob"], s[f"{pre}_bin_edges_x"], s[f"{pre}_bin_edges_y"])
    assert abs(js - float(g["tic_js"])) <= 1e-4


@pytest.mark.gpu
def test_tic_more_components(dev):
    """k = 1..8 components of an arbitrary projection, N at the limits."""
    from dff_amd import binding
    rng = np.random.default_rng(3)
    for N, k in ((4, 1), (13, 3), (64, 8)):
        x = rng.standard_normal((130, N, 3)).astype(np.float32) * 5
        F = binding.struct_tic_num_features(N)
        mean, A = rng.standard_normal(F), rng.standard_normal((F, k))
        got = binding.struct_tic(torch.from_numpy(x).to(dev), mean, A).cpu().numpy()
        ref = (tic_features64(x) - mean) @ A
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 10, 35, 56, 61])
def test_contacts_exact(dev, N):
    from dff_amd import binding
    rng = np.random.default_rng(N)
    for n in (0, 1, 63, 64, 65, 1000):
        x = (rng.standard_normal((n, N, 3)) * 6).astype(np.float32)
        folded = torch_contacts((rng.standard_normal((1, N, 3)) * 6).astype(np.float32), 8.0)[0]
        for offset in (3, 0):
            counts, mism = binding.struct_contacts(torch.from_numpy(x).to(dev), 8.0, folded.to(torch.uint8), offset)
            c = torch_contacts(x, 8.0)
            assert np.array_equal(counts.cpu().numpy(), c.sum(0).numpy()), (n, offset)
            assert np.array_equal(mism.cpu().numpy(), triu_mismatch(c, folded, offset)), (n, offset)
        counts, mism = binding.struct_contacts(torch.from_numpy(x).to(dev), 8.0)
        assert mism is None and np.array_equal(counts.cpu().numpy(), torch_contacts(x, 8.0).sum(0).numpy())


@pytest.mark.gpu
def test_entry_points_reject_bad_arguments(dev):
    from dff_amd import binding
    x = torch.zeros((4, 3, 3), device=dev)
    with pytest.raises(ValueError):
        binding.struct_dihedrals(x)                 # n_beads < 4
    with pytest.raises(ValueError):
        binding.struct_tic(torch.zeros((4, 5, 3), device=dev), np.zeros(12), np.zeros((12, 9)))   # k > 8


@pytest.mark.gpu
@pytest.mark.parametrize("mol", MOLS)
def test_rmsd_and_contact_evaluators_end_to_end(dev, golden, mol):
    e = ev()
    g = golden(f"struct_ref_{mol}.npz")
    re = e.RmsdEvaluator(mol, g["folded"], "", saved_ref_dir=str(GOLDEN))
    xr = torch.from_numpy(x_rmsd(g))
    re.eval("Samples", xr, 100, float(g["rmsd_cutoff"]), save_dynamics=True)
    got = re.plot_dict["Samples"]
    ref = g["rmsd"]
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got["rmsd"]), ~ok)
    assert np.all(np.abs(got["rmsd"][ok] - ref[ok]) <= 1e-5 + 1e-6 * ref[ok])
    # the curve is the reference's, up to frames within the RMSD tolerance of a bin edge (which may change bins)
    edges = np.linspace(0, float(g["rmsd_cutoff"]), 101)
    near = np.zeros(len(ref), bool)
    near[ok] = (np.abs(ref[ok][:, None] - edges[None]) <= 1e-5 + 1e-6 * ref[ok][:, None]).any(-1)
    assert near.sum() <= 3
    mixed = ref.copy()
    mixed[near] = got["rmsd"][near]
    expect = e.rmsd_curve(mixed, 100, float(g["rmsd_cutoff"]))["energies"]
    assert np.array_equal(got["energies"], expect, equal_nan=True)
    if not near.any():
        assert np.array_equal(got["energies"], g["rmsd_energies"], equal_nan=True)
    ce = e.ContactEvaluator(mol, g["folded"], "", contact_cutoff=10)
    assert np.array_equal(ce.contacts_folded.numpy(), g["contacts_folded"])
    ncc = ce.normalized_contact_count(torch.from_numpy(g["x"]))
    assert torch.equal(ncc, torch.from_numpy(g["contact_counts"]) / len(g["x"]))
    bce, mean = ce.contact_bce(torch.from_numpy(g["x"]))
    d = np.abs(bce.view(np.int32).astype(np.int64) - g["bce"].astype(np.float32).view(np.int32).astype(np.int64))
    assert d.max() <= 1 and abs(float(mean) - float(g["bce_mean"])) <= 1e-6 * abs(float(g["bce_mean"]))


def _tica_npz(s, mol, path):
    pre = f"tica_{mol}_testset"
    np.savez(path, **{k: s[f"{pre}_{k}"] for k in ("mean", "coeff", "gt_prob", "bin_edges_x", "bin_edges_y")})


@pytest.mark.gpu
def test_evaluator_end_to_end(dev, golden, tmp_path):
    e = ev()
    s = saved_refs(golden)
    # alanine: Dihedral JS from the saved probabilities (the reference's pickle format)
    (tmp_path / "saved_dih_probs_ala2_testset.pickle").write_bytes(pickle.dumps(s["dih_probs_ala2_testset"]))
    ga = golden("struct_ref_ala2.npz")
    xa = torch.from_numpy(ga["x"])
    res = e.Evaluator(xa[:2000], None, "alanine_dipeptide", saved_ref_dir=str(tmp_path)).eval(xa, 0)
    assert set(res) == {"Dihedral JS", "PWD JS"}
    assert abs(res["Dihedral JS"] - float(ga["dih_js"])) <= 1e-4
    # chignolin: TIC JS from the saved model (.npz and the reference's own pickle), PWD JS from ref_data
    g = golden("struct_ref_chignolin.npz")
    _tica_npz(s, "chignolin", tmp_path / "saved_TICA_CHIGNOLIN_testset.npz")
    x = torch.from_numpy(g["x"])
    res = e.Evaluator(x[:1000], None, "chignolin", eval_folder=str(tmp_path), saved_ref_dir=str(tmp_path)).eval(x, 3)
    assert set(res) == {"TIC JS", "PWD JS"} and abs(res["TIC JS"] - float(g["tic_js"])) <= 1e-4
    assert os.path.exists(tmp_path / "results-3.json")
    tp = e.TicEvaluator(None, "chignolin", saved_ref=os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))
    assert abs(tp.eval(x)[0] - float(g["tic_js"])) <= 1e-4
    # protein G: no TIC, no PWD; BBA without a saved TICA: a clear error
    assert e.Evaluator(None, None, "protein_g", saved_ref_dir=str(tmp_path)).eval(x, 0) == {}
    with pytest.raises(NotImplementedError):
        e.Evaluator(x, None, "bba", saved_ref_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        tp.eval(x, plot_tic=True)


@pytest.mark.gpu
def test_metrics_on_ddpm_samples(dev, golden, tmp_path):
    """Frames drawn by the DDPM sampler from the synthetic chignolin weights give finite metrics."""
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.score import GraphTransformer
    from oracle import synth
    e = ev()
    _, N, H, L = synth.SHIPPED_CONFIGS["chignolin"]
    model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                             use_distances=False, conservative=True,
                             state_dict=synth.synth_gnn_params(N, H, L, decoder_scale=1e-2))
    diff = GaussianDiffusion(model, num_atoms=N, timesteps=1000, norm_factor=3.113133430480957)
    diff.seed(1)
    x = diff.sample(256).contiguous()
    s = saved_refs(golden)
    _tica_npz(s, "chignolin", tmp_path / "saved_TICA_CHIGNOLIN_testset.npz")
    tic = e.TicEvaluator(None, "chignolin", saved_ref=str(tmp_path / "saved_TICA_CHIGNOLIN_testset.npz"))
    assert np.isfinite(tic.transform(x)).all()
    from dff_amd import binding
    assert torch.isfinite(binding.struct_dihedrals(x)).all()
    f = golden("struct_folded.npz")["chignolin"]
    re = e.RmsdEvaluator("chignolin", f)
    assert np.isfinite(re.rmsd(x)).all()
    bce, mean = e.ContactEvaluator("chignolin", f).contact_bce(x)
    assert np.isfinite(bce).all() and np.isfinite(float(mean))
