#!/usr/bin/env python3
"""Generate the golden vectors of the structure metrics (RMSD, dihedrals, TIC, contacts) by running the REFERENCE.

Run once, from any directory, with a checkout of the reference project (the tests never read it):

    python tests/golden/make_golden_struct.py REFERENCE_ROOT

Writes DATA only:
  struct_folded.npz        folded C-alpha coordinates (Angstrom) of chignolin, trp-cage, BBA, villin, protein G
                           ({protid}.pdb by process_pdb's rule) and the 5 beads of ala2_cg.pdb, with the superposed RMSD
                           of each to the reference's coarse-grained {protid}-0-c-alpha.pdb (a different frame)
  struct_saved_refs.npz    the reference's saved references as arrays: TICA mean / sqrt_inv_cov[:, :2] / singular
                           values / gt_prob / bin edges for chignolin and trp-cage (test and val sets), chignolin's
                           C00, the ala2 phi / psi probabilities, the five RMSD free-energy curves
  saved_TICA_CHIGNOLIN_testset.pickle   the reference's pickle itself (for the restricted unpickler's test)
  struct_ref_<mol>.npz     seeded synthetic frames (rotated, translated, perturbed folded structures at several noise
                           scales; for RMSD also with non-finite entries at nonfinite_at) and what the reference's evaluators.py computes on them:
                           DihedralEnergiesEvaluator.eval, TicEvaluator.eval, RmsdEvaluator.eval, the
                           _get_samp_contacts sum and the per-frame BCE of _eval_bce_dynamics

evaluators.py is imported with mdtraj, deeptime and its dataset module stubbed.  Only mdtraj's two primitives are
transcribed, in float64 numpy: compute_dihedrals (b1 = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3,
c2 = b1 x b2, atan2((b1 . c1) |b2|, c1 . c2)) and rmsd (both structures centred on their mean; Kabsch with the
reflection correction = the minimum over proper rotations, the same value QCP gives).  The stub TICA projects with
the pickled arrays: (f - mean) @ sqrt_inv_cov[:, :dim].  Everything else -- feature order, histograms, divergences,
BCE -- is the reference's own code.
"""
import enum
import os
import shutil
import sys
import types

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else sys.exit("usage: make_golden_struct.py REFERENCE_ROOT")
OUT = os.path.dirname(os.path.abspath(__file__))
PDBS = os.path.join(REF, "datasets", "folded_pdbs")
SAVED = os.path.join(REF, "evaluate", "saved_references")
MOLS = {"chignolin": "CLN025", "trp_cage": "2JOF", "bba": "1FME", "villin": "2F4K", "protein_g": "NuG2"}


# ---- mdtraj's two primitives, float64 numpy ----
def dihedrals64(xyz, ind):
    x = np.asarray(xyz, np.float64)
    ind = np.asarray(ind)
    b1 = x[:, ind[:, 1]] - x[:, ind[:, 0]]
    b2 = x[:, ind[:, 2]] - x[:, ind[:, 1]]
    b3 = x[:, ind[:, 3]] - x[:, ind[:, 2]]
    c1 = np.cross(b2, b3)
    c2 = np.cross(b1, b2)
    p1 = (b1 * c1).sum(-1) * np.sqrt((b2 * b2).sum(-1))
    p2 = (c1 * c2).sum(-1)
    return np.arctan2(p1, p2)


def kabsch_rmsd64(xyz, ref):
    """min over proper rotations R of sqrt(mean |R (x - mean x) - (r - mean r)|^2), per frame"""
    x = np.asarray(xyz, np.float64)
    r = np.asarray(ref, np.float64)
    x = x - x.mean(1, keepdims=True)
    r = r - r.mean(0)
    out = np.empty(len(x))
    for s, a in enumerate(x):
        H = a.T @ r
        U, S, Vt = np.linalg.svd(H)
        d = np.sign(np.linalg.det(U @ Vt))
        S[-1] *= d
        msd = ((a * a).sum() + (r * r).sum() - 2.0 * S.sum()) / len(a)
        out[s] = np.sqrt(max(msd, 0.0))
    return out


class Trajectory:
    def __init__(self, xyz, topology=None):
        self.xyz = np.asarray(xyz)
        self.topology = topology


class Folded:
    def __init__(self, ca_angstrom):
        self.xyz = (np.asarray(ca_angstrom, np.float32) / np.float32(10))[None]
        self.topology = None


md = types.ModuleType("mdtraj")
md.Trajectory = Trajectory
md.compute_dihedrals = lambda traj, ind: dihedrals64(traj.xyz, ind)
md.rmsd = lambda traj, ref: kabsch_rmsd64(traj.xyz, ref.xyz[0])


class _Inert:
    def __new__(cls, *a, **k):
        return object.__new__(cls)

    def __setstate__(self, state):
        self.__dict__.update(state)


class TICA(_Inert):
    """array projection with the pickled whitening: (f - mean) @ sqrt_inv_cov[:, :dim]"""

    def transform(self, f):
        w = self._model._whitening_instantaneous
        return (np.asarray(f) - w.mean) @ w.sqrt_inv_cov[:, :self._dim]

    __call__ = transform


def stub_module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


sys.modules["mdtraj"] = md
stub_module("deeptime")
stub_module("deeptime.decomposition", TICA=TICA)
stub_module("deeptime.decomposition._tica", TICA=TICA)
stub_module("deeptime.decomposition._koopman", CovarianceKoopmanModel=type("CovarianceKoopmanModel", (_Inert,), {}))
stub_module("deeptime.covariance")
stub_module("deeptime.covariance._covariance", WhiteningTransform=type("WhiteningTransform", (_Inert,), {}),
            CovarianceModel=type("CovarianceModel", (_Inert,), {}))
stub_module("deeptime.basis")
stub_module("deeptime.basis._base", Concatenation=type("Concatenation", (_Inert,), {}))
stub_module("deeptime.basis._monomials", Identity=type("Identity", (_Inert,), {}))
stub_module("datasets")
stub_module("datasets.dataset_utils_empty", get_dataset=None,
            Molecules=enum.Enum("Molecules", {k.upper(): v for k, v in MOLS.items()}))
import matplotlib  # noqa: E402

matplotlib.use("Agg")
if not hasattr(np, "NaN"):
    np.NaN = np.nan            # the reference's mse (evaluators_CGflowmatching.py:24) was written for numpy 1.x
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
import evaluate.evaluators as ev  # noqa: E402  (reference)

from dff_amd.evaluate import folded_ca  # noqa: E402

FOLDED = {m: folded_ca(os.path.join(PDBS, f"{p}.pdb"), m) for m, p in MOLS.items()}
ev.process_pdb = lambda path, mol_name: Folded(FOLDED[mol_name.lower()])


def cg_ca(path):
    return np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in open(path)
                     if l.startswith(("ATOM", "HETATM"))], np.float64)


def rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], 1)


def perturbed(folded, n, seed, scales=(0.1, 0.5, 1.0, 2.0, 4.0)):
    rng = np.random.default_rng(seed)
    c = folded - folded.mean(0)
    sig = np.asarray(scales)[np.arange(n) % len(scales)]
    x = c[None] + sig[:, None, None] * rng.standard_normal((n,) + c.shape)
    x = np.einsum("sij,snj->sni", rotations(rng, n), x) + rng.uniform(-20, 20, (n, 1, 3))
    return x.astype(np.float32)


def main():
    os.chdir(os.path.join(REF, "evaluate"))      # the reference's default saved_references/ paths are relative
    folded = {}
    for m, p in MOLS.items():
        cg = cg_ca(os.path.join(PDBS, f"{p}-0-c-alpha.pdb"))
        assert len(cg) == len(FOLDED[m]), (m, len(cg), len(FOLDED[m]))
        folded[m] = FOLDED[m]
        folded[f"{m}_rmsd_to_cg"] = kabsch_rmsd64(FOLDED[m][None], cg)[0]
        print(f"  {m}: {len(cg)} C-alphas, RMSD to {p}-0-c-alpha.pdb {folded[f'{m}_rmsd_to_cg']:.4f} A")
    ala = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in open(os.path.join(PDBS, "ala2_cg.pdb"))
                    if l.startswith("ATOM")], np.float64)
    folded["ala2"] = ala
    np.savez_compressed(os.path.join(OUT, "struct_folded.npz"), **folded)

    saved = {}
    for m in ("CHIGNOLIN", "TRP_CAGE"):
        for es in ("testset", "valset"):
            tica, gt, ex, ey = ev.pickle.load(open(os.path.join(SAVED, f"saved_TICA_{m}_{es}.pickle"), "rb"))
            w = tica._model._whitening_instantaneous
            t = f"tica_{m.lower()}_{es}"
            saved[f"{t}_mean"] = w.mean
            saved[f"{t}_coeff"] = w.sqrt_inv_cov[:, :2]
            saved[f"{t}_singular_values"] = tica._model._singular_values
            saved[f"{t}_gt_prob"], saved[f"{t}_bin_edges_x"], saved[f"{t}_bin_edges_y"] = gt, ex, ey
            if m == "CHIGNOLIN" and es == "testset":
                saved[f"{t}_cov_00"] = tica._model._cov._cov_00
                saved[f"{t}_instantaneous_coefficients"] = tica._model._instantaneous_coefficients
    saved["dih_probs_ala2_testset"] = ev.pickle.load(open(os.path.join(SAVED, "saved_dih_probs_ala2_testset.pickle"), "rb"))
    for m in MOLS:
        d = ev.pickle.load(open(os.path.join(SAVED, f"saved_rmsd_{m.upper()}_reference_total.pickle"), "rb"))
        saved[f"rmsd_{m}_bin_mids"], saved[f"rmsd_{m}_energies"] = d["bin_mids"], d["energies"]
    np.savez_compressed(os.path.join(OUT, "struct_saved_refs.npz"), **saved)
    shutil.copyfile(os.path.join(SAVED, "saved_TICA_CHIGNOLIN_testset.pickle"),
                    os.path.join(OUT, "saved_TICA_CHIGNOLIN_testset.pickle"))

    captured = {}
    ev.plt.plot = lambda y, *a, **k: captured.__setitem__("y", np.asarray(y))   # _eval_bce_dynamics plots bce[start:stop]
    ev.plt.savefig = lambda *a, **k: None
    ev.TicEvaluator._plot_tic = lambda self, *a, **k: None     # eval's return needs `fig` bound (evaluators.py:488)

    # alanine dipeptide: Dihedral JS against the saved probabilities
    x = perturbed(ala, 4000, 11, scales=(0.05, 0.2, 0.4, 0.8))
    e = ev.DihedralEnergiesEvaluator(None, None, saved_ref=os.path.join(SAVED, "saved_dih_probs_ala2_testset.pickle"))
    res = e.eval(torch.from_numpy(x))
    tors = dihedrals64(x, [[0, 1, 2, 3], [1, 2, 3, 4]])
    np.savez_compressed(os.path.join(OUT, "struct_ref_ala2.npz"), x=x, torsions=tors,
                        probs=ev.get_prob(tors, n_bins=61), dih_mse=res[0], dih_js=res[1], dih_kl_1=res[2],
                        dih_kl_2=res[3])
    print(f"  ala2: Dihedral JS {res[1]:.6f}")

    for i, m in enumerate(MOLS):
        f = FOLDED[m]
        N = len(f)
        x = perturbed(f, {"chignolin": 4096, "trp_cage": 2048}.get(m, 1024), 100 + i)
        out = {"x": x, "folded": f}
        if m in ("chignolin", "trp_cage"):
            te = ev.TicEvaluator(None, m, eval_folder="", data_folder="", folded_pdb_folder=PDBS,
                                 saved_ref=os.path.join(SAVED, f"saved_TICA_{m.upper()}_testset.pickle"))
            feats = te.get_tic_features(torch.from_numpy(x), te.folded)
            out["tic_proj"] = te.tica(feats)
            out["tic_js"] = te.eval(torch.from_numpy(x), "golden", plot_tic=True)[0]
            print(f"  {m}: TIC JS {out['tic_js']:.6f}")
        # RMSD: NaN / inf frames as the reference's valid_mask sees them
        xr = x.copy()
        bad = np.array([[5, 3, 1], [17, 0, 0], [40, N - 1, 2]])
        bad_val = np.array([np.nan, np.inf, -np.inf], np.float32)
        xr[tuple(bad.T)] = bad_val
        out["nonfinite_at"], out["nonfinite_val"] = bad, bad_val      # x_rmsd = x with these entries
        re = ev.RmsdEvaluator(m, "", "")
        cut = re.cutoff_dict_ref[m]
        re.eval("Samples", torch.from_numpy(xr), 100, cut, save_dynamics=True)
        out["rmsd"] = re.plot_dict["Samples"]["rmsd"]
        out["rmsd_bin_mids"], out["rmsd_energies"] = re.plot_dict["Samples"]["bin_mids"], re.plot_dict["Samples"]["energies"]
        out["rmsd_cutoff"] = cut
        re.eval("Auto", torch.from_numpy(xr), 50, None)
        out["rmsd_auto_bin_mids"], out["rmsd_auto_energies"] = re.plot_dict["Auto"]["bin_mids"], re.plot_dict["Auto"]["energies"]
        # contacts: counts over frames and the per-frame BCE (offset 3)
        ce = ev.ContactEvaluator(m, "", "", contact_cutoff=10)
        out["contacts_folded"] = ce.contacts_folded.numpy()
        out["contact_counts"] = ce._get_samp_contacts(torch.from_numpy(x)).sum(0).numpy()
        out["bce_mean"] = ce._eval_bce_dynamics(torch.from_numpy(x), "golden", 0, len(x), 1.0, save=False).numpy()
        out["bce"] = captured.pop("y")
        np.savez_compressed(os.path.join(OUT, f"struct_ref_{m}.npz"), **out)
        print(f"  {m}: {N} beads, mean RMSD {np.nanmean(out['rmsd']):.3f} A, mean BCE {float(out['bce_mean']):.3f}")


if __name__ == "__main__":
    main()
