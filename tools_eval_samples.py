#!/usr/bin/env python3
"""Score a sample file the way the reference's Evaluator does (evaluate/evaluators.py:28-111): reads the
sample-{mode}.pt that sample.py writes ((n, N, 3) Angstrom) and a saved-references directory (the reference's
evaluate/saved_references, or .npz TICA models), and prints Evaluator.eval() as one JSON line.  Optional extras:
the RMSD free-energy curve and the contact BCE to the folded structure of a folded PDB.

    python tools_eval_samples.py SAMPLES.pt MOL SAVED_REF_DIR [--ref-data VAL.pt] [--folded-pdb PDB]
                                 [--tica-fit-data TRAJ.pt [--lagtime 100]]

Without a saved TICA reference for MOL, --tica-fit-data fits one on the GPU (a (n, N, 3) trajectory in Angstrom, or a
list of them, in time order) and writes it to SAVED_REF_DIR as saved_TICA_{MOL}_{evalset}.npz; --ref-data is then the
validation data it is histogrammed on.
"""
import argparse
import json

import numpy as np
import torch

import dff_amd  # noqa: F401
from dff_amd import evaluate


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("samples", help="sample-{mode}.pt written by sample.py")
    ap.add_argument("mol", help="molecule name as sample.py's --mol (alanine_dipeptide_*, chignolin, ...)")
    ap.add_argument("saved_ref_dir", help="directory of saved references")
    ap.add_argument("--ref-data", default=None, help="reference structures (.pt, (n, N, 3) Angstrom) where no saved "
                                                     "reference exists (PWD at offset 0)")
    ap.add_argument("--evalset", default="testset")
    ap.add_argument("--folded-pdb", default=None, help="folded PDB: also report the RMSD curve and the contact BCE")
    ap.add_argument("--tica-fit-data", default=None, help="time-ordered trajectories (.pt: (n, N, 3) Angstrom or a list "
                                                          "of them) to fit a TICA model on where none is saved")
    ap.add_argument("--lagtime", type=int, default=100, help="TICA lag time in frames (with --tica-fit-data)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    x = torch.load(a.samples, map_location="cpu").float().contiguous()
    ref = torch.load(a.ref_data, map_location="cpu").float() if a.ref_data else None
    fit = torch.load(a.tica_fit_data, map_location="cpu") if a.tica_fit_data else None
    if isinstance(fit, torch.Tensor):
        fit = fit.float()
    elif fit is not None:
        fit = [torch.as_tensor(t).float() for t in fit]
    res = evaluate.Evaluator(ref, None, a.mol, evalsetname=a.evalset, saved_ref_dir=a.saved_ref_dir,
                             tica_fit_data=fit, tica_lagtime=a.lagtime, device=a.device).eval(x, 0)
    if a.folded_pdb:
        mol = a.mol.lower()
        re = evaluate.RmsdEvaluator(mol, a.folded_pdb, saved_ref_dir=a.saved_ref_dir, device=a.device)
        rmsd = re.rmsd(x)
        res["RMSD mean"] = float(np.nanmean(rmsd))
        curve = evaluate.rmsd_curve(rmsd, evaluate.RMSD_NBINS_REF, evaluate.RMSD_CUTOFF_REF.get(mol))
        res["RMSD curve"] = {"bin_mids": curve["bin_mids"].tolist(),
                             "energies": [None if not np.isfinite(v) else float(v) for v in curve["energies"]]}
        _, mean = evaluate.ContactEvaluator(mol, a.folded_pdb, device=a.device).contact_bce(x)
        res["Contact BCE"] = float(mean)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
