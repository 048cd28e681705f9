#!/usr/bin/env python3
"""HBM-roofline measurement of the structure-metric kernels (dff_struct_rmsd / _dihedrals / _tic / _contacts) at the
output sizes of BASELINE.json's configs, as tools_bench_pwd.py does for the PWD kernels.  Algorithmic bytes per pass
= n * N * 12 (the structures, read once); the outputs are at most (N - 3) / 3N of that.  TIC projects onto 2
components; contacts write the per-frame mismatches against a folded contact map (offset 3).  Prints one JSON line
per config."""
import json
import sys

import torch

import dff_amd
from dff_amd import binding

PEAK_HBM = 8.0e12
CASES = [("chignolin config 2 (10240 x 10)", 10, 10240), ("chignolin iid config 3 (100000 x 10)", 10, 100000),
         ("villin config 4 (819200 x 35)", 35, 819200), ("protein G config 5 (409600 x 56)", 56, 409600)]


def ev_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    for name, N, n in CASES:
        x = torch.randn((n, N, 3), device="cuda") * 5.0
        ref = torch.randn((N, 3)) * 5.0
        F = binding.struct_tic_num_features(N)
        mean = torch.randn(F, dtype=torch.float64, device="cuda")
        coeff = torch.randn((F, 2), dtype=torch.float64, device="cuda")
        folded = (torch.cdist(ref, ref) < 8.0).to(torch.uint8).cuda()
        fns = {"rmsd": lambda: binding.struct_rmsd(x, ref), "dihedrals": lambda: binding.struct_dihedrals(x),
               "tic": lambda: binding.struct_tic(x, mean, coeff),
               "contacts": lambda: binding.struct_contacts(x, 8.0, folded, 3)}
        byts = n * N * 12
        row = {"workload": name, "n": n, "n_beads": N, "tic_features": F, "hbm_bytes_per_pass": byts}
        for k, fn in fns.items():
            t = ev_time(fn, 20)
            row[f"{k}_ms"] = t * 1e3
            row[f"{k}_frac_hbm"] = byts / t / PEAK_HBM
        print(json.dumps(row))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
