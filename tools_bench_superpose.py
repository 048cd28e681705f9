#!/usr/bin/env python3
"""Timing of dff_superpose at the output sizes of BASELINE.json's configs (the shapes of tools_bench_struct.py), in three
configurations -- rmsd only, + aligned frames, + ensemble statistics (no aligned frames) -- beside dff_struct_rmsd, which
reads the same n * N * 12 bytes and runs the same Jacobi sweeps without the eigenvectors.  "+ aligned" writes another
n * N * 12 bytes.  Device events around `reps` back-to-back calls after one warm-up call per shape and configuration;
the configurations alternate within each of `rounds` rounds, and the median and the spread over the rounds are printed.
One JSON line per shape."""
import json
import statistics
import sys

import torch

import dff_amd
from dff_amd import binding

PEAK_HBM = 8.0e12
CASES = [("chignolin config 2 (10240 x 10)", 10, 10240), ("chignolin iid config 3 (100000 x 10)", 10, 100000),
         ("villin config 4 (819200 x 35)", 35, 819200), ("protein G config 5 (409600 x 56)", 56, 409600)]


def ev_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main(reps=20, rounds=5):
    dff_amd.load_library()
    torch.manual_seed(0)
    for name, N, n in CASES:
        x = torch.randn((n, N, 3), device="cuda") * 5.0
        ref = (torch.randn((N, 3)) * 5.0).cuda()
        out = torch.empty_like(x)
        ws = torch.empty(binding.superpose_workspace_bytes(n, N), dtype=torch.uint8, device="cuda")
        fns = {"struct_rmsd": lambda: binding.struct_rmsd(x, ref),
               "superpose_rmsd": lambda: binding.superpose(x, ref, aligned=False, rmsd=True),
               "superpose_aligned": lambda: binding.superpose(x, ref, rmsd=True, out=out),
               "superpose_stats": lambda: binding.superpose(x, ref, aligned=False, rmsd=True, stats=True, workspace=ws)}
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(ev_time(fn, reps))
        byts = n * N * 12
        row = {"workload": name, "n": n, "n_beads": N, "hbm_bytes_read": byts, "reps": reps, "rounds": rounds}
        for k, t in times.items():
            med = statistics.median(t)
            row[f"{k}_ms"] = med * 1e3
            row[f"{k}_spread"] = (max(t) - min(t)) / med
            row[f"{k}_frac_hbm"] = byts * (2 if k == "superpose_aligned" else 1) / med / PEAK_HBM
        for k in ("superpose_rmsd", "superpose_aligned", "superpose_stats"):
            row[f"{k}_over_struct_rmsd"] = row[f"{k}_ms"] / row["struct_rmsd_ms"]
        print(json.dumps(row))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
