#!/usr/bin/env python3
"""Timing of the state kernels (dff_struct_tic_assign / dff_kmeans_step / dff_transition_counts) next to dff_struct_tic,
at the output sizes of BASELINE.json's configs, as tools_bench_struct.py does for the structure metrics (HIP events).

struct_tic and struct_tic_assign (k = 2, K = 4, labels only) are timed in five alternating repeats; the bar is
assign_min <= tic_min * (tic_max / tic_min + 0.05): the fused kernel does the same loads and the same F k fp64 FMAs.
Algorithmic bytes per pass: n * N * 12 for the two frame kernels, n * (16 + 4) for kmeans_step (d = 2, K = 4: points
in, labels out), n * 4 * (1 + 3) for transition_counts (K = 4, lags 1, 10, 100: every label read once per role),
against the 8 TB/s the other struct tools use.  Prints one JSON line per config."""
import json
import sys

import torch

import dff_amd
from dff_amd import binding

PEAK_HBM = 8.0e12
CASES = [("chignolin config 2 (10240 x 10)", 10, 10240), ("chignolin iid config 3 (100000 x 10)", 10, 100000),
         ("villin config 4 (819200 x 35)", 35, 819200), ("protein G config 5 (409600 x 56)", 56, 409600)]
REPEATS = 5


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
    ok = True
    for name, N, n in CASES:
        x = torch.randn((n, N, 3), device="cuda") * 5.0
        F = binding.struct_tic_num_features(N)
        mean = torch.randn(F, dtype=torch.float64, device="cuda")
        coeff = torch.randn((F, 2), dtype=torch.float64, device="cuda") / F ** 0.5
        pts = binding.struct_tic(x, mean, coeff)
        centers = pts[torch.randperm(n, device="cuda")[:4]].clone()
        labels = binding.struct_tic_assign(x, mean, coeff, centers)
        ws = torch.empty(max(binding.kmeans_workspace_bytes(n, 2, 4), 1), dtype=torch.uint8, device="cuda")
        lengths = [n // 100] * 100 if n % 100 == 0 else [n]
        tic, assign = [], []
        for _ in range(REPEATS):
            tic.append(ev_time(lambda: binding.struct_tic(x, mean, coeff), 20))
            assign.append(ev_time(lambda: binding.struct_tic_assign(x, mean, coeff, centers), 20))
        spread = max(tic) / min(tic)
        bar = min(tic) * (spread + 0.05)
        t_km = min(ev_time(lambda: binding.kmeans_step(pts, centers, workspace=ws), 20) for _ in range(REPEATS))
        t_tc = min(ev_time(lambda: binding.transition_counts(labels, lengths, (1, 10, 100), 4), 20)
                   for _ in range(REPEATS))
        row = {"workload": name, "n": n, "n_beads": N, "tic_features": F,
               "struct_tic_ms": [t * 1e3 for t in tic], "struct_tic_assign_ms": [t * 1e3 for t in assign],
               "struct_tic_spread": spread, "assign_over_tic": min(assign) / min(tic),
               "assign_within_bar": min(assign) <= bar,
               "struct_tic_frac_hbm": n * N * 12 / min(tic) / PEAK_HBM,
               "struct_tic_assign_frac_hbm": n * N * 12 / min(assign) / PEAK_HBM,
               "kmeans_step_ms": t_km * 1e3, "kmeans_step_bytes_per_s": n * 20 / t_km,
               "kmeans_step_frac_hbm": n * 20 / t_km / PEAK_HBM,
               "transition_counts_ms": t_tc * 1e3, "transition_counts_bytes_per_s": n * 16 / t_tc,
               "transition_counts_frac_hbm": n * 16 / t_tc / PEAK_HBM, "trajectories": len(lengths)}
        ok = ok and row["assign_within_bar"]
        print(json.dumps(row))
        sys.stdout.flush()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
