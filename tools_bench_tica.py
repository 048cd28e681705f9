#!/usr/bin/env python3
"""Timing of the TICA fitting kernels (csrc/dff_tica.hip) at the reference's dataset sizes, on seeded synthetic frames.

Per molecule: the features pass (dff_struct_tic_features over all n frames) and the moments pass (one dff_tica_moments
call over the same frames as one trajectory at lag 100, which computes its own features chunk by chunk), timed with
device events after a warm-up.  FLOP counts come from the shapes:
  flop_model = 3 w F^2            the three fp64 F x F products over the w = n - lag frame pairs (M_0's two, M_tau's
                                  symmetrised one) at 2 FLOP per multiply-add on their upper triangles
  flop_mfma  = 2 * 2 w NT 64^2    what the kernel issues: two SYRKs (u u^T, v v^T) over NT upper-triangular 64 x 64
                                  tiles, NT = NB (NB + 1) / 2, NB = ceil(F / 64)
and the achieved fp64 rate is set against 78.6 TFLOP/s, AMD's published FP64 matrix peak for the MI355X (a spec-sheet
figure, not measured here).  The host baseline is numpy float64 (X^T X + Y^T Y, X^T Y + Y^T X) on HOST_FRAMES frames,
measured at that smaller n and scaled linearly to the full n.  Kernel-by-kernel times: run this under
`rocprofv3 --kernel-trace --stats` (--only MOL --reps 1 keeps that run short).  One JSON line per molecule.

    python tools_bench_tica.py [--only MOL] [--reps 3] [--no-host]
"""
import argparse
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding

FP64_MATRIX_PEAK = 78.6e12          # AMD's published MI355X FP64 matrix rate (spec sheet)
LAG = 100
HOST_FRAMES = 20000
DATASETS = [("chignolin", 10, 534743), ("trp_cage", 20, 1044000), ("bba", 28, 1114545), ("villin", 35, 627907),
            ("protein_g", 56, 1849251)]


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
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dff_amd.load_library()
    for mol, N, n in DATASETS:
        if a.only and mol != a.only:
            continue
        g = torch.Generator(device="cuda").manual_seed(N)
        x = torch.randn((n, N, 3), device="cuda", generator=g) * 3.0
        x += torch.arange(N, device="cuda", dtype=torch.float32)[None, :, None] * 3.8
        F = binding.struct_tic_num_features(N)
        NB = (F + 63) // 64
        NT = NB * (NB + 1) // 2
        w = n - LAG
        t_feat = ev_time(lambda: binding.struct_tic_features(x), a.reps)
        shift = binding.struct_tic_features(x[:1])[0].double()
        acc = [torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((F,), (F,), (F, F), (F, F))]
        ws = torch.empty(binding.tica_workspace_bytes(N, n, LAG), dtype=torch.uint8, device="cuda")
        t_mom = ev_time(lambda: binding.tica_moments(x, [n], LAG, shift, *acc, workspace=ws), a.reps)
        flop_model, flop_mfma = 3.0 * w * F * F, 4.0 * w * NT * 64 * 64
        row = {"molecule": mol, "n_frames": n, "n_beads": N, "features": F, "lagtime": LAG, "pairs": w,
               "features_pass_s": t_feat, "features_bytes_written": n * F * 4,
               "moments_pass_s": t_mom, "flop_model": flop_model, "flop_mfma": flop_mfma,
               "tflops_model": flop_model / t_mom / 1e12, "tflops_mfma": flop_mfma / t_mom / 1e12,
               "frac_of_published_fp64_matrix_peak_78.6": flop_mfma / t_mom / FP64_MATRIX_PEAK}
        if not a.no_host:
            f = binding.struct_tic_features(x[:HOST_FRAMES]).cpu().numpy().astype(np.float64)
            f -= f[0]
            t0 = time.perf_counter()
            X, Y = f[:-LAG], f[LAG:]
            _ = X.T @ X + Y.T @ Y, X.T @ Y + Y.T @ X
            t_host = time.perf_counter() - t0
            row["host_numpy_fp64_frames"] = HOST_FRAMES
            row["host_numpy_fp64_s_at_those_frames"] = t_host
            row["host_numpy_fp64_s_scaled_to_n"] = t_host * w / (HOST_FRAMES - LAG)
        print(json.dumps(row))
        sys.stdout.flush()
        del x, acc, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
