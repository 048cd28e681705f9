#!/usr/bin/env python3
"""What the denoising loss costs on top of the score: dff_denoise_loss against dff_score alone on the same inputs (HIP events),
for chignolin at batch 4096 and villin at batch 1024, synthetic weights.

dff_denoise_loss = dff_q_sample + the score + the loss kernel (+ the two-stage total); the difference of the two timings is
the cost of the new kernels.  Algorithmic traffic of the two of them with in-kernel noise: q_sample reads x0 and writes x_t
(24 N bytes per sample), the loss kernel reads the model output (12 N): 36 N bytes per sample, plus 12 N per kernel when the
noise is supplied.  Five alternating repeats, minimum of each; one JSON line per config."""
import json
import sys

import numpy as np
import torch

import dff_amd
from dff_amd.score import GraphTransformer
import synth_weights as synth

CASES = [("chignolin", 4096), ("villin", 1024)]
REPEATS, REPS = 5, 20


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
    for cfg, B in CASES:
        _, N, H, L = synth.SHIPPED_CONFIGS[cfg]
        model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                                 use_distances=False, conservative=True, state_dict=synth.synth_gnn_params(N, H, L))
        nat = model.native
        x0 = torch.from_numpy(synth.normal((B, N, 3), 31, 1).astype(np.float32)).cuda()
        x0 = x0 - x0.mean(1, keepdim=True)
        t = torch.full((B,), 20, dtype=torch.int32, device="cuda")
        z = torch.randn_like(x0)
        xt, tn = nat.q_sample(x0, t, seed=1, return_tnorm=True)
        total = torch.zeros(2, dtype=torch.float64, device="cuda")
        score, philox, supplied, qs = [], [], [], []
        for _ in range(REPEATS):
            score.append(ev_time(lambda: nat.score(xt, tn), REPS))
            philox.append(ev_time(lambda: nat.denoise_loss(x0, t, seed=1, total=total), REPS))
            supplied.append(ev_time(lambda: nat.denoise_loss(x0, t, noise=z, total=total), REPS))
            qs.append(ev_time(lambda: nat.q_sample(x0, t, seed=1), REPS))
        s, p, u = min(score), min(philox), min(supplied)
        print(json.dumps({"workload": cfg, "batch": B, "n_beads": N, "kernel": nat.last_launch()[0],
                          "score_us": s * 1e6, "denoise_loss_philox_us": p * 1e6, "denoise_loss_supplied_us": u * 1e6,
                          "q_sample_alone_us": min(qs) * 1e6, "extra_philox_us": (p - s) * 1e6, "extra_supplied_us": (u - s) * 1e6,
                          "extra_philox_over_score": (p - s) / s, "extra_supplied_over_score": (u - s) / s,
                          "score_spread": max(score) / s, "algorithmic_bytes_per_sample": 36 * N}))
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
