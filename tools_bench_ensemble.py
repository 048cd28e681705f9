#!/usr/bin/env python3
"""Time of the nearest-structure search dff_rmsd_nearest (csrc/dff_ensemble.hip) at evaluation sizes, against the only
route the library had before it: one dff_struct_rmsd launch per candidate structure, each reading all n queries.

The baseline is SCALED: the loop runs over the first BASE_SUBSET candidates only and its time is multiplied by
m / BASE_SUBSET (every launch does the same work, so the loop is linear in m; running all 10^4 launches would add
minutes and no information).  It leaves out the running minimum a real loop would also keep.  HIP events around the
enqueued work, one warm-up call, the median of REPS.  Frames are random walks with 3.8 A bonds.  Prints one JSON line per
shape, then one line with the split of the kernel time into a per-pair part (the Jacobi eigenvalue iteration, the key
and its reduction) and a part per k-step of 4 beads (operand loads and fp64 MFMAs), fitted over the bead counts."""
import json
import statistics
import sys

import numpy as np
import torch

import dff_amd
from dff_amd import binding

SHAPES = [(10240, 10240, 10), (100000, 10000, 10), (100000, 10000, 35), (50000, 10000, 56)]
BASE_SUBSET = 64
REPS = 5


def walks(n, N, gen):
    step = torch.randn((n, N, 3), device="cuda", generator=gen)
    step = step * (3.8 / step.norm(dim=-1, keepdim=True))
    return step.cumsum(1).contiguous()


def ev_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    dff_amd.load_library()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    rows = []
    for n, m, N in SHAPES:
        x, y = walks(n, N, gen), walks(m, N, gen)
        ws = torch.empty(binding.rmsd_nearest_workspace_bytes(n, m, N), dtype=torch.uint8, device="cuda")
        t = ev_times(lambda: binding.rmsd_nearest(x, y, workspace=ws), REPS)
        refs = [y[r].clone() for r in range(BASE_SUBSET)]

        def loop():
            for r in refs:
                binding.struct_rmsd(x, r)

        tb = ev_times(loop, 3)
        ms, base = statistics.median(t), statistics.median(tb) * m / BASE_SUBSET
        row = {"n": n, "m": m, "n_beads": N, "nearest_ms": ms, "nearest_ms_min": min(t), "nearest_ms_max": max(t),
               "pairs_per_s": n * m / (ms * 1e-3), "ns_per_pair": ms * 1e6 / (n * m),
               "struct_rmsd_loop_ms_scaled": base, "loop_candidates_timed": BASE_SUBSET, "speedup_vs_scaled_loop": base / ms}
        rows.append(row)
        print(json.dumps(row))
        sys.stdout.flush()
    # ns per pair = a + b * (k-steps = ceil(N / 4)), least squares over the shapes
    ks = np.array([(r["n_beads"] + 3) // 4 for r in rows], np.float64)
    per = np.array([r["ns_per_pair"] for r in rows])
    A = np.stack([np.ones_like(ks), ks], 1)
    (a, b), *_ = np.linalg.lstsq(A, per, rcond=None)
    print(json.dumps({"fit_ns_per_pair": {"per_pair": a, "per_kstep": b},
                      "share_per_pair_part": {str(r["n_beads"]): a / (a + b * k) for r, k in zip(rows, ks)}}))


if __name__ == "__main__":
    main()
