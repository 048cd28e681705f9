#!/usr/bin/env python3
"""Timing of the Markov-state-model calls (dff_micro_kmeans_step, dff_micro_transition_counts, dff_msm_reversible_steps) by the
protocol of tools_bench_autocorr.py (HIP events, the minimum of five windows of 20 calls, max / min spread shown) at
n in {100 000, 819 200} points or frames, d in {2, 8} coordinates and K in {64, 256, 1024} states.  One JSON line per case.

kmeans   assignment alone and the whole Lloyd step, in ms, point-centre pairs per second (n K) and fp64 FMAs per second (n K d)
         next to the public vector-fp64 peak of the MI355X (78.6 TFLOP/s = 39.3e12 FMA/s); at K = 64 next to dff_kmeans_step,
         the route that existed before (labels are checked to be equal).
counts   three lag times over 80 equal trajectories of a metastable path, in ms and (frame, lag) pairs per second; at K = 64
         next to dff_transition_counts (counts are checked to be equal).
sweeps   microseconds per sweep of the reversible estimator from calls of 200 sweeps, for both drivers (one launch per sweep,
         one workgroup for all sweeps; the bits are checked to be equal) and the library's own choice, next to the same sweep
         written in torch on the device, (S / (q[:, None] + q[None, :])).sum(1), the only previous device route, and next to
         the numpy sweep on the host; K^2 divisions per sweep.  K = 8, 16 and 32 are timed too: they are where the two drivers
         cross, and what the library's choice between them rests on.
`python tools_bench_msm.py [kmeans] [counts] [sweeps]` runs the named parts (all three by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding

PEAK_FMA = 39.3e12
POINTS = (100000, 819200)
STATES = (64, 256, 1024)
TRAJECTORIES = 80          # divides every n of POINTS
REPEATS = 5
SWEEPS = 200
SWEEP_STATES = (8, 16, 32) + STATES          # the small ones decide which driver the library picks


def ev_time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def timed(fn, reps=20):
    """(minimum in ms, max / min) over REPEATS windows"""
    t = [ev_time(fn, reps) for _ in range(REPEATS)]
    return min(t) * 1e3, max(t) / min(t)


def bench_kmeans():
    ok = True
    for n in POINTS:
        for d in (2, 8):
            pts = torch.randn((n, d), dtype=torch.float64, device="cuda") + 4.0 * torch.randint(0, 3, (n, 1), device="cuda")
            for K in STATES:
                centers = pts[torch.randperm(n, device="cuda")[:K]].contiguous()
                ws = torch.empty(binding.micro_kmeans_workspace_bytes(n, d, K), dtype=torch.uint8, device="cuda")
                row = {"call": "kmeans", "n": n, "d": d, "K": K, "workspace_MB": ws.numel() / 2 ** 20}
                for name, acc in (("assign", False), ("lloyd", True)):
                    ms, spread = timed(lambda: binding.micro_kmeans_step(pts, centers, accumulate=acc, workspace=ws))
                    row.update({f"{name}_ms": ms, f"{name}_spread": spread, f"{name}_pairs_per_s": n * K / (ms * 1e-3),
                                f"{name}_fma_per_s": n * K * d / (ms * 1e-3), f"{name}_frac_fp64_peak": n * K * d / (ms * 1e-3) / PEAK_FMA})
                if K <= 64:
                    ws0 = torch.empty(binding.kmeans_workspace_bytes(n, d, K), dtype=torch.uint8, device="cuda")
                    same = torch.equal(binding.micro_kmeans_step(pts, centers, accumulate=False)["labels"],
                                       binding.kmeans_step(pts, centers, accumulate=False)["labels"])
                    ok = ok and same
                    row["labels_equal"] = same
                    for name, acc in (("assign", False), ("lloyd", True)):
                        ms, spread = timed(lambda: binding.kmeans_step(pts, centers, accumulate=acc, workspace=ws0))
                        row.update({f"kmeans_step_{name}_ms": ms, f"kmeans_step_{name}_spread": spread,
                                    f"{name}_over_kmeans_step": row[f"{name}_ms"] / ms})
                print(json.dumps(row))
                sys.stdout.flush()
    return ok


def metastable(n, K, stay=0.98):
    jump = torch.rand(n, device="cuda") > stay
    idx = torch.where(jump, torch.arange(n, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"))
    last = torch.cummax(idx, 0).values
    return torch.randint(0, K, (n,), device="cuda")[last].to(torch.int32).contiguous()


def bench_counts():
    ok = True
    lags = [1, 10, 100]
    for n in POINTS:
        lengths = [n // TRAJECTORIES] * TRAJECTORIES
        for K in STATES:
            labels = metastable(n, K)
            got = binding.micro_transition_counts(labels, lengths, lags, K)
            pairs = int(got.sum().cpu())
            ms, spread = timed(lambda: binding.micro_transition_counts(labels, lengths, lags, K))
            row = {"call": "counts", "n": n, "K": K, "lags": lags, "pairs": pairs, "counts_ms": ms, "counts_spread": spread,
                   "pairs_per_s": pairs / (ms * 1e-3)}
            if K <= 64:
                same = torch.equal(got, binding.transition_counts(labels, lengths, lags, K))
                ok = ok and same
                ms0, spread0 = timed(lambda: binding.transition_counts(labels, lengths, lags, K))
                row.update({"counts_equal": same, "transition_counts_ms": ms0, "transition_counts_spread": spread0,
                            "counts_over_transition_counts": ms / ms0})
            print(json.dumps(row))
            sys.stdout.flush()
    return ok


def bench_sweeps():
    ok = True
    for K in SWEEP_STATES:
        rng = np.random.default_rng(K)
        Cm = np.zeros((K, K))
        idx = np.arange(K)
        Cm[idx, (idx + 1) % K] = rng.integers(1, 20, K)
        m = K * K // 8
        Cm[rng.integers(0, K, m), rng.integers(0, K, m)] += rng.integers(1, 20, m)
        Cm[idx, idx] = rng.integers(100, 2000, K)
        S, c = Cm + Cm.T, Cm.sum(axis=1)
        Sd, cd = torch.from_numpy(S).cuda(), torch.from_numpy(c).cuda()
        x0 = 0.5 * Sd.sum(1)
        ws = torch.empty(binding.msm_workspace_bytes(K), dtype=torch.uint8, device="cuda")
        row = {"call": "sweeps", "K": K, "nonzero_share": float((S != 0).mean()), "sweeps_per_call": SWEEPS}
        results = {}
        for name, driver in (("auto", 0), ("launch_per_sweep", 1), ("one_workgroup", 2)):
            binding.debug_msm_driver(driver)
            x = x0.clone()
            err = binding.msm_reversible_steps(Sd, cd, x, SWEEPS, workspace=ws)
            results[name] = (x.cpu(), err.cpu())
            ms, spread = timed(lambda: binding.msm_reversible_steps(Sd, cd, x, SWEEPS, workspace=ws), reps=5)
            row.update({f"{name}_us_per_sweep": ms * 1e3 / SWEEPS, f"{name}_spread": spread,
                        f"{name}_divisions_per_s": float(K * K) * SWEEPS / (ms * 1e-3)})
        binding.debug_msm_driver(0)
        same = all(torch.equal(results["auto"][i], results[k][i]) for k in results for i in (0, 1))
        ok = ok and same
        row["drivers_equal"] = same

        def torch_sweeps():
            x = x0
            for _ in range(SWEEPS):
                q = cd / x
                x = (Sd / (q[:, None] + q[None, :])).sum(1)
            return x
        rel = float(((torch_sweeps().cpu() - results["auto"][0]) / results["auto"][0]).abs().max())
        ms, spread = timed(torch_sweeps, reps=5)
        row.update({"torch_us_per_sweep": ms * 1e3 / SWEEPS, "torch_spread": spread, "torch_rel_diff": rel,
                    "auto_over_torch": row["auto_us_per_sweep"] / (ms * 1e3 / SWEEPS)})
        xh, t0 = 0.5 * S.sum(axis=1), time.perf_counter()
        for _ in range(5):
            q = c / xh
            xh = np.divide(S, q[:, None] + q[None, :], out=np.zeros_like(S), where=S != 0).sum(axis=1)
        row["numpy_us_per_sweep"] = (time.perf_counter() - t0) / 5 * 1e6
        ok = ok and rel < 1e-9
        print(json.dumps(row))
        sys.stdout.flush()
    return ok


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    what = sys.argv[1:] or ["kmeans", "counts", "sweeps"]
    ok = True
    for name, fn in (("kmeans", bench_kmeans), ("counts", bench_counts), ("sweeps", bench_sweeps)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
