#!/usr/bin/env python3
"""Timing of dff_sym_eig_topk and of bootstrap_msm with either eigensolver, by the protocol of tools_bench_msm_passage.py (HIP
events, the minimum of five windows, max / min spread shown).  One JSON line per case.  Every baseline is a route that existed
before the call, never the new code.

topk     milliseconds per call for P symmetrised metastable matrices of K states, K in {64, 200, 256, 1024} x P in {3, 16, 128},
         k = 4, without and with vectors, the library's choice of path.  Per row: the mean 100 MHz ticks the workgroups spent in
         reduction, bisection and vectors (the kernel leaves them at the head of each problem's slice of the workspace); the
         reduction's memory rate against 8 K^3 / 3 bytes per problem (the trailing triangle read and written once per column) and
         its fp64 rate against 4 K^3 / 3 flops per problem, next to the public peaks of the MI355X (8 TB/s, 78.6 TFLOP/s vector fp64).
         Baselines on the same matrices: a numpy host loop (np.linalg.eigvalsh / eigh per problem, timed on at most 4 problems and
         scaled to P: the loop is linear in P) and batched torch.linalg.eigvalsh / eigh on the device (what it raises is recorded
         when it does not run).  The eigenvalues are checked against numpy's.
sweep    both forced paths over K = 16 .. the LDS limit x P in {3, 16, 128, 1024}, with vectors: what the limit rests on.
end2end  bootstrap_msm at K = 200, B = 100 on the three-well process of tools_bench_msm_passage.py (40 trajectories x 2 000
         frames, lag 10), wall time with eigensolver="host" (the parent commit's route) and "device", and the eigensolver's
         share: the host loop of eigvalsh over the same fitted models against one msm_spectrum call.
`python tools_bench_msm_eig.py [topk] [sweep] [end2end]` runs the named parts (all by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate
from tools_bench_msm import timed          # the protocol: HIP events, the minimum of five windows, max / min spread

STATES = (64, 200, 256, 1024)
BATCHES = (3, 16, 128)
K_TOP = 4
PEAK_FP64, PEAK_BYTES = 78.6e12, 8.0e12
LAG = 10


def metastable(K, seed):
    """pi^(1/2) T pi^(-1/2) of a reversible chain with four metastable blocks: eigenvalues 1, three close to 1, the rest below"""
    rng = np.random.default_rng(seed)
    of = np.arange(K) * 4 // K
    X = rng.uniform(0.5, 1.5, (K, K))
    X = 0.5 * (X + X.T) * np.where(of[:, None] == of[None, :], 1.0, 1e-4)
    X += np.diag(rng.uniform(2.0, 4.0, K) * X.sum(axis=1))
    r = np.sqrt(X.sum(axis=1) / X.sum())
    M = X / X.sum() / r[:, None] / r[None, :]
    return 0.5 * (M + M.T)


def batch(K, P, distinct=4):
    """P problems on `distinct` matrices (the others repeat them: the timing does not depend on the values)"""
    Ms = [metastable(K, 100 * K + i) for i in range(min(P, distinct))]
    a = torch.from_numpy(np.stack(Ms)).cuda()[torch.arange(P, device="cuda") % len(Ms)].contiguous()
    return Ms, a


def call_row(K, P, vectors, path, check=True):
    Ms, a = batch(K, P)
    ks = np.full(P, K, np.int32)
    ws = torch.zeros(binding.sym_eig_workspace_bytes(P, K), dtype=torch.uint8, device="cuda")
    binding.debug_sym_eig_path(path)
    try:
        call = lambda: binding.sym_eig_topk(a, ks, K_TOP, vectors=vectors, workspace=ws)      # noqa: E731
        w, _, status = call()
        ms, spread = timed(call, reps=2 if K >= 1024 else 10)
    finally:
        binding.debug_sym_eig_path(0)
    ticks = ws[8 * P:].view(torch.float64).view(P, 4 + K * K)[:, :3].cpu().numpy().mean(axis=0) * 1e-5      # ms
    row = {"K": K, "P": P, "k": K_TOP, "vectors": bool(vectors), "ms": ms, "spread": spread, "us_per_problem": ms * 1e3 / P,
           "reduction_ms": float(ticks[0]), "bisection_ms": float(ticks[1]), "vectors_ms": float(ticks[2]),
           "solved": bool((status == 0).all())}
    if ticks[0] > 0:
        row.update({"reduction_gbytes_per_s": P * 8 * K ** 3 / 3 / (ticks[0] * 1e-3) / 1e9,
                    "reduction_share_of_hbm_peak": P * 8 * K ** 3 / 3 / (ticks[0] * 1e-3) / PEAK_BYTES,
                    "reduction_gflops": P * 4 * K ** 3 / 3 / (ticks[0] * 1e-3) / 1e9,
                    "reduction_share_of_fp64_peak": P * 4 * K ** 3 / 3 / (ticks[0] * 1e-3) / PEAK_FP64})
    ok = row["solved"]
    if check:
        wh = w.cpu().numpy()
        worst = max(float(np.abs(wh[p] - np.linalg.eigvalsh(Ms[p])[::-1][:K_TOP]).max()) for p in range(min(P, len(Ms))))
        row["max_diff_to_numpy"] = worst
        ok = ok and worst < 1e-12
    return row, ok, (Ms, a)


def bench_topk():
    ok = True
    for K in STATES:
        for P in BATCHES:
            for vectors in (False, True):
                row, good, (Ms, a) = call_row(K, P, vectors, 0)
                ok = ok and good
                row["call"] = "topk"
                host = np.linalg.eigh if vectors else np.linalg.eigvalsh
                m = min(P, 4 if K < 1024 else 2)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for p in range(m):
                        host(Ms[p % len(Ms)])
                    t.append(time.perf_counter() - t0)
                row.update({"numpy_loop_ms": min(t) * 1e3 * P / m, "numpy_timed_on": m, "numpy_over_call": min(t) * 1e3 * P / m / row["ms"]})
                try:
                    dev = torch.linalg.eigh if vectors else torch.linalg.eigvalsh
                    dev(a)
                    ms, spread = timed(lambda: dev(a), reps=1 if K >= 1024 else 3)
                    row.update({"torch_ms": ms, "torch_spread": spread, "torch_over_call": ms / row["ms"]})
                except Exception as e:                               # noqa: BLE001  (what this build raises is the record)
                    row["torch_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                print(json.dumps(row))
                sys.stdout.flush()
    return ok


def bench_sweep():
    L = binding.sym_eig_lds_limit()
    for K in [v for v in (16, 32, 64, 96, 128, 144, 160, 176) if v <= L]:
        for P in (3, 16, 128, 1024):
            row = {"call": "sweep", "K": K, "P": P}
            for name, path in (("lds", 1), ("workspace", 2)):
                r, _, _ = call_row(K, P, True, path, check=False)
                row[f"{name}_ms"] = r["ms"]
                row[f"{name}_reduction_ms"] = r["reduction_ms"]
            row["workspace_over_lds"] = row["workspace_ms"] / row["lds_ms"]
            print(json.dumps(row))
            sys.stdout.flush()
    return True


def bench_end2end(K=200, Bn=100):
    M = np.array([[0.98, 0.015, 0.005], [0.02, 0.97, 0.01], [0.004, 0.016, 0.98]])
    rng = np.random.default_rng(8)
    n_traj, n_frames = 40, 2000
    s = rng.integers(0, 3, n_traj)
    cum = np.cumsum(M, axis=1)
    paths = np.empty((n_traj, n_frames), np.int64)
    for t in range(n_frames):
        paths[:, t] = s
        s = np.minimum((rng.random(n_traj)[:, None] >= cum[s]).sum(axis=1), 2)
    wells = np.array([[0.0, 0.0], [6.0, 1.0], [2.0, 7.0]])
    pts = wells[paths.reshape(-1)] + rng.standard_normal((paths.size, 2))
    lengths = [n_frames] * n_traj
    labels = evaluate.MicrostateKMeans(K, seed=2, max_iter=20).fit(pts).transform(pts)

    def wall(fn, repeats=3):
        best, r = float("inf"), None
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return r, best
    run = lambda solver, B=Bn: evaluate.bootstrap_msm(labels, LAG, lengths, K, n_resamples=B, seed=1, eigensolver=solver)  # noqa: E731
    run("host", 2), run("device", 2)                                  # warm
    host, t_host = wall(lambda: run("host"))
    devi, t_dev = wall(lambda: run("device"))
    plan = evaluate._BootstrapPlan("bench", labels, LAG, lengths, K, Bn, None, 1, None, 1e-12, 1_000_000, 256, None, "cuda:0")
    models = [m for _, ms in plan.batches() for m in ms]
    _, t_eigvalsh = wall(lambda: [m.timescales(3) for m in models])
    _, t_spectrum = wall(lambda: evaluate.msm_spectrum(models, k=3))
    fin = np.isfinite(host.timescales) & np.isfinite(devi.timescales)
    agree = float(np.max(np.abs(host.timescales[fin] - devi.timescales[fin]) / host.timescales[fin]))
    print(json.dumps({"call": "end2end", "K": K, "B": Bn, "frames": int(paths.size), "lag": LAG,
                      "bootstrap_msm_host_s": t_host, "bootstrap_msm_device_s": t_dev, "host_over_device": t_host / t_dev,
                      "eigvalsh_loop_of_B_models_s": t_eigvalsh, "msm_spectrum_of_B_models_s": t_spectrum,
                      "max_rel_diff_timescales": agree, "n_active_min": int(host.n_active.min()),
                      "same_nan_pattern": bool(np.array_equal(np.isnan(host.timescales), np.isnan(devi.timescales)))}))
    return agree < 1e-6


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    what = sys.argv[1:] or ["topk", "sweep", "end2end"]
    ok = True
    for name, fn in (("topk", bench_topk), ("sweep", bench_sweep), ("end2end", bench_end2end)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
