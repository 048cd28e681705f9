#!/usr/bin/env python3
"""Timing of dff_msm_dirichlet_solve and of evaluate.bootstrap_passage, by the protocol of tools_bench_msm.py (HIP events, the
minimum of five windows, max / min spread shown).  One JSON line per case.  Every baseline is a route that existed before the
call, never the new code.

solve    milliseconds per call for P problems of K states with K - 6 interior states, K in {64, 256, 1024} x P in {3, 48, 384},
         the library's choice of path; fp64 FLOP/s against n^3 / 3 per problem and against the public vector-fp64 peak of the
         MI355X (78.6 TFLOP/s).  Baselines on the same W and b: torch.linalg.solve, batched, on the device (what it raises is
         recorded when it does not run), and a numpy host loop (np.linalg.solve per problem, timed on at most 8 problems and
         scaled to P: the loop is linear in P).  u is checked against the numpy solution.
paths    the LDS path against the forced blocked path at the LDS limit (K = limit + 6), P in {3, 48, 384}.
         (The VALU trailing update against the MFMA one: `phases`.)
sweep    both forced paths over interior counts 16 .. the LDS limit x P in {3, 48, 384, 1024}: what the limit rests on from below
         (above it the LDS path is refused; DESIGN.md section 19 keeps the figures of the build whose limit was 192).
phases   where one workgroup of the blocked path spends its time at K = 1024 (and 256), with the trailing update on the fp64 VALU
         and on v_mfma_f64_16x16x4_f64 (the debug knob's paths 3 and 4; the library ships the faster one): the kernel leaves the 100 MHz ticks of
         formation, panels (diagonal block and the rows under it), trailing updates and back substitution in the first four
         doubles of each problem's slice of the workspace; mean over the problems, in ms and as shares.
end2end  bootstrap_passage at K = 200, B = 100 on the three-well process of tools_bench_msm_bootstrap.py (40 trajectories x
         2 000 frames, lag 10), wall time, against the host loop over the same fitted models (np.linalg.solve on I - T_II, three
         systems per resample), with the share of the resample loop itself (counts, estimator) timed by bootstrap_msm.
`python tools_bench_msm_passage.py [solve] [paths] [sweep] [phases] [end2end]` runs the named parts (all by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate
from tools_bench_msm import timed          # the protocol: HIP events, the minimum of five windows, max / min spread

STATES = (64, 256, 1024)
BATCHES = (3, 48, 384)
BOUNDARY = 6
PEAK_FP64 = 78.6e12
LAG = 10


def flux_problem(K, seed):
    """a symmetric flux matrix: a ring, K^2 / 8 random entries, heavy diagonals (a metastable model), scaled to sum 1"""
    rng = np.random.default_rng(seed)
    Cm = np.zeros((K, K))
    idx = np.arange(K)
    Cm[idx, (idx + 1) % K] = rng.integers(1, 20, K)
    m = K * K // 8
    Cm[rng.integers(0, K, m), rng.integers(0, K, m)] += rng.integers(1, 20, m)
    Cm[idx, idx] = rng.integers(100, 2000, K)
    X = Cm + Cm.T
    return X / X.sum()


def system(X, n):
    """W, b of the MFPT (lag 1) to the last K - n states"""
    off = X.copy()
    np.fill_diagonal(off, 0.0)
    W = -X[:n, :n]
    W[np.arange(n), np.arange(n)] = off.sum(axis=1)[:n]
    return W, X.sum(axis=1)[:n].copy()


def batch(K, P, distinct=4):
    """P problems on `distinct` matrices (the others repeat them: the timing does not depend on the values)"""
    n = K - BOUNDARY
    Xs = [flux_problem(K, 100 * K + i) for i in range(min(P, distinct))]
    flux = torch.from_numpy(np.stack(Xs)).cuda()[torch.arange(P, device="cuda") % len(Xs)].contiguous()
    role = torch.zeros((P, K), dtype=torch.int32, device="cuda")
    role[:, n:] = 1
    g = torch.zeros((P, K), dtype=torch.float64, device="cuda")
    s = torch.ones((P, K), dtype=torch.float64, device="cuda")
    return Xs, flux, role, g, s, n


def solve_row(K, P, path, check=True):
    Xs, flux, role, g, s, n = batch(K, P)
    ks = np.full(P, K, np.int32)
    ws = torch.empty(binding.msm_dirichlet_workspace_bytes(P, K), dtype=torch.uint8, device="cuda")
    u = torch.empty((P, K), dtype=torch.float64, device="cuda")
    binding.debug_msm_dirichlet_path(path)
    try:
        call = lambda: binding.msm_dirichlet_solve(flux, ks, role, g, s, u=u, workspace=ws)      # noqa: E731
        _, status = call()
        ms, spread = timed(call, reps=3 if K >= 1024 else 10)
    finally:
        binding.debug_msm_dirichlet_path(0)
    row = {"K": K, "P": P, "interior": n, "ms": ms, "spread": spread, "us_per_problem": ms * 1e3 / P,
           "gflops": P * n ** 3 / 3 / (ms * 1e-3) / 1e9, "share_of_fp64_peak": P * n ** 3 / 3 / (ms * 1e-3) / PEAK_FP64,
           "solved": bool((status == 0).all())}
    ok = row["solved"]
    if check:
        uh = u.cpu().numpy()
        worst = 0.0
        for p in range(min(P, len(Xs))):
            W, b = system(Xs[p], n)
            want = np.linalg.solve(W, b)
            worst = max(worst, float(np.abs(uh[p, :n] - want).max() / np.abs(want).max()))
        row["max_rel_diff_to_numpy"] = worst
        ok = ok and worst < 1e-6
    return row, ok, (Xs, n)


def bench_solve():
    ok = True
    for K in STATES:
        for P in BATCHES:
            row, good, (Xs, n) = solve_row(K, P, 0)
            ok = ok and good
            row["call"] = "solve"
            Wb = [system(X, n) for X in Xs]
            # torch.linalg.solve, batched on the device, on the same systems
            try:
                pick = torch.arange(P, device="cuda") % len(Wb)
                W = torch.from_numpy(np.stack([w for w, _ in Wb])).cuda()[pick].contiguous()
                b = torch.from_numpy(np.stack([v for _, v in Wb])).cuda()[pick].contiguous()
                torch.linalg.solve(W, b)
                ms, spread = timed(lambda: torch.linalg.solve(W, b), reps=1 if K >= 1024 else 3)
                row.update({"torch_solve_ms": ms, "torch_solve_spread": spread, "torch_over_call": ms / row["ms"]})
                del W, b
            except Exception as e:                                   # noqa: BLE001  (what this build raises is the record)
                row["torch_solve_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            m = min(P, 8)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                for p in range(m):
                    np.linalg.solve(*Wb[p % len(Wb)])
                t.append(time.perf_counter() - t0)
            row.update({"numpy_loop_ms": min(t) * 1e3 * P / m, "numpy_timed_on": m, "numpy_over_call": min(t) * 1e3 * P / m / row["ms"]})
            print(json.dumps(row))
            sys.stdout.flush()
    return ok


def bench_paths():
    ok = True
    L = binding.msm_dirichlet_lds_limit()
    for P in BATCHES:
        row = {"call": "paths", "K": L + BOUNDARY, "P": P, "interior": L}
        for name, path in (("lds", 0), ("global", 2)):           # limit interior states: the library's choice IS the LDS path
            r, good, _ = solve_row(L + BOUNDARY, P, path, check=(P == BATCHES[0]))
            ok = ok and good
            row.update({f"{name}_ms": r["ms"], f"{name}_spread": r["spread"], f"{name}_gflops": r["gflops"]})
        row["global_over_lds"] = row["global_ms"] / row["lds_ms"]
        print(json.dumps(row))
        sys.stdout.flush()
    return ok


def bench_sweep():
    L = binding.msm_dirichlet_lds_limit()
    for n in [v for v in (16, 32, 64, 96, 128, 160, 192) if v <= L]:
        for P in (3, 48, 384, 1024):
            row = {"call": "sweep", "interior": n, "P": P}
            for name, path in (("lds", 1 if n + BOUNDARY <= L + 1 else 0), ("global", 2)):     # (by size where forcing is refused)
                r, _, _ = solve_row(n + BOUNDARY, P, path, check=False)
                row[f"{name}_ms"] = r["ms"]
            row["global_over_lds"] = row["global_ms"] / row["lds_ms"]
            print(json.dumps(row))
            sys.stdout.flush()
    return True


def bench_phases():
    for K in (256, 1024):
        for P in (3, 384):
            Xs, flux, role, g, s, n = batch(K, P)
            ks = np.full(P, K, np.int32)
            ws = torch.zeros(binding.msm_dirichlet_workspace_bytes(P, K), dtype=torch.uint8, device="cuda")
            for engine, path in (("valu", 3), ("mfma", 4)):          # the blocked path with either trailing update
                binding.debug_msm_dirichlet_path(path)
                try:
                    binding.msm_dirichlet_solve(flux, ks, role, g, s, workspace=ws)
                    ms, _ = timed(lambda: binding.msm_dirichlet_solve(flux, ks, role, g, s, workspace=ws), reps=3)
                finally:
                    binding.debug_msm_dirichlet_path(0)
                slices = ws[8 * P:].view(torch.float64).view(P, K * K + 32 * K)[:, :4].cpu().numpy()      # ticks of 10 ns
                mean = slices.mean(axis=0) * 1e-5                                                           # ms
                names = ("formation", "panels", "trailing", "back_substitution")
                row = {"call": "phases", "trailing_update": engine, "K": K, "P": P, "interior": n, "call_ms": ms,
                       "in_kernel_ms": float(mean.sum())}
                row.update({f"{k}_ms": float(v) for k, v in zip(names, mean)})
                row.update({f"{k}_share": float(v / mean.sum()) for k, v in zip(names, mean)})
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
    km = evaluate.MicrostateKMeans(K, seed=2, max_iter=20).fit(pts)
    labels = km.transform(pts)
    near = lambda w: np.sort(np.argsort(np.linalg.norm(km.cluster_centers - wells[w], axis=1))[:10])  # noqa: E731  (ten centres per well)
    A, Bs = near(0), near(2)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    wall(lambda: evaluate.bootstrap_passage(labels, LAG, A, Bs, lengths, K, n_resamples=2, seed=1))        # warm
    bs, t_new = wall(lambda: evaluate.bootstrap_passage(labels, LAG, A, Bs, lengths, K, n_resamples=Bn, seed=1))
    _, t_msm = wall(lambda: evaluate.bootstrap_msm(labels, LAG, lengths, K, n_resamples=Bn, seed=1))       # the resample loop alone
    plan = evaluate._BootstrapPlan("bench", labels, LAG, lengths, K, Bn, None, 1, None, 1e-12, 1_000_000, 256, None, "cuda:0")
    models = [m for _, ms in plan.batches() for m in ms]

    def host_loop():
        out = np.full((len(models), 2), np.nan)
        for i, m in enumerate(models):
            try:
                a, b, role, g, s = evaluate._passage_problems(m, A, Bs, "bench")
            except ValueError:
                continue
            u = [evaluate._host_dirichlet(m.transition_matrix, r, gg, ss) for r, gg, ss in zip(role, g, s)]
            pi = m.stationary_distribution
            out[i] = np.dot(pi[a], u[0][a]) / pi[a].sum(), np.dot(pi[b], u[1][b]) / pi[b].sum()
        return out
    host, t_host = wall(host_loop)

    def device_solves():
        return evaluate._passage_batch(models, A, Bs, K, torch.device("cuda:0"))
    device_solves()
    (rows, _), t_dev = wall(device_solves)
    fin = np.isfinite(host[:, 0]) & np.isfinite(bs.mfpt_ab)
    agree = float(np.max(np.abs(host[fin, 0] - bs.mfpt_ab[fin]) / np.abs(host[fin, 0]))) if fin.any() else float("nan")
    iv = bs.interval(0.95)
    print(json.dumps({"call": "end2end", "K": K, "B": Bn, "frames": int(paths.size), "lag": LAG, "n_A": int(A.size), "n_B": int(Bs.size),
                      "bootstrap_passage_s": t_new, "bootstrap_msm_s": t_msm, "device_solves_of_B_models_s": t_dev,
                      "host_solves_of_B_models_s": t_host, "host_over_device_solves": t_host / t_dev,
                      "max_rel_diff_mfpt_ab_host_vs_device": agree, "n_failed": bs.n_failed, "mfpt_ab": bs.point["mfpt_ab"],
                      "mfpt_ab_interval": iv["mfpt_ab"], "mfpt_ba": bs.point["mfpt_ba"], "mfpt_ba_interval": iv["mfpt_ba"]}))
    return bool(fin.any()) and agree < 1e-6


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    what = sys.argv[1:] or ["solve", "paths", "sweep", "phases", "end2end"]
    ok = True
    for name, fn in (("solve", bench_solve), ("paths", bench_paths), ("sweep", bench_sweep), ("phases", bench_phases),
                     ("end2end", bench_end2end)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
