#!/usr/bin/env python3
"""Timing of dff_msm_propagate and of chapman_kolmogorov on top of it, by the protocol of tools_bench_msm_eig.py (HIP events, the
minimum of five windows, max / min spread shown).  One JSON line per case.  Every baseline is a route that existed before the
call, never the new code.

call     milliseconds per call for P row-stochastic metastable matrices of K states, K in {64, 200, 256, 1024} x P in
         {3, 16, 128, 600} x S in {5, 256} steps, M = R = 4, the library's choice of path, every problem on a matrix of its own.
         Per row: the matrix traffic P S K^2 8 bytes per second (what the streamed path reads; the LDS path reads each matrix once)
         and the fused multiply-adds P S M K^2 per second, next to the public peaks of the MI355X (8 TB/s, 78.6 TFLOP/s vector fp64
         = 39.3 T fma/s).  Baselines on the same problems: a batched torch.matmul chain on the device in fp64 (w = w @ T and
         w @ obs^T per step) and a numpy host loop (timed on at most 4 problems and scaled to P: the loop is linear in P).  The
         outputs are checked against numpy's.
sweep    both forced paths over K = 16 .. the largest K that fits LDS x P in {3, 16, 128, 1024}, S = 64, M = R = 4: what the LDS
         limit rests on.
rows     M = R = 16 at K = 112 (LDS) and K = 1024 (streamed) against M = R = 4: what further start rows cost.
end2end  chapman_kolmogorov at K = 200, B = 100, multiples 1 .. 5 on the three-well process of tools_bench_msm_eig.py (40
         trajectories x 2 000 frames, lag 10), wall time with the device propagator and with a numpy propagator behind
         evaluate.propagator (the parent commit's only route), and the propagation's share of each.
`python tools_bench_msm_propagate.py [call] [sweep] [rows] [end2end]` runs the named parts (all by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate
from tools_bench_msm import timed          # the protocol: HIP events, the minimum of five windows, max / min spread

STATES = (64, 200, 256, 1024)
BATCHES = (3, 16, 128, 600)
STEPS = (5, 256)
PEAK_FMA, PEAK_BYTES = 39.3e12, 8.0e12
LAG = 10


def metastable(K, seed):
    """the row-stochastic T of a reversible chain with four metastable blocks"""
    rng = np.random.default_rng(seed)
    of = np.arange(K) * 4 // K
    X = rng.uniform(0.5, 1.5, (K, K))
    X = 0.5 * (X + X.T) * np.where(of[:, None] == of[None, :], 1.0, 1e-4)
    X += np.diag(rng.uniform(2.0, 4.0, K) * X.sum(axis=1))
    return X / X.sum(axis=1)[:, None]


def batch(K, P, M, R, distinct=4):
    """P problems, each with a matrix of its own in memory (`distinct` different ones: the timing does not depend on the values)"""
    Ts = [metastable(K, 100 * K + i) for i in range(min(P, distinct))]
    rng = np.random.default_rng(K)
    w0 = rng.uniform(0.0, 1.0, (M, K))
    w0 /= w0.sum(axis=1)[:, None]
    obs = rng.normal(size=(R, K))
    idx = torch.arange(P, device="cuda") % len(Ts)
    t = torch.from_numpy(np.stack(Ts)).cuda()[idx].contiguous()
    return Ts, w0, obs, t, torch.from_numpy(w0).cuda().expand(P, M, K).contiguous(), torch.from_numpy(obs).cuda().expand(P, R, K).contiguous()


def numpy_chain(T, w0, obs, S):
    out = np.empty((S + 1, len(w0), len(obs)))
    w = w0
    for s in range(S + 1):
        out[s] = w @ obs.T
        if s < S:
            w = w @ T
    return out


def torch_chain(t, w0, obs, S):
    out = torch.empty((t.shape[0], S + 1, w0.shape[1], obs.shape[1]), dtype=torch.float64, device=t.device)
    w, ot = w0, obs.transpose(1, 2)
    for s in range(S + 1):
        out[:, s] = torch.bmm(w, ot)
        if s < S:
            w = torch.bmm(w, t)
    return out


def call_row(K, P, S, M, R, path, check=True):
    Ts, w0, obs, t, w0d, obsd = batch(K, P, M, R)
    ks = np.full(P, K, np.int32)
    ws = torch.zeros(binding.msm_propagate_workspace_bytes(P, K, M, R), dtype=torch.uint8, device="cuda")
    binding.debug_msm_propagate_path(path)
    try:
        call = lambda: binding.msm_propagate(t, None, ks, w0d, obsd, S, workspace=ws)      # noqa: E731
        out, _, status = call()
        ms, spread = timed(call, reps=2 if K * K * S * P > 1 << 32 else 10)
    finally:
        binding.debug_msm_propagate_path(0)
    sec = ms * 1e-3
    row = {"K": K, "P": P, "S": S, "M": M, "R": R, "ms": ms, "spread": spread, "us_per_problem_step": ms * 1e3 / P / max(S, 1),
           "matrix_gbytes_per_s": P * S * K * K * 8 / sec / 1e9, "share_of_hbm_peak": P * S * K * K * 8 / sec / PEAK_BYTES,
           "gfma_per_s": P * S * M * K * K / sec / 1e9, "share_of_fp64_peak": P * S * M * K * K / sec / PEAK_FMA,
           "solved": bool((status == 0).all())}
    ok = row["solved"]
    if check:
        oh = out[:len(Ts)].cpu().numpy()
        worst = max(float(np.abs(oh[p] - numpy_chain(Ts[p], w0, obs, S)).max()) for p in range(len(Ts)))
        row["max_diff_to_numpy"] = worst
        ok = ok and worst < 1e-12
    return row, ok, (Ts, w0, obs, t, w0d, obsd)


def bench_call():
    ok = True
    for K in STATES:
        for P in BATCHES:
            for S in STEPS:
                row, good, (Ts, w0, obs, t, w0d, obsd) = call_row(K, P, S, 4, 4, 0)
                ok = ok and good
                row["call"] = "call"
                m = min(P, 4 if K < 1024 else 2)
                tt = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for p in range(m):
                        numpy_chain(Ts[p % len(Ts)], w0, obs, S)
                    tt.append(time.perf_counter() - t0)
                row.update({"numpy_loop_ms": min(tt) * 1e3 * P / m, "numpy_timed_on": m, "numpy_over_call": min(tt) * 1e3 * P / m / row["ms"]})
                ms, spread = timed(lambda: torch_chain(t, w0d, obsd, S), reps=1 if K * K * S * P > 1 << 30 else 3)
                row.update({"torch_ms": ms, "torch_spread": spread, "torch_over_call": ms / row["ms"]})
                print(json.dumps(row))
                sys.stdout.flush()
                del t, w0d, obsd
    return ok


def bench_sweep():
    L = binding.msm_propagate_lds_limit()
    for K in [v for v in (16, 32, 64, 96, 104, 112, 120) if v <= L]:
        for P in (3, 16, 128, 1024):
            row = {"call": "sweep", "K": K, "P": P, "S": 64}
            for name, path in (("lds", 1), ("streamed", 2)):
                r, _, _ = call_row(K, P, 64, 4, 4, path, check=False)
                row[f"{name}_ms"] = r["ms"]
            row["streamed_over_lds"] = row["streamed_ms"] / row["lds_ms"]
            print(json.dumps(row))
            sys.stdout.flush()
    return True


def bench_rows():
    for K, P, S in ((112, 128, 64), (1024, 16, 16)):
        row = {"call": "rows", "K": K, "P": P, "S": S}
        for M in (4, 8, 16):
            r, _, _ = call_row(K, P, S, M, M, 0, check=False)
            row[f"m{M}_ms"] = r["ms"]
        print(json.dumps(row))
        sys.stdout.flush()
    return True


class NumpyPropagator:
    """the parent commit's only route to the same numbers: `w @ T` per problem on the host"""
    seconds = 0.0

    def __init__(self, device):
        pass

    def __call__(self, t, mat_of, ks, w0, obs, n_steps, want_last=False):
        t0 = time.perf_counter()
        P, M, _ = w0.shape
        out = np.empty((P, n_steps + 1, M, obs.shape[1]))
        for p in range(P):
            K = int(ks[p])
            out[p] = numpy_chain(t[int(mat_of[p])].reshape(-1)[:K * K].reshape(K, K), w0[p, :, :K], obs[p, :, :K], n_steps)
        NumpyPropagator.seconds += time.perf_counter() - t0
        return out, None, np.zeros(P, np.int32)


class TimedDevicePropagator(evaluate._DevicePropagator):
    seconds = 0.0

    def __call__(self, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = super().__call__(*args, **kw)
        TimedDevicePropagator.seconds += time.perf_counter() - t0
        return r


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
    sets = evaluate.metastable_sets(evaluate.MarkovStateModel(LAG).fit(labels, lengths, K), 3)
    run = lambda B=Bn: evaluate.chapman_kolmogorov(labels, LAG, sets, (1, 2, 3, 4, 5), lengths, K, n_resamples=B, seed=1)   # noqa: E731
    device_route = evaluate.propagator
    res = {}
    for name, cls in (("device", TimedDevicePropagator), ("numpy", NumpyPropagator)):
        evaluate.propagator = cls
        try:
            run(2)                                                   # warm
            best, share, ck = float("inf"), 0.0, None
            for _ in range(3):
                cls.seconds = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ck = run()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt < best:
                    best, share = dt, cls.seconds
            res[name] = (best, share, ck)
        finally:
            evaluate.propagator = device_route
    a, b = res["device"][2], res["numpy"][2]
    fin = np.isfinite(a.predicted_resamples) & np.isfinite(b.predicted_resamples)
    agree = float(np.abs(a.predicted_resamples[fin] - b.predicted_resamples[fin]).max())
    print(json.dumps({"call": "end2end", "K": K, "B": Bn, "frames": int(paths.size), "lag": LAG, "multiples": [1, 2, 3, 4, 5],
                      "sets": [len(s) for s in sets], "chapman_kolmogorov_device_s": res["device"][0],
                      "chapman_kolmogorov_numpy_s": res["numpy"][0], "numpy_over_device": res["numpy"][0] / res["device"][0],
                      "propagation_device_s": res["device"][1], "propagation_numpy_s": res["numpy"][1],
                      "max_abs_diff_predicted": agree, "ck_max_abs_diff": a.max_abs_diff, "share_inside": a.share_inside}))
    return agree < 1e-12


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    what = sys.argv[1:] or ["call", "sweep", "rows", "end2end"]
    ok = True
    for name, fn in (("call", bench_call), ("sweep", bench_sweep), ("rows", bench_rows), ("end2end", bench_end2end)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
