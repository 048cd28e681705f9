#!/usr/bin/env python3
"""Timing of dff_hmm_estep and of HiddenMarkovModel.fit on top of it, by the protocol of tools_bench_msm_eig.py (HIP events, the
minimum of five windows, max / min spread shown).  One JSON line per case.  Every baseline is a route that existed before the
call, never the new code.

estep    one E-step: n in {100 000, 819 200} frames x m in {2, 4, 8} hidden states x K in {64, 1 024} symbols x (80 trajectories
         at lag 1, 80 trajectories at lag 10, ONE trajectory at lag 1).  Per row: milliseconds, frames / s, the fused
         multiply-adds n (m^3 + 3 m^2) per second (m^3: the chunk products; 3 m^2: forward, backward and xi of the apply pass)
         next to the 39.3e12 / s of the MI355X's fp64 vector units, the bytes moved (labels four times, the posteriors written
         and read, the emission partials written and read) next to the 8 TB/s of its HBM, the share of every launch (by stopping
         the call after 1 .. 5 launches: dff_debug_hmm_stages) and the workspace.  Baselines on the same inputs: a numpy
         sequential forward-backward on the host, timed on at most 20 000 frames and SCALED to n (it is linear in n), and a torch
         loop over the time steps on the device, vectorised over the chains, timed where it has at most 12 000 steps.  The
         log-likelihood is checked against the torch loop's.
end2end  HiddenMarkovModel.fit at K = 200, m = 4, 80 000 frames in 80 trajectories, lag 10: wall time, and its split into the
         E-steps' device time (events), their read-backs and the host M-step.
`python tools_bench_hmm.py [estep] [end2end] [--rows i,j,...] [--windows W]` runs the named parts (all by default)."""
import argparse
import json
import time

import numpy as np
import torch

import dff_amd  # noqa: F401
from dff_amd import binding, evaluate

PEAK_FMA, PEAK_BYTES = 39.3e12, 8.0e12
STAGES = ("parameters", "products", "carries", "apply", "emissions", "reductions")


def rows():
    out = []
    for n in (100_000, 819_200):
        for m in (2, 4, 8):
            for K in (64, 1024):
                for n_traj, lag in ((80, 1), (80, 10), (1, 1)):
                    out.append({"n": n, "m": m, "K": K, "n_traj": n_traj, "lag": lag})
    return out


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


def timed(fn, reps=5, windows=5):
    """(minimum in ms, max / min) over the windows"""
    t = [ev_time(fn, reps) for _ in range(windows)]
    return min(t) * 1e3, max(t) / min(t)


def model(m, K, seed=0):
    rng = np.random.default_rng(100 * m + K + seed)
    A = rng.uniform(0.01, 0.05, (m, m)) + np.diag(rng.uniform(0.8, 0.95, m))
    A /= A.sum(axis=1)[:, None]
    centre = (np.arange(m) + 0.5) * K / m                           # every hidden state emits around its own stretch of the symbols
    B = np.exp(-0.5 * ((np.arange(K)[None, :] - centre[:, None]) / (0.75 * K / m)) ** 2) + 1e-3
    B /= B.sum(axis=1)[:, None]
    return A, B, np.full(m, 1.0 / m)


def simulate(A, B, p0, n_traj, length, seed=1):
    """labels (n_traj * length,) int32 of the model's trajectories, all trajectories advanced together"""
    rng = np.random.default_rng(seed)
    cA, cB = np.cumsum(A, axis=1), np.cumsum(B, axis=1)
    m, K = B.shape
    h = np.minimum(np.searchsorted(np.cumsum(p0), rng.random(n_traj)), m - 1)
    out = np.empty((n_traj, length), np.int32)
    for t in range(length):
        out[:, t] = np.minimum((cB[h] < rng.random(n_traj)[:, None]).sum(axis=1), K - 1)
        h = np.minimum((cA[h] < rng.random(n_traj)[:, None]).sum(axis=1), m - 1)
    return out.reshape(-1)


def labels_of(n, m, K, n_traj):
    """n labels in n_traj equal trajectories: drawn from the model when that takes few steps, else uniform (the timing does not
    depend on the values)"""
    A, B, p0 = model(m, K)
    if n // n_traj <= 12_000:
        return simulate(A, B, p0, n_traj, n // n_traj)
    return np.random.default_rng(n).integers(0, K, n).astype(np.int32)


def numpy_forward_backward(labels, A, B, p0):
    """one chain, sequential, scaled: the host route -> log-likelihood"""
    L, m = len(labels), len(p0)
    al, c = np.empty((L, m)), np.empty(L)
    a = p0 * B[:, labels[0]]
    for t in range(L):
        if t:
            a = (a @ A) * B[:, labels[t]]
        c[t] = a.sum()
        a = a / c[t]
        al[t] = a
    be, xi, gs = np.ones(m), np.zeros((m, m)), np.zeros_like(B)
    for t in range(L - 1, -1, -1):
        g = al[t] * be
        gs[:, labels[t]] += g / g.sum()
        if t == 0:
            break
        w = B[:, labels[t]] * be
        x = al[t - 1][:, None] * A * w[None, :]
        xi += x / x.sum()
        be = A @ w / c[t]
    return float(np.log(c).sum())


def torch_forward_backward(lab, A, B, p0):
    """all chains at once (lab: (chains, L) int64 on the device), one loop over the time steps: the device route -> log-likelihood"""
    R, L = lab.shape
    m = A.shape[0]
    Bt = B.t().contiguous()
    al = torch.empty((L, R, m), dtype=torch.float64, device=lab.device)
    c = torch.empty((L, R), dtype=torch.float64, device=lab.device)
    a = p0[None, :] * Bt[lab[:, 0]]
    for t in range(L):
        if t:
            a = (a @ A) * Bt[lab[:, t]]
        c[t] = a.sum(dim=1)
        a = a / c[t][:, None]
        al[t] = a
    be = torch.ones((R, m), dtype=torch.float64, device=lab.device)
    xi = torch.zeros((m, m), dtype=torch.float64, device=lab.device)
    gs = torch.zeros_like(Bt)
    for t in range(L - 1, -1, -1):
        g = al[t] * be
        gs.index_add_(0, lab[:, t], g / g.sum(dim=1, keepdim=True))
        if t == 0:
            break
        w = Bt[lab[:, t]] * be
        x = al[t - 1][:, :, None] * A[None] * w[:, None, :]
        xi += (x / x.sum(dim=(1, 2), keepdim=True)).sum(dim=0)
        be = (w @ A.t()) / c[t][:, None]
    return float(torch.log(c).sum())


def estep_row(r, windows, baselines=True):
    n, m, K, n_traj, lag = r["n"], r["m"], r["K"], r["n_traj"], r["lag"]
    A, B, p0 = model(m, K)
    labels = labels_of(n, m, K, n_traj)
    lengths = [n // n_traj] * n_traj
    lab = torch.from_numpy(labels).cuda()
    par = [torch.from_numpy(x).cuda() for x in (A, B, p0)]
    need = binding.hmm_workspace_bytes(n, lengths, lag, m, K)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    call = lambda: binding.hmm_estep(lab, lengths, lag, *par, chain_loglik=False, post=False, workspace=ws)      # noqa: E731
    res = call()
    status = int(res["status"].cpu())
    loglik = float(res["stats"][0].cpu())
    reps = 3 if n > 200_000 else 10
    ms, spread = timed(call, reps, windows)
    cum = []
    try:
        for s in range(1, 6):
            binding.debug_hmm_stages(s)
            cum.append(timed(call, reps, 3)[0])
    finally:
        binding.debug_hmm_stages(0)
    cum.append(ms)
    share = {name: max(cum[i] - (cum[i - 1] if i else 0.0), 0.0) / ms for i, name in enumerate(STAGES)}
    sec = ms * 1e-3
    n_chains, n_chunks = binding.hmm_plan(lengths, lag)
    fma = n * (m ** 3 + 3 * m * m)
    moved = 16 * n + 16 * n * m + 16 * ((n + 1023) // 1024) * K * m
    row = dict(r, chunk=binding.hmm_chunk(), chains=n_chains, chunks=n_chunks, ms=ms, spread=spread, frames_per_s=n / sec,
               gfma_per_s=fma / sec / 1e9, share_of_fp64_peak=fma / sec / PEAK_FMA, gbytes_per_s=moved / sec / 1e9,
               share_of_hbm_peak=moved / sec / PEAK_BYTES, share=share, workspace_mb=need / 2 ** 20, status=status)
    if not baselines:
        return row, status == 0
    # the host route: one chain of at most 20 000 frames, scaled to n
    sub = labels[:min(n // n_traj, 20_000):1]
    t0 = time.perf_counter()
    numpy_forward_backward(sub, A, B, p0)
    row["numpy_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * n / len(sub)
    row["numpy_frames_timed"] = len(sub)
    # the device route: a torch loop over the steps of all chains
    steps = -(-(n // n_traj) // lag)
    row["torch_ms"] = None
    if steps <= 12_000 and (n // n_traj) % lag == 0:
        chains = torch.from_numpy(labels.reshape(n_traj, steps, lag)).cuda().permute(0, 2, 1).reshape(n_traj * lag, steps).long()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll = torch_forward_backward(chains, *par)
        torch.cuda.synchronize()
        row["torch_ms"] = (time.perf_counter() - t0) * 1e3
        row["loglik_rel_diff_to_torch"] = abs(loglik - ll) / abs(ll)
    row["speedup_over_numpy"] = row["numpy_ms_scaled"] / ms
    row["speedup_over_torch"] = row["torch_ms"] / ms if row["torch_ms"] else None
    ok = status == 0 and row.get("loglik_rel_diff_to_torch", 0.0) < 1e-10
    return row, ok


def end2end():
    m, K, n_traj, length, lag = 4, 200, 80, 1000, 10
    A, B, p0 = model(m, K)
    labels = simulate(A, B, p0, n_traj, length)
    lengths = [length] * n_traj
    spent = {"estep_wall": 0.0, "m_step": 0.0, "calls": 0}
    device_estep = evaluate._DeviceHmmEstep.__call__
    m_step = evaluate.HiddenMarkovModel._m_step

    def timed_estep(self, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = device_estep(self, *a, **k)
        spent["estep_wall"] += time.perf_counter() - t0
        spent["calls"] += 1
        return out

    def timed_m_step(self, *a, **k):
        t0 = time.perf_counter()
        out = m_step(self, *a, **k)
        spent["m_step"] += time.perf_counter() - t0
        return out
    evaluate._DeviceHmmEstep.__call__, evaluate.HiddenMarkovModel._m_step = timed_estep, timed_m_step
    try:
        evaluate.HiddenMarkovModel(m, lag).fit(labels, lengths, K)                                   # warm: kernels loaded
        spent.update(estep_wall=0.0, m_step=0.0, calls=0)
        t0 = time.perf_counter()
        h = evaluate.HiddenMarkovModel(m, lag).fit(labels, lengths, K)
        wall = time.perf_counter() - t0
    finally:
        evaluate._DeviceHmmEstep.__call__, evaluate.HiddenMarkovModel._m_step = device_estep, m_step
    lab = torch.from_numpy(labels).cuda()
    par = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (h.transition_matrix, h.observation_probabilities, h.initial_distribution)]
    ws = torch.zeros(binding.hmm_workspace_bytes(len(labels), lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    dev_ms, _ = timed(lambda: binding.hmm_estep(lab, lengths, lag, *par, chain_loglik=False, post=False, workspace=ws), 10)
    device = dev_ms * 1e-3 * spent["calls"]
    return {"part": "end2end", "K": K, "m": m, "frames": len(labels), "lag": lag, "n_iter": h.n_iter, "converged": bool(h.converged),
            "wall_ms": wall * 1e3, "estep_device_ms": device * 1e3, "estep_upload_and_readback_ms": (spent["estep_wall"] - device) * 1e3,
            "m_step_host_ms": spent["m_step"] * 1e3, "initial_model_and_rest_ms": (wall - spent["estep_wall"] - spent["m_step"]) * 1e3,
            "timescales": [float(v) for v in h.timescales()]}


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parts", nargs="*", choices=["estep", "end2end", []], help="the parts to run (all by default)")
    ap.add_argument("--rows", type=lambda s: [int(v) for v in s.split(",")], default=None, help="indices into the estep rows")
    ap.add_argument("--windows", type=int, default=5)
    return ap


def main():
    a = build_parser().parse_args()
    parts = a.parts or ["estep", "end2end"]
    ok = True
    if "estep" in parts:
        all_rows = rows()
        for i in (a.rows if a.rows is not None else range(len(all_rows))):
            row, good = estep_row(all_rows[i], a.windows)
            ok = ok and good
            print(json.dumps(dict(row, part="estep", row=i)), flush=True)
    if "end2end" in parts:
        print(json.dumps(end2end()), flush=True)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
