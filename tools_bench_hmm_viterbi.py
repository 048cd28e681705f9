#!/usr/bin/env python3
"""Timing of dff_hmm_viterbi by the protocol of tools_bench_hmm.py (HIP events, the minimum of five windows, max / min spread
shown) on its grid, models and labels.  One JSON line per row.  Every baseline is a route that existed before the call.

n in {100 000, 819 200} frames x m in {2, 4, 8} hidden states x K in {64, 1 024} symbols x (80 trajectories at lag 1, 80
trajectories at lag 10, ONE trajectory at lag 1).  Per row: milliseconds, frames / s, the additions n (m^3 + 2 m^2) per second
(m^3: the chunk products; m^2 each: the apply pass and its compares), the bytes moved per call (the labels three times, one
back-pointer word per frame written and read, the path written: 24 n, plus per chunk the product written and read and the
carries) next to the 8 TB/s of the MI355X's HBM, the share of every launch (by stopping the call after 1 .. 6 launches:
dff_debug_hmm_viterbi_stages) and the workspace.  Baselines on the same inputs:
  (a) numpy sequential Viterbi on the host, timed on at most 20 000 frames of one chain and SCALED to n (it is linear in n);
  (b) a torch loop over the time steps on the device, vectorised over the chains, timed where it has at most 12 000 steps;
  (c) the route to a per-frame state series that existed: dff_hmm_estep with posteriors, then argmax.
The path is checked against (b) where (b) runs (its score, since ties may fall differently), and always against the log-probability
of its own path recomputed on the device.
`python tools_bench_hmm_viterbi.py [--rows i,j,...] [--windows W] [--no-baselines]`."""
import argparse
import json
import time

import numpy as np
import torch

import dff_amd  # noqa: F401
from dff_amd import binding
from tools_bench_hmm import PEAK_BYTES, labels_of, model, rows, timed

STAGES = ("parameters", "products", "forward carries", "apply", "backward carries", "backtrack", "finish")


def numpy_viterbi(labels, la, lb, lp):
    """one chain, sequential: the host route -> (path, log-probability)"""
    L, m = len(labels), len(lp)
    d = lp + lb[:, labels[0]]
    psi = np.zeros((L, m), np.int64)
    for t in range(1, L):
        x = d[:, None] + la
        psi[t] = x.argmax(axis=0)
        d = x.max(axis=0) + lb[:, labels[t]]
    path = np.empty(L, np.int32)
    s = int(d.argmax())
    for t in range(L - 1, -1, -1):
        path[t] = s
        s = psi[t, s]
    return path, float(d.max())


def torch_viterbi(lab, la, lb, lp):
    """all chains at once (lab: (chains, L) int64 on the device), one loop over the time steps: the device route ->
    (path (chains, L), log-probabilities (chains,))"""
    R, L = lab.shape
    lbt = lb.t().contiguous()
    d = lp[None, :] + lbt[lab[:, 0]]
    psi = torch.zeros((L, R, la.shape[0]), dtype=torch.int64, device=lab.device)
    for t in range(1, L):
        mx, psi[t] = (d[:, :, None] + la[None]).max(dim=1)
        d = mx + lbt[lab[:, t]]
    best, s = d.max(dim=1)
    path = torch.empty((L, R), dtype=torch.int64, device=lab.device)
    for t in range(L - 1, -1, -1):
        path[t] = s
        s = psi[t].gather(1, s[:, None])[:, 0]
    return path.t(), best


def path_scores(chains, path, la, lb, lp):
    """ln P(path, labels) of every chain on the device: chains, path (R, L) int64"""
    v = lp[path[:, 0]] + lb[path[:, 0], chains[:, 0]]
    if path.shape[1] > 1:
        v = v + (la[path[:, :-1], path[:, 1:]] + lb[path[:, 1:], chains[:, 1:]]).sum(dim=1)
    return v


def bench_row(r, windows, baselines=True):
    n, m, K, n_traj, lag = r["n"], r["m"], r["K"], r["n_traj"], r["lag"]
    A, B, p0 = model(m, K)
    labels = labels_of(n, m, K, n_traj)
    lengths = [n // n_traj] * n_traj
    lab = torch.from_numpy(labels).cuda()
    par = [torch.from_numpy(x).cuda() for x in (A, B, p0)]
    logs = [torch.log(x) for x in par]
    need = binding.hmm_viterbi_workspace_bytes(n, lengths, lag, m, K)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    call = lambda: binding.hmm_viterbi(lab, lengths, lag, *logs, chain_logprob=True, workspace=ws)      # noqa: E731
    res = call()
    status = int(res["status"].cpu())
    reps = 3 if n > 200_000 else 10
    ms, spread = timed(call, reps, windows)
    cum = []
    try:
        for s in range(1, 7):
            binding.debug_hmm_viterbi_stages(s)
            cum.append(timed(call, reps, 3)[0])
    finally:
        binding.debug_hmm_viterbi_stages(0)
    cum.append(ms)
    share = {name: max(cum[i] - (cum[i - 1] if i else 0.0), 0.0) / ms for i, name in enumerate(STAGES)}
    sec = ms * 1e-3
    n_chains, n_chunks = binding.hmm_plan(lengths, lag)
    MP = 2 if m <= 2 else (4 if m <= 4 else 8)
    adds = n * (m ** 3 + 2 * m * m)
    moved = 24 * n + n_chunks * (16 * MP * MP + 16 * MP + 16)
    row = dict(r, chunk=binding.hmm_chunk(), chains=n_chains, chunks=n_chunks, ms=ms, spread=spread, frames_per_s=n / sec,
               gadds_per_s=adds / sec / 1e9, mbytes_moved=moved / 1e6, gbytes_per_s=moved / sec / 1e9,
               share_of_hbm_peak=moved / sec / PEAK_BYTES, share=share, workspace_mb=need / 2 ** 20, status=status)
    # the call's own log-probabilities against the score of its own path
    steps = -(-(n // n_traj) // lag)
    even = (n // n_traj) % lag == 0
    ok = status == 0
    if even:
        to_chains = lambda x: x.reshape(n_traj, steps, lag).permute(0, 2, 1).reshape(n_traj * lag, steps).long()     # noqa: E731
        chains = to_chains(lab)
        own = path_scores(chains, to_chains(res["path"]), *logs)
        row["logprob_rel_diff_to_own_path"] = float(((own - res["chain_logprob"]).abs() / res["chain_logprob"].abs()).max())
        ok = ok and row["logprob_rel_diff_to_own_path"] < 1e-10
    if not baselines:
        return row, ok
    # (a) the host route: one chain of at most 20 000 frames, scaled to n
    sub = labels[:min(n // n_traj, 20_000)]
    host = [np.log(x) for x in (A, B, p0)]
    t0 = time.perf_counter()
    numpy_viterbi(sub, *host)
    row["numpy_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * n / len(sub)
    row["numpy_frames_timed"] = len(sub)
    # (b) the device route: a torch loop over the steps of all chains
    row["torch_ms"] = None
    if steps <= 12_000 and even:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, best = torch_viterbi(chains, *logs)
        torch.cuda.synchronize()
        row["torch_ms"] = (time.perf_counter() - t0) * 1e3
        row["logprob_rel_diff_to_torch"] = float(((best - res["chain_logprob"]).abs() / best.abs()).max())
        ok = ok and row["logprob_rel_diff_to_torch"] < 1e-10
    # (c) the existing route to a state series: the E-step with posteriors, then argmax
    ews = torch.zeros(binding.hmm_workspace_bytes(n, lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    post = torch.empty((n, m), dtype=torch.float64, device="cuda")
    estep = lambda: torch.argmax(binding.hmm_estep(lab, lengths, lag, *par, chain_loglik=False, post=post, workspace=ews)["post"], dim=1)     # noqa: E731
    row["estep_argmax_ms"] = timed(estep, reps, 3)[0]
    row["speedup_over_numpy"] = row["numpy_ms_scaled"] / ms
    row["speedup_over_torch"] = row["torch_ms"] / ms if row["torch_ms"] else None
    row["speedup_over_estep_argmax"] = row["estep_argmax_ms"] / ms
    return row, ok


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=lambda s: [int(v) for v in s.split(",")], default=None, help="indices into the rows")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true", help="time the call alone (the chunk-length sweep)")
    return ap


def main():
    a = build_parser().parse_args()
    ok = True
    all_rows = rows()
    for i in (a.rows if a.rows is not None else range(len(all_rows))):
        row, good = bench_row(all_rows[i], a.windows, not a.no_baselines)
        ok = ok and good
        print(json.dumps(dict(row, part="viterbi", row=i)), flush=True)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
