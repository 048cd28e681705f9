#!/usr/bin/env python3
"""Timing of Baum-Welch on the device (dff_hmm_fit_steps, HiddenMarkovModel(m_step="device"), bootstrap_hmm) against the host
M-step route, HiddenMarkovModel(m_step="host"), which is timed in the same run: wall time of whole fits, HIP events for the
share of the M-step launch (the protocol of tools_bench_hmm.py).  One JSON line per row.

The case is tools_bench_hmm.py's end-to-end one: K = 200 symbols, m = 4 hidden states, 80 000 frames in 80 trajectories, lag 10,
max_iter = 1 000, accuracy 1e-3, reversible -- once on that tool's weakly metastable model and once on a strongly metastable one
(diagonal 0.999 at the lag), where the serial sweeps of the reversible estimator dominate the M-step.
fit        m_step="host", then m_step="device" with steps_per_sync in {1, 8, 32, 128}: wall ms (the minimum of --windows fits after
           a warm-up fit), E-steps, sweeps per M-step (rev_sweeps / n_iter), the ratio to the host route.  The host route is
           left out on the strongly metastable model.
share      32 steps of dff_hmm_fit_steps from the fitted parameters against 32 dff_hmm_estep calls on them, by HIP events: the
           share of the control + M-step launch in a step.
bootstrap  bootstrap_hmm with --resamples resamples (100) from the fitted point model: wall ms, ms per resample, E-steps per
           resample, and the host route's warm-started refit of the first three resamples for comparison.
spread     the same fit on --datasets independently simulated datasets of the weakly metastable model (20): the standard deviation
           of the timescales and of the sorted populations over them, to put next to the bootstrap's.
The strongly metastable model runs --strong-max-iter iterations at the most (200): an M-step there takes milliseconds.
`python tools_bench_hmm_fit.py [--parts fit share bootstrap spread] [--datasets D] [--resamples B] [--windows W] [--max-iter N] [--strong-max-iter N]`."""
import argparse
import json
import time

import numpy as np
import torch

import dff_amd  # noqa: F401
import tools_bench_hmm as base
from dff_amd import binding, evaluate

CASE = dict(K=200, m=4, n_traj=80, length=1000, lag=10, max_iter=1000)
STEPS_PER_SYNC = (1, 8, 32, 128)
DIAGONALS = (None, 0.999)                                           # None: the model of tools_bench_hmm.py; else A's diagonal at the lag


def case_labels(diagonal, seed=1):
    """(labels, lengths) of the case; diagonal: that of the hidden transition matrix AT THE LAG (per frame: its lag-th root)"""
    m, K = CASE["m"], CASE["K"]
    A, B, p0 = base.model(m, K)
    if diagonal is not None:
        d = diagonal ** (1.0 / CASE["lag"])
        A = np.full((m, m), (1.0 - d) / (m - 1))
        np.fill_diagonal(A, d)
    return base.simulate(A, B, p0, CASE["n_traj"], CASE["length"], seed=seed), [CASE["length"]] * CASE["n_traj"]


def wall(fn, windows):
    fn()                                                            # warm: kernels loaded, allocator filled
    best, out = float("inf"), None
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def model_of(m_step, max_iter, steps_per_sync=32):
    return evaluate.HiddenMarkovModel(CASE["m"], CASE["lag"], max_iter=max_iter, m_step=m_step, steps_per_sync=steps_per_sync)


def fit_rows(diagonal, windows, max_iter):
    labels, lengths = case_labels(diagonal)
    lab = torch.from_numpy(labels).cuda()
    initial = evaluate.initial_hmm(lab, CASE["lag"], CASE["m"], lengths, CASE["K"])
    rows, host_ms = [], None
    if diagonal is None:
        host_ms, h = wall(lambda: model_of("host", max_iter).fit(lab, lengths, CASE["K"], initial=initial), windows)
        rows.append({"m_step": "host", "wall_ms": host_ms, "n_iter": h.n_iter, "converged": bool(h.converged)})
    for sps in STEPS_PER_SYNC:
        ms, d = wall(lambda: model_of("device", max_iter, sps).fit(lab, lengths, CASE["K"], initial=initial), windows)
        rows.append({"m_step": "device", "steps_per_sync": sps, "wall_ms": ms, "n_iter": d.n_iter, "converged": bool(d.converged),
                     "sweeps_per_m_step": d.rev_sweeps / max(d.n_iter, 1), "rev_unconverged": d.rev_unconverged,
                     "host_over_device": host_ms / ms if host_ms else None, "timescales": [float(v) for v in d.timescales()]})
    return [dict(r, part="fit", diagonal=diagonal, max_iter=max_iter) for r in rows], (lab, lengths, d)


def share_row(diagonal, lab, lengths, fitted, steps=32):
    m, K, lag = CASE["m"], CASE["K"], CASE["lag"]
    host = [np.ascontiguousarray(x) for x in (fitted.transition_matrix, fitted.observation_probabilities, fitted.initial_distribution)]
    ws = torch.zeros(binding.hmm_fit_workspace_bytes(lab.numel(), lengths, lag, m, K), dtype=torch.uint8, device="cuda")
    par = [torch.from_numpy(x).cuda() for x in host]
    estep_ms, _ = base.timed(lambda: binding.hmm_estep(lab, lengths, lag, *par, chain_loglik=False, post=False, workspace=ws), steps)
    state = torch.zeros(8, dtype=torch.int32, device="cuda")

    def run():
        for t, x in zip(par, host):
            t.copy_(torch.from_numpy(x))
        state.zero_()
        binding.hmm_fit_steps(lab, lengths, lag, *par, True, steps, 1e-300, state=state, workspace=ws)
    run()
    st0 = binding.hmm_fit_state_dict(state.cpu().numpy())
    ms, spread = base.timed(run, 1)
    step_ms = ms / steps
    return {"part": "share", "diagonal": diagonal, "estep_ms": estep_ms, "fit_step_ms": step_ms, "spread": spread,
            "m_step_launch_ms": step_ms - estep_ms, "m_step_share": 1.0 - estep_ms / step_ms, "sweeps_per_m_step": st0["rev_sweeps"] / steps,
            "us_per_sweep": (step_ms - estep_ms) * 1e3 / max(st0["rev_sweeps"] / steps, 1.0)}


def bootstrap_row(diagonal, lab, lengths, fitted, resamples, max_iter):
    kw = dict(n_resamples=resamples, seed=0, max_iter=max_iter, point=fitted)
    evaluate.bootstrap_hmm(lab, CASE["lag"], CASE["m"], lengths, CASE["K"], **dict(kw, n_resamples=2))             # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bs = evaluate.bootstrap_hmm(lab, CASE["lag"], CASE["m"], lengths, CASE["K"], **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    start = (fitted.transition_matrix, fitted.observation_probabilities, fitted.initial_distribution)
    host_ms, host_iter = [], []
    for b in range(min(3, resamples)):
        lab_b, len_b = evaluate.resampled_labels(lab, bs.unit_lengths, bs.weights[b])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = model_of("host", max_iter).fit(lab_b, len_b, CASE["K"], initial=start, renumber=False)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        host_iter.append(h.n_iter)
    return {"part": "bootstrap", "diagonal": diagonal, "resamples": resamples, "wall_ms": ms, "ms_per_resample": ms / resamples,
            "n_iter_mean": float(bs.n_iter.mean()), "n_failed": bs.n_failed, "converged": int(bs.converged.sum()),
            "host_refit_ms_mean_of_3": float(np.mean(host_ms)), "host_refit_n_iter": host_iter,
            "host_over_device_per_resample": float(np.mean(host_ms)) / (ms / resamples),
            "point_timescales": [float(v) for v in fitted.timescales()], "timescales_std": [float(v) for v in bs.std("timescales")],
            "lifetimes_std": [float(v) for v in bs.std("lifetimes")], "stationary_std": [float(v) for v in bs.std("stationary")]}


def spread_row(datasets, max_iter):
    ts, pops, iters = [], [], []
    for seed in range(100, 100 + datasets):
        labels, lengths = case_labels(None, seed=seed)
        h = model_of("device", max_iter).fit(torch.from_numpy(labels).cuda(), lengths, CASE["K"])
        ts.append(h.timescales())
        pops.append(h.stationary_distribution)                      # largest first
        iters.append(h.n_iter)
    ts, pops = np.array(ts), np.array(pops)
    return {"part": "spread", "datasets": datasets, "timescales_mean": [float(v) for v in ts.mean(axis=0)],
            "timescales_std": [float(v) for v in ts.std(axis=0, ddof=1)], "sorted_populations_std": [float(v) for v in pops.std(axis=0, ddof=1)],
            "n_iter_mean": float(np.mean(iters))}


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", choices=["fit", "share", "bootstrap", "spread"], default=["fit", "share", "bootstrap", "spread"])
    ap.add_argument("--datasets", type=int, default=20)
    ap.add_argument("--resamples", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=CASE["max_iter"])
    ap.add_argument("--strong-max-iter", type=int, default=200)
    return ap


def main():
    a = build_parser().parse_args()
    if a.parts == ["spread"]:
        print(json.dumps(spread_row(a.datasets, a.max_iter)), flush=True)
        return
    for diagonal in DIAGONALS:
        max_iter = a.max_iter if diagonal is None else min(a.max_iter, a.strong_max_iter)
        rows, (lab, lengths, fitted) = fit_rows(diagonal, a.windows, max_iter)
        if "fit" in a.parts:
            for r in rows:
                print(json.dumps(r), flush=True)
        if "share" in a.parts:
            print(json.dumps(share_row(diagonal, lab, lengths, fitted)), flush=True)
        if "bootstrap" in a.parts and diagonal is None:
            print(json.dumps(bootstrap_row(diagonal, lab, lengths, fitted, a.resamples, max_iter)), flush=True)
        if "spread" in a.parts and diagonal is None:
            print(json.dumps(spread_row(a.datasets, max_iter)), flush=True)


if __name__ == "__main__":
    main()
