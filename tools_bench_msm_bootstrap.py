#!/usr/bin/env python3
"""Timing of the bootstrap calls (dff_micro_resampled_counts, dff_msm_reversible_steps_batched) and of evaluate.bootstrap_msm,
by the protocol of tools_bench_msm.py (HIP events, the minimum of five windows of 20 calls, max / min spread shown).  One JSON
line per case.  Every baseline is the route that existed before these calls, never the new code.

sweeps   microseconds per sweep of B problems of K states, K in {8, 64, 256, 1024} x B in {16, 128}, from calls of 50 sweeps:
         the batched call on both drivers (one launch per sweep, one looping workgroup per problem) and the library's choice,
         against B consecutive dff_msm_reversible_steps calls (the library's choice of driver there); divisions per second
         (B K^2 per sweep).  x and err of the batched call are checked to be the single calls' bits.
counts   milliseconds for B weighted count matrices, n in {100 000, 819 200} x K in {64, 256, 1024} x B in {16, 128}, units =
         80 trajectories and units = blocks of 1 000 frames, against B calls of dff_micro_transition_counts on label arrays
         gathered per resample with torch (index_select of the drawn units' frames; the gather is timed with them, as the
         old route needs it).  The baseline counts the pairs INSIDE each drawn unit, so it loses the pairs that cross a block
         boundary: it is not the same estimator for blocks, only the nearest thing the old calls could do.  With trajectories
         as units the two agree, and that is checked.
end2end  bootstrap_msm at K = 200, B = 100 on the three-well process of tests/test_msm.py (40 trajectories x 2 000 frames, lag
         10), wall time, with the host shares (largest_connected_set, compaction, eigvalsh) timed separately, against B
         MarkovStateModel.fit_counts + timescales calls on the same resampled counts.
crossover  both drivers of the batched call over K in {33 .. 1024} x B in {1 .. 512} (not run by default): what the library's
         choice between them rests on.
`python tools_bench_msm_bootstrap.py [sweeps] [counts] [end2end] [crossover]` runs the named parts (the first three by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate
from tools_bench_msm import timed          # the protocol: HIP events, the minimum of five windows, max / min spread

SWEEPS = 50
SWEEP_STATES = (8, 64, 256, 1024)
BATCHES = (16, 128)
POINTS = (100000, 819200)
COUNT_STATES = (64, 256, 1024)
TRAJECTORIES = 80
BLOCK = 1000
LAG = 10


def counts_problem(K, seed):
    rng = np.random.default_rng(seed)
    Cm = np.zeros((K, K))
    idx = np.arange(K)
    Cm[idx, (idx + 1) % K] = rng.integers(1, 20, K)
    m = K * K // 8
    Cm[rng.integers(0, K, m), rng.integers(0, K, m)] += rng.integers(1, 20, m)
    Cm[idx, idx] = rng.integers(100, 2000, K)
    return Cm + Cm.T, Cm.sum(axis=1)


def bench_sweeps():
    ok = True
    for K in SWEEP_STATES:
        for Bn in BATCHES:
            probs = [counts_problem(K, 1000 * K + b) for b in range(Bn)]
            S = torch.from_numpy(np.stack([s for s, _ in probs])).cuda()
            c = torch.from_numpy(np.stack([v for _, v in probs])).cuda()
            x0 = 0.5 * S.sum(2)
            ks = np.full(Bn, K, np.int32)
            ws = torch.empty(binding.msm_batched_workspace_bytes(Bn, K), dtype=torch.uint8, device="cuda")
            ws1 = torch.empty(binding.msm_workspace_bytes(K), dtype=torch.uint8, device="cuda")
            row = {"call": "sweeps", "K": K, "B": Bn, "sweeps_per_call": SWEEPS, "S_MB": S.numel() * 8 / 2 ** 20,
                   "single_driver": binding.msm_driver_for(K)}
            xs = x0.clone()
            errs = [binding.msm_reversible_steps(S[b], c[b], xs[b], SWEEPS, workspace=ws1) for b in range(Bn)]
            want_x, want_err = xs.cpu(), torch.stack(errs, 1).cpu()

            def singles():
                for b in range(Bn):
                    binding.msm_reversible_steps(S[b], c[b], xs[b], SWEEPS, workspace=ws1)
            ms, spread = timed(singles, reps=2)
            row.update({"singles_us_per_sweep": ms * 1e3 / SWEEPS, "singles_spread": spread,
                        "singles_divisions_per_s": float(Bn) * K * K * SWEEPS / (ms * 1e-3)})
            for name, driver in (("auto", 0), ("launch_per_sweep", 1), ("one_workgroup_per_problem", 2)):
                binding.debug_msm_driver(driver)
                x = x0.clone()
                err = binding.msm_reversible_steps_batched(S, c, ks, x, SWEEPS, workspace=ws)
                same = torch.equal(x.cpu(), want_x) and torch.equal(err.cpu(), want_err)
                ok = ok and same
                ms, spread = timed(lambda: binding.msm_reversible_steps_batched(S, c, ks, x, SWEEPS, workspace=ws), reps=5)
                row.update({f"{name}_us_per_sweep": ms * 1e3 / SWEEPS, f"{name}_spread": spread, f"{name}_bits_equal": same,
                            f"{name}_divisions_per_s": float(Bn) * K * K * SWEEPS / (ms * 1e-3),
                            f"singles_over_{name}": row["singles_us_per_sweep"] / (ms * 1e3 / SWEEPS)})
            binding.debug_msm_driver(0)
            print(json.dumps(row))
            sys.stdout.flush()
    return ok


def bench_crossover():
    """both drivers of the batched call over K x B, without the baseline: what the library's choice between them rests on"""
    for K in (33, 64, 128, 256, 512, 1024):
        for Bn in (1, 2, 4, 8, 16, 32, 64, 128, 512):
            if Bn * K * K * 8 > 1 << 30:
                continue
            S1, c1 = counts_problem(K, K)
            S = torch.from_numpy(S1).cuda().repeat(Bn, 1, 1).contiguous()
            c = torch.from_numpy(c1).cuda().repeat(Bn, 1).contiguous()
            x = 0.5 * S.sum(2)
            ks = np.full(Bn, K, np.int32)
            ws = torch.empty(binding.msm_batched_workspace_bytes(Bn, K), dtype=torch.uint8, device="cuda")
            row = {"call": "crossover", "K": K, "B": Bn}
            for name, driver in (("launch_per_sweep", 1), ("one_workgroup_per_problem", 2)):
                binding.debug_msm_driver(driver)
                ms, spread = timed(lambda: binding.msm_reversible_steps_batched(S, c, ks, x, SWEEPS, workspace=ws), reps=5)
                row[f"{name}_us_per_sweep"] = ms * 1e3 / SWEEPS
            binding.debug_msm_driver(0)
            row["loop_over_launch"] = row["one_workgroup_per_problem_us_per_sweep"] / row["launch_per_sweep_us_per_sweep"]
            print(json.dumps(row))
            sys.stdout.flush()
    return True


def metastable(n, K, stay=0.98):
    jump = torch.rand(n, device="cuda") > stay
    idx = torch.where(jump, torch.arange(n, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"))
    last = torch.cummax(idx, 0).values
    return torch.randint(0, K, (n,), device="cuda")[last].to(torch.int32).contiguous()


def bench_counts():
    ok = True
    for n in POINTS:
        lengths = [n // TRAJECTORIES] * TRAJECTORIES
        for units_name, units in (("trajectories", np.asarray(lengths, np.int64)), ("blocks", evaluate.resampling_units(lengths, BLOCK))):
            starts = np.concatenate([[0], np.cumsum(units)[:-1]])
            for K in COUNT_STATES:
                labels = metastable(n, K)
                for Bn in BATCHES:
                    w = evaluate.bootstrap_weights(len(units), Bn, 1)
                    wd = torch.from_numpy(w).cuda()
                    ws = torch.empty(binding.micro_resampled_counts_workspace_bytes(len(lengths), len(units)), dtype=torch.uint8,
                                     device="cuda")
                    got = binding.micro_resampled_counts(labels, lengths, units, LAG, K, wd, workspace=ws)
                    ms, spread = timed(lambda: binding.micro_resampled_counts(labels, lengths, units, LAG, K, wd, workspace=ws), reps=5)
                    # the old route: per resample, gather the drawn units' frames (host index table built once, outside the
                    # timing) and count on them as trajectories of their own
                    drawn = [np.repeat(np.arange(len(units)), w[b]) for b in range(Bn)]
                    index = [torch.from_numpy(np.concatenate([np.arange(starts[u], starts[u] + units[u]) for u in d])).cuda() for d in drawn]
                    lens = [units[d].tolist() for d in drawn]

                    def old():
                        return [binding.micro_transition_counts(labels.index_select(0, index[b]), lens[b], [LAG], K) for b in range(Bn)]
                    ms0, spread0 = timed(old, reps=2)
                    row = {"call": "counts", "n": n, "K": K, "B": Bn, "units": units_name, "n_units": int(len(units)), "lag": LAG,
                           "resampled_ms": ms, "resampled_spread": spread, "gather_and_B_calls_ms": ms0, "baseline_spread": spread0,
                           "baseline_over_resampled": ms0 / ms, "weighted_pairs_per_s": float(got.sum().cpu()) / (ms * 1e-3),
                           "counters_MB": Bn * K * K * 8 / 2 ** 20}
                    if units_name == "trajectories":
                        same = torch.equal(torch.stack([r[0] for r in old()]), got.view(torch.int64))
                        ok = ok and same
                        row["counts_equal"] = same
                    print(json.dumps(row))
                    sys.stdout.flush()
    return ok


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

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    wall(lambda: evaluate.bootstrap_msm(labels, LAG, lengths, K, n_resamples=2, seed=1))              # warm
    bs, t_new = wall(lambda: evaluate.bootstrap_msm(labels, LAG, lengths, K, n_resamples=Bn, seed=1))
    counts = evaluate.resampled_counter(labels, np.asarray(lengths), bs.unit_lengths, LAG, K, torch.device("cuda:0"))(bs.weights)

    def old():
        ms = [evaluate.MarkovStateModel(LAG).fit_counts(Cb) for Cb in counts]
        return ms, [m.timescales(3) for m in ms]
    (models, _), t_old = wall(old)
    same = all(np.array_equal(m.timescales(3), bs.timescales[b], equal_nan=True) for b, m in enumerate(models))
    t0 = time.perf_counter()
    acts = [evaluate.largest_connected_set(Cb) for Cb in counts]
    t_sets = time.perf_counter() - t0
    t0 = time.perf_counter()
    for Cb, act in zip(counts, acts):
        Ca = np.array(Cb, np.float64)[np.ix_(act, act)]
        _ = Ca + Ca.T, Ca.sum(axis=1)
    t_compact = time.perf_counter() - t0
    t0 = time.perf_counter()
    for m in models:
        m.timescales(3)
    t_eig = time.perf_counter() - t0
    lo, hi = bs.interval(0.95)
    print(json.dumps({"call": "end2end", "K": K, "B": Bn, "frames": int(paths.size), "lag": LAG, "bootstrap_msm_s": t_new,
                      "B_fit_counts_s": t_old, "fit_counts_over_bootstrap": t_old / t_new, "same_timescales": same,
                      "host_connected_sets_s": t_sets, "host_compaction_s": t_compact, "host_eigvalsh_s": t_eig,
                      "sweeps_mean": float(bs.n_iter.mean()), "sweeps_max": int(bs.n_iter.max()), "n_failed": bs.n_failed,
                      "timescales": bs.point.timescales(3).tolist(), "lo": lo.tolist(), "hi": hi.tolist(), "std": bs.std().tolist()}))
    return same


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    what = sys.argv[1:] or ["sweeps", "counts", "end2end"]
    ok = True
    for name, fn in (("sweeps", bench_sweeps), ("counts", bench_counts), ("end2end", bench_end2end), ("crossover", bench_crossover)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
