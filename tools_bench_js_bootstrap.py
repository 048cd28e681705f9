#!/usr/bin/env python3
"""Timing of the Jensen-Shannon bootstrap calls (dff_unit_hist, dff_resampled_js) by the protocol of tools_bench_msm.py (HIP
events, the minimum of five windows, max / min spread shown).  One JSON line per case.  Every baseline is a route that existed
before these calls, never the new code.

score    milliseconds for the JS of B resamples x C channels from the units' histograms, on three shapes -- 10 beads / 55 pairs
         and 35 beads / 630 pairs with the bins of 0.1 Angstrom PWD histograms (pair (i, j) reaches 3.8 |i - j| + 8 Angstrom), and
         one 100 x 100 grid -- with U in {64, 256, 1024} units and B in {100, 1000} resamples, against
           matmul   the only previous device route: weights.double() @ hist.double() and the JS in torch, which writes all
                    B C ld resampled histograms to memory as doubles (hist is converted outside the timing);
           numpy    the host loop: one integer matmul per channel and evaluate.js_divergence per (b, c) (one window of one
                    call; at B = 100 only, and not for 630 pairs at U = 1024).
         The kernel's result is checked against the matmul route (|d| <= 1e-12) and its totals to be exact.
hist     milliseconds for the units' histograms of n = 200 000 frames in U = 256 units: the 100 x 100 grid (one channel) and 55
         channels of PWD-sized bins, against torch.bincount on a flattened (unit, channel, bin) index.
`python tools_bench_js_bootstrap.py [score] [hist]` runs the named parts (both by default)."""
import json
import sys
import time

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate

REPEATS = 5
UNITS = (64, 256, 1024)
RESAMPLES = (100, 1000)


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


def timed(fn, reps=10):
    """(minimum in ms, max / min) over REPEATS windows"""
    t = [ev_time(fn, reps) for _ in range(REPEATS)]
    return min(t) * 1e3, max(t) / min(t)


def pwd_bins(n_beads):
    i, j = np.triu_indices(n_beads, 0)
    return (np.floor((3.8 * np.abs(i - j) + 8.0) / 0.1) + 1).astype(np.int32)


def shapes():
    return (("10 beads / 55 pairs", pwd_bins(10)), ("35 beads / 630 pairs", pwd_bins(35)), ("100 x 100 grid", np.array([10000], np.int32)))


def binned(n, nbins, seed):
    """int32 CUDA (n, C): a Gaussian blob of indices around the middle of every channel, 2 % outside"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nb = torch.from_numpy(nbins).cuda().double()
    z = torch.randn((n, len(nbins)), generator=g, device="cuda", dtype=torch.float64)
    idx = torch.floor(nb * (0.5 + 0.2 * z)).to(torch.int32)
    return torch.where((idx >= 0) & (idx < nb.to(torch.int32)), idx, torch.full_like(idx, -1)).contiguous()


def unit_histograms(U, nbins, seed, frames_per_unit=400):
    units = np.full(U, frames_per_unit, np.int64)
    return binding.unit_hist(binned(int(units.sum()), nbins, seed), units, nbins)


def torch_js(wd, hd, ref, mask, shape):
    """the previous device route: (B, U) @ (U, C ld) in fp64, then the JS of every row in torch"""
    H = (wd @ hd).view(shape)
    p = H / H.sum(2, keepdim=True) + 1e-10
    q = (ref / ref.sum(1, keepdim=True))[None] + 1e-10
    m = (p + q) / 2
    return 0.5 * ((p * torch.log(p / m) + q * torch.log(q / m)) * mask).sum(2)


def numpy_js(hist, nbins, w, ref):
    out = np.empty((len(w), len(nbins)))
    for c, nb in enumerate(nbins):
        h = w.astype(np.int64) @ hist[:, c, :nb].astype(np.int64)
        for b in range(len(w)):
            out[b, c] = evaluate.js_divergence(h[b].astype(np.float64), ref[c, :nb])
    return out


def bench_score():
    ok = True
    for name, nbins in shapes():
        C, ld = len(nbins), int(nbins.max())
        for U in UNITS:
            hist = unit_histograms(U, nbins, 7)
            ref = unit_histograms(1, nbins, 8, 20000)[0].double().contiguous() + 0.5
            mask = (torch.arange(ld, device="cuda")[None] < torch.from_numpy(nbins).cuda()[:, None]).double()
            ref = ref * mask
            hd = hist.double().view(U, C * ld)
            ws = torch.empty(binding.resampled_js_workspace_bytes(U, C), dtype=torch.uint8, device="cuda")
            for Bn in RESAMPLES:
                w = evaluate.bootstrap_weights(U, Bn, 1)
                wu = torch.from_numpy(w).cuda()
                wd = wu.double()
                js, tot = binding.resampled_js(hist, nbins, wu, ref, workspace=ws)
                ms, spread = timed(lambda: binding.resampled_js(hist, nbins, wu, ref, workspace=ws))
                want = torch_js(wd, hd, ref, mask, (Bn, C, ld))
                err = float((js - want).abs().max())
                exact = bool(torch.equal(tot.view(torch.int64), (wd @ hd).view(Bn, C, ld).sum(2).to(torch.int64)))
                ms0, spread0 = timed(lambda: torch_js(wd, hd, ref, mask, (Bn, C, ld)), reps=3)
                madds = float(Bn) * U * int(nbins.sum())
                row = {"call": "score", "shape": name, "C": C, "ld": ld, "bins": int(nbins.sum()), "U": U, "B": Bn,
                       "tile": binding.resampled_js_path_for(Bn, C), "resampled_js_ms": ms, "spread": spread,
                       "multiply_adds_per_s": madds / (ms * 1e-3), "hist_MB": U * C * ld * 4 / 2 ** 20,
                       "matmul_route_ms": ms0, "matmul_spread": spread0, "matmul_over_kernel": ms0 / ms,
                       "materialised_MB": Bn * C * ld * 8 / 2 ** 20, "max_abs_diff_to_matmul_route": err, "totals_exact": exact}
                ok = ok and err <= 1e-12 and exact
                if Bn == RESAMPLES[0] and not (C > 100 and U > 256):
                    hh, rh = hist.cpu().numpy(), ref.cpu().numpy()
                    t0 = time.perf_counter()
                    nj = numpy_js(hh, nbins, w, rh)
                    row["numpy_loop_ms"] = (time.perf_counter() - t0) * 1e3
                    row["numpy_over_kernel"] = row["numpy_loop_ms"] / ms
                    row["max_abs_diff_to_numpy"] = float(np.abs(nj - js.cpu().numpy()).max())
                print(json.dumps(row))
                sys.stdout.flush()
    return ok


def bench_hist(n=200000, U=256):
    ok = True
    units = evaluate.sample_units(n, n_blocks=U)
    for name, nbins in (shapes()[2], shapes()[0]):
        C, ld = len(nbins), int(nbins.max())
        bins = binned(n, nbins, 3)
        ws = torch.empty(binding.unit_hist_workspace_bytes(U, C), dtype=torch.uint8, device="cuda")
        got = binding.unit_hist(bins, units, nbins, workspace=ws)
        ms, spread = timed(lambda: binding.unit_hist(bins, units, nbins, workspace=ws))
        unit_of = torch.repeat_interleave(torch.arange(U, device="cuda"), torch.from_numpy(units).cuda())

        def old():
            flat = ((unit_of[:, None] * C + torch.arange(C, device="cuda")[None]) * ld + bins).reshape(-1)
            return torch.bincount(flat[bins.reshape(-1) >= 0], minlength=U * C * ld).view(U, C, ld)
        same = bool(torch.equal(old(), got.to(torch.int64)))
        ms0, spread0 = timed(old, reps=3)
        ok = ok and same
        print(json.dumps({"call": "hist", "shape": name, "n": n, "C": C, "ld": ld, "U": U, "unit_hist_ms": ms, "spread": spread,
                          "indices_per_s": float(n) * C / (ms * 1e-3), "bincount_ms": ms0, "bincount_spread": spread0,
                          "bincount_over_kernel": ms0 / ms, "equal": same}))
        sys.stdout.flush()
    return ok


def main():
    dff_amd.load_library()
    what = sys.argv[1:] or ["score", "hist"]
    ok = True
    for name, fn in (("score", bench_score), ("hist", bench_hist)):
        if name in what:
            ok = fn() and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
