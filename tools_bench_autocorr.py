#!/usr/bin/env python3
"""Timing of dff_autocorr at the output sizes of BASELINE.json's configs, by the protocol of tools_bench_kinetics.py (HIP events,
the minimum of five windows of 20 calls, max / min spread shown): 10 240, 100 000, 819 200 and 409 600 frames in 80 equal
trajectories, d in {1, 2} components, max_lag in {256, 4096}.

Per case: the call with every output (sxy, sx, sy, count: four fp64 FMAs per pair and component, the count's once) and with
sxy alone (one), in ms, pair-products per second (sum over the lags of the pairs inside trajectories, times d) and fp64 FMAs
per second next to the public vector-fp64 peak of the MI355X (78.6 TFLOP/s = 39.3e12 FMA/s).
Next to it the only previous device route to an ACF: torch rfft / irfft per trajectory batch, zero-padded to twice the length
(Wiener-Khinchin).  That route gives sxy only, and handles neither non-finite frames nor unequal lengths.  It is checked
against the kernel on this finite, equal-length input to 1e-9 of C(0) before it is timed.  Prints one JSON line per case."""
import json
import sys

import torch

import dff_amd
from dff_amd import binding

PEAK_FMA = 39.3e12
FRAMES = (10240, 100000, 819200, 409600)
TRAJECTORIES = 80          # divides every n of FRAMES
REPEATS = 5


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


def timed(fn):
    """(minimum in ms, max / min) over REPEATS windows"""
    t = [ev_time(fn) for _ in range(REPEATS)]
    return min(t) * 1e3, max(t) / min(t)


def fft_sxy(g, T, L):
    """sum over the trajectories of the lagged products of g (n, d) = (P T, d), already shifted: (L + 1, d)"""
    x = g.view(-1, T, g.shape[1]).transpose(1, 2)                   # (P, d, T)
    f = torch.fft.rfft(x, n=2 * T, dim=-1)
    ac = torch.fft.irfft(f.real * f.real + f.imag * f.imag, n=2 * T, dim=-1)[..., :min(L, T - 1) + 1].sum(0).t()
    out = torch.zeros((L + 1, g.shape[1]), dtype=g.dtype, device=g.device)
    out[:ac.shape[0]] = ac
    return out


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    ok = True
    for n in FRAMES:
        T = n // TRAJECTORIES
        for d in (1, 2):
            # a series that relaxes over ~33 frames: a moving sum of white noise
            c = torch.cumsum(torch.randn((n, d), dtype=torch.float64, device="cuda"), 0)
            x = c.clone()
            x[33:] -= c[:-33]
            lengths = [T] * TRAJECTORIES
            shift = x.mean(0).contiguous()
            for L in (256, 4096):
                ws = torch.empty(binding.autocorr_workspace_bytes(n, d, L), dtype=torch.uint8, device="cuda")
                full = binding.autocorr(x, lengths, L, shift, workspace=ws)
                pairs = int(full["count"].sum().cpu())
                row = {"n": n, "d": d, "max_lag": L, "trajectories": TRAJECTORIES, "pairs": pairs, "workspace_MB": ws.numel() / 2 ** 20}
                ms, spread = timed(lambda: binding.autocorr(x, lengths, L, shift, workspace=ws))
                row.update({"autocorr_ms": ms, "autocorr_spread": spread, "pair_products_per_s": pairs * d / (ms * 1e-3),
                            "fma_per_s": pairs * (3 * d + 1) / (ms * 1e-3), "frac_fp64_peak": pairs * (3 * d + 1) / (ms * 1e-3) / PEAK_FMA})
                ms1, spread1 = timed(lambda: binding.autocorr(x, lengths, L, shift, sx=False, sy=False, count=False, workspace=ws))
                row.update({"sxy_only_ms": ms1, "sxy_only_spread": spread1, "sxy_only_pair_products_per_s": pairs * d / (ms1 * 1e-3),
                            "sxy_only_frac_fp64_peak": pairs * d / (ms1 * 1e-3) / PEAK_FMA})
                g = x - shift
                ref = fft_sxy(g, T, L)
                err = float(((ref - full["sxy"]).abs() / full["sxy"][:1]).max().cpu())
                fms, fspread = timed(lambda: fft_sxy(x - shift, T, L))
                row.update({"fft_ms": fms, "fft_spread": fspread, "fft_err_over_c0": err, "fft_equal": err <= 1e-9,
                            "sxy_only_over_fft": ms1 / fms, "autocorr_over_fft": ms / fms})
                print(json.dumps(row))
                sys.stdout.flush()
                ok = ok and err <= 1e-9
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
