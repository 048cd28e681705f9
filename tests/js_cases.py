"""The fp64 numpy oracle of the Jensen-Shannon bootstrap kernels (dff_unit_hist, dff_resampled_js) and the cases its two test
files share: per-unit histograms by np.bincount, the resampled JS written with evaluate.js_divergence on float64, and the
seeded case generator.  Not a test; imported by tests/test_js_bootstrap_host.py and tests/test_js_bootstrap.py."""
import functools

import numpy as np

from dff_amd import evaluate

# the bins-per-channel rows of the resample-and-score grid: drawn from {1, 2, 63, 64, 65, 1025, 30719}, C in {1, 5}
NBINS_ROWS = ((1,), (64,), (30719,), (1, 2, 63, 64, 65), (65, 1025, 2, 30719, 64))
UNITS = (1, 3, 70, 300)
RESAMPLES = (1, 7, 130)
JS_ATOL = 1e-13        # |kernel - oracle| per (b, c): sum |terms| <= ~2, a few ulp per term, <= 16 ulp from the fixed-order tree
                       # over <= 2 * 30719 terms -> ~6e-15; the bar leaves ~18 x


def unit_hists(bins, nbins, units, ld=None):
    """uint32 (U, C, ld): hist[u, c, k] = #{t in unit u: bins[t, c] == k}; an index < 0 or >= nbins[c] is not counted."""
    bins = np.asarray(bins).reshape(len(bins), -1)
    nbins = np.asarray(nbins, np.int64)
    ld = int(nbins.max()) if ld is None else ld
    out = np.zeros((len(units), bins.shape[1], ld), np.uint32)
    start = 0
    for u, ln in enumerate(units):
        for c, nb in enumerate(nbins):
            col = bins[start:start + ln, c]
            col = col[(col >= 0) & (col < nb)]
            out[u, c, :nb] = np.bincount(col, minlength=nb)
        start += ln
    return out


def resampled_hist(hist, weights, c, nb):
    """uint64 (B, nb): sum_u w[b, u] hist[u, c, :nb], exact"""
    h, w = hist[:, c, :nb], np.asarray(weights)
    if float(w.max(initial=0)) * float(h.sum(axis=0, dtype=np.float64).max(initial=0)) < 2.0 ** 53:     # every sum an exact integer
        return (w.astype(np.float64) @ h.astype(np.float64)).astype(np.uint64)
    out = np.zeros((len(w), nb), np.uint64)
    for u in range(h.shape[0]):
        out += w[:, u, None].astype(np.uint64) * h[u][None].astype(np.uint64)
    return out


def ref_ok(r):
    r = np.asarray(r, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = r.sum()
    return bool(np.isfinite(r).all() and (r >= 0).all() and np.isfinite(s) and s > 0)


def resampled_js(hist, nbins, weights, ref):
    """(js float64 (B, C), total uint64 (B, C)): evaluate.js_divergence of every resample's histogram and the reference's on
    float64; NaN where the resample holds no count or the reference channel cannot be normalised"""
    B, C = len(weights), len(nbins)
    js, tot = np.full((B, C), np.nan), np.zeros((B, C), np.uint64)
    for c, nb in enumerate(nbins):
        h = resampled_hist(hist, weights, c, int(nb))
        tot[:, c] = h.sum(axis=1, dtype=np.uint64)
        if not ref_ok(ref[c, :nb]):
            continue
        for b in range(B):
            if tot[b, c]:
                js[b, c] = evaluate.js_divergence(h[b].astype(np.float64), np.asarray(ref[c, :nb], np.float64))
    return js, tot


@functools.lru_cache(maxsize=6)
def histograms(U, row, seed=0):
    """(hist uint32 (U, C, ld), ref float64 (C, ld)) for a row of NBINS_ROWS: sparse counts (two thirds of the entries 0, a few
    units empty), a reference with zeros among positive densities; what lies beyond nbins[c] in a row is junk that must not count"""
    rng = np.random.default_rng([seed, U, len(row), max(row)])
    C, ld = len(row), max(row) + (max(row) % 2)
    hist = rng.integers(0, 40, (U, C, ld), dtype=np.uint32)
    hist[rng.random((U, C, ld)) < 0.66] = 0
    if U > 2:
        hist[rng.integers(0, U, max(1, U // 10))] = 0
    ref = rng.random((C, ld)) * (rng.random((C, ld)) < 0.7)
    for c, nb in enumerate(row):
        hist[0, c, 0] = 3                                   # no channel without a count or without a reference
        ref[c, 0] = 0.25
        hist[:, c, nb:] = 7
        ref[c, nb:] = 1e9
    hist.setflags(write=False)
    ref.setflags(write=False)
    return hist, ref


def weights(U, B, seed=0):
    """bootstrap_weights' multinomial rows, the last one (of three or more) all ones"""
    w = evaluate.bootstrap_weights(U, B, seed + 1)
    if B >= 3:
        w[-1] = 1
    return w


def binned_frames(n, nbins, seed=0, bad=0.05):
    """int32 (n, C): indices in 0 .. nbins[c] - 1, a share `bad` of them -1 (or far below) and as many >= nbins[c]"""
    rng = np.random.default_rng([seed, n])
    out = np.empty((n, len(nbins)), np.int32)
    for c, nb in enumerate(nbins):
        col = rng.integers(0, nb, n)
        r = rng.random(n)
        col[r < bad] = np.where(rng.random(n) < 0.5, -1, -2 ** 31)[r < bad]
        col[r > 1 - bad] = (nb + rng.integers(0, 3, n) * 5000)[r > 1 - bad]
        out[:, c] = col
    return out


class OracleResampler:
    """behind evaluate.js_resampler: the oracle above with the device resampler's signature; `calls` keeps the weights of every
    call since a test last cleared it"""
    calls = []

    def __init__(self, device=None):
        pass

    def __call__(self, unit_hist, nbins, ref, weights):
        OracleResampler.calls.append(np.array(weights))
        return resampled_js(np.asarray(unit_hist), np.asarray(nbins), np.asarray(weights), np.asarray(ref, np.float64))
