"""dff_autocorr on the GPU against the naive numpy oracle of oracle/autocorr.py, and the relaxation analysis on top of it.

The kernel's constants (csrc/dff_autocorr.hip): a TILE of 512 start frames per workgroup pass, 128 per wave; a lag CHUNK of 512
lags per workgroup, 8 consecutive lags per lane; the sizes below sit around both.

What is compared how:
- integers   g integer-valued, |g| <= 2^10, n <= 2^15: every product is < 2^20 and every sum < 2^35, exact in fp64 in any order
             -> torch.equal with the oracle on sxy, sx, sy and count.
- reals      |S_gpu - S_oracle| <= (count[l] + 2) 2^-52 sabs[l, c] for sxy, sabs = sum |g_t g_{t+l}|; the same with sum |g_t| for sx
             and sum |g_{t+l}| for sy.  DERIVED: a sum of `count` terms in any order is off by at most (count - 1) u sum |terms|,
             u = 2^-53, on either side, the products add one rounding each on the oracle's side (the kernel's are fused), and
             g = series - shift is the same single rounding on both sides.  numpy's own sums sit at 0.0023 of the bar against
             math.fsum; one dropped pair is ~sabs / count, ~10^7 bars.  count must be exact.
- AR(1)      phi = 0.9: tau_int = 1/2 + phi / (1 - phi) = 9.5, -1 / ln(phi) = 9.49.  Sokal's estimator has a relative standard
             deviation of sqrt(2 (2 W + 1) / n) ~ 2.7 % at n = 262144, W ~ 47: 15 % is more than five of them.
"""
import math

import numpy as np
import pytest
import torch

from oracle.autocorr import Acf, lagged_sums, usable_mean
from oracle.kinetics import native_q, scripted_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

TILE, CHUNK = 512, 512
U = 2.0 ** -52
KEYS = ("sxy", "sx", "sy")


def gpu_sums(x, lengths, L, shift=None, fill=0xFF, **kw):
    """binding.autocorr on a dirty workspace -> dict of host tensors"""
    x = np.asarray(x, np.float64)
    xd = to_dev(x.reshape(len(x), -1))
    sd = None if shift is None else to_dev(np.asarray(shift, np.float64).reshape(-1))
    ws = torch.full((max(B().autocorr_workspace_bytes(xd.shape[0], xd.shape[1], L), 8),), fill, dtype=torch.uint8, device="cuda")
    return {k: v.cpu() for k, v in B().autocorr(xd, lengths, L, sd, workspace=ws, **kw).items()}


def assert_exact(got, want, L, what):
    assert got["count"].dtype == torch.int64 and got["sxy"].dtype == torch.float64
    bad = np.flatnonzero(got["count"].numpy() != want["count"][:L + 1])
    assert torch.equal(got["count"], torch.from_numpy(want["count"][:L + 1])), f"{what}: count differs at lags {bad[:8]}"
    for k in KEYS:
        bad = np.argwhere(got[k].numpy() != want[k][:L + 1])
        assert torch.equal(got[k], torch.from_numpy(want[k][:L + 1])), f"{what}: {k} differs at (lag, c) {bad[:4].tolist()}"


def integer_series(n, d, seed):
    return np.random.default_rng(seed).integers(-1000, 1001, (n, d)).astype(np.float64)


def ragged(n):
    """unequal lengths with 0, 1 and 2 among them"""
    head = [0, 1, 2, 0, 63, 1, 130, 2]
    return head + [n - sum(head)] if n > sum(head) + 1 else [n]


# ---------------------------------------------------------------- 1. exact parity on integers
@pytest.mark.parametrize("d", [1, 3, 8])
def test_integer_parity_around_tile_and_chunk(dev, d):
    for n in (TILE - 1, TILE, TILE + 1, 3 * TILE + 7):
        x = integer_series(n, d, 10 * n + d)
        for lengths in ([n], ragged(n)):
            want = lagged_sums(x, 600, lengths)                      # a lag's sums do not depend on max_lag
            for L in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 600):
                assert_exact(gpu_sums(x, lengths, L), want, L, f"d={d} n={n} {len(lengths)} trajectories max_lag={L}")
            assert want["count"][-1] == sum(max(v - 600, 0) for v in lengths)


def test_integer_parity_layouts(dev):
    # 80 equal trajectories, max_lag longer than every one of them: the lags from 100 on are never reached
    x = integer_series(8000, 2, 1)
    want = lagged_sums(x, 600, [100] * 80)
    got = gpu_sums(x, [100] * 80, 600)
    assert_exact(got, want, 600, "80 x 100")
    assert int(got["count"][99]) == 80 and not got["count"][100:].any() and not got["sxy"][100:].any() and not got["sx"][100:].any()
    assert_exact(gpu_sums(x, [100] * 40 + [0] + [100] * 40, 150), want, 150, "80 x 100 and an empty one")
    # 130 unequal trajectories: beyond one group of 64 run starts
    n = 20000
    x = integer_series(n, 3, 2)
    cuts = np.sort(np.random.default_rng(130).integers(0, n + 1, 129))
    cuts[40] = cuts[41]
    lengths = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
    assert len(lengths) == 130 and 0 in lengths and len(set(lengths)) > 100
    want = lagged_sums(x, 600, lengths)
    assert_exact(gpu_sums(x, lengths, 600), want, 600, "130 ragged")
    assert want["count"][600] == 0 < want["count"][500] < want["count"][1] < n     # the longest has 579 frames
    one = lagged_sums(x, 600)
    assert_exact(gpu_sums(x, [n], 600), one, 600, "one trajectory of 20000")
    assert one["count"][600] == n - 600 and not np.array_equal(one["sxy"], want["sxy"])          # the boundaries matter


def test_integer_parity_shift_and_null_outputs(dev):
    n, L = 3 * TILE + 7, 600
    x = integer_series(n, 3, 3)
    lengths = ragged(n)
    shift = np.array([17.0, -5.0, 0.0])
    want = lagged_sums(x, L, lengths, shift)
    plain = lagged_sums(x, L, lengths)
    assert not np.array_equal(want["sxy"], plain["sxy"])
    full = gpu_sums(x, lengths, L, shift)
    assert_exact(full, want, L, "integer shift")
    assert_exact(gpu_sums(x, lengths, L, None), plain, L, "NULL shift")
    for kw in (dict(sx=False, sy=False, count=False), dict(sx=False), dict(sy=False, count=False), dict(sx=False, sy=False)):
        got = gpu_sums(x, lengths, L, shift, **kw)
        assert set(got) == {"sxy"} | {k for k in ("sx", "sy", "count") if kw.get(k, True)}
        for k, v in got.items():
            assert torch.equal(v, full[k]), (kw, k)
    # n == 0 zeroes the outputs
    got = B().autocorr(torch.empty((0, 2), dtype=torch.float64, device="cuda"), [], 5)
    assert all(v.shape[0] == 6 and not v.cpu().any() for v in got.values())
    got = B().autocorr(torch.empty((0, 2), dtype=torch.float64, device="cuda"), [0, 0], 0)
    assert all(not v.cpu().any() for v in got.values())


# ---------------------------------------------------------------- 2. / 3. real values, non-finite frames
def assert_within_bar(got, want, what):
    L = len(got["count"]) - 1
    assert torch.equal(got["count"], torch.from_numpy(want["count"][:L + 1])), f"{what}: count differs"
    cnt = want["count"][:L + 1, None].astype(np.float64)
    for k, scale in (("sxy", "sabs"), ("sx", "sgx"), ("sy", "sgy")):
        err = np.abs(got[k].numpy() - want[k][:L + 1])
        bar = (cnt + 2) * U * want[scale][:L + 1]
        worst = np.nanmax(np.where(bar > 0, err / np.where(bar > 0, bar, 1), 0))
        print(f"[autocorr] {what}: {k} worst |S_gpu - S_oracle| / bar = {worst:.4f}, largest error {err.max():.3e}")
        assert (err <= bar).all(), f"{what}: {k} misses the bar at (lag, c) {np.argwhere(err > bar)[:4].tolist()}: {worst:.3f} bars"


def random_walk():
    rng = np.random.default_rng(7)
    return np.cumsum(rng.standard_normal((5000, 2)), 0) * 0.1


WALK_LENGTHS = [1200, 0, 1, 3799]


def test_real_parity(dev):
    x = random_walk()
    shift = x.mean(0)
    want = lagged_sums(x, 300, WALK_LENGTHS, shift)
    assert_within_bar(gpu_sums(x, WALK_LENGTHS, 300, shift), want, "random walk")
    assert want["count"][300] == 900 + 3499


def test_non_finite_frames(dev):
    x = random_walk()
    starts = np.concatenate([[0], np.cumsum(WALK_LENGTHS)])
    rng = np.random.default_rng(8)
    where = np.concatenate([rng.integers(0, 5000, 40), [0, 1199, 1200, 1201, 4999, TILE - 1, TILE, 4 * TILE - 1, 4 * TILE]])
    for i, t in enumerate(where):
        x[t, i % 2] = (np.nan, np.inf, -np.inf)[i % 3]
    assert not np.isfinite(x[[0, 1199, 1200, 1201, 4999, TILE - 1, TILE]]).all(1).any() and starts.tolist() == [0, 1200, 1200, 1201, 5000]
    shift = usable_mean(x)
    want = lagged_sums(x, 300, WALK_LENGTHS, shift)
    n_bad = int((~np.isfinite(x).all(1)).sum())
    assert want["count"][0] == 5000 - n_bad and want["count"][1] < 5000 - n_bad - 3
    assert_within_bar(gpu_sums(x, WALK_LENGTHS, 300, shift), want, "non-finite frames")
    # every frame unusable: zeros from the call, NaN through autocorrelation
    y = random_walk()
    y[:, 1] = np.nan
    got = gpu_sums(y, WALK_LENGTHS, 300, np.zeros(2))
    assert all(not v.any() for v in got.values())
    a = ev().autocorrelation(y, 300, WALK_LENGTHS)
    assert np.isnan(a.acf).all() and np.isnan(a.cov).all() and not a.counts.any() and a.n_usable == 0


# ---------------------------------------------------------------- 4. determinism
def test_determinism(dev):
    x = random_walk()
    shift = x.mean(0)
    a = gpu_sums(x, WALK_LENGTHS, 300, shift, fill=0xFF)            # 0xFF bytes: NaN doubles in the workspace
    b = gpu_sums(x, WALK_LENGTHS, 300, shift, fill=0xFF)
    z = gpu_sums(x, WALK_LENGTHS, 300, shift, fill=0)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
        assert torch.equal(a[k].view(torch.uint8), z[k].view(torch.uint8)), f"{k} depends on the workspace's contents"
    # the wrapper converts once: a float32, non-contiguous input equals its converted copy
    wide = torch.from_numpy(np.repeat(x, 2, axis=1).astype(np.float32))
    view = wide[:, ::2]
    assert not view.is_contiguous() and view.dtype == torch.float32
    want = ev().autocorrelation(view.double().contiguous(), 300, WALK_LENGTHS)
    for src in (view, view.numpy(), view.cuda()):
        got = ev().autocorrelation(src, 300, WALK_LENGTHS)
        for k in ("acf", "cov", "counts", "mean", "variance"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), k
    one = ev().autocorrelation(view[:, 0], 300, WALK_LENGTHS)                                    # (n,) is (n, 1)
    assert one.acf.shape == (301, 1) and np.allclose(one.acf[:, 0], want.acf[:, 0], rtol=0, atol=1e-12)
    glo = ev().autocorrelation(view, 300, WALK_LENGTHS, estimator="global")
    assert np.allclose(glo.variance, want.variance, rtol=1e-12, atol=0) and not np.array_equal(glo.cov[1:], want.cov[1:])


# ---------------------------------------------------------------- 5. stream order
AC_N, AC_L = 5000, 100
AC_LENGTHS = np.array([1, 2047, 1, 2000, 951], np.int64)


def autocorr_spec():
    b = B()
    x = random_walk()
    ws = torch.empty(b.autocorr_workspace_bytes(AC_N, 2, AC_L), dtype=torch.uint8, device="cuda")
    outs = {k: ((AC_L + 1, 2), torch.float64) for k in KEYS}
    outs["count"] = ((AC_L + 1,), torch.int64)
    return Spec("dff_autocorr", {"series": (to_dev(x), float("nan")), "shift": (to_dev(x.mean(0)), 1.0)}, outs,
                lambda _, bufs: raw("dff_autocorr", 0, ptr(bufs["series"]), AC_N, 2, AC_LENGTHS.ctypes.data, len(AC_LENGTHS), AC_L,
                                    ptr(bufs["shift"]), ptr(bufs["sxy"]), ptr(bufs["sx"]), ptr(bufs["sy"]), ptr(bufs["count"]),
                                    ptr(bufs["ws"]), bufs["ws"].numel(), stream_of(bufs["series"])),
                work={"ws": ws}, wrap=lambda _, bufs: b.autocorr(bufs["series"], AC_LENGTHS, AC_L, bufs["shift"]))


def test_stream_order_autocorr(gate, side):  # noqa: F811
    ref = analysis_call(autocorr_spec(), gate, side)
    assert int(ref["count"][0]) == AC_N and float(ref["sxy"][0].min()) > 0      # nothing like the zeros of the poison


def test_fence_autocorr():
    """The memory contract (tests/fence.py): every buffer in one arena, the (slots, K, lags) partials and the frames-left table
    at exactly dff_autocorr_workspace_bytes."""
    spec = autocorr_spec()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


# ---------------------------------------------------------------- 6. a known process
def test_ar1_end_to_end(dev):
    phi, P, T, L = 0.9, 64, 4096, 256
    rng = np.random.default_rng(0)
    x = np.empty((P, T))
    x[:, 0] = rng.standard_normal(P) / math.sqrt(1 - phi * phi)     # the stationary law
    eps = rng.standard_normal((P, T))
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + eps[:, t]
    series, lengths = x.reshape(-1), [T] * P
    got = ev().autocorrelation(series, L, lengths)
    want = Acf(series, L, lengths)
    assert np.array_equal(got.counts, want.counts) and got.counts[L] == P * (T - L)
    err = np.abs(got.acf - want.acf).max()
    tau, W, converged = ev().integrated_autocorr_time(got.acf)
    te = ev().crossing_time(got.acf)
    print(f"[autocorr] AR(1): |acf - oracle| {err:.3e}, tau_int {tau:.4f} (window {W}), 1/e time {te:.4f}, "
          f"ess {ev().effective_sample_size(got.n_usable, tau):.0f} of {got.n_usable}")
    assert err <= 1e-10
    assert abs(got.mean[0] - series.mean()) <= 1e-12 and abs(got.variance[0] - series.var()) <= 1e-10
    assert converged and abs(tau - 9.5) <= 0.15 * 9.5
    assert abs(te + 1 / math.log(phi)) <= 0.15 * (-1 / math.log(phi))


# ---------------------------------------------------------------- 7. the evaluator
SCRIPT = [[0.3, 0.0, 0.3, 1.0, 0.3, 0.0], [1.0, 0.3, 0.0, 0.3], [0.0, 0.3, 1.0, 1.0, 0.3]]     # one list per trajectory
REPEAT = 40


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-9, abs=1e-9)


def test_relaxation_evaluator(dev, golden):
    f = golden("struct_folded.npz")["chignolin"].astype(np.float64)
    x, _ = scripted_frames(f, sum(SCRIPT, []), REPEAT, 0.05, len(f))
    lengths = [len(s) * REPEAT for s in SCRIPT]
    L, dt = 100, 0.2
    e = ev().RelaxationEvaluator("chignolin", f, cv="q", max_lag=L, frame_time=dt, ref_data=x, ref_traj_lengths=lengths)
    res = e.eval(x, lengths)
    # the oracle: Q in float64 rounded to the float32 the series is defined in, its ACF, and the dict from them
    pairs, r0 = ev().native_pairs(f)
    q = native_q(x, pairs, r0).astype(np.float32)
    differ = int((e.series["samples"] != q).sum())
    print(f"[autocorr] chignolin: {differ} of {len(q)} frames of the GPU's Q differ from the rounded oracle, by at most "
          f"{np.abs(e.series['samples'].astype(np.float64) - q).max():.3e}")
    assert np.abs(e.series["samples"].astype(np.float64) - q).max() <= 2.0 ** -23
    oracle = Acf(q, L, lengths)
    want = ev().RelaxationEvaluator.summarize(oracle, dt)
    want["samples_nonfinite"] = 0.0
    assert set(want) == set(ev().RelaxationEvaluator.KEYS)
    assert set(res) == set(want) | {k + "_ref" for k in want} | {"log10_tau_int_ratio"}
    for k, v in want.items():
        assert close(res[k], v), (k, res[k], v)
        assert res[k + "_ref"] == res[k] or (math.isnan(res[k]) and math.isnan(res[k + "_ref"])), k
    assert res["log10_tau_int_ratio"] == 0.0 and res["tau_int"] > dt and res["ess"] < len(x)
    assert np.abs(e.acf["samples"].acf - oracle.acf).max() <= 1e-9 and e.acf["samples"].acf.shape == (L + 1, 1)
    # without reference data there are no _ref keys; the frames as ONE trajectory also pair across the two joints
    one = ev().RelaxationEvaluator("chignolin", f, cv="q", max_lag=L)
    r1 = one.eval(x)
    assert set(r1) == set(want) and one.acf["samples"].counts[1] == len(x) - 1 and e.acf["samples"].counts[1] == len(x) - 3
    # the RMSD and the TICs run through the same path: shapes and keys
    rm = ev().RelaxationEvaluator("chignolin", f, cv="rmsd", max_lag=L).eval(x, lengths)
    assert set(rm) == set(want) and rm["tau_int"] > 0
    F = B().struct_tic_num_features(len(f))
    rng = np.random.default_rng(5)
    tic = ev().RelaxationEvaluator("chignolin", cv="tic", tica=(np.zeros(F), rng.standard_normal((F, 3)) * 0.1), max_lag=L)
    rt = tic.eval(x, lengths)
    assert set(rt) == set(want) and all(len(rt[k]) == 3 for k in want if k != "samples_nonfinite") and tic.acf["samples"].acf.shape == (L + 1, 3)
