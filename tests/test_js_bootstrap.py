"""The Jensen-Shannon bootstrap on the GPU: dff_unit_hist against np.bincount (exact), dff_resampled_js against the fp64 oracle
of tests/js_cases.py (|d| <= 1e-13 per (b, c), totals exact) over units x resamples x bins-per-channel rows, its NaN rules,
64-bit sums, determinism (call to call, split of the batch, dirty workspace, every resample tile), the evaluators'
eval_bootstrap against eval() and the oracle, and the stream order of the two calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import js_cases as jc
from oracle import frames
from oracle import pwd_metric as om
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def device_js(hist, nbins, w, ref, workspace=None, total=True):
    # (torch.tensor copies: the shared cases are read-only)
    js, tot = B().resampled_js(torch.tensor(hist).cuda().view(torch.int32), nbins, to_dev(w), torch.tensor(ref).cuda(), total=total,
                               workspace=workspace)
    return js.cpu().numpy(), (tot.cpu().numpy() if total else None)


# ---------------------------------------------------------------- 1. per-unit histograms
def check_unit_hist(n, nbins, units, ld, seed):
    bins = jc.binned_frames(n, nbins, seed)
    got = B().unit_hist(to_dev(bins).reshape(n, len(nbins)), units, nbins, ld=ld)
    want = jc.unit_hists(bins, nbins, units, ld)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    return want


def test_unit_hist_equals_bincount(dev):
    units = [0, 1, 63, 64, 65, 0, 1000 - 193]
    want = check_unit_hist(1000, (1, 17, 300), units, 301, seed=1)
    assert want[:, :, 300].sum() == 0 and want[6].sum() > 0 and want[0].sum() == 0 and 0.85 * 3000 < want.sum() < 0.95 * 3000


def test_unit_hist_without_frames_zeroes_its_output(dev):
    for units in ([0], [0, 0, 0]):
        got = B().unit_hist(torch.empty((0, 2), dtype=torch.int32, device=dev), units, (5, 9), ld=12)
        assert got.shape == (len(units), 2, 12) and int(got.abs().sum()) == 0


def test_unit_hist_tiles_over_more_bins_than_one_lds_tile(dev):
    """10 000 bins: two tiles of 8192; 30 000 frames in a long and two short units, every tile boundary index among them"""
    n, nb = 30000, 10000
    bins = jc.binned_frames(n, (nb,), seed=2)
    bins[:8, 0] = [0, 8191, 8192, 8193, 9999, 10000, -1, 8191]
    units = [20000, 9999, 1]
    got = B().unit_hist(to_dev(bins), units, (nb,))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), jc.unit_hists(bins, (nb,), units))


def test_evaluate_unit_histograms_accepts_one_channel_vectors(dev):
    bins = jc.binned_frames(500, (40,), seed=3)[:, 0]
    got = ev().unit_histograms(to_dev(bins), [40], [100, 400])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), jc.unit_hists(bins, (40,), [100, 400]))


# ---------------------------------------------------------------- 2. resample and score
@pytest.mark.parametrize("row", jc.NBINS_ROWS, ids=lambda r: "bins" + "-".join(map(str, r)))
@pytest.mark.parametrize("Bn", jc.RESAMPLES)
@pytest.mark.parametrize("U", jc.UNITS)
def test_resampled_js_against_the_oracle(U, Bn, row, dev):
    hist, ref = jc.histograms(U, row)
    w = jc.weights(U, Bn)
    js, tot = device_js(hist, row, w, ref)
    want_js, want_tot = jc.resampled_js(hist, row, w, ref)
    assert np.array_equal(tot, want_tot), "totals must be exact"
    assert np.array_equal(np.isnan(js), np.isnan(want_js))
    ok = ~np.isnan(want_js)
    err = np.abs(js[ok] - want_js[ok]).max() if ok.any() else 0.0
    print(f"[js] U {U} B {Bn} bins {row}: worst |kernel - oracle| {err:.3e} over {ok.sum()} values, JS {np.nanmin(want_js):.4f} .. "
          f"{np.nanmax(want_js):.4f}")
    assert ok.any() and err <= jc.JS_ATOL
    assert device_js(hist, row, w, ref, total=False)[1] is None


def test_nan_rules_are_confined(dev):
    row = (65, 1025, 2, 300, 64)
    hist, ref = (a.copy() for a in jc.histograms(70, (65, 1025, 2, 30719, 64)))
    hist, ref = np.ascontiguousarray(hist[:, :, :1026]), np.ascontiguousarray(ref[:, :1026])
    w = jc.weights(70, 7)
    w[2] = 0                                             # a resample without a unit
    hist[5, :, 1], hist[5, 1, :] = 2, 0
    w[4], w[4, 5] = 0, 3                                 # a resample of one unit, which has no count in channel 1 only
    ref[0, :65] = 0                                      # a reference channel without mass
    ref[2, 1] = -0.5                                     # a negative entry
    ref[4, 63] = np.nan
    js, tot = device_js(hist, row, w, ref)
    want_js, want_tot = jc.resampled_js(hist, row, w, ref)
    assert np.array_equal(tot, want_tot) and (tot[2] == 0).all() and tot[4, 1] == 0 and (tot[4, [0, 2, 3, 4]] > 0).all()
    nan = np.zeros((7, 5), bool)
    nan[2], nan[:, [0, 2, 4]], nan[4, 1] = True, True, True
    assert np.array_equal(np.isnan(js), nan) and np.array_equal(np.isnan(want_js), nan)
    assert np.abs(js[~nan] - want_js[~nan]).max() <= jc.JS_ATOL
    ref[3, 7] = np.inf                                   # an infinite entry: that column only
    assert np.array_equal(np.isnan(device_js(hist, row, w, ref)[0]), nan | (np.arange(5) == 3)[None])


def test_weights_up_to_2_pow_32_do_not_overflow(dev):
    rng = np.random.default_rng(8)
    hist = rng.multinomial(1 << 18, np.full(63, 1 / 63), size=(4, 2)).astype(np.uint32)          # (4, 2, 63), 2^20 per channel
    assert (hist.sum(axis=(0, 2)) == 1 << 20).all()
    top = np.uint32(0xFFFFFFFF)
    w = np.array([[top] * 4, [top, 0, 1, top], [1, 1, 1, 1], [0, 0, top, 0]], np.uint32)
    ref = rng.random((2, 63))
    js, tot = device_js(hist, (63, 63), w, ref)
    want_js, want_tot = jc.resampled_js(hist, (63, 63), w, ref)
    assert int(tot[0, 0]) == (2 ** 32 - 1) * 2 ** 20 and np.array_equal(tot, want_tot)
    assert np.isfinite(js).all() and np.abs(js - want_js).max() <= jc.JS_ATOL
    assert np.abs(js[0] - js[2]).max() <= jc.JS_ATOL                       # a common factor changes no probability


# ---------------------------------------------------------------- 3. determinism
def test_bits_do_not_depend_on_call_batch_workspace_or_tile(dev):
    row, U, Bn = (65, 1025, 2, 30719, 64), 300, 130
    hist, ref = jc.histograms(U, row)
    w = jc.weights(U, Bn)
    hd, rd, wd = torch.tensor(hist).cuda().view(torch.int32), torch.tensor(ref).cuda(), to_dev(w)
    bnd = B()
    ws = torch.zeros(bnd.resampled_js_workspace_bytes(U, len(row)), dtype=torch.uint8, device=dev)
    js0, tot0 = bnd.resampled_js(hd, row, wd, rd, workspace=ws)
    js1, tot1 = bnd.resampled_js(hd, row, wd, rd, workspace=ws)
    assert torch.equal(js0.view(torch.int64), js1.view(torch.int64)) and torch.equal(tot0.view(torch.int64), tot1.view(torch.int64))
    ws.fill_(0xFF)
    js2, _ = bnd.resampled_js(hd, row, wd, rd, workspace=ws)
    assert torch.equal(js0.view(torch.int64), js2.view(torch.int64)), "a dirty workspace changed the result"
    for b in (0, 7, 64, 129):                                             # row b alone, and in a split of the batch
        one, _ = bnd.resampled_js(hd, row, wd[b:b + 1].contiguous(), rd)
        assert torch.equal(one.view(torch.int64), js0[b:b + 1].view(torch.int64)), b
    parts = torch.cat([bnd.resampled_js(hd, row, wd[s:e].contiguous(), rd)[0] for s, e in ((0, 3), (3, 100), (100, 130))])
    assert torch.equal(parts.view(torch.int64), js0.view(torch.int64))
    try:
        for tile in (1, 2, 4, 8):
            bnd.debug_resampled_js_path(tile)
            assert bnd.resampled_js_path_for(Bn, len(row)) == tile
            jst, tott = bnd.resampled_js(hd, row, wd, rd)
            assert torch.equal(jst.view(torch.int64), js0.view(torch.int64)), f"tile {tile} gives other bits"
            assert torch.equal(tott.view(torch.int64), tot0.view(torch.int64))
    finally:
        bnd.debug_resampled_js_path(0)


def test_more_units_than_one_weight_chunk(dev):
    """1500 units: the weights pass through LDS in two chunks of 1024, restaged for every 256 bins"""
    rng = np.random.default_rng(11)
    U, row = 1500, (700, 3)
    hist = rng.integers(0, 5, (U, 2, 700), dtype=np.uint32)
    ref = rng.random((2, 700))
    w = jc.weights(U, 9)
    js, tot = device_js(hist, row, w, ref)
    want_js, want_tot = jc.resampled_js(hist, row, w, ref)
    assert np.array_equal(tot, want_tot) and np.abs(js - want_js).max() <= jc.JS_ATOL


# ---------------------------------------------------------------- 4. the evaluators
def float32_js_distance():
    """|mean over pairs of the reference's float32 js_divergence - the same on float64| on the golden chignolin histograms
    (the reference's saved gt histograms against 1000 seeded frames): a property of the reference's arithmetic, measured on the
    CPU.  MEASURED: 1.31e-8 (JS 0.33094652 in float32, 0.33094651 in float64)."""
    g = np.load(os.path.join(GOLDEN, "pwd_chignolin_ref.npz"))
    off = np.concatenate(([0], np.cumsum(g["gt_hist_len"])))
    gt = [g["gt_hist"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    x, offset = g["x_samp"], int(g["offset"])
    nb = om.nbins_for(np.maximum(g["gt_max"], om.pair_max(x, offset)))
    j32, j64 = np.empty(len(gt)), np.empty(len(gt))
    for i, (h, hg, b) in enumerate(zip(om.histograms(x, offset, nb), gt, nb)):
        hg = np.concatenate((hg, np.zeros(max(int(b) - len(hg), 0), np.float32)))
        j32[i] = ev().js_divergence(hg.astype(np.float32), np.asarray(h).astype(np.float32))
        j64[i] = ev().js_divergence(hg.astype(np.float64), np.asarray(h).astype(np.float64))
    assert j32.mean() == float(g["js"])
    return abs(j32.mean() - j64.mean())


def test_pwd_eval_bootstrap(dev, tmp_path):
    e = ev()
    x = frames.synth_chain_frames(600, 10, 31)
    val = frames.synth_chain_frames(800, 10, 32)
    pe = e.PwdEvaluator(torch.from_numpy(val), mol_name="synth", offset=3, saved_ref=str(tmp_path / "none.pickle"))
    units = e.sample_units(600, n_blocks=12)
    assert units.tolist() == [50] * 12
    hist, nb, ref, got_units = pe.unit_histograms(torch.from_numpy(x), units)
    assert hist.shape == (12, 28, int(nb.max())) and np.array_equal(got_units, units)
    hmax = torch.tensor([pe.resolution * int(b) for b in nb], dtype=torch.float64).float()
    whole = B().pwd_hist(to_dev(x), 3, torch.from_numpy(nb), hmax)
    assert torch.equal(hist.sum(dim=0, dtype=torch.int32), whole), "the units' histograms do not add up to the single call's"
    assert int(whole.sum()) == 600 * 28
    bs = pe.eval_bootstrap(torch.from_numpy(x), n_blocks=12, n_resamples=16, seed=5)
    assert np.array_equal(bs.weights, e.bootstrap_weights(12, 16, 5)) and bs.per_channel.shape == (16, 28)
    want, _ = jc.resampled_js(hist.cpu().numpy().view(np.uint32), nb, bs.weights, ref)
    assert np.abs(bs.per_channel - want).max() <= jc.JS_ATOL
    point = float(pe.eval(torch.from_numpy(x)))
    bar = 4 * float32_js_distance()
    print(f"[js] PWD: eval() {point:.10f}, bootstrap point {bs.point:.10f}, |d| {abs(point - bs.point):.3e}, bar {bar:.3e}; "
          f"std {bs.std():.3e}, bias {bs.bias():.3e}, interval {bs.interval()}")
    assert abs(bs.point - point) <= bar
    assert bs.n_failed == 0 and bs.std() > 0 and bs.bias() > 0                 # finite histograms bias a JS upward
    # two frames made NaN: dropped whole, their units one frame shorter
    xn = x.copy()
    xn[7, 3, 1] = np.nan
    xn[599, 0, 0] = np.inf
    bn = pe.eval_bootstrap(torch.from_numpy(xn), n_blocks=12, n_resamples=4, seed=5)
    assert pe.samples_nonfinite == 2 and bn.unit_lengths.tolist() == [49] + [50] * 10 + [49]
    keep = np.ones(600, bool)
    keep[[7, 599]] = False
    assert abs(bn.point - float(pe.eval(torch.from_numpy(x[keep])))) <= bar
    with pytest.raises(ValueError, match="n_blocks"):
        pe.eval_bootstrap(torch.from_numpy(x), n_blocks=12, n_resamples=4, max_bytes=1000)


def test_tic_eval_bootstrap(dev, golden):
    e = ev()
    x = torch.from_numpy(golden("struct_ref_chignolin.npz")["x"][:500])
    tic = e.TicEvaluator(None, "chignolin", saved_ref=os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))
    units = e.sample_units(500, n_blocks=10)
    hist, nb, ref, _ = tic.unit_histograms(x, units)
    proj = tic.transform(x)
    counts = np.histogram2d(proj[:, 0], proj[:, 1], bins=[tic.bin_edges_x, tic.bin_edges_y])[0]
    assert nb.tolist() == [101 * 101] and hist.shape == (10, 1, 101 * 101)
    assert np.array_equal(hist.sum(dim=0).cpu().numpy().reshape(101, 101), counts.astype(np.int64)) and counts.sum() > 300
    bs = tic.eval_bootstrap(x, n_blocks=10, n_resamples=16, seed=2)
    js_density = float(tic.eval(x)[0])
    # what density=True adds: counts / (total x bin area) instead of counts, then the same normalisation -- the rounding of
    # the bin areas, measured on the host with numpy on both sides (MEASURED: 0.0 on this grid: the areas round alike)
    area = abs(js_density - e.js_divergence(tic.gt_prob.flatten(), counts.flatten()))
    bar = 4 * area + jc.JS_ATOL                       # + the kernel's own distance from numpy's sum (tests/js_cases.py)
    print(f"[js] TIC: eval() {js_density:.12f}, bootstrap point {bs.point:.12f}, |d| {abs(js_density - bs.point):.3e}, "
          f"bin-area rounding {area:.3e}; std {bs.std():.3e}, bias {bs.bias():.3e}")
    assert abs(bs.point - js_density) <= bar
    assert bs.per_channel.shape == (16, 1) and bs.n_failed == 0 and bs.std() > 0


def test_dihedral_eval_bootstrap(dev, golden, tmp_path):
    e = ev()
    x = torch.from_numpy(golden("struct_ref_ala2.npz")["x"][:2000])
    de = e.DihedralEnergiesEvaluator(x[:1000], saved_ref=str(tmp_path / "none.pickle"))
    bs = de.eval_bootstrap(x, n_blocks=20, n_resamples=8)
    js = float(de.eval(x)[1])
    print(f"[js] dihedral: eval() {js:.12f}, bootstrap point {bs.point:.12f}, |d| {abs(js - bs.point):.3e}")
    assert bs.per_channel.shape == (8, 1) and bs.n_failed == 0
    tors = de.torsions(x)
    counts = np.histogram2d(tors[:, 0], tors[:, 1], bins=np.linspace(-np.pi, np.pi, 61))[0]
    area = abs(js - e.js_divergence(counts.flatten(), de.gt_probs.flatten()))
    assert abs(bs.point - js) <= 4 * area + jc.JS_ATOL


# ---------------------------------------------------------------- 5. stream order
S_NBINS = np.array([17, 300, 1], np.int32)
S_UNITS = np.array([0, 1, 63, 64, 65, 0, 807], np.int64)


def unit_hist_spec():
    bins = jc.binned_frames(1000, S_NBINS, seed=1)
    ws = torch.empty(B().unit_hist_workspace_bytes(7, 3), dtype=torch.uint8, device="cuda")
    return Spec("dff_unit_hist", {"bins": (to_dev(bins), 0)}, {"hist": ((7, 3, 301), torch.int32)},
                lambda _, b: raw("dff_unit_hist", 0, ptr(b["bins"]), 1000, 3, S_UNITS.ctypes.data_as(C.c_void_p), 7,
                                 S_NBINS.ctypes.data_as(C.c_void_p), 301, ptr(b["hist"]), ptr(b["ws"]), b["ws"].numel(),
                                 stream_of(b["bins"])),
                work={"ws": ws},
                wrap=lambda _, b: {"hist": B().unit_hist(b["bins"], S_UNITS, S_NBINS, ld=301)})


def resampled_js_spec():
    hist = jc.unit_hists(jc.binned_frames(1000, S_NBINS, seed=1), S_NBINS, S_UNITS, 301)
    w = jc.weights(7, 9)
    ref = np.random.default_rng(3).random((3, 301))
    ws = torch.empty(B().resampled_js_workspace_bytes(7, 3), dtype=torch.uint8, device="cuda")

    def wrapped(_, b):
        js, tot = B().resampled_js(b["hist"], S_NBINS, b["w"], b["ref"])
        return {"js": js, "total": tot.view(torch.int64)}
    return Spec("dff_resampled_js",
                {"hist": (to_dev(hist).view(torch.int32), 1), "w": (to_dev(w), 0), "ref": (to_dev(ref), float("nan"))},
                {"js": ((9, 3), torch.float64), "total": ((9, 3), torch.int64)},
                lambda _, b: raw("dff_resampled_js", 0, ptr(b["hist"]), 7, 3, 301, S_NBINS.ctypes.data_as(C.c_void_p), ptr(b["w"]), 9,
                                 ptr(b["ref"]), ptr(b["js"]), ptr(b["total"]), ptr(b["ws"]), b["ws"].numel(), stream_of(b["hist"])),
                work={"ws": ws}, wrap=wrapped)


def test_unit_hist_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(unit_hist_spec(), gate, side)
    assert 2500 < int(ref["hist"].sum()) < 3000


def test_resampled_js_is_ordered_on_its_stream(gate, side):
    ref = analysis_call(resampled_js_spec(), gate, side)
    assert bool(torch.isfinite(ref["js"]).all()) and int(ref["total"].min()) > 0


def _fence(spec):
    """The memory contract (tests/fence.py): both patterns at both placements against one reference."""
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


def test_fence_unit_hist():
    """the unit starts and nbins at exactly dff_unit_hist_workspace_bytes; 301 bins of ld 301: the last tile of bins is partial"""
    _fence(unit_hist_spec())


@pytest.mark.parametrize("tile", [0, 1, 2, 4, 8])
def test_fence_resampled_js(tile):
    """every tile of resamples (9 resamples: a partial last tile for 2, 4 and 8), the workspace at exactly
    dff_resampled_js_workspace_bytes"""
    B().debug_resampled_js_path(tile)
    try:
        _fence(resampled_js_spec())
    finally:
        B().debug_resampled_js_path(0)
