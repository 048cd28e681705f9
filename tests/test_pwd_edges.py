"""The PWD histogram kernels (csrc/dff_pwd.hip) where they can be wrong without tests/test_pwd_metric.py noticing: values
that sit on a bin edge, the launch layouts that ordinary shapes never reach, and non-finite input.

CPU part: the launch plan of dff_pwd_hist (dff_pwd_hist_plan, host only) swept over every bead count; the numpy oracle
(oracle/pwd_metric.py) against torch on the edge set; and a check that the edge set tells the reference's bin formula from
its near misses.  GPU part (-m gpu): the kernels bit for bit against the oracle, every case asserting through the plan
that it runs the layout it is there for.  All comparisons are integer or bit equality.
"""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import pwd_metric as om
from oracle import synth

gpu = pytest.mark.gpu
f32 = np.float32

LDS_BYTES = 160 * 1024
LDS_SLOTS = 30720           # DFF_PWD_LDS_BINS: uint32 histogram slots of a workgroup
MAX_BINS = 30719            # the largest max_bins: ldl = max_bins | 1 must be <= LDS_SLOTS


def _plan(N, off, max_bins, n):
    from dff_amd import binding
    return binding.pwd_hist_plan(N, off, max_bins, n)


# ------------------------------------------------------------------ CPU: the launch plan
PLAN_BINS = [1, 2] + [b + d for b in (120, 240, 480, 960, 1920, 3840, 7680, 15360, 30720) for d in (-1, 0, 1)]
PLAN_N = [1, 63, 700, 4097, 10 ** 6]


def test_plan_sweep():
    """Every N in 2..64 at offsets 0, 1, 3: the layout fits the LDS, gives every pair one lane, covers every structure,
    and comes in whole rounds of 8 structure chunks."""
    from dff_amd import binding
    assert binding.PWD_MAX_BINS == MAX_BINS
    tiles = set()
    lanes = set()
    for N in range(2, 65):
        for off in (0, 1, 3):
            npairs = len(om.triu_pairs(N, off)[0])
            if npairs == 0:
                with pytest.raises(ValueError):
                    _plan(N, off, 8, 63)
                continue
            for mb in PLAN_BINS:
                if mb > MAX_BINS:
                    with pytest.raises(ValueError, match=str(mb)):
                        _plan(N, off, mb, 63)
                    continue
                for n in PLAN_N:
                    p = _plan(N, off, mb, n)
                    what = (N, off, mb, n, p)
                    PC, ldl = 1 << p["pc_log2"], p["ldl"]
                    assert p["n_pairs"] == npairs, what
                    assert p["tile_n"] in (64, 32), what
                    assert 0 <= p["pc_log2"] <= 8, what
                    assert ldl % 2 == 1 and mb <= ldl <= mb + 1, what
                    assert PC * ldl <= LDS_SLOTS, what
                    assert p["lds_bytes"] == p["tile_n"] * 3 * N * 4 + PC * ldl * 4 + 16 <= LDS_BYTES, what
                    # every pair belongs to exactly one (pair chunk, lane): chunk p >> pc_log2 < npc, lane p & (PC - 1), and
                    # no pair chunk is empty
                    assert (p["npc"] - 1) * PC < npairs <= p["npc"] * PC, what
                    # a workgroup with fewer pairs than lanes would waste LDS another layout could use
                    assert PC == 1 or PC // 2 < npairs, what
                    assert p["chunk"] > 0 and p["chunk"] % 64 == 0 and p["chunk"] % p["tile_n"] == 0, what
                    assert (p["chunks"] - 1) * p["chunk"] < n <= p["chunks"] * p["chunk"], what
                    assert p["chunks_rounded"] % 8 == 0 and 0 <= p["chunks_rounded"] - p["chunks"] < 8, what
                    assert p["grid"] == p["chunks_rounded"] * p["npc"] < 2 ** 31, what
                    # the 32-structure tile is taken only where it doubles the pair lanes
                    if p["tile_n"] == 32:
                        slots64 = min((LDS_BYTES - 64 - 64 * 3 * N * 4) // 4, LDS_SLOTS)
                        assert PC * ldl > slots64, what
                    tiles.add(p["tile_n"])
                    lanes.add(p["pc_log2"])
    assert tiles == {64, 32} and lanes == set(range(9))


def test_plan_named_layouts():
    """The layouts the GPU cases below are there for, and the two ends of the bin range."""
    for N in range(2, 65):
        assert _plan(N, 1, MAX_BINS, 300)["pc_log2"] == 0
        with pytest.raises(ValueError, match="30720"):
            _plan(N, 1, MAX_BINS + 1, 300)
    assert _plan(56, 3, 239, 333)["tile_n"] == 32 and _plan(56, 3, 240, 333)["tile_n"] == 64
    assert _plan(56, 3, 119, 333)["tile_n"] == 32 and _plan(56, 3, 120, 333)["tile_n"] == 64
    assert _plan(64, 0, 119, 130)["tile_n"] == 32
    p = _plan(4, 1, MAX_BINS, 300)
    assert (p["npc"], p["lds_bytes"], p["tile_n"]) == (6, 125964, 64)
    for bad in [(1, 0, 8, 10), (65, 0, 8, 10), (10, 10, 8, 10), (10, 3, 0, 10), (10, 3, 8, -1)]:
        with pytest.raises(ValueError):
            _plan(*bad)
    assert _plan(10, 3, 8, 0)["grid"] == 0


# ------------------------------------------------------------------ the edge set
EDGE_NBS = (1, 2, 7, 111, 296, 1000, 3001)


@functools.lru_cache(maxsize=None)
def edge_values(nb):
    """The float32 values k * 0.1, k = 0..nb, with their one and two float32 neighbours on each side, exact 0 and the
    exact hmax = float32(0.1 * nb); sorted, distinct, within [0, hmax]."""
    hmax = f32(0.1 * nb)
    e = (np.arange(nb + 1) * 0.1).astype(f32)
    vs, up, dn = [e, np.array([0, hmax], f32)], e, e
    for _ in range(2):
        up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(-np.inf))
        vs += [up, dn]
    v = np.unique(np.concatenate(vs))
    v = v[(v >= 0) & (v <= hmax)]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def edge_set():
    v = np.unique(np.concatenate([edge_values(nb) for nb in EDGE_NBS]))
    v.setflags(write=False)
    return v


def as_distances(v):
    """The values a pair of beads can realise exactly: (v, 0, 0) - (0, 0, 0) has the distance sqrt(v * v) == v unless v * v
    underflows, which the few subnormal neighbours of 0 do."""
    return v[(v == 0) | (v >= f32(1e-18))]


def frames_on_x(cols):
    """(n, 1 + len(cols), 3): bead 0 at the origin, bead k at (cols[k - 1], 0, 0)."""
    x = np.zeros((len(cols[0]), 1 + len(cols), 3), f32)
    for k, c in enumerate(cols):
        x[:, k + 1, 0] = c
    return x


def bins_of(v, nb, mx):
    """the oracle's bin of every v in [0, mx] (om.histc's formula)"""
    return np.minimum((v * f32(nb) / mx).astype(np.int64), nb - 1)


# ------------------------------------------------------------------ CPU: oracle == torch on the edge set; the set has teeth
def test_edge_set_size():
    assert 14000 < len(edge_set()) < 16000
    assert sum(len(edge_values(nb)) for nb in EDGE_NBS) > 22000
    for nb in EDGE_NBS:
        v = edge_values(nb)
        assert v[0] == 0 and v[-1] == f32(0.1 * nb) and v[1] == np.nextafter(f32(0), f32(1))


def test_oracle_histc_equals_torch_on_edges():
    for nb in EDGE_NBS:
        for v in (edge_values(nb), edge_set()):           # the bins' own edges; every edge, those past hmax dropped
            ref = torch.histc(torch.from_numpy(v.copy()), bins=nb, min=0, max=0.1 * nb).numpy().astype(np.int64)
            got = om.histc(v, nb, 0.1 * nb)
            assert np.array_equal(got, ref), nb
            assert got.sum() == (v <= f32(0.1 * nb)).sum()


def test_oracle_nbins_equals_torch_on_edges():
    """every value of the set as a pair's maximum: the bin count, and the histogram of the set under that maximum for a
    sub-sample of about 2000 of them"""
    v = edge_set()
    ref = (torch.div(torch.from_numpy(v.copy()), 0.1, rounding_mode="floor") + 1).to(torch.int64).numpy()
    nbs = om.nbins_for(v)
    assert np.array_equal(nbs, ref)
    assert nbs.min() == 1 and nbs.max() >= 3001
    tv = torch.from_numpy(v.copy())
    for nb in np.unique(nbs[::7]):                       # ~2100 maxima share these ~430 bin counts
        ref = torch.histc(tv, bins=int(nb), min=0, max=0.1 * int(nb)).numpy().astype(np.int64)
        assert np.array_equal(om.histc(v, int(nb), 0.1 * int(nb)), ref), nb


def test_edge_set_discriminates():
    """The set must tell the reference's (v * nb) / mx in float32 from a reciprocal multiply and from binning in float64:
    1630 and 1819 of the 22097 values differ (measured once on the CPU); the floors of 1000 keep the set from losing its
    teeth unnoticed."""
    recip = f64 = total = 0
    for nb in EDGE_NBS:
        v, mx = edge_values(nb), f32(0.1 * nb)
        pos = bins_of(v, nb, mx)
        pos_recip = np.minimum((v * (f32(nb) / mx)).astype(np.int64), nb - 1)
        pos_f64 = np.minimum((v.astype(np.float64) * nb / np.float64(mx)).astype(np.int64), nb - 1)
        recip += int((pos != pos_recip).sum())
        f64 += int((pos != pos_f64).sum())
        total += len(v)
    print(f"edge set: {total} values, {recip} differ under v * (nb / mx), {f64} under float64 binning")
    assert recip >= 1000 and f64 >= 1000


def test_oracle_distance_is_exact_on_x_axis():
    v = as_distances(edge_set())
    assert len(edge_set()) - len(v) <= 2                  # only the two subnormal neighbours of 0 are dropped
    assert np.array_equal(om.pwd_triu(frames_on_x([v]), 1)[:, 0], v)
    for s in (f32(0.5), f32(2.0)):                        # a power-of-two scale keeps every value exact
        assert np.array_equal(om.pwd_triu(frames_on_x([v * s]), 1)[:, 0], v * s)


# ------------------------------------------------------------------ GPU: the kernels against the oracle
def _hist(x, off, nbins, hmax):
    from dff_amd import binding
    nb = torch.as_tensor(np.asarray(nbins), dtype=torch.int32)
    return binding.pwd_hist(torch.from_numpy(np.ascontiguousarray(x)).cuda(), off, nb,
                            torch.from_numpy(np.asarray(hmax, f32))).cpu().numpy()


def _hmax(nbins):
    return np.array([f32(0.1 * int(b)) for b in nbins], f32)


def _check_hists(x, off, nbins, kernel_nonfinite=False):
    """dff_pwd_hist at hmax = float32(0.1 * nbins) == the oracle's histograms for every pair, and nothing beyond a pair's
    own bins; returns the counts"""
    got = _hist(x, off, nbins, _hmax(nbins))
    with np.errstate(all="ignore"):
        ref = om.histograms(x, off, nbins, kernel_nonfinite=kernel_nonfinite)
    assert got.shape == (len(ref), max(int(b) for b in nbins))
    for p, r in enumerate(ref):
        bad = np.flatnonzero(got[p, :len(r)] != r)
        assert bad.size == 0, f"pair {p}: {bad.size} of {len(r)} bins differ, first at bin {bad[0]}"
        assert not got[p, len(r):].any(), f"pair {p}: counts beyond its {len(r)} bins"
    return got


@gpu
@pytest.mark.parametrize("nb", EDGE_NBS)
def test_hip_edge_frames_one_pair(nb):
    """every edge value as the distance of a single pair, binned at that nb: one pair lane.  (A build of the kernel that
    bins with d * (bf / m) fails this for every nb >= 7: 1126 of the 22083 frames land in another bin on the MI355X.)"""
    from dff_amd import binding
    v = as_distances(edge_values(nb))
    x = frames_on_x([v])
    p = _plan(2, 1, nb, len(v))
    assert (p["pc_log2"], p["npc"], p["n_pairs"]) == (0, 1, 1)
    mx = binding.pwd_max(torch.from_numpy(x).cuda(), 1).cpu().numpy()
    assert mx.tolist() == [f32(0.1 * nb)] and np.array_equal(mx, om.pair_max(x, 1))
    got = _check_hists(x, 1, [nb])
    assert got.sum() == len(v)
    # the whole edge set at these bins: the values past hmax are dropped on both sides
    w = as_distances(edge_set())
    got = _check_hists(frames_on_x([w]), 1, [nb])
    assert got.sum() == (w <= f32(0.1 * nb)).sum()


@gpu
def test_hip_edge_frames_empty_workgroups():
    """700 frames at 8 bins: 11 structure chunks of 64 rounded to 16, five workgroups without a structure"""
    p = _plan(2, 1, 8, 700)
    assert (p["chunk"], p["chunks"], p["chunks_rounded"], p["grid"]) == (64, 11, 16, 16)
    v = as_distances(edge_set())
    v = np.resize(v[v <= f32(0.9)], 700)                  # the 45 values around the 9 lowest edges, cyclically: every chunk gets them
    assert len(np.unique(v)) > 40
    got = _check_hists(frames_on_x([v]), 1, [8])
    assert got.sum() == (v <= f32(0.8)).sum() < 700


def _six_pairs():
    """N = 4: beads 1..3 at (v, v / 2, 2 v) on the x axis, so the pairs (0, k) sit on the edges of their own, unequal
    bin counts; pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)"""
    v = as_distances(edge_values(296))
    x = frames_on_x([v, v * f32(0.5), v * f32(2.0)])
    return x, [296, 148, 592, 111, 7, 1000]


@gpu
def test_hip_six_pairs_unequal_nbins():
    """six pairs on eight lanes (two dead), every pair with its own bin count"""
    x, nbins = _six_pairs()
    p = _plan(4, 1, max(nbins), len(x))
    assert (p["n_pairs"], p["pc_log2"], p["npc"]) == (6, 3, 1)
    got = _check_hists(x, 1, nbins)
    assert got[0].sum() == got[1].sum() == got[2].sum() == len(x)       # each within its own hmax, to the last value


@gpu
def test_hip_row_stride():
    """the raw ABI with ld = max_bins + 3: rows land at the caller's stride and the padding columns stay zero"""
    from stream_gate import ptr, raw, stream_of
    x, nbins = _six_pairs()
    mb = max(nbins)
    ld = mb + 3
    xd = torch.from_numpy(x).cuda()
    nb_d = torch.tensor(nbins, dtype=torch.int32).cuda()
    hm_d = torch.from_numpy(_hmax(nbins)).cuda()
    hist = torch.full((6, ld), -1, dtype=torch.int32).cuda()          # the call zeroes all of it first
    raw("dff_pwd_hist", 0, ptr(xd), len(x), 4, 1, ptr(nb_d), ptr(hm_d), mb, ld, ptr(hist), stream_of(xd))
    hist = hist.cpu().numpy()
    assert not hist[:, mb:].any()
    for p, r in enumerate(om.histograms(x, 1, nbins)):
        assert np.array_equal(hist[p, :len(r)], r) and not hist[p, len(r):].any()


def _gauss(n, N, scale, seed):
    return (synth.normal((n, N, 3), 77, seed) * scale).astype(f32)


@gpu
@pytest.mark.parametrize("nb,pc_log2,npc,live_last", [(960, 4, 2, 12), (7679, 2, 7, 4)])
def test_hip_pair_chunks(nb, pc_log2, npc, live_last):
    """28 pairs over several pair chunks: few pair lanes per workgroup, the last chunk partly dead"""
    N, off, n = 10, 3, 333
    p = _plan(N, off, nb, n)
    assert (p["n_pairs"], p["pc_log2"], p["npc"]) == (28, pc_log2, npc)
    assert 28 - (npc - 1) * (1 << pc_log2) == live_last
    x = _gauss(n, N, 25.0, nb)
    got = _check_hists(x, off, [nb] * 28)
    assert got.sum() > 0.8 * 28 * n                       # the data do fill the range: most distances are binned


@gpu
def test_hip_largest_bin_count():
    """30719 bins: one pair lane per workgroup, six pair chunks, 125 964 bytes of LDS; 30720 is refused by name"""
    from dff_amd import binding
    N, off, n = 4, 1, 300
    p = _plan(N, off, MAX_BINS, n)
    assert (p["pc_log2"], p["npc"], p["lds_bytes"], p["ldl"]) == (0, 6, 125964, MAX_BINS)
    x = _gauss(n, N, 400.0, 5)
    got = _check_hists(x, off, [MAX_BINS] * 6)
    assert got.sum() > 0.9 * 6 * n and np.flatnonzero(got.sum(0)).max() > 15000
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="30720"):
        binding.pwd_hist(xd, off, torch.full((6,), MAX_BINS + 1, dtype=torch.int32), torch.full((6,), 3072.0))


@gpu
@pytest.mark.parametrize("N,off,n,nb,tile", [(56, 3, 333, 239, 32), (64, 0, 130, 119, 32), (56, 3, 333, 240, 64)])
def test_hip_tile(N, off, n, nb, tile):
    """the 32-structure tile (n no multiple of it) and its control one bin further, where the 64-structure tile stays"""
    p = _plan(N, off, nb, n)
    assert p["tile_n"] == tile and p["pc_log2"] == (8 if (N, tile) == (64, 32) else 7 if tile == 32 else 6)
    assert n % 32 != 0
    x = _gauss(n, N, 3.0, N + nb)
    npairs = p["n_pairs"]
    got = _check_hists(x, off, [nb] * npairs)
    assert 0.5 * npairs * n < got.sum() <= npairs * n
    # unequal bin counts under the same maximum: the same layout
    nbins = 1 + (np.arange(npairs) * 37) % nb
    nbins[npairs // 2] = nb
    _check_hists(x, off, nbins.tolist())


# ------------------------------------------------------------------ GPU: non-finite input
def _damaged_frames():
    """300 frames of 10 beads with NaN, +Inf and -Inf in single coordinates of beads 0, 4 and 9 (frames 0, 63, 64, 299 and
    20 random ones), one frame with a finite coordinate of 3e19 whose squared difference overflows, and an all-NaN frame
    appended as the 301st: the pairs of the other beads see 300 good frames."""
    n, N = 300, 10
    x = _gauss(n, N, 3.0, 11)
    rng = np.random.default_rng(5)
    frames = [0, 63, 64, 299] + rng.choice(np.setdiff1d(np.arange(1, 299), [63, 64, 65]), 21, replace=False).tolist()
    vals = [np.nan, np.inf, -np.inf]
    for k, s in enumerate(frames[:-1]):
        x[s, (0, 4, 9)[k % 3], (k // 3) % 3] = vals[(k // 2) % 3]
    x[frames[-1], 4, 1] = 3e19
    x[65, 0, 0] = x[65, 9, 0] = np.inf                    # both beads of pair (0, 9) at +Inf: Inf - Inf = NaN
    return np.concatenate([x, np.full((1, N, 3), np.nan, f32)]), (0, 4, 9)


@gpu
def test_hip_nonfinite_contract():
    """dff_pwd_max skips NaN distances and keeps +Inf; dff_pwd_hist drops both and counts the rest (include/dff.h)"""
    from dff_amd import binding
    x, bad_beads = _damaged_frames()
    off = 3
    with np.errstate(all="ignore"):
        pwd = om.pwd_triu(x, off)
        ref_max = om.pair_max(x, off, kernel_nonfinite=True)
    assert np.isnan(pwd).any() and np.isposinf(pwd).any() and not np.isnan(ref_max).any()
    mx = binding.pwd_max(torch.from_numpy(x).cuda(), off).cpu().numpy()
    assert np.array_equal(mx, ref_max)
    i, j = om.triu_pairs(10, off)
    touched = np.isin(i, bad_beads) | np.isin(j, bad_beads)
    assert np.isposinf(mx[touched]).any() and np.isfinite(mx[~touched]).all() and 0 < (~touched).sum() < len(i)
    fin = np.where(np.isfinite(pwd), pwd, 0).max(axis=0)
    nbins = om.nbins_for(fin).tolist()
    got = _check_hists(x, off, nbins, kernel_nonfinite=True)
    totals = got.sum(1)
    assert np.array_equal(totals, np.isfinite(pwd).sum(0))
    assert (totals[~touched] == 300).all() and (totals[touched] < 300).all()
    # an all-NaN input: no maximum, nothing counted
    xn = torch.full((70, 10, 3), float("nan")).cuda()
    assert binding.pwd_max(xn, off).cpu().numpy().tolist() == [0.0] * len(i)
    assert not binding.pwd_hist(xn, off, torch.full((len(i),), 5, dtype=torch.int32), torch.full((len(i),), 0.5)).any()


@gpu
@pytest.mark.parametrize("hmax", [0.0, -1.0, float("inf"), float("nan")])
def test_binding_refuses_bad_hmax(hmax):
    from dff_amd import binding
    x = torch.zeros((3, 10, 3), device="cuda")
    hm = torch.full((28,), 0.5)
    hm[17] = hmax
    with pytest.raises(ValueError, match="hmax"):
        binding.pwd_hist(x, 3, torch.full((28,), 5, dtype=torch.int32), hm)


@gpu
def test_evaluator_leaves_nonfinite_frames_out(golden, tmp_path):
    """seven non-finite frames among the samples, three among the reference structures: the same JS, bit for bit"""
    from dff_amd.evaluate import PwdEvaluator
    g = golden("pwd_synth_n10_off3.npz")

    def damaged(x, at):
        out = np.insert(x, at, x[:len(at)], axis=0)
        rows = np.asarray(at) + np.arange(len(at))
        for k, r in enumerate(rows):
            if k == 0:
                out[r] = np.nan
            else:
                out[r, k % 10, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
        return torch.from_numpy(out)

    xs = damaged(g["x_samp"], [0, 1, 64, 64, 200, len(g["x_samp"]) - 1, len(g["x_samp"])])
    e = PwdEvaluator(damaged(g["x_val"], [0, 63, len(g["x_val"])]), mol_name="synth", offset=3,
                     saved_ref=str(tmp_path / "ref.pickle"))
    assert e.refs_nonfinite == 3 and e.samples_nonfinite == 0
    assert np.array_equal(e.gt_max.numpy(), g["gt_max"])
    js = e.eval(xs)
    assert isinstance(js, float) and js == float(g["js"]) and e.samples_nonfinite == 7
    assert e.eval(torch.from_numpy(g["x_samp"])) == float(g["js"]) and e.samples_nonfinite == 0
    e2 = PwdEvaluator(None, mol_name="synth", offset=3, saved_ref=str(tmp_path / "ref.pickle"))
    assert e2.refs_nonfinite == 0 and e2.eval(xs.cuda()) == float(g["js"]) and e2.samples_nonfinite == 7


@gpu
def test_evaluator_refusals(golden, tmp_path):
    from dff_amd.evaluate import PwdEvaluator
    g = golden("pwd_synth_n10_off3.npz")
    ref = str(tmp_path / "ref.pickle")
    e = PwdEvaluator(torch.from_numpy(g["x_val"]), mol_name="synth", offset=3, saved_ref=ref)
    with pytest.raises(ValueError, match="no finite frame"):
        e.eval(torch.full((5, 10, 3), float("nan")))
    with pytest.raises(ValueError, match="no finite frame"):
        PwdEvaluator(torch.full((5, 10, 3), float("inf")), mol_name="synth", offset=3, saved_ref=str(tmp_path / "none.pickle"))
    for coord in (3e19, 5000.0):                           # the square overflows; 5000 Angstrom need > 30719 bins
        x = g["x_samp"].copy()
        x[17, 6, 2] = coord
        with pytest.raises(ValueError) as err:
            e.eval(torch.from_numpy(x))
        msg = str(err.value)
        assert "nbins must be" not in msg and "3071.9" in msg and "30719" in msg
        assert "beads 0 and 6 (pair 3)" in msg                # the first of the pairs of bead 6
        d = float(re.search(r"reaches (\S+) Angstrom", msg).group(1))
        assert d == float("inf") if coord == 3e19 else 4900 < d < 5100
    assert e.eval(torch.from_numpy(g["x_samp"])) == float(g["js"])     # and the evaluator is none the worse for it
