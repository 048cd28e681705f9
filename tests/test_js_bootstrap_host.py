"""Host side of the Jensen-Shannon bootstrap: bin_indices_1d / bin_indices_2d against np.histogram / np.histogram2d on every
edge, sample_units, JsBootstrap's statistics, bootstrap_js and Evaluator.eval_bootstrap on the oracle (tests/js_cases.py)
behind the js_resampler seam, the symbols and every host refusal of dff_unit_hist / dff_resampled_js.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import js_cases as jc
from dff_amd import binding, evaluate
from support import owning_unit, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("dff_unit_hist_workspace_bytes", "dff_unit_hist", "dff_resampled_js_workspace_bytes", "dff_resampled_js",
         "dff_resampled_js_path_for", "dff_debug_resampled_js_path")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used


@pytest.fixture
def on_host(monkeypatch):
    """evaluate.js_resampler -> the numpy oracle"""
    jc.OracleResampler.calls = []
    monkeypatch.setattr(evaluate, "js_resampler", jc.OracleResampler)
    return jc.OracleResampler


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_library_and_package():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_unit_hist"][1]) == 12 and len(binding.SYMBOLS["dff_resampled_js"][1]) == 14
    for name in ("bin_indices_1d", "bin_indices_2d", "sample_units", "unit_histograms", "js_resampler", "bootstrap_js", "JsBootstrap"):
        assert name in dff_amd.__all__ and getattr(dff_amd, name) is getattr(evaluate, name)
    for cls in (evaluate.PwdEvaluator, evaluate.TicEvaluator, evaluate.DihedralEnergiesEvaluator, evaluate.Evaluator):
        assert callable(cls.eval_bootstrap)
    assert '#include "dff_jsboot.hip"' in owning_unit("dff_jsboot.hip")
    assert "dff_jsboot.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_workspace_bytes_do_not_grow_with_resamples_or_bins():
    lib = binding.load_library()
    assert binding.unit_hist_workspace_bytes(7, 3) == (7 + 1 + 3) * 8
    assert binding.resampled_js_workspace_bytes(7, 3) == (3 + 21 + 3) * 8          # no B, no ld among its arguments
    assert binding.resampled_js_workspace_bytes(65536, 1) == (1 + 65536 + 1) * 8
    for fn in (lib.dff_unit_hist_workspace_bytes, lib.dff_resampled_js_workspace_bytes):
        for bad in ((0, 1), (65537, 1), (1, 0), (1, (1 << 18) + 1)):
            assert fn(*bad) == -1, bad
    with pytest.raises(ValueError, match="resampling units must be 1..65536"):
        binding.resampled_js_workspace_bytes(0, 1)


def test_refusals_before_any_device_call():
    lib = binding.load_library()

    def uh(n=10, C_=2, units=(4, 6), nbins=(3, 5), ld=5, bins=FAKE, hist=FAKE, ws=FAKE, wsb=1 << 20, U=None):
        units, nbins = np.array(units, np.int64), np.array(nbins, np.int32)
        return lib.dff_unit_hist(0, bins, n, C_, p(units), len(units) if U is None else U, p(nbins), ld, hist, ws, wsb, None)
    refused(lib, uh(U=0), "resampling units must be 1..65536")
    refused(lib, uh(U=65537), "resampling units must be 1..65536")
    refused(lib, uh(C_=0), "channels must be 1..262144")
    refused(lib, uh(ld=0), "row stride ld must be 1..1048576")
    refused(lib, uh(ld=(1 << 20) + 1), "row stride ld must be 1..1048576")
    refused(lib, uh(units=[0] * 65536, C_=1, nbins=(1,), ld=1 << 17, n=0), "U C ld must not exceed 2^32")
    refused(lib, uh(nbins=(3, 6)), "channel 1 has 6 bins, must be 1..ld = 5")
    refused(lib, uh(nbins=(0, 5)), "channel 0 has 0 bins")
    refused(lib, uh(units=(4, 5)), "unit lengths sum to 9, not n = 10")
    refused(lib, uh(units=(4, 7)), "unit lengths sum to more than n = 10")
    refused(lib, uh(units=(11, -1)), "unit lengths sum to more than n = 10")
    refused(lib, uh(units=(10, -1, 1)), "unit 1 has negative length")
    refused(lib, uh(n=-1), "negative count")
    refused(lib, uh(n=(1 << 31) + 1, units=((1 << 31) + 1,)), "more than 2^31 frames")
    refused(lib, uh(bins=None), "null bins")
    refused(lib, uh(hist=None), "null output")
    refused(lib, uh(wsb=(2 + 1 + 2) * 8 - 1), "workspace of 39 bytes, 40 needed")
    refused(lib, uh(ws=C.c_void_p(4100)), "8-byte aligned")

    def rj(U=3, C_=2, ld=5, nbins=(3, 5), B=4, hist=FAKE, w=FAKE, ref=FAKE, js=FAKE, ws=FAKE, wsb=1 << 20):
        nbins = np.array(nbins, np.int32)
        return lib.dff_resampled_js(0, hist, U, C_, ld, p(nbins), w, B, ref, js, None, ws, wsb, None)
    refused(lib, rj(U=0), "resampling units must be 1..65536")
    refused(lib, rj(U=65537), "resampling units must be 1..65536")
    refused(lib, rj(C_=0), "channels must be 1..262144")
    refused(lib, rj(ld=0), "row stride ld must be 1..1048576")
    refused(lib, rj(U=65536, C_=1, nbins=(1,), ld=1 << 17), "U C ld must not exceed 2^32")
    refused(lib, rj(nbins=(6, 5)), "channel 0 has 6 bins, must be 1..ld = 5")
    refused(lib, rj(B=0), "resamples must be 1..4096")
    refused(lib, rj(B=4097), "resamples must be 1..4096")
    for null in ("hist", "w", "ref", "js"):
        refused(lib, rj(**{null: None}), "null histograms / weights / reference / output")
    refused(lib, rj(wsb=(2 + 6 + 2) * 8 - 1), "workspace of 79 bytes, 80 needed")
    refused(lib, rj(ws=C.c_void_p(4100)), "8-byte aligned")


def test_resample_tile_choice():
    """the power of two that holds min(B, 8) resamples per workgroup, halved until the call has 512 workgroups; every tile gives the same bits (GPU test)"""
    lib = binding.load_library()
    assert lib.dff_debug_resampled_js_path(0) == 0
    want = {(1, 1): 1, (100, 1): 1, (1000, 1): 1, (4096, 1): 8, (2048, 1): 4, (1024, 1): 2, (100, 55): 8, (16, 55): 1, (200, 28): 8,
            (1, 630): 1, (2, 630): 2, (3, 630): 4, (5, 630): 8, (7, 100): 1, (1, 1 << 18): 1}
    for (Bn, Cn), tb in want.items():
        assert binding.resampled_js_path_for(Bn, Cn) == tb, (Bn, Cn)
    for forced in (1, 2, 4, 8):
        assert lib.dff_debug_resampled_js_path(forced) == 0
        assert [binding.resampled_js_path_for(*s) for s in ((1, 1), (4096, 630))] == [forced] * 2
    refused(lib, lib.dff_debug_resampled_js_path(3), "0 (by shape) or 1, 2, 4, 8")
    assert lib.dff_debug_resampled_js_path(0) == 0
    for bad in ((0, 1), (4097, 1), (1, 0)):
        assert lib.dff_resampled_js_path_for(*bad) == -1, bad


# ---------------------------------------------------------------- binning
def edge_values(edges):
    """every edge, its two float64 neighbours, the mid points, just outside both ends, NaN and the infinities"""
    e = np.asarray(edges, np.float64)
    v = np.concatenate((e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), (e[1:] + e[:-1]) / 2,
                        [e[0] - 1.0, e[-1] + 1.0, np.nan, np.inf, -np.inf]))
    return v


def counts_of(idx, nb):
    idx = idx.numpy()
    assert idx.dtype == np.int32 and idx.min() >= -1 and idx.max() < nb
    return np.bincount(idx[idx >= 0], minlength=nb)


def tic_edges():
    t = evaluate.load_tica_reference(os.path.join(GOLDEN, "saved_TICA_CHIGNOLIN_testset.pickle"))
    return np.asarray(t["bin_edges_x"]), np.asarray(t["bin_edges_y"])


@pytest.mark.parametrize("which", ["tic_x", "tic_y", "dihedral", "uneven"])
def test_bin_indices_1d_counts_equal_np_histogram(which):
    ex, ey = tic_edges()
    edges = {"tic_x": ex, "tic_y": ey, "dihedral": np.linspace(-np.pi, np.pi, 61), "uneven": np.array([-1.0, 0.0, 0.125, 3.0])}[which]
    rng = np.random.default_rng(5)
    v = np.concatenate((edge_values(edges), rng.uniform(edges[0] - 0.1, edges[-1] + 0.1, 5000)))
    idx = evaluate.bin_indices_1d(torch.from_numpy(v), edges)
    finite = v[np.isfinite(v)]
    assert np.array_equal(counts_of(idx, len(edges) - 1), np.histogram(finite, bins=edges)[0])
    got = idx.numpy()
    assert got[np.flatnonzero(v == edges[-1])[0]] == len(edges) - 2                     # the last edge: the last bin
    assert (got[~np.isfinite(v)] == -1).all() and (got[(v < edges[0]) | (v > edges[-1])] == -1).all()
    v32 = v.astype(np.float32)                                                         # float32 values are compared as float64
    assert np.array_equal(counts_of(evaluate.bin_indices_1d(torch.from_numpy(v32), edges), len(edges) - 1),
                          np.histogram(v32[np.isfinite(v32)].astype(np.float64), bins=edges)[0])


@pytest.mark.parametrize("which", ["tic", "dihedral"])
def test_bin_indices_2d_counts_equal_np_histogram2d(which):
    ex, ey = tic_edges() if which == "tic" else (np.linspace(-np.pi, np.pi, 61),) * 2
    rng = np.random.default_rng(6)
    vx, vy = edge_values(ex), edge_values(ey)
    x = np.concatenate((np.repeat(vx, 7)[:2000], rng.uniform(ex[0] - 0.1, ex[-1] + 0.1, 6000)))
    y = np.concatenate((np.tile(vy, 7)[:2000], rng.uniform(ey[0] - 0.1, ey[-1] + 0.1, 6000)))
    xy = np.stack((x, y), axis=1)
    idx = evaluate.bin_indices_2d(torch.from_numpy(xy), ex, ey)
    ok = np.isfinite(xy).all(axis=1)
    want = np.histogram2d(x[ok], y[ok], bins=[ex, ey])[0]
    nb = (len(ex) - 1) * (len(ey) - 1)
    assert np.array_equal(counts_of(idx, nb).reshape(want.shape), want.astype(np.int64))      # ix * ny + iy = flatten()
    assert (idx.numpy()[~ok] == -1).all()
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        evaluate.bin_indices_2d(torch.zeros(4, 3), ex, ey)


# ---------------------------------------------------------------- units
def test_sample_units():
    for n, k in ((1000, 256), (1000, 7), (256, 256), (5, 256), (1, 1)):
        u = evaluate.sample_units(n, n_blocks=k)
        assert u.dtype == np.int64 and u.sum() == n and len(u) == min(k, n)
        assert u.max() - u.min() <= 1 and (np.diff(u) <= 0).all() and (u[: n % len(u)] == n // len(u) + 1).all()
    lengths = [700, 0, 1, 64, 0, 235]
    assert np.array_equal(evaluate.sample_units(1000, lengths), evaluate.resampling_units(lengths))
    assert np.array_equal(evaluate.sample_units(1000, lengths, block_frames=100), evaluate.resampling_units(lengths, 100))
    assert evaluate.sample_units(1000, lengths, block_frames=100).sum() == 1000
    with pytest.raises(ValueError, match="add up to"):
        evaluate.sample_units(999, lengths)
    with pytest.raises(ValueError):
        evaluate.sample_units(0)
    assert evaluate.sample_units(0, [0, 0]).tolist() == [0, 0]           # empty trajectories stay, as units without a frame
    with pytest.raises(ValueError, match="no frames"):
        evaluate.sample_units(0, [0, 0], block_frames=10)


# ---------------------------------------------------------------- statistics
def test_js_bootstrap_statistics_with_nan_rows():
    rng = np.random.default_rng(2)
    per = rng.random((40, 3))
    per[3, 1] = per[17] = np.nan
    b = evaluate.JsBootstrap(per, np.array([0.2, 0.4, 0.6]), None, None)
    assert np.array_equal(b.values[np.isfinite(b.values)], per.mean(axis=1)[np.isfinite(per).all(axis=1)])
    assert b.n_failed == 2 and abs(b.point - 0.4) < 1e-15
    assert b.std() == evaluate.percentile_std(b.values[:, None])[0]
    for conf in (0.95, 0.5):
        lo, hi = evaluate.percentile_interval(b.values[:, None], conf)
        assert b.interval(conf) == (lo[0], hi[0])
    fin = b.values[np.isfinite(b.values)]
    assert b.bias() == fin.mean() - b.point and lo[0] <= np.median(fin) <= hi[0]
    dead = evaluate.JsBootstrap(np.full((4, 2), np.nan), np.array([0.1, 0.1]), None, None)
    assert dead.n_failed == 4 and np.isnan(dead.std()) and np.isnan(dead.bias()) and np.isnan(dead.interval()[0])


# ---------------------------------------------------------------- bootstrap_js on the oracle
def test_bootstrap_js_on_the_oracle(on_host):
    nbins = np.array([17, 300, 1], np.int32)
    units = np.array([0, 1, 63, 64, 65, 0, 807], np.int64)
    bins = jc.binned_frames(1000, nbins, seed=3)
    hist = jc.unit_hists(bins, nbins, units)
    ref = np.random.default_rng(4).random((3, 300))
    bs = evaluate.bootstrap_js(hist, nbins, ref, n_resamples=25, seed=9, unit_lengths=units, resample_batch=7)
    assert np.array_equal(bs.weights, evaluate.bootstrap_weights(len(units), 25, 9)) and bs.weights.dtype == np.uint32
    assert [len(w) for w in on_host.calls] == [7, 7, 7, 4, 1] and np.array_equal(on_host.calls[-1], np.ones((1, 7), np.uint32))
    assert np.array_equal(np.concatenate(on_host.calls[:-1]), bs.weights)
    pooled = jc.unit_hists(bins, nbins, [1000])[0]
    for c, nb in enumerate(nbins):
        assert bs.point_per_channel[c] == evaluate.js_divergence(pooled[c, :nb].astype(np.float64), ref[c, :nb])
    assert bs.point == bs.point_per_channel.mean() and bs.per_channel.shape == (25, 3) and bs.values.shape == (25,)
    assert np.array_equal(bs.per_channel, jc.resampled_js(hist, nbins, bs.weights, ref)[0])
    assert np.array_equal(bs.values, bs.per_channel.mean(axis=1)) and np.array_equal(bs.unit_lengths, units)
    assert bs.n_failed == 0 and bs.std() > 0 and bs.interval()[0] < bs.interval()[1]
    one = evaluate.bootstrap_js(hist, nbins, ref, weights=bs.weights[:3])                  # given weights; any split, the same bits
    assert np.array_equal(one.per_channel, bs.per_channel[:3])
    with pytest.raises(ValueError, match=r"weights must be \(B, 7\)"):
        evaluate.bootstrap_js(hist, nbins, ref, weights=np.ones((3, 6), np.uint32))


class _FixedMetric:
    """a sub-evaluator of Evaluator.eval_bootstrap on fixed binned frames: records what it was given"""

    def __init__(self, nbins, seed):
        self.nbins, self.seed, self.seen = np.array(nbins, np.int32), seed, None

    def eval_bootstrap(self, samples, **kw):
        self.seen = kw
        units = kw["unit_lengths"]
        hist = jc.unit_hists(jc.binned_frames(len(samples), self.nbins, self.seed), self.nbins, units)
        ref = np.random.default_rng(self.seed).random((len(self.nbins), int(self.nbins.max())))
        return evaluate.bootstrap_js(hist, self.nbins, ref, weights=kw["weights"], unit_lengths=units)


@pytest.mark.parametrize("mol", ["chignolin", "alanine_dipeptide", "protein_g"])
def test_evaluator_eval_bootstrap_keys_and_joint_weights(mol, on_host):
    e = object.__new__(evaluate.Evaluator)
    e.mol_name, e.eval_folder = mol, None
    e.tic = e.dihedral_evaluator = first = _FixedMetric([400], 1)
    e.pwd_evaluator = pwd = _FixedMetric([30, 41, 17], 2)
    samples = np.zeros((500, 10, 3), np.float32)
    res = e.eval_bootstrap(samples, traj_lengths=[200, 300], block_frames=50, n_resamples=12, seed=4)
    keys = {"protein_g": [], "chignolin": ["TIC JS", "PWD JS"], "alanine_dipeptide": ["Dihedral JS", "PWD JS"]}[mol]
    assert set(res) == {k + s for k in keys for s in ("", "_lo", "_hi", "_std", "_bias")} | {"n_units", "n_resamples"}
    assert res["n_units"] == 10 and res["n_resamples"] == 12
    if keys:
        w = evaluate.bootstrap_weights(10, 12, 4)
        assert np.array_equal(first.seen["weights"], w) and first.seen["weights"] is pwd.seen["weights"]     # resampled jointly
        assert np.array_equal(first.seen["unit_lengths"], [50] * 10)
        for k in keys:
            assert res[k + "_lo"] <= res[k + "_hi"] and res[k + "_std"] > 0 and np.isfinite(res[k + "_bias"]) and res[k] > 0
    assert evaluate.Evaluator.eval_bootstrap(e, samples, n_blocks=7, n_resamples=3)["n_units"] == 7


def test_tool_arguments():
    text = open(os.path.join(ROOT, "tools_eval_samples.py")).read()
    for flag in ("--js-bootstrap", "--block-frames", "--js-blocks"):
        assert flag in text
    assert '"js_bootstrap"' in text and "eval_bootstrap" in text
