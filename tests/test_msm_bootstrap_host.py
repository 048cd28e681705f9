"""Host side of the Markov-state-model bootstrap: the symbols and refusals of dff_micro_resampled_counts /
dff_msm_reversible_steps_batched (refused on the host, before any device call), resampling_units and bootstrap_weights,
bootstrap_msm on numpy stand-ins behind its two device seams against the from-scratch oracle (oracle/msm_bootstrap.py)
and against MarkovStateModel.fit_counts resample by resample, the percentile intervals, MsmEvaluator's dict with and without
a bootstrap, the tool's arguments, and the calibration of the error bars on a two-state chain with a known timescale.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from dff_amd import binding, evaluate
from oracle import msm_bootstrap as boot
from oracle import msm as oracle
from standins import OracleSweeps
from support import refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_micro_resampled_counts_workspace_bytes", "dff_micro_resampled_counts", "dff_msm_batched_workspace_bytes",
         "dff_msm_reversible_steps_batched", "dff_msm_batched_driver_for")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_micro_resampled_counts"][1]) == 15
    assert len(binding.SYMBOLS["dff_msm_reversible_steps_batched"][1]) == 13
    assert binding.SYMBOLS["dff_msm_batched_workspace_bytes"][0] is C.c_longlong
    assert binding.MSM_MAX_BATCH == evaluate.MSM_MAX_BATCH == 4096
    for src in ("dff_msm.hip", "dff_msm_batch.hip"):                     # one copy of the row arithmetic
        text = open(os.path.join(ROOT, "two-for-one-diffusion_amd", "csrc", src)).read()
        assert "dff_msm_rows.h" in text or "dff_msm.hip" in text
        assert not re.search(r"double\s+msm_(q|row)\s*\(", text), src


def test_workspace_bytes():
    lib = binding.load_library()
    assert binding.micro_resampled_counts_workspace_bytes(3, 5) == (4 + 6) * 8
    assert binding.micro_resampled_counts_workspace_bytes(0, 1 << 20) == (1 + (1 << 20) + 1) * 8
    for bad in ((-1, 1), (1, 0), (1, (1 << 20) + 1)):
        assert lib.dff_micro_resampled_counts_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="resampling units must be 1..1048576"):
        binding.micro_resampled_counts_workspace_bytes(1, 0)
    assert binding.msm_batched_workspace_bytes(1, 1) == 24 and binding.msm_batched_workspace_bytes(70, 300) == (2 * 70 * 300 + 70) * 8
    for bad in ((0, 4), (4097, 4), (4, 0), (4, 1025)):
        assert lib.dff_msm_batched_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="problems must be 1..4096"):
        binding.msm_batched_workspace_bytes(4097, 4)


def test_refusals_before_any_device_call():
    lib = binding.load_library()
    ten = np.array([10], np.int64)

    def rc(n=10, lengths=ten, units=ten, lag=1, K=4, B=2, labels=FAKE, weights=FAKE, ws=FAKE, wsb=1 << 20):
        return lib.dff_micro_resampled_counts(0, labels, n, p(lengths), len(lengths), p(units), len(units), lag, K, weights, B, FAKE,
                                              ws, wsb, None)
    refused(lib, rc(K=0), "states must be 1..1024")
    refused(lib, rc(K=1025), "states must be 1..1024")
    refused(lib, rc(B=0), "resamples must be 1..4096")
    refused(lib, rc(B=4097), "resamples must be 1..4096")
    refused(lib, rc(K=1024, B=257), "must not exceed 2^28")
    assert lib.dff_micro_resampled_counts(0, FAKE, 10, p(ten), 1, p(ten), 0, 1, 4, FAKE, 2, FAKE, FAKE, 1 << 20, None) == 1
    assert "resampling units must be 1..1048576" in lib.dff_last_error().decode()
    refused(lib, rc(lag=0), "must be >= 1")
    refused(lib, rc(n=-1), "negative count")
    refused(lib, rc(n=(1 << 31) + 1, lengths=np.array([(1 << 31) + 1], np.int64)), "more than 2^31 frames")
    refused(lib, rc(labels=None), "null labels")
    refused(lib, rc(lengths=np.array([4, 5], np.int64)), "sum to 9, not n = 10")
    refused(lib, rc(units=np.array([4, 5], np.int64)), "unit lengths sum to 9, not n = 10")
    refused(lib, rc(units=np.array([4, 7], np.int64)), "unit lengths sum to more than n = 10")
    refused(lib, rc(units=np.array([10, -1], np.int64)), "unit 1 has negative length")
    refused(lib, rc(weights=None), "null weights")
    refused(lib, rc(wsb=31), "workspace of 31 bytes, 32 needed")
    refused(lib, rc(ws=C.c_void_p(4100)), "8-byte aligned")

    def ms(ks=(4, 3), Kmax=4, steps=1, skip=None, wsb=1 << 20, ws=FAKE, B=None, sym=FAKE):
        ks = np.array(ks, np.int32)
        return lib.dff_msm_reversible_steps_batched(0, sym, FAKE, p(ks), skip, len(ks) if B is None else B, Kmax, FAKE, steps, None,
                                                    ws, wsb, None)
    refused(lib, ms(B=0), "problems must be 1..4096")
    refused(lib, ms(ks=[1] * 4097, Kmax=1), "problems must be 1..4096")
    refused(lib, ms(Kmax=0), "states must be 1..1024")
    refused(lib, ms(Kmax=1025), "states must be 1..1024")
    refused(lib, ms(steps=-1), "negative n_steps")
    refused(lib, ms(ks=(4, 5)), "problem 1 has 5 states, must be 1..Kmax = 4")
    refused(lib, ms(ks=(0, 4)), "problem 0 has 0 states")
    refused(lib, ms(sym=None), "null matrices")
    refused(lib, ms(wsb=(2 * 2 * 4 + 2) * 8 - 1), "workspace of 143 bytes, 144 needed")
    refused(lib, ms(ws=C.c_void_p(4100)), "8-byte aligned")


def test_batched_driver_choice():
    """the measured crossover: one looping workgroup per problem up to 32 states as the single call, and
    beyond that from 4 live problems on at 64 states, 8 at 128 and 256, 16 at 512, 32 at 1024"""
    lib = binding.load_library()
    assert lib.dff_debug_msm_driver(0) == 0
    loop_from = {1: 1, 32: 1, 33: 4, 64: 4, 127: 4, 128: 8, 256: 8, 257: 9, 512: 16, 1024: 32}
    for K, first in loop_from.items():
        for Bn in (1, 2, 3, 4, 7, 8, 9, 15, 16, 31, 32, 4096):
            assert binding.msm_batched_driver_for(Bn, K) == (2 if Bn >= first else 1), (K, Bn)
    for forced in (1, 2):
        assert lib.dff_debug_msm_driver(forced) == 0
        assert [binding.msm_batched_driver_for(Bn, K) for Bn, K in ((1, 1), (1, 1024), (4096, 64))] == [forced] * 3
    assert lib.dff_debug_msm_driver(0) == 0
    for bad in ((0, 4), (4097, 4), (4, 0), (4, 1025)):
        assert lib.dff_msm_batched_driver_for(*bad) == -1, bad
    assert [binding.msm_driver_for(K) for K in (32, 33)] == [2, 1]          # the single call's choice stands


def test_package_reexports():
    for name in ("resampling_units", "bootstrap_weights", "bootstrap_msm", "MsmBootstrap", "implied_timescales_bootstrap"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("micro_resampled_counts", "micro_resampled_counts_workspace_bytes", "msm_reversible_steps_batched",
                 "msm_batched_workspace_bytes"):
        assert callable(getattr(binding, name))
    assert callable(evaluate.resampled_counter) and callable(evaluate.batched_reversible_sweeper)


# ---------------------------------------------------------------- units and weights
def test_resampling_units():
    for lengths, bf in (([5, 0, 3], None), ([5, 0, 3], 2), ([5, 0, 3], 10), ([5, 0, 3], 1), ([4, 4], 2), ([], None), ([], 3),
                        ([0, 0], 4), ([7], 7), ([7], 6)):
        got = evaluate.resampling_units(lengths, bf)
        assert got.dtype == np.int64 and got.tolist() == boot.units(lengths, bf).tolist(), (lengths, bf)
        assert got.sum() == sum(lengths)
    assert evaluate.resampling_units([5, 0, 3]).tolist() == [5, 0, 3]                   # the trajectories, empty ones included
    assert evaluate.resampling_units([5, 0, 3], 2).tolist() == [2, 2, 1, 2, 1]          # a shorter last block is its own unit
    assert evaluate.resampling_units([5, 0, 3], 10).tolist() == [5, 3]
    assert evaluate.resampling_units([3, 2], 1).tolist() == [1] * 5
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="block_frames"):
            evaluate.resampling_units([5], bad)
    with pytest.raises(ValueError, match="negative"):
        evaluate.resampling_units([5, -1])


def test_bootstrap_weights_are_the_pinned_draws():
    for n_units, B, seed in ((1, 1, 0), (7, 3, 5), (200, 65, 12345)):
        w = evaluate.bootstrap_weights(n_units, B, seed)
        want = np.random.default_rng(seed).multinomial(n_units, np.full(n_units, 1 / n_units), size=B)
        assert w.dtype == np.uint32 and w.shape == (B, n_units) and np.array_equal(w, want)
        assert np.array_equal(w, boot.weights(n_units, B, seed)) and (w.sum(axis=1) == n_units).all()
    with pytest.raises(ValueError):
        evaluate.bootstrap_weights(0, 3, 1)
    with pytest.raises(ValueError):
        evaluate.bootstrap_weights(3, 0, 1)


# ---------------------------------------------------------------- connected sets by reachability
def test_reachability_shortcut_gives_the_oracles_connected_sets():
    """largest_connected_set settles the usual count matrix (a giant component and a few lost states) by a few array searches
    and leaves the rest to its Tarjan walk: the same sets either way, ties and all."""
    taken = 0
    for seed in range(300):
        rng = np.random.default_rng(seed)
        K = int(rng.integers(1, 40))
        c = (rng.random((K, K)) < rng.choice([0.5, 1.0, 1.5, 3.0, 8.0]) / K) * rng.integers(1, 9, (K, K))
        want = oracle.largest_connected_set(c)
        assert np.array_equal(evaluate.largest_connected_set(c), want), seed
        fast = evaluate._largest_by_reachability(c > 0)
        taken += fast is not None
        assert fast is None or (fast.dtype == np.int64 and np.array_equal(fast, want)), seed
    assert 50 < taken < 300                                           # both routes are exercised
    labels, lengths, w = boot.five_state_case()
    for Cb in boot.weighted_counts(labels, lengths, lengths, 2, 5, w):
        assert np.array_equal(evaluate._largest_by_reachability(Cb > 0), oracle.largest_connected_set(Cb))
    chain = np.diag(np.ones(299), 1)                                  # deeper than the searches go: left to Tarjan
    assert evaluate._largest_by_reachability(chain > 0) is None and evaluate.largest_connected_set(chain).tolist() == [0]
    two = np.zeros((7, 7))                                            # two components of three: the lower index wins
    for a, b in ((4, 5), (5, 6), (6, 4), (1, 3), (3, 2), (2, 1), (3, 4)):
        two[a, b] = 2
    assert evaluate._largest_by_reachability(two > 0).tolist() == [1, 2, 3]
    assert evaluate._largest_by_reachability(np.zeros((0, 0), bool)) is None


# ---------------------------------------------------------------- the pipeline on stand-ins
@pytest.fixture
def on_oracle(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "resampled_counter", boot.Counter)
    monkeypatch.setattr(evaluate, "batched_reversible_sweeper", boot.Sweeper)
    boot.Counter.calls = boot.Sweeper.calls = 0


five_state_case = boot.five_state_case


def same_model(m, f, K, what):
    """a MarkovStateModel-like result against the oracle's dict of one resample"""
    assert np.array_equal(m.active_set, f["active_set"]) and m.n_iter == f["n_iter"] and bool(m.converged) == f["converged"], what
    assert m.transition_matrix.shape == f["T"].shape and np.abs(m.transition_matrix - f["T"]).max() <= 1e-14, what
    assert np.abs(m.stationary_distribution - f["pi"]).max() <= 1e-14, what


def test_bootstrap_on_stand_ins_equals_the_oracle_and_fit_counts(on_oracle):
    labels, lengths, w = five_state_case()
    lag, K, k = 2, 5, 3
    settings = dict(tol=1e-12, max_iter=100000, steps_per_sync=16)
    bs = evaluate.bootstrap_msm(labels, lag, lengths, K, weights=w, k=k, device="cpu", **settings)
    want = boot.bootstrap(labels, lengths, lengths, lag, K, w, k=k, **settings)
    assert isinstance(bs, evaluate.MsmBootstrap) and bs.timescales.shape == (len(w), k) and bs.stationary.shape == (len(w), K)
    assert np.array_equal(bs.weights, w) and bs.weights.dtype == np.uint32 and bs.unit_lengths.tolist() == lengths
    assert np.array_equal(bs.n_active, want["n_active"]) and np.array_equal(bs.converged, want["converged"])
    assert np.array_equal(bs.n_iter, want["n_iter"]) and np.allclose(bs.active_count_share, want["share"], rtol=1e-15, atol=0)
    assert sorted(set(bs.n_active.tolist()))[:2] == [1, 4] and 5 in bs.n_active            # collapsed, lost a state, whole
    assert bs.n_active[2] == 1 and bs.n_iter[2] == 0 and bs.converged[2] and np.isnan(bs.timescales[2]).all()
    assert bs.stationary[2].tolist() == [1.0, 0, 0, 0, 0] and bs.n_active[1] == 4 and bs.stationary[1, 4] == 0.0
    assert len(set(bs.n_iter[bs.n_active > 1].tolist())) > 1                                # they stop in different sweeps
    assert np.array_equal(np.isnan(bs.timescales), np.isnan(want["timescales"]))
    ok = ~np.isnan(bs.timescales)
    assert np.allclose(bs.timescales[ok], want["timescales"][ok], rtol=1e-9, atol=0)
    assert np.abs(bs.stationary - want["stationary"]).max() <= 1e-14 and np.allclose(bs.stationary.sum(axis=1), 1.0)
    # resample by resample: MarkovStateModel.fit_counts of the oracle's weighted counts, bit for bit
    for b, Cb in enumerate(want["counts"]):
        m = evaluate.MarkovStateModel(lag, device="cpu", **settings).fit_counts(Cb)
        same_model(m, want["fits"][b], K, b)
        assert m.n_iter == bs.n_iter[b] and m.converged == bs.converged[b] and m.active_count_share == bs.active_count_share[b]
        assert m.timescales(k).tobytes() == bs.timescales[b].tobytes(), b
        full = np.zeros(K)
        full[m.active_set] = m.stationary_distribution
        assert full.tobytes() == bs.stationary[b].tobytes(), b
    # the point model is the plain counts' model
    plain = oracle.transition_counts(labels, lengths, [lag], K)[0]
    assert np.array_equal(bs.point.count_matrix, plain) and np.array_equal(want["counts"][0].astype(np.int64), plain)
    assert bs.point.timescales(k).tobytes() == bs.timescales[0].tobytes()
    # batches of one resample, blocks as units, drawn weights
    one = evaluate.bootstrap_msm(labels, lag, lengths, K, weights=w, k=k, resample_batch=1, device="cpu", **settings)
    assert one.timescales.tobytes() == bs.timescales.tobytes() and np.array_equal(one.n_iter, bs.n_iter)
    blocks = evaluate.bootstrap_msm(labels, lag, lengths, K, n_resamples=6, block_frames=150, seed=4, k=k, device="cpu", **settings)
    ub = boot.units(lengths, 150)
    assert blocks.unit_lengths.tolist() == ub.tolist() == [150, 150, 150, 150, 100, 150, 150, 100, 150, 150, 150, 50]
    assert np.array_equal(blocks.weights, boot.weights(len(ub), 6, 4))
    wantb = boot.bootstrap(labels, lengths, ub, lag, K, blocks.weights, k=k, **settings)
    assert np.array_equal(blocks.n_iter, wantb["n_iter"]) and np.array_equal(blocks.n_active, wantb["n_active"])
    okb = ~np.isnan(wantb["timescales"])
    assert np.array_equal(~np.isnan(blocks.timescales), okb) and np.allclose(blocks.timescales[okb], wantb["timescales"][okb], rtol=1e-9)


def test_max_iter_exhausted_and_bad_arguments(on_oracle):
    labels, lengths, w = five_state_case()
    bs = evaluate.bootstrap_msm(labels, 1, lengths, 5, weights=w[:2], k=2, max_iter=3, steps_per_sync=2, device="cpu")
    want = boot.bootstrap(labels, lengths, lengths, 1, 5, w[:2], k=2, max_iter=3, steps_per_sync=2)
    assert not bs.converged.any() and bs.n_iter.tolist() == [3, 3] == want["n_iter"].tolist() and bs.n_failed == 2
    assert not bs.point.converged and bs.point.n_iter == 3 and boot.Sweeper.calls == 2
    assert np.allclose(bs.timescales, want["timescales"], rtol=1e-12)
    zero = evaluate.bootstrap_msm(labels, 1, lengths, 5, weights=w[:2], max_iter=0, device="cpu")
    assert zero.n_iter.tolist() == [0, 0] and not zero.converged.any() and boot.Sweeper.calls == 2
    for kw, what in ((dict(weights=np.ones((2, 3))), "weights"), (dict(weights=-np.ones((2, 4))), "weights"),
                     (dict(weights=np.full((1, 4), 2.0 ** 32)), "weights"), (dict(n_states=0), "n_states"),
                     (dict(n_states=1025), "n_states"), (dict(k=0), "k must"), (dict(resample_batch=0), "resample_batch"),
                     (dict(resample_batch=4097), "resample_batch"), (dict(tol=0.0), "tol"), (dict(n_resamples=0), "n_resamples"),
                     (dict(block_frames=0), "block_frames")):
        args = dict(n_states=5, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            evaluate.bootstrap_msm(labels, 1, lengths, **args)
    with pytest.raises(ValueError, match="lagtime"):
        evaluate.bootstrap_msm(labels, 0, lengths, 5, device="cpu")
    with pytest.raises(ValueError, match="no resampling units"):
        evaluate.bootstrap_msm(np.zeros(0, np.int32), 1, [], 3, device="cpu")


def test_intervals_std_and_n_failed():
    rng = np.random.default_rng(0)
    ts = rng.lognormal(2.0, 0.5, (41, 3))
    ts[[3, 17], 2] = np.nan
    ts[5] = np.nan
    conv = np.ones(41, bool)
    conv[[7, 5]] = False
    bs = evaluate.MsmBootstrap(ts, None, None, None, conv, None, None, None, None)
    assert bs.n_failed == 4                                          # 3, 17 (no third timescale), 5 (both), 7 (not converged)
    for conf in (0.95, 0.9, 0.5):
        lo, hi = bs.interval(conf)
        wlo, whi = boot.interval(ts, conf)
        assert np.allclose(lo, wlo, rtol=1e-14) and np.allclose(hi, whi, rtol=1e-14) and (lo < hi).all()
    assert np.allclose(bs.interval()[0], boot.interval(ts, 0.95)[0], rtol=1e-14)
    assert np.allclose(bs.std(), boot.std(ts), rtol=1e-13)
    empty = evaluate.MsmBootstrap(np.full((4, 2), np.nan), None, None, None, np.ones(4, bool), None, None, None, None)
    assert np.isnan(empty.interval()[0]).all() and np.isnan(empty.std()).all() and empty.n_failed == 4
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match="confidence"):
            bs.interval(bad)


def test_implied_timescales_bootstrap(on_oracle):
    labels, lengths, _ = five_state_case()
    point, lo, hi = evaluate.implied_timescales_bootstrap(labels, [1, 3], lengths, 5, k=2, n_resamples=5, seed=2, confidence=0.8,
                                                          steps_per_sync=16, device="cpu")
    assert point.shape == lo.shape == hi.shape == (2, 2)
    for i, lag in enumerate((1, 3)):
        want = boot.bootstrap(labels, lengths, lengths, lag, 5, boot.weights(4, 5, 2), k=2, steps_per_sync=16)
        wlo, whi = boot.interval(want["timescales"], 0.8)
        assert np.allclose(lo[i], wlo, rtol=1e-9, equal_nan=True) and np.allclose(hi[i], whi, rtol=1e-9, equal_nan=True)
        plain = boot.fit_counts(oracle.transition_counts(labels, lengths, [lag], 5)[0], lag, 2, steps_per_sync=16)
        assert np.allclose(point[i], plain["timescales"], rtol=1e-9)


# ---------------------------------------------------------------- the evaluator
@pytest.fixture
def host_evaluator(on_oracle, monkeypatch):
    """MsmEvaluator without a device: frames ARE state indices (n, 1, 1), the projection is the index itself, assignment
    rounds it, the plain counts are the oracle's."""
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.MsmEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None: {"labels": proj[:, 0].round().to(torch.int32)})
    monkeypatch.setattr(binding, "micro_transition_counts",
                        lambda lab, lengths, lags, K: torch.from_numpy(oracle.transition_counts(lab.numpy(), lengths, lags, K)))

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        return evaluate.MsmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), n_microstates=5, lagtime=2, n_timescales=2,
                                     frame_time=0.5, centers=np.arange(5.0).reshape(5, 1), device="cpu", **kw)
    return make


def frames_of(labels):
    return np.where(labels < 0, 0, labels).astype(np.float64).reshape(-1, 1, 1)


def test_evaluator_without_bootstrap_is_unchanged_and_with_it_gains_exactly_the_new_keys(host_evaluator):
    labels, lengths, _ = five_state_case()
    labels = np.where(labels < 0, 0, labels)
    refs = labels[::-1].copy()
    ref_lengths = lengths[::-1]
    keys = set(evaluate.MsmEvaluator.KEYS)
    assert keys == {"timescales", "n_active", "active_count_share", "converged", "samples_nonfinite"}
    old = host_evaluator().eval(frames_of(labels), lengths)
    plain = evaluate.MarkovStateModel(2, device="cpu").fit_counts(oracle.transition_counts(labels, lengths, [2], 5)[0])
    assert old == evaluate.MsmEvaluator.summarize(plain, 2, 0.5, 0) and set(old) == keys
    e0 = host_evaluator(ref_data=frames_of(refs), ref_traj_lengths=ref_lengths)
    old_ref = e0.eval(frames_of(labels), lengths)
    assert set(old_ref) == keys | {k + "_ref" for k in keys} | {"log10_timescale_ratio", "stationary_js"} and e0.bootstraps == {}
    new_keys = {"timescales_lo", "timescales_hi", "timescales_std", "bootstrap_failed"}
    e1 = host_evaluator(n_bootstrap=7, confidence=0.8, bootstrap_seed=11)
    got = e1.eval(frames_of(labels), lengths)
    assert set(got) == keys | new_keys and {k: got[k] for k in keys} == old and set(e1.bootstraps) == {"samples"}
    want = boot.bootstrap(labels, lengths, lengths, 2, 5, boot.weights(4, 7, 11), k=2)
    lo, hi = boot.interval(want["timescales"], 0.8)
    assert np.allclose(got["timescales_lo"], 0.5 * lo, rtol=1e-9) and np.allclose(got["timescales_hi"], 0.5 * hi, rtol=1e-9)
    assert np.allclose(got["timescales_std"], 0.5 * boot.std(want["timescales"]), rtol=1e-8)
    assert got["bootstrap_failed"] == float(np.sum(~want["converged"] | np.isnan(want["timescales"][:, -1])))
    e2 = host_evaluator(ref_data=frames_of(refs), ref_traj_lengths=ref_lengths, n_bootstrap=7, block_frames=100, bootstrap_seed=11)
    both = e2.eval(frames_of(labels), lengths)
    assert set(both) == set(old_ref) | new_keys | {k + "_ref" for k in new_keys} | {"log10_timescale_ratio_lo", "log10_timescale_ratio_hi"}
    assert {k: both[k] for k in old_ref} == old_ref and set(e2.bootstraps) == {"samples", "refs"}
    us, ur = boot.units(lengths, 100), boot.units(ref_lengths, 100)
    ws, wr = boot.weights(len(us), 7, 11), boot.weights(len(ur), 7, 12)                     # another seed for the reference
    assert np.array_equal(e2.bootstraps["samples"].weights, ws) and np.array_equal(e2.bootstraps["refs"].weights, wr)
    a = boot.bootstrap(labels, lengths, us, 2, 5, ws, k=2)["timescales"]
    b = boot.bootstrap(refs, ref_lengths, ur, 2, 5, wr, k=2)["timescales"]
    rlo, rhi = boot.interval(np.log10(a / b), 0.95)
    assert np.allclose(both["log10_timescale_ratio_lo"], rlo, atol=1e-9) and np.allclose(both["log10_timescale_ratio_hi"], rhi, atol=1e-9)
    for kw in (dict(n_bootstrap=-1), dict(confidence=1.0), dict(block_frames=0), dict(block_frames=2.5)):
        with pytest.raises(ValueError):
            host_evaluator(**kw)


class FramesDataset:
    """dataset-like: [:] is a tuple whose first entry is the frames, as the reference's datasets give them"""

    def __init__(self, frames):
        self.frames = frames

    def __getitem__(self, i):
        return self.frames[i], None


@pytest.mark.parametrize("n_bootstrap", [0, 3])
def test_reference_as_tensor_array_or_dataset_gives_one_reference_result(host_evaluator, n_bootstrap):
    labels, lengths, _ = five_state_case()
    frames = frames_of(labels)
    got = [host_evaluator(ref_data=form, ref_traj_lengths=lengths, n_bootstrap=n_bootstrap).ref_result
           for form in (torch.from_numpy(frames), frames, FramesDataset(frames))]
    assert got[0] is not None and set(evaluate.MsmEvaluator.KEYS) <= set(got[0])
    assert repr(got[0]) == repr(got[1]) == repr(got[2])                                      # repr: NaN compares equal to itself
    assert host_evaluator(ref_data=None).ref_result is None


def test_msm_bootstrap_arguments_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    a = ap.parse_args(base + ["--msm", "--msm-states", "9", "--msm-lag", "2"])
    assert a.msm_bootstrap is None and a.msm_block_frames is None and a.msm_confidence is None
    assert tool.msm_bootstrap_arguments(a) == {} and tool.msm_arguments(a) == (9, 2)
    a = ap.parse_args(base + ["--msm", "--msm-states", "9", "--msm-lag", "2", "--msm-bootstrap", "100"])
    assert tool.msm_bootstrap_arguments(a) == {"n_bootstrap": 100, "block_frames": None, "confidence": 0.95}
    a = ap.parse_args(base + ["--msm", "h.pt", "--msm-states", "9", "--msm-lag", "2", "--msm-bootstrap", "50", "--msm-block-frames",
                              "1000", "--msm-confidence", "0.9"])
    assert tool.msm_bootstrap_arguments(a) == {"n_bootstrap": 50, "block_frames": 1000, "confidence": 0.9}
    for bad in (["--msm-bootstrap", "0"], ["--msm-bootstrap", "x"], ["--msm-block-frames", "0"], ["--msm-confidence", "1"],
                ["--msm-confidence", "0"], ["--msm-confidence", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--msm"] + bad)
    with pytest.raises(SystemExit, match="needs --msm"):                                    # refused without --msm
        tool.msm_bootstrap_arguments(ap.parse_args(base + ["--msm-bootstrap", "10"]))
    for alone in (["--msm-block-frames", "10"], ["--msm-confidence", "0.9"]):
        with pytest.raises(SystemExit, match="--msm-bootstrap"):
            tool.msm_bootstrap_arguments(ap.parse_args(base + ["--msm"] + alone))


# ---------------------------------------------------------------- calibration
CAL_DATASETS, CAL_RESAMPLES, CAL_SEED = 100, 200, 7000
COVERAGE_MIN, STD_FACTOR = 0.75, 1.5


def test_calibration_on_a_two_state_chain(monkeypatch):
    """p01 = 0.05, p10 = 0.10: t2 = -1 / ln 0.85 = 6.153 frames.  200 trajectories of 200 frames, B = 200 resamples of the
    trajectories, 100 independently generated datasets, bootstrap_msm itself on numpy stand-ins.  The 90 % interval must hold
    the true value in at least 75 % of the datasets, and the mean bootstrap standard deviation must lie within a factor 1.5
    of the standard deviation of the point estimate across the datasets.  (A numpy run of the protocol over 200 datasets gave
    coverage 0.88, across-dataset std 0.141, mean bootstrap std 0.129.)"""
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "resampled_counter", boot.FastCounter)
    monkeypatch.setattr(evaluate, "batched_reversible_sweeper", boot.FastSweeper)
    assert abs(boot.TRUE_T2 - 6.153) < 1e-3
    point, stds, inside = [], [], 0
    for d in range(CAL_DATASETS):
        labels, lengths = boot.two_state_dataset(CAL_SEED + d)
        bs = evaluate.bootstrap_msm(labels, 1, lengths, 2, n_resamples=CAL_RESAMPLES, seed=d, k=1, steps_per_sync=32, device="cpu")
        assert bs.n_failed == 0 and bs.timescales.shape == (CAL_RESAMPLES, 1)
        if d == 0:                                                   # the estimator agrees with the closed form of two states
            closed = boot.two_state_t2(boot.FastCounter(labels, lengths, lengths, 1, 2, None)(bs.weights))
            assert np.allclose(bs.timescales[:, 0], closed, rtol=1e-8)
        lo, hi = bs.interval(0.90)
        inside += bool(lo[0] <= boot.TRUE_T2 <= hi[0])
        stds.append(bs.std()[0])
        point.append(bs.point.timescales(1)[0])
    coverage, across, mean_std = inside / CAL_DATASETS, float(np.std(point, ddof=1)), float(np.mean(stds))
    print(f"calibration: coverage of the 90 % interval {coverage:.2f}, across-dataset std {across:.4f}, mean bootstrap std "
          f"{mean_std:.4f} (ratio {mean_std / across:.3f}), mean point estimate {np.mean(point):.4f} (true {boot.TRUE_T2:.4f})")
    assert coverage >= COVERAGE_MIN, coverage
    assert across / STD_FACTOR <= mean_std <= across * STD_FACTOR, (mean_std, across)
