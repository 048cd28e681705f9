"""dff_struct_native_q / dff_core_states / dff_label_runs on the GPU against the naive numpy oracle of oracle/kinetics.py.

What is compared how:
- Q       |Q_gpu - Q_oracle| <= 2^-23 absolute: the kernel computes in fp64 and rounds to fp32 once, device and numpy exp differ
          by a few fp64 ulps, so only the final rounding can differ -- one fp32 spacing below 1.  NaN exactly where the oracle has it.
- states  torch.equal with the oracle's loop on the same fp32 values, labels and core; integer work, exact.
- runs    every array equal to the oracle's loop, and the true count.
- scripted folding   frames folded + w (extended helix - folded) + 0.05 A noise, w following a script over three trajectories of
          unequal length; the oracle's Q is ~0.998 at w = 0, 0.84 - 0.86 (chignolin) / 0.55 - 0.56 (villin) at w = 0.3 and <= 0.10
          at w = 1, so with lo = 0.2, hi = 0.9 the script fixes every label; the test asserts the margin instead of assuming it.
"""
import numpy as np
import pytest
import torch

from oracle.kinetics import core_states, label_runs, native_q, scripted_frames
from oracle.frames import chain_frames, noisy_ensemble, splitmix_labels
from oracle.struct_metric import kabsch64_batch
from fence import COMBINATIONS, fenced
from paths_cases import CARRY_STRETCH, carry_case
from stream_gate import N_FRAMES, Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, on_device, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

Q_BAR = 2.0 ** -23
GOLDEN_MOL = {10: "chignolin", 35: "villin"}
LO, HI = 0.2, 0.9


# ---------------------------------------------------------------- 1. fraction of native contacts
def q_frames(golden, N, n=1000):
    """(frames, template): a noisy ensemble around the golden folded structure where there is one of N beads, chain frames else"""
    if N in GOLDEN_MOL:
        f = golden("struct_folded.npz")[GOLDEN_MOL[N]].astype(np.float64)
        return noisy_ensemble(np.random.default_rng(100 + N), f, n, 1.0), f
    x = chain_frames(n, N, 200 + N)
    return x, x[0].astype(np.float64)


def pair_lists(template, N):
    golden_like = N in GOLDEN_MOL
    return {"one": (np.array([[2, 0]], np.int32), np.array([np.linalg.norm(template[2] - template[0])], np.float32)),
            "native": ev().native_pairs(template, *((10.0, 3) if golden_like else (15.0, 1))),
            "all": ev().native_pairs(template, 1e6, 1)}


def q_gpu(x, pairs, r0, beta=5.0, lam=1.2):
    xd = x if isinstance(x, torch.Tensor) else to_dev(np.ascontiguousarray(x, np.float32))
    return B().struct_native_q(xd, pairs, r0, beta, lam).cpu().numpy()


def assert_q(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at {np.flatnonzero(np.isnan(got))[:8]}, the oracle's at {np.flatnonzero(np.isnan(want))[:8]}"
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok]).max() if ok.any() else 0.0
    print(f"[kinetics] {what}: {ok.sum()} frames, |Q - oracle| {err:.3e} (bar {Q_BAR:.3e}), Q {np.nanmin(want):.4f} .. {np.nanmax(want):.4f}")
    assert err <= Q_BAR, f"{what}: Q off by {err:.3e}"


@pytest.mark.parametrize("N", [4, 10, 35, 64])
def test_q_parity(dev, golden, N):
    x, template = q_frames(golden, N)
    xd = to_dev(x)
    for name, (pairs, r0) in pair_lists(template, N).items():
        assert len(pairs) == {"one": 1, "all": N * (N - 1) // 2}.get(name, len(pairs)) and len(pairs) >= 1
        want = native_q(x, pairs, r0)
        full = q_gpu(xd, pairs, r0)
        assert_q(full, want, f"N={N} {name} ({len(pairs)} pairs)")
        assert 0.0 <= np.nanmin(want) and np.nanmax(want) <= 1.0 and np.ptp(want) > 1e-3
        for n in (1, 63, 64, 65):                       # around the 64-frame tile; a frame's value depends on nothing else
            assert np.array_equal(q_gpu(xd[:n].clone(), pairs, r0), full[:n]), (N, name, n)
    # another beta and lambda
    pairs, r0 = pair_lists(template, N)["native"]
    assert_q(q_gpu(xd, pairs, r0, 2.0, 1.5), native_q(x, pairs, r0, 2.0, 1.5), f"N={N} beta 2 lambda 1.5")


def test_q_special_frames(dev, golden):
    x, template = q_frames(golden, 10, 200)
    pairs, r0 = pair_lists(template, 10)["all"]
    x[3, 2, 1] = np.nan
    x[70, 0, 0] = np.inf
    x[150, 9, 2] = -np.inf
    x[5] = chain_frames(1, 10, 9)[0] * np.float32(1e30)            # huge and finite: every distance ~1e30
    x[9, 4] = x[9, 0]                                              # two coincident beads
    x[10, :] = x[10, 0]                                            # all beads coincident
    want = native_q(x, pairs, r0)
    got = q_gpu(x, pairs, r0)
    assert_q(got, want, "special frames")
    assert np.flatnonzero(np.isnan(got)).tolist() == [3, 70, 150]
    assert got[5] == 0.0 and want[5] == 0.0 and np.isfinite(got[9]) and got[10] > 0.99
    # an input view that is not 16-byte aligned: the scalar tile loads
    for n in (200, 65):
        assert np.array_equal(q_gpu(on_device(x[:n], dev, False), pairs, r0), got[:n], equal_nan=True), n
        assert np.array_equal(q_gpu(on_device(x[:n], dev, True), pairs, r0), got[:n], equal_nan=True), n


def test_q_bad_pair_makes_every_frame_nan(dev, golden):
    x, template = q_frames(golden, 10, 130)
    pairs, r0 = pair_lists(template, 10)["native"]
    assert np.isfinite(q_gpu(x, pairs, r0)).all()
    for where, bad in ((0, (0, 10)), (len(pairs) - 1, (10, 3)), (7, (4, 4)), (3, (-1, 5)), (5, (2, 1 << 20)), (6, (-(1 << 31), 0))):
        p = pairs.copy()
        p[where] = bad
        got = q_gpu(x, p, r0)
        assert np.isnan(got).all() and np.isnan(native_q(x, p, r0)).all(), bad
    assert np.isfinite(q_gpu(x, pairs[:, ::-1].copy(), r0)).all()          # (j, i) is as good as (i, j)


def test_q_bitwise_slices_and_repeats(dev, golden):
    x, template = q_frames(golden, 35, 1000)
    pairs, r0 = pair_lists(template, 35)["native"]
    xd = to_dev(x)
    full = q_gpu(xd, pairs, r0)
    assert np.array_equal(full, q_gpu(xd, pairs, r0))
    for a, b in ((37, 411), (0, 1), (999, 1000), (64, 128)):
        assert np.array_equal(q_gpu(xd[a:b].clone(), pairs, r0), full[a:b]), (a, b)
    assert np.array_equal(ev().native_contacts_q(x, template).cpu().numpy(), full)


# ---------------------------------------------------------------- 2. core states
def cv_series(n, seed):
    """a slow walk folded into 0 .. 1 with stretches in both cores, exact threshold values, NaN and +-inf: float32"""
    rng = np.random.default_rng(seed)
    cv = np.abs(((0.55 + np.cumsum(rng.standard_normal(n)) * 0.08) % 2.0) - 1.0).astype(np.float32)
    k = max(n // 50, 1)
    for val in (np.float32(LO), np.float32(HI), np.nextafter(np.float32(LO), np.float32(1)), np.nextafter(np.float32(HI), np.float32(0)),
                np.nan, np.inf, -np.inf):
        cv[rng.integers(0, n, k)] = val
    return cv


def ragged7(n):
    return [1, 1, 2, 63, 64, 65, n - 196]


def ragged130(n):
    rng = np.random.default_rng(130)
    cuts = np.sort(rng.integers(0, n + 1, 129))
    cuts[40] = cuts[41]                                             # an empty trajectory
    return np.diff(np.concatenate([[0], cuts, [n]])).tolist()


def states_gpu(cv, lengths, lo=LO, hi=HI):
    """binding.core_states with a dirty workspace -> (labels, core) on the host"""
    cvd = to_dev(np.asarray(cv, np.float32))
    ws = torch.full((max(B().kinetics_workspace_bytes(len(cv)), 8),), 0xFF, dtype=torch.uint8, device="cuda")
    lab, core = B().core_states(cvd, lengths, lo, hi, return_core=True, workspace=ws)
    return lab.cpu(), core.cpu()


def assert_states(cv, lengths, what):
    want_lab, want_core = core_states(cv, LO, HI, lengths)
    lab, core = states_gpu(cv, lengths)
    assert lab.dtype == torch.int32 and core.dtype == torch.int8
    bad = np.flatnonzero(lab.numpy() != want_lab)
    assert torch.equal(lab, torch.from_numpy(want_lab)), f"{what}: {len(bad)} labels differ, first at frame {bad[:5]}"
    assert torch.equal(core, torch.from_numpy(want_core)), f"{what}: core differs"
    return want_lab


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 70001])
def test_core_states_sizes(dev, n):
    cv = cv_series(n, 300 + n) if n else np.empty(0, np.float32)
    lab = assert_states(cv, [n], f"n={n}, one trajectory")
    if n > 196:
        assert_states(cv, ragged7(n), f"n={n}, ragged")
    if n == 70001:
        assert {-1, 0, 1} <= set(lab.tolist())
        assert_states(cv, [0, n, 0], "empty trajectories around one")


def test_core_states_layouts(dev):
    n = 70001
    cv = cv_series(n, 41)
    one = assert_states(cv, [n], "one trajectory")
    r130 = ragged130(n)
    assert len(r130) == 130 and sum(r130) == n and 0 in r130
    many = assert_states(cv, r130, "130 ragged trajectories")
    assert not np.array_equal(one, many)                            # the boundaries matter on this series
    assert_states(cv[:70000], [700] * 100, "100 equal trajectories")
    assert_states(cv[:70000], [700] * 50 + [0] + [700] * 50, "100 equal trajectories and an empty one")
    assert_states(cv[:64 * 300], [300] * 64, "64 equal trajectories")
    assert_states(cv[:6500], list(range(1, 66)) + [6500 - 65 * 33], "66 ragged trajectories")


def test_core_states_carry_through_whole_workgroups(dev):
    """a core visit followed by >= 50 000 frames between the cores: the carry passes through whole workgroups untouched"""
    M = np.float32(0.5)
    a = np.full(56000, M)
    a[0], a[52001] = 1.0, 0.0                                       # folded for 52 000 frames, then the other core
    b = np.full(51000, M)                                           # never visits a core
    c = np.full(53000, M)
    c[51999] = np.nan                                               # a reset after 50 000 frames
    c[1] = 0.0
    cv = np.concatenate([a, b, c]).astype(np.float32)
    lab = assert_states(cv, [len(a), len(b), len(c)], "long dwells")
    assert (lab[:52001] == 1).all() and (lab[52001:56000] == 0).all() and (lab[56000:107000] == -1).all()
    assert lab[107000] == -1 and (lab[107001:107000 + 51999] == 0).all() and (lab[107000 + 51999:] == -1).all()
    assert_states(cv, [len(cv)], "long dwells, one trajectory")


def test_core_states_boundaries(dev):
    """a core hit on the last frame before a boundary, the next trajectory starting between the cores: -1 there.  Boundaries at
    the edges of waves (64), scan steps (256) and workgroups (2048) and next to them"""
    lengths = [64, 192, 1, 255, 1536, 2048, 2047, 1, 2049, 63, 65, 4096, 3]
    n = sum(lengths)
    cv = np.full(n, 0.5, np.float32)
    ends = np.cumsum(lengths) - 1
    cv[ends] = np.where(np.arange(len(ends)) % 2 == 0, 1.0, 0.0)
    lab = assert_states(cv, lengths, "core hit on every last frame")
    assert (lab[ends] >= 0).all() and (np.delete(lab, ends) == -1).all()
    # thresholds: equality counts as inside the core
    lo32, hi32 = np.float32(LO), np.float32(HI)
    cv = np.array([0.5, lo32, 0.5, np.nextafter(hi32, np.float32(0)), hi32, 0.5, np.nextafter(lo32, np.float32(1)), lo32], np.float32)
    lab, core = states_gpu(cv, [len(cv)])
    assert lab.tolist() == [-1, 0, 0, 0, 1, 1, 1, 0] and core.tolist() == [-1, 0, -1, -1, 1, -1, -1, 0]
    for bad in (np.nan, np.inf, -np.inf):
        lab, core = states_gpu(np.array([1.0, 0.5, bad, 0.5, 0.0, bad, 1.0], np.float32), [7])
        assert lab.tolist() == [1, 1, -1, -1, 0, -1, 1] and core.tolist() == [1, -1, -1, -1, 0, -1, 1], bad
    # negative thresholds, and the evaluate-level wrapper
    lab = ev().core_states(np.array([-3.0, -1.5, 0.0, -1.5, -2.0], np.float32), -2.0, -1.0).cpu()
    assert lab.tolist() == [0, 0, 1, 1, 0]
    with pytest.raises(ValueError, match="lo must be < hi"):
        B().core_states(to_dev(np.zeros(4, np.float32)), [4], 0.9, 0.2)


# ---------------------------------------------------------------- 3. runs
def run_labels(n):
    """labels 0 .. 3 with -1s: single-frame runs in the first half, longer runs (repeats of 1 .. 40) in the second"""
    lab = splitmix_labels(n, 4)
    h = n // 2
    rng = np.random.default_rng(n)
    rep = np.repeat(splitmix_labels(n - h, 4), rng.integers(1, 41, n - h))[:n - h]
    lab[h:] = rep
    return lab


def runs_gpu(labels, lengths):
    res = B().label_runs(to_dev(np.asarray(labels, np.int32)), lengths,
                         workspace=torch.full((max(B().kinetics_workspace_bytes(len(labels)), 8),), 0xFF, dtype=torch.uint8, device="cuda"))
    k = int(res["n_runs"].cpu())
    return {key: res[key].cpu().numpy() for key in ("start", "length", "label", "flags")}, k


def assert_runs(labels, lengths, what):
    want = label_runs(labels, lengths)
    got, k = runs_gpu(labels, lengths)
    assert k == len(want["start"]), f"{what}: {k} runs, the oracle has {len(want['start'])}"
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key][:k], want[key]), f"{what}: {key} differs"
    assert want["length"].sum() == len(labels)
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 70001])
def test_label_runs_sizes(dev, n):
    lab = run_labels(n) if n else np.empty(0, np.int32)
    assert_runs(lab, [n], f"n={n}, one trajectory")
    if n > 196:
        assert_runs(lab, ragged7(n), f"n={n}, ragged")
    if n:
        assert_runs(np.full(n, 7, np.int32), [n], f"n={n}, one run")
        assert_runs(np.arange(n, dtype=np.int32) % 2 - 1, [n], f"n={n}, every frame a run")


def test_label_runs_layouts(dev):
    n = 70001
    lab = run_labels(n)
    one = assert_runs(lab, [n], "one trajectory")
    many = assert_runs(lab, ragged130(n), "130 ragged trajectories")
    assert len(many["start"]) > len(one["start"]) and set(many["flags"].tolist()) == {0, 1, 2, 3}
    assert_runs(lab[:70000], [700] * 100, "100 equal trajectories")
    assert_runs(lab[:64 * 300], [300] * 64, "64 equal trajectories")
    assert_runs(np.full(70000, -1, np.int32), [700] * 100, "constant labels: one run per trajectory")
    assert_runs(np.full(n, 2, np.int32), ragged130(n), "constant labels, ragged")
    assert_runs(lab[:6500], list(range(1, 66)) + [6500 - 65 * 33], "66 ragged trajectories")
    # the evaluate-level wrapper trims to the true count
    got = ev().label_runs(lab, ragged130(n))
    for key in many:
        assert np.array_equal(got[key], many[key]), key


@pytest.mark.parametrize("case", ["one", "periodic", "groups"])
def test_carry_scan_second_chunk(dev, case):
    """more than 256 blocks in one launch (paths_cases.carry_case): both scans' carry kernel runs two chunks"""
    cv, lengths = carry_case(case)
    lab = assert_states(cv, lengths, f"carry scan, {case}")
    runs = assert_runs(lab, lengths, f"carry scan, {case}")
    if case == "one":
        s = CARRY_STRETCH
        assert (lab[s] == 0).all() and lab[s.stop] == 1 and len(runs["start"]) == 76987
        assert runs["start"][-1] == s.stop and runs["length"][-1] == 1 and runs["flags"][-1] == 2
        assert runs["start"][-2] <= s.start - 1 and runs["start"][-2] + runs["length"][-2] == s.stop
    if case == "groups":                                            # runs on both sides of the first launch group's end
        cut = sum(lengths[:64])
        assert (runs["start"] < cut).sum() > 5 and (runs["start"] >= cut).sum() > 5 and (np.diff(runs["start"]) > 0).all()


def test_label_runs_max_runs(dev):
    n = 20000
    lab = run_labels(n)
    lengths = ragged7(n)
    want = label_runs(lab, lengths)
    k = len(want["start"])
    labd = to_dev(lab)
    ln = np.asarray(lengths, np.int64)
    ws = torch.empty(B().kinetics_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for max_runs in (0, 1, 1000, k - 1, k, k + 5):
        size = k + 16
        out = {"start": torch.full((size,), 123, dtype=torch.int64, device="cuda"), "length": torch.full((size,), 123, dtype=torch.int64, device="cuda"),
               "label": torch.full((size,), 123, dtype=torch.int32, device="cuda"), "flags": torch.full((size,), 123, dtype=torch.uint8, device="cuda")}
        cnt = torch.full((1,), 123, dtype=torch.int64, device="cuda")
        raw("dff_label_runs", 0, ptr(labd), n, ln.ctypes.data, len(ln), max_runs, ptr(out["start"]), ptr(out["length"]), ptr(out["label"]),
            ptr(out["flags"]), ptr(cnt), ptr(ws), ws.numel(), stream_of(labd))
        assert int(cnt) == k, max_runs                              # the true count, whatever fits
        m = min(max_runs, k)
        for key, t in out.items():
            assert np.array_equal(t[:m].cpu().numpy(), want[key][:m]), (max_runs, key)
            assert bool((t[m:] == 123).all()), f"max_runs={max_runs}: {key} touched beyond the runs written"


# ---------------------------------------------------------------- 4. scripted folding
SCRIPT = [[0.3, 0.0, 0.3, 1.0, 0.3, 0.0], [1.0, 0.3, 0.0, 0.3], [0.0, 0.3, 1.0, 1.0, 0.3]]     # one list per trajectory
REPEAT = 40
N_FOLDING, N_UNFOLDING = 2, 2          # labels - F F U U F | U U F F | F F U U U: trajectory 1 unfolds and folds once, 2 folds, 3 unfolds


def scripted(golden, mol):
    f = golden("struct_folded.npz")[mol].astype(np.float64)
    x, w = scripted_frames(f, sum(SCRIPT, []), REPEAT, 0.05, len(f))
    return f, x, w, [len(s) * REPEAT for s in SCRIPT]


def check_scripted(e, x, lengths, cv_oracle, lo, hi, folded_label):
    res = e.eval(x, lengths)
    s = e.series["samples"]
    assert np.abs(s["cv"] - cv_oracle).max() < 1e-3 / 2            # the GPU's series is the oracle's, far inside the margin
    assert res["n_folding"] == N_FOLDING and res["n_unfolding"] == N_UNFOLDING
    want_lab, _ = core_states(s["cv"], lo, hi, lengths)              # the oracle pipeline on the GPU's own series
    assert np.array_equal(s["labels"], want_lab)
    runs = label_runs(want_lab, lengths)
    for key in runs:
        assert np.array_equal(s["runs"][key], runs[key]), key
    want = ev().FoldingKineticsEvaluator.summarize(ev().dwell_summary(runs, e.frame_time), folded_label, 1 - folded_label)
    assert set(want) <= set(res) and (e.ref_result is not None or set(want) == set(res))
    for key, v in want.items():
        assert (np.isnan(v) and np.isnan(res[key])) or res[key] == pytest.approx(v, rel=1e-12, abs=0.0), (key, res[key], v)
    assert res["undetermined_share"] == pytest.approx(REPEAT / len(x), rel=1e-12)          # trajectory 1 starts between the cores
    return res


@pytest.mark.parametrize("mol", ["chignolin", "villin"])
def test_scripted_folding_q(dev, golden, mol):
    f, x, w, lengths = scripted(golden, mol)
    pairs, r0 = ev().native_pairs(f)
    q = native_q(x, pairs, r0)
    print(f"[kinetics] {mol}: oracle Q at w = 0 / 0.3 / 1: " + " / ".join(f"{q[w == v].min():.4f} .. {q[w == v].max():.4f}" for v in (0.0, 0.3, 1.0)))
    assert np.abs(q - LO).min() > 1e-3 and np.abs(q - HI).min() > 1e-3, "an oracle Q lies within 1e-3 of a threshold"
    assert (q[w == 0.0] > HI).all() and (q[w == 1.0] < LO).all() and ((q[w == 0.3] > LO) & (q[w == 0.3] < HI)).all()
    e = ev().FoldingKineticsEvaluator(mol, f, cv="q", lo=LO, hi=HI, frame_time=0.2, ref_data=x, ref_traj_lengths=lengths)
    res = check_scripted(e, x, lengths, q, LO, HI, 1)
    assert res["rate_folding"] == pytest.approx(N_FOLDING / (e.series["samples"]["summary"]["frames"][0] * 0.2), rel=1e-12)
    # the reference data are the samples: the same numbers, ratios of one
    for key in ev().FoldingKineticsEvaluator.KEYS:
        assert res[key + "_ref"] == res[key] or (np.isnan(res[key]) and np.isnan(res[key + "_ref"])), key
    assert res["log10_rate_ratio_folding"] == 0.0 and res["log10_rate_ratio_unfolding"] == 0.0 and res["folded_share_diff"] == 0.0
    # as ONE trajectory the jump from the folded end of trajectory 1 to the unfolded start of trajectory 2 counts as well
    one = ev().FoldingKineticsEvaluator(mol, f, cv="q", lo=LO, hi=HI).eval(x)
    assert one["n_folding"] == N_FOLDING and one["n_unfolding"] == N_UNFOLDING + 1


@pytest.mark.parametrize("mol", ["chignolin", "villin"])
def test_scripted_folding_rmsd(dev, golden, mol):
    f, x, w, lengths = scripted(golden, mol)
    r = kabsch64_batch(x, f.astype(np.float32))
    lo = 0.5 * (r[w == 0.0].max() + r[w == 0.3].min())
    hi = 0.5 * (r[w == 0.3].max() + r[w == 1.0].min())
    print(f"[kinetics] {mol}: oracle RMSD at w = 0 / 0.3 / 1: " + " / ".join(f"{r[w == v].min():.3f} .. {r[w == v].max():.3f}" for v in (0.0, 0.3, 1.0))
          + f" -> lo {lo:.3f}, hi {hi:.3f}")
    assert np.abs(r - lo).min() > 1e-3 and np.abs(r - hi).min() > 1e-3, "an oracle RMSD lies within 1e-3 of a threshold"
    assert (r[w == 0.0] < lo).all() and (r[w == 1.0] > hi).all() and ((r[w == 0.3] > lo) & (r[w == 0.3] < hi)).all()
    e = ev().FoldingKineticsEvaluator(mol, f, cv="rmsd", lo=lo, hi=hi)
    res = check_scripted(e, x, lengths, r, np.float32(lo), np.float32(hi), 0)
    assert "folded_share_ref" not in res and res["samples_nonfinite"] == 0.0


# ---------------------------------------------------------------- 5. stream order
def native_q_spec():
    b, n, N = B(), N_FRAMES, 10
    x = chain_frames(n, N, 61)
    pairs, r0 = ev().native_pairs(x[0].astype(np.float64), 1e6, 1)
    P = len(pairs)
    poison_pairs = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
    poison_pairs[:, 1] = 1
    return Spec("dff_struct_native_q", {"x": (to_dev(x), float("nan")), "pairs": (to_dev(pairs), poison_pairs), "r0": (to_dev(r0), 1.0)},
                {"q": ((n,), torch.float32)},
                lambda _, bufs: raw("dff_struct_native_q", 0, ptr(bufs["x"]), n, N, ptr(bufs["pairs"]), ptr(bufs["r0"]), P, 5.0, 1.2,
                                    ptr(bufs["q"]), stream_of(bufs["x"])),
                wrap=lambda _, bufs: {"q": b.struct_native_q(bufs["x"], bufs["pairs"], bufs["r0"], 5.0, 1.2)})


KIN_N = 5000                                                        # three workgroups of the scans
KIN_LENGTHS = np.array([1, 2047, 1, 2000, 951], np.int64)


def core_states_spec():
    b, n = B(), KIN_N
    ws = torch.empty(b.kinetics_workspace_bytes(n), dtype=torch.uint8, device="cuda")

    def wrap(_, bufs):
        lab, core = b.core_states(bufs["cv"], KIN_LENGTHS, LO, HI, return_core=True)
        return {"labels": lab, "core": core.view(torch.uint8)}
    # core_dev is handed over as bytes (the gate has sentinels for uint8, not int8): -1 reads 255, never the sentinel 0x7b
    return Spec("dff_core_states", {"cv": (to_dev(cv_series(n, 71)), 0.5)},
                {"labels": ((n,), torch.int32), "core": ((n,), torch.uint8)},
                lambda _, bufs: raw("dff_core_states", 0, ptr(bufs["cv"]), n, KIN_LENGTHS.ctypes.data, len(KIN_LENGTHS), LO, HI,
                                    ptr(bufs["labels"]), ptr(bufs["core"]), ptr(bufs["ws"]), bufs["ws"].numel(), stream_of(bufs["cv"])),
                work={"ws": ws}, wrap=wrap)


def label_runs_spec():
    b, n = B(), KIN_N
    lab = run_labels(n)
    k = len(label_runs(lab, KIN_LENGTHS)["start"])                  # outputs of exactly the runs: every entry is written
    ws = torch.empty(b.kinetics_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    return Spec("dff_label_runs", {"labels": (to_dev(lab), 0)},
                {"start": ((k,), torch.int64), "length": ((k,), torch.int64), "label": ((k,), torch.int32), "flags": ((k,), torch.uint8),
                 "n_runs": ((1,), torch.int64)},
                lambda _, bufs: raw("dff_label_runs", 0, ptr(bufs["labels"]), n, KIN_LENGTHS.ctypes.data, len(KIN_LENGTHS), k,
                                    ptr(bufs["start"]), ptr(bufs["length"]), ptr(bufs["label"]), ptr(bufs["flags"]), ptr(bufs["n_runs"]),
                                    ptr(bufs["ws"]), bufs["ws"].numel(), stream_of(bufs["labels"])),
                work={"ws": ws}, wrap=lambda _, bufs: b.label_runs(bufs["labels"], KIN_LENGTHS, max_runs=k)), k


def test_stream_order_native_q(gate, side):  # noqa: F811
    ref = analysis_call(native_q_spec(), gate, side)
    assert bool(torch.isfinite(ref["q"]).all()) and float(ref["q"].max() - ref["q"].min()) > 1e-3


def test_stream_order_core_states(gate, side):  # noqa: F811
    ref = analysis_call(core_states_spec(), gate, side)
    assert {-1, 0, 1} <= set(ref["labels"].cpu().tolist())          # nothing like the all -1 of the poison


def test_stream_order_label_runs(gate, side):  # noqa: F811
    spec, k = label_runs_spec()
    ref = analysis_call(spec, gate, side)
    assert int(ref["n_runs"]) == k > len(KIN_LENGTHS)               # the poison (constant labels) has one run per trajectory


@pytest.mark.parametrize("make", [native_q_spec, core_states_spec, lambda: label_runs_spec()[0]], ids=["native_q", "core_states", "label_runs"])
def test_fence(make):
    """The memory contract (tests/fence.py): every buffer in one arena, the scans' carries at exactly
    dff_kinetics_workspace_bytes, the run arrays at exactly the number of runs."""
    spec = make()
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)
