"""Host side of the superposition on a reference (dff_superpose): the float64 oracle the GPU tests of test_superpose.py
compare against (oracle/struct_metric.py: superpose64, horn_gap) held to kabsch64_batch and to its own invariants, the share
of frames the gap filter (GAP_MIN, MAX_EXCLUDED of tests/support.py) excludes on the golden data, the symbol table,
the argument refusals (all on the host, before any device call), the generalised-Procrustes loop of mean_structure on a
numpy stand-in for the kernel, the reductions of FlexibilityEvaluator and the package re-exports.  No GPU."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import dff_amd  # noqa: F401
from dff_amd import binding, evaluate

from oracle.frames import noisy_ensemble, rand_rot
from oracle.struct_metric import kabsch64_batch, stats64, superpose64
from support import GAP_MIN, MAX_EXCLUDED, MOLS, golden_frames

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---------------------------------------------------------------- the oracle as the kernel's stand-in
def numpy_aligner(calls=None):
    """aligner(xyz, ref) -> (dsum, dsq, count) for evaluate.mean_structure / rmsf, from the oracle"""
    def aligner(xyz, ref):
        if calls is not None:
            calls.append(np.array(ref, np.float64))
        o = superpose64(np.asarray(torch.as_tensor(xyz)), ref)
        return stats64(o, ref)[:3]
    return aligner


# ---------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("mol", ["chignolin", "villin", "ala2"])
def test_oracle_is_a_minimiser_and_agrees_with_kabsch64_batch(golden, mol):
    x, f = golden_frames(golden, mol)
    x = x[:512]
    o = superpose64(x, f)
    want = kabsch64_batch(x, f)
    ok = o["finite"]
    assert np.array_equal(np.isnan(o["rmsd"]), np.isnan(want))
    assert np.abs(o["rmsd"][ok] - want[ok]).max() <= 1e-9
    R = o["R"][ok]
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    plain = np.sqrt(((o["aligned"][ok] - f.astype(np.float64)) ** 2).sum((1, 2)) / x.shape[1])
    assert np.abs(plain - want[ok]).max() <= 1e-9


@pytest.mark.parametrize("mol", MOLS + ["ala2"])
def test_gap_filter_excludes_at_most_two_percent_of_the_goldens(golden, mol):
    x, f = golden_frames(golden, mol)
    o = superpose64(x, f)
    excluded = float((o["gap"][o["finite"]] < GAP_MIN).mean())
    print(f"[superpose] {mol}: {excluded:.4%} of the finite frames below gap {GAP_MIN}, smallest gap {np.nanmin(o['gap']):.4g}")
    assert excluded <= MAX_EXCLUDED
    if mol != "ala2":
        assert excluded == 0.0          # the statistics of these sets are compared strictly


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in ("dff_superpose_workspace_bytes", "dff_superpose"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_superpose"][1]) == 14
    assert binding.SYMBOLS["dff_superpose_workspace_bytes"][0] is C.c_longlong


def test_workspace_bytes():
    lib = binding.load_library()
    for n, N in ((-1, 10), (10, 3), (10, 65), (10, 0), (1 << 62, 10)):
        assert lib.dff_superpose_workspace_bytes(n, N) == -1
        with pytest.raises(ValueError):
            binding.superpose_workspace_bytes(n, N)
    assert binding.superpose_workspace_bytes(0, 10) == 0
    assert binding.superpose_workspace_bytes(1, 10) == binding.superpose_workspace_bytes(64, 10) == 41 * 8
    assert binding.superpose_workspace_bytes(65, 64) == 2 * 257 * 8
    big = binding.superpose_workspace_bytes(10 ** 9, 64)                # bounded in n
    assert big == binding.superpose_workspace_bytes(10 ** 10, 64) and big % (257 * 8) == 0 and big <= 16 << 20


def test_bad_arguments_are_refused_on_the_host():
    """every call here is refused before the library touches a device: it runs on a machine without one, and the buffers
    are host memory that a launch would never be given"""
    lib = binding.load_library()
    N, n = 10, 100
    x = np.zeros((n, N, 3), np.float32)
    ref = np.zeros((N, 3), np.float32)
    out = np.zeros((n, N, 3), np.float32)
    acc = np.zeros(4 * N + 1, np.float64)
    ws = np.zeros(binding.superpose_workspace_bytes(n, N) + 8, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731

    def call(x_=p(x), n_=n, N_=N, ref_=p(ref), aligned=p(out), dsum=None, ws_=None, ws_bytes=0):
        return lib.dff_superpose(0, x_, n_, N_, ref_, aligned, None, None, dsum, None, None, ws_, ws_bytes, None)

    need = binding.superpose_workspace_bytes(n, N)
    for what, kw in (("negative", dict(n_=-1)), ("n_beads", dict(N_=3)), ("n_beads", dict(N_=65)), ("null frames", dict(x_=None)),
                     ("null reference", dict(ref_=None)), ("workspace", dict(dsum=p(acc))),
                     ("workspace", dict(dsum=p(acc), ws_=p(ws), ws_bytes=need - 1)),
                     ("aligned", dict(dsum=p(acc), ws_=C.c_void_p(ws.ctypes.data + 1), ws_bytes=need))):
        assert call(**kw) == 1, what                                     # DFF_EINVAL
        assert what in lib.dff_last_error().decode()
    x3 = torch.zeros((5, 3, 3))
    with pytest.raises(ValueError):
        binding.superpose(x3, np.zeros((3, 3)))                          # not a CUDA tensor: refused by the wrapper


# ---------------------------------------------------------------- mean_structure on the numpy stand-in
SIGMA, N_ENS = 0.3, 2048


@pytest.fixture(scope="module")
def ensemble():
    rng = np.random.default_rng(2048)
    template = rng.standard_normal((10, 3)) * 4
    return template, noisy_ensemble(rng, template, N_ENS, SIGMA)


def test_mean_structure_converges_to_the_template(ensemble):
    """the bar of the GPU test, on the oracle alone: the mean of n noisy copies is sigma sqrt(3 / n) ~ 0.04 sigma from the
    template in RMSD; 0.1 sigma is asserted"""
    template, x = ensemble
    calls = []
    mean, n_iter = evaluate.mean_structure(x, aligner=numpy_aligner(calls))
    assert 1 <= n_iter <= 10 and len(calls) == n_iter
    assert mean.shape == (10, 3) and mean.dtype == np.float64
    d = evaluate.kabsch_rmsd64(mean, template)
    print(f"[superpose] mean structure after {n_iter} passes: {d / SIGMA:.4f} sigma from the template")
    assert d <= 0.1 * SIGMA
    assert np.array_equal(calls[0], x[0].astype(np.float64))            # ref=None: the first finite frame
    # from a given reference, and on a torch tensor
    mean2, _ = evaluate.mean_structure(torch.from_numpy(x), template, aligner=numpy_aligner())
    assert evaluate.kabsch_rmsd64(mean2, mean) <= 1e-3


def test_mean_structure_max_iter_exhaustion_warns(ensemble):
    _, x = ensemble
    calls = []
    with pytest.warns(RuntimeWarning, match="mean_structure"):
        mean, n_iter = evaluate.mean_structure(x[:200], max_iter=2, tol=1e-12, aligner=numpy_aligner(calls))
    assert n_iter == 2 and len(calls) == 2 and np.isfinite(mean).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        evaluate.mean_structure(x[:200], max_iter=10, tol=1e-3, aligner=numpy_aligner())
    with pytest.raises(ValueError, match="max_iter"):
        evaluate.mean_structure(x, max_iter=0, aligner=numpy_aligner())


def test_mean_structure_starts_from_the_first_finite_frame(ensemble):
    _, x = ensemble
    y = x[:64].copy()
    y[0, 3, 1] = np.nan
    y[1, 0, 0] = np.inf
    calls = []
    evaluate.mean_structure(y, max_iter=1, tol=1e9, aligner=numpy_aligner(calls))
    assert np.array_equal(calls[0], y[2].astype(np.float64))
    with pytest.raises(ValueError, match="finite"):
        evaluate.mean_structure(np.full((3, 10, 3), np.nan, np.float32), aligner=numpy_aligner())


def test_rmsf_from_sums_and_on_the_stand_in(ensemble):
    template, x = ensemble
    d = np.array([[[1.0, 0, 0], [0, 2.0, 0]], [[-1.0, 0, 0], [0, 2.0, 0]]])         # two frames, two beads
    got = evaluate.rmsf_from_sums(d.sum(0), (d * d).sum((0, 2)), 2)
    assert np.allclose(got, [1.0, 0.0], atol=1e-15)
    assert np.isnan(evaluate.rmsf_from_sums(np.zeros((2, 3)), np.zeros(2), 0)).all()
    # every bead of the synthetic ensemble fluctuates by about sigma sqrt(3) (a little less: the superposition absorbs
    # 6 of the 30 degrees of freedom)
    prof = evaluate.rmsf(x, "mean", aligner=numpy_aligner())
    assert prof.shape == (10,) and np.all(prof > 0.6 * SIGMA * np.sqrt(3)) and np.all(prof < 1.1 * SIGMA * np.sqrt(3))
    assert np.array_equal(evaluate.rmsf(x, template, aligner=numpy_aligner()),
                          evaluate.rmsf_from_sums(*numpy_aligner()(x, template)))
    with pytest.raises(ValueError, match="mean"):
        evaluate.rmsf(x, "median", aligner=numpy_aligner())


# ---------------------------------------------------------------- FlexibilityEvaluator.summarize
def test_flexibility_summarize_on_hand_made_profiles():
    rng = np.random.default_rng(5)
    mean = rng.standard_normal((4, 3)) * 3
    a, b = np.array([1.0, 2.0, 3.0, 4.0]), np.array([1.5, 2.0, 2.0, 4.0])
    r = evaluate.FlexibilityEvaluator.summarize(a, b, mean @ rand_rot(rng).T + 5.0, mean, samples_nonfinite=2, refs_nonfinite=1)
    assert set(r) == {"rmsf_mae", "rmsf_max_abs", "rmsf_pearson", "mean_structure_rmsd", "samples_nonfinite", "refs_nonfinite"}
    assert all(type(v) is float for v in r.values())
    assert r["rmsf_mae"] == pytest.approx(1.5 / 4) and r["rmsf_max_abs"] == 1.0
    assert r["rmsf_pearson"] == pytest.approx(np.corrcoef(a, b)[0, 1], rel=1e-12)
    # a rotated and shifted copy is no distance away: Ga + Gb - 2 lambda cancels to ~1e-16 (Ga + Gb), ~1e-7 A in the root
    assert r["mean_structure_rmsd"] <= 1e-6
    assert r["samples_nonfinite"] == 2.0 and r["refs_nonfinite"] == 1.0
    r = evaluate.FlexibilityEvaluator.summarize(a, a, mean * np.array([-1.0, 1.0, 1.0]), mean)
    assert r["rmsf_mae"] == 0.0 and r["rmsf_pearson"] == pytest.approx(1.0) and r["mean_structure_rmsd"] > 0.1   # a mirror image is
    assert np.isnan(evaluate.FlexibilityEvaluator.summarize(np.ones(4), b, mean, mean)["rmsf_pearson"])
    with pytest.raises(ValueError):
        evaluate.FlexibilityEvaluator.summarize(a, b[:3], mean, mean)


def test_flexibility_evaluator_raises_without_library(monkeypatch):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.FlexibilityEvaluator(torch.zeros((3, 4, 3)), device="cpu")


def test_chunk_bookkeeping_of_superpose_and_superpose_stats(monkeypatch):
    """a stub for binding.superpose: every chunk lands at its offset, and the chunks' sums are added"""
    calls = []

    def stub(x, ref, aligned=True, rot=False, rmsd=False, stats=False, out=None, workspace=None):
        calls.append((len(x), stats, out is not None))
        if out is not None:
            out.copy_(x + 1)
        res = {"rot": torch.arange(len(x), dtype=torch.float64)[:, None, None].expand(len(x), 3, 3)} if rot else {}
        if stats:
            assert workspace is not None
            res.update(dsum=x.double().sum(0), dsq=x.double().sum((0, 2)), count=torch.tensor([len(x)]))
        return res
    monkeypatch.setattr(binding, "superpose", stub)
    monkeypatch.setattr(binding, "superpose_workspace_bytes", lambda n, N: 8 * n)
    x = torch.arange(7 * 4 * 3, dtype=torch.float32).reshape(7, 4, 3)
    ref = np.zeros((4, 3))
    al, rot = evaluate.superpose(x, ref, return_rotations=True, chunk=3, device="cpu")
    assert calls == [(3, False, True), (3, False, True), (1, False, True)]
    assert torch.equal(al, x + 1) and rot[:, 0, 0].tolist() == [0, 1, 2, 0, 1, 2, 0]
    del calls[:]
    dsum, dsq, count = evaluate.superpose_stats(x, ref, chunk=4, device="cpu")
    assert calls == [(4, True, False), (3, True, False)] and count == 7
    assert np.array_equal(dsum, x.double().sum(0).numpy()) and np.array_equal(dsq, x.double().sum((0, 2)).numpy())
    with pytest.raises(ValueError, match="chunk"):
        evaluate.superpose(x, ref, chunk=0, device="cpu")
    with pytest.raises(ValueError, match="beads"):
        evaluate.superpose(x, np.zeros((5, 3)), device="cpu")


# ---------------------------------------------------------------- re-exports and the tool's arguments
def test_package_reexports():
    for name in ("superpose", "mean_structure", "rmsf", "FlexibilityEvaluator"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__


def test_flexibility_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.flexibility is None and a.write_aligned is None
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--flexibility", "heldout.pt", "--write-aligned", "out.pt", "--folded-pdb", "f.pdb"])
    assert a.flexibility == "heldout.pt" and a.write_aligned == "out.pt"
