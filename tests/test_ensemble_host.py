"""Host side of the nearest-structure RMSD between two ensembles (dff_rmsd_nearest / dff_rmsd_matrix): the binding's
symbol table, the reductions of EnsembleCoverageEvaluator on hand-made nearest-RMSD arrays, the chunk bookkeeping of
nearest_rmsd against a stub that records its calls, and the --coverage arguments of tools_eval_samples.py.  No GPU."""
import math

import numpy as np
import pytest
import torch

import dff_amd  # noqa: F401
from dff_amd import binding, evaluate

NAN = float("nan")


def test_symbols_declared():
    for name in ("dff_rmsd_nearest_workspace_bytes", "dff_rmsd_nearest", "dff_rmsd_matrix"):
        assert name in binding.SYMBOLS
    res, args = binding.SYMBOLS["dff_rmsd_nearest"]
    assert len(args) == 12                       # device, x, n, y, m, N, self_first, rmsd, index, ws, ws bytes, stream
    assert len(binding.SYMBOLS["dff_rmsd_matrix"][1]) == 8
    assert binding.SYMBOLS["dff_rmsd_nearest_workspace_bytes"][0] is not None


def test_package_reexports():
    assert dff_amd.nearest_rmsd is evaluate.nearest_rmsd
    assert dff_amd.rmsd_matrix is evaluate.rmsd_matrix
    assert dff_amd.EnsembleCoverageEvaluator is evaluate.EnsembleCoverageEvaluator


# ---------------------------------------------------------------- reductions
def test_share_within_inclusive_exclusive_and_nan():
    d = torch.tensor([0.5, 1.0, 1.5, NAN, 2.0], dtype=torch.float32)
    assert evaluate.share_within(d, 1.0) == 2 / 4                      # 1.0 itself counts: d <= delta
    assert evaluate.share_within(d, 1.0, inclusive=False) == 1 / 4     # d < delta
    assert evaluate.share_within(d, 2.0) == 1.0
    assert evaluate.share_within(d, 0.25) == 0.0
    assert math.isnan(evaluate.share_within(torch.tensor([NAN, NAN]), 1.0))
    assert math.isnan(evaluate.share_within(torch.empty(0), 1.0))


def test_nearest_summary_leaves_nan_out():
    d = torch.tensor([3.0, NAN, 1.0, 2.0, NAN, 6.0], dtype=torch.float32)
    s = evaluate.nearest_summary(d, "novelty", ("mean", "median", "min", "max"))
    assert s == {"novelty_rmsd_mean": 3.0, "novelty_rmsd_median": 2.5, "novelty_rmsd_min": 1.0, "novelty_rmsd_max": 6.0}
    s = evaluate.nearest_summary(torch.tensor([3.0, 1.0, NAN, 2.0]), "x", ("median",))
    assert s == {"x_rmsd_median": 2.0}
    s = evaluate.nearest_summary(torch.tensor([NAN]), "x")
    assert set(s) == {"x_rmsd_mean", "x_rmsd_median"} and all(math.isnan(v) for v in s.values())


def test_summary_matches_numpy_on_random_arrays():
    rng = np.random.default_rng(0)
    for k in (1, 2, 7, 64):
        v = rng.random(k).astype(np.float32) * 5
        v[rng.random(k) < 0.2] = np.nan
        if np.isnan(v).all():
            v[0] = 1.0
        s = evaluate.nearest_summary(torch.from_numpy(v), "d", ("mean", "median", "min", "max"))
        f = v[~np.isnan(v)].astype(np.float64)
        assert s["d_rmsd_mean"] == pytest.approx(f.mean(), rel=1e-12)
        assert s["d_rmsd_median"] == pytest.approx(np.median(f), rel=1e-12)
        assert s["d_rmsd_min"] == f.min() and s["d_rmsd_max"] == f.max()


@pytest.fixture
def evaluator(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    return evaluate.EnsembleCoverageEvaluator(torch.zeros((3, 4, 3)), "mol", (2.0, 1.0, 4.0), device="cpu")


def test_evaluator_summarize(evaluator):
    nov = torch.tensor([0.0, 1.0, 2.0, 4.0, 4.5, NAN])
    cov = torch.tensor([0.5, 3.0, NAN])
    div = torch.tensor([1.0, 0.999, 0.2, 3.0, 5.0, NAN])
    r = evaluator.summarize(nov, cov, div, samples_nonfinite=1, refs_nonfinite=1)
    assert all(type(v) is float for v in r.values())
    assert r["novelty_rmsd_mean"] == pytest.approx(11.5 / 5) and r["novelty_rmsd_median"] == 2.0
    assert r["novelty_rmsd_min"] == 0.0
    assert (r["precision@1"], r["precision@2"], r["precision@4"]) == (2 / 5, 3 / 5, 4 / 5)
    assert r["coverage_rmsd_mean"] == 1.75 and r["coverage_rmsd_median"] == 1.75 and r["coverage_rmsd_max"] == 3.0
    assert (r["recall@1"], r["recall@2"], r["recall@4"]) == (0.5, 0.5, 1.0)
    assert r["diversity_rmsd_mean"] == pytest.approx((1.0 + 0.999 + 0.2 + 3.0 + 5.0) / 5, rel=1e-6)
    assert r["diversity_rmsd_median"] == 1.0
    assert r["duplicates@1"] == 2 / 5            # strictly closer than the smallest threshold: 1.0 itself is no duplicate
    assert "duplicates@2" not in r and "duplicates@4" not in r
    assert r["samples_nonfinite"] == 1.0 and r["refs_nonfinite"] == 1.0


def test_evaluator_counts_nonfinite_refs_and_rejects_bad_thresholds(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    ref = torch.zeros((5, 4, 3))
    ref[1, 2, 0] = NAN
    ref[4, 0, 2] = float("inf")
    assert evaluate.EnsembleCoverageEvaluator(ref, device="cpu").refs_nonfinite == 2
    with pytest.raises(ValueError, match="thresholds"):
        evaluate.EnsembleCoverageEvaluator(ref, thresholds=(), device="cpu")
    with pytest.raises(ValueError, match="thresholds"):
        evaluate.EnsembleCoverageEvaluator(ref, thresholds=(1.0, 0.0), device="cpu")


def test_evaluator_raises_without_library(monkeypatch):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.EnsembleCoverageEvaluator(torch.zeros((3, 4, 3)), device="cpu")


# ---------------------------------------------------------------- chunk bookkeeping of nearest_rmsd
class Stub:
    """stands in for binding.rmsd_nearest: records (first query value, queries, candidates, self_first) and returns the
    query's own tag as its RMSD and 1000 + tag as its index"""

    def __init__(self):
        self.calls = []

    def __call__(self, x, y, self_first=-1, workspace=None):
        assert workspace is not None and x.is_contiguous() and y.is_contiguous()
        self.calls.append((int(x[0, 0, 0]), len(x), len(y), self_first))
        tag = x[:, 0, 0]
        return tag.to(torch.float32), (tag + 1000).to(torch.int64)


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(binding, "rmsd_nearest", s)
    monkeypatch.setattr(binding, "rmsd_nearest_workspace_bytes", lambda n, m, N: 8 * n)
    return s


def tagged(n, N=4):
    x = torch.zeros((n, N, 3))
    x[:, 0, 0] = torch.arange(n, dtype=torch.float32)
    return x


@pytest.mark.parametrize("chunk,starts", [(1, list(range(7))), (3, [0, 3, 6]), (7, [0]), (100, [0]), (None, [0])])
def test_nearest_rmsd_chunks(stub, chunk, starts):
    x, y = tagged(7), tagged(5)
    r, i = evaluate.nearest_rmsd(x, y, chunk=chunk, device="cpu")
    size = 7 if chunk is None else chunk
    assert stub.calls == [(o, min(size, 7 - o), 5, -1) for o in starts]     # every call sees all the candidates
    assert r.dtype == torch.float32 and i.dtype == torch.int64
    assert r.tolist() == list(range(7)) and i.tolist() == [1000 + k for k in range(7)]   # each chunk lands at its offset


@pytest.mark.parametrize("same_object", [True, False])
def test_nearest_rmsd_self_first_per_chunk(stub, same_object):
    x = tagged(10)
    y = x if same_object else x.clone()
    r, i = evaluate.nearest_rmsd(x, y, exclude_self=True, chunk=4, device="cpu")
    assert stub.calls == [(0, 4, 10, 0), (4, 4, 10, 4), (8, 2, 10, 8)]      # self_first = the chunk's first query
    assert r.tolist() == list(range(10))


def test_nearest_rmsd_argument_checks(stub):
    with pytest.raises(ValueError, match="exclude_self"):
        evaluate.nearest_rmsd(tagged(7), tagged(5), exclude_self=True, device="cpu")
    with pytest.raises(ValueError, match="beads"):
        evaluate.nearest_rmsd(tagged(7, 4), tagged(5, 6), device="cpu")
    with pytest.raises(ValueError, match="chunk"):
        evaluate.nearest_rmsd(tagged(7), tagged(5), chunk=0, device="cpu")
    with pytest.raises(ValueError):
        evaluate.nearest_rmsd(torch.zeros((7, 12)), tagged(5), device="cpu")
    r, i = evaluate.nearest_rmsd(tagged(0), tagged(5), device="cpu")
    assert stub.calls == [] and r.shape == (0,) and i.shape == (0,)


def test_evaluator_eval_runs_the_three_searches(stub, evaluator):
    samples = tagged(6)
    r = evaluator.eval(samples)
    # novelty: samples against the 3 references; coverage: references against the 6 samples; diversity: samples against
    # themselves, self excluded
    assert stub.calls == [(0, 6, 3, -1), (0, 3, 6, -1), (0, 6, 6, 0)]
    assert r["novelty_rmsd_mean"] == 2.5 and r["coverage_rmsd_max"] == 0.0 and r["samples_nonfinite"] == 0.0


# ---------------------------------------------------------------- tools_eval_samples.py --coverage
def test_coverage_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.coverage is None and a.rmsd_thresholds == (1.0, 2.0, 4.0) and a.coverage_subsample is None
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--coverage", "train.pt", "--rmsd-thresholds", "0.5,3",
                       "--coverage-subsample", "1000"])
    assert a.coverage == "train.pt" and a.rmsd_thresholds == (0.5, 3.0) and a.coverage_subsample == 1000
    for bad in ("1,x", "", "1,-2", "0"):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--coverage", "t.pt", "--rmsd-thresholds", bad])


def test_coverage_subsample_is_even_and_keeps_the_ends():
    import tools_eval_samples as tool
    x = tagged(101)
    assert tool.subsample(x, None) is x and tool.subsample(x, 101) is x and tool.subsample(x, 500) is x
    s = tool.subsample(x, 11)
    assert s[:, 0, 0].tolist() == [10.0 * k for k in range(11)]
    assert tool.subsample(x, 1)[:, 0, 0].tolist() == [0.0]
