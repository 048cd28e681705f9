"""Host side of RMSD clustering (dff_rmsd_neighbors / dff_gromos_steps): the symbols, the refusals of bad arguments (on
the host, before any device call: they run on a machine without one), the numpy oracle of the greedy loop on hand-built
graphs, the reductions of RmsdClusterEvaluator on given labels, the package's re-exports and the --clusters arguments of
tools_eval_samples.py.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
from oracle.cluster import gromos, neighbors, pack, pick_cutoff, unpack
from dff_amd import binding, evaluate

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_rmsd_neighbors", "dff_gromos_workspace_bytes", "dff_gromos_steps")


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_rmsd_neighbors"][1]) == 8      # device, x, n, N, cutoff, adj, degree, stream
    assert len(binding.SYMBOLS["dff_gromos_steps"][1]) == 13
    assert binding.SYMBOLS["dff_gromos_workspace_bytes"][0] is C.c_longlong


def test_workspace_bytes():
    lib = binding.load_library()
    for n in (-1, (1 << 18) + 1, 1 << 40):
        assert lib.dff_gromos_workspace_bytes(n) == -1
        with pytest.raises(ValueError, match="frame"):
            binding.gromos_workspace_bytes(n)
    # the alive mask (one bit per frame, in 64-bit words) and one key
    assert binding.gromos_workspace_bytes(0) == 8
    assert binding.gromos_workspace_bytes(1) == binding.gromos_workspace_bytes(64) == 16
    assert binding.gromos_workspace_bytes(65) == 24
    assert binding.gromos_workspace_bytes(1 << 18) == (4096 + 1) * 8


def test_neighbors_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n, N = 100, 10
    x = np.zeros((n, N, 3), np.float32)
    adj = np.zeros((n, 2), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731

    def call(n_=n, N_=N, cutoff=2.0, x_=p(x), adj_=p(adj)):
        return lib.dff_rmsd_neighbors(0, x_, n_, N_, cutoff, adj_, None, None)

    for what, kw in (("n_beads must be 4..64", dict(N_=3)), ("n_beads must be 4..64", dict(N_=65)),
                     ("negative frame count", dict(n_=-1)), ("more than 2^18 frames", dict(n_=(1 << 18) + 1)),
                     ("cutoff must be finite and >= 0", dict(cutoff=float("nan"))),
                     ("cutoff must be finite and >= 0", dict(cutoff=float("inf"))),
                     ("cutoff must be finite and >= 0", dict(cutoff=-0.5)),
                     ("null frames", dict(x_=None)), ("null adjacency matrix", dict(adj_=None))):
        assert call(**kw) == 1, what                                     # DFF_EINVAL
        assert what in lib.dff_last_error().decode(), (what, lib.dff_last_error().decode())
    assert call(n_=0, x_=None, adj_=None) == 0                           # n == 0: a valid no-op, nothing is touched
    with pytest.raises(ValueError):
        binding.rmsd_neighbors(torch.zeros((5, 4, 3)), 1.0)              # not a CUDA tensor: refused by the wrapper


def test_gromos_steps_refuses_bad_arguments_on_the_host():
    lib = binding.load_library()
    n = 100
    need = binding.gromos_workspace_bytes(n)
    adj = np.zeros((n, 2), np.uint64)
    out = np.zeros(n, np.int32)
    prog = np.zeros(2, np.int32)
    ws = np.zeros(need + 8, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731

    def call(n_=n, adj_=p(adj), steps=1, kmax=10, labels=p(out), progress=p(prog), ws_=p(ws), ws_bytes=need):
        return lib.dff_gromos_steps(0, adj_, n_, 1, steps, kmax, labels, p(out), p(out), progress, ws_, ws_bytes, None)

    for what, kw in (("negative frame count", dict(n_=-1)), ("more than 2^18 frames", dict(n_=(1 << 18) + 1)),
                     ("negative n_steps", dict(steps=-1)), ("max_clusters must be >= 1", dict(kmax=0)),
                     ("max_clusters must be >= 1", dict(kmax=-3)), ("null adjacency matrix", dict(adj_=None)),
                     ("null output", dict(labels=None)), ("null progress", dict(progress=None)),
                     ("workspace of %d bytes, %d needed" % (need - 1, need), dict(ws_bytes=need - 1)),
                     ("workspace of 0 bytes", dict(ws_=None, ws_bytes=0)),
                     ("8-byte aligned", dict(ws_=C.c_void_p(ws.ctypes.data + 1)))):
        assert call(**kw) == 1, what
        assert what in lib.dff_last_error().decode(), (what, lib.dff_last_error().decode())
    with pytest.raises(ValueError, match="adj"):
        binding.gromos_steps(torch.zeros((5, 1), dtype=torch.int64), {}, 1)   # not a CUDA tensor


# ---------------------------------------------------------------- the oracle on hand-built graphs
def graph(n, edges, finite=None):
    A = np.zeros((n, n), bool)
    for a, b in edges:
        A[a, b] = A[b, a] = True
    fin = np.ones(n, bool) if finite is None else np.asarray(finite, bool)
    A[np.arange(n), np.arange(n)] = fin
    return A


def clique(nodes):
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def test_oracle_two_cliques_joined_by_a_bridge():
    # clique {0..4} (5 frames), clique {5..8} (4), frame 9 is a neighbour of 4 and of 5, frame 10 alone
    A = graph(11, clique([0, 1, 2, 3, 4]) + clique([5, 6, 7, 8]) + [(4, 9), (9, 5)])
    labels, centers, sizes = gromos(A)
    # frame 4 has the 5 of its clique and the bridge: 6; it takes its clique and the bridge with it
    assert centers.tolist() == [4, 5, 10] and sizes.tolist() == [6, 4, 1]
    assert labels.tolist() == [0] * 5 + [1] * 4 + [0, 2]
    # the cap: frames beyond it keep -1
    labels, centers, sizes = gromos(A, max_clusters=1)
    assert centers.tolist() == [4] and labels.tolist() == [0] * 5 + [-1] * 4 + [0, -1]


def test_oracle_breaks_a_tie_by_index():
    # two triangles of equal degree: the one with the lower index goes first, and inside it its lowest frame is the centre
    A = graph(7, clique([4, 5, 6]) + clique([1, 2, 3]))
    labels, centers, sizes = gromos(A)
    assert centers.tolist() == [1, 4, 0] and sizes.tolist() == [3, 3, 1] and labels.tolist() == [2, 0, 0, 0, 1, 1, 1]
    # a path 0 - 1 - 2 - 3: frames 1 and 2 tie at 3; 1 wins and leaves 3 alone
    labels, centers, sizes = gromos(graph(4, [(0, 1), (1, 2), (2, 3)]))
    assert centers.tolist() == [1, 3] and sizes.tolist() == [3, 1] and labels.tolist() == [0, 0, 0, 1]


def test_oracle_all_singletons_and_the_cap():
    labels, centers, sizes = gromos(graph(6, []))
    assert labels.tolist() == list(range(6)) and centers.tolist() == list(range(6)) and sizes.tolist() == [1] * 6
    labels, centers, sizes = gromos(graph(6, []), max_clusters=4)
    assert labels.tolist() == [0, 1, 2, 3, -1, -1] and centers.tolist() == [0, 1, 2, 3]
    # a pair first, then the singleton tail in ascending order
    labels, centers, sizes = gromos(graph(6, [(3, 5)]))
    assert labels.tolist() == [1, 2, 3, 0, 4, 0] and centers.tolist() == [3, 0, 1, 2, 4] and sizes.tolist() == [2, 1, 1, 1, 1]


def test_oracle_non_finite_frame():
    D = np.array([[0.0, 1.0, np.nan, 3.0], [1.0, 0.0, np.nan, 1.5], [np.nan] * 4, [3.0, 1.5, np.nan, 0.0]])
    fin = np.array([True, True, False, True])
    A = neighbors(D, 1.5, fin)
    assert not A[2].any() and not A[:, 2].any() and A[0, 0] and A[1, 3] and not A[0, 3]
    labels, centers, sizes = gromos(A)
    assert labels.tolist() == [0, 0, -1, 0] and centers.tolist() == [1] and sizes.tolist() == [3]
    assert np.array_equal(neighbors(D, 1.0, fin), graph(4, [(0, 1)], fin))       # d <= cutoff: 1.0 itself counts


def test_oracle_bits_round_trip_and_cutoff_picker():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 130):
        A = rng.random((n, n)) < 0.3
        w = pack(A)
        assert w.shape == (n, (n + 63) // 64) and w.dtype == np.int64
        bits = unpack(w, n)
        assert np.array_equal(bits[:, :n], A) and not bits[:, n:].any()
    assert pack(np.eye(65, dtype=bool))[64, 1] == 1 and pack(np.eye(65, dtype=bool))[63, 0] == np.int64(-2 ** 63)
    D = np.zeros((4, 4))
    D[np.triu_indices(4, 1)] = [1.0, 1.1, 1.5, 1.6, 1.7, 3.0]
    assert pick_cutoff(D, 0.9, 2.0) == (pytest.approx(1.3), pytest.approx(0.2))
    with pytest.raises(ValueError):
        pick_cutoff(D, 2.0, 2.9)


# ---------------------------------------------------------------- the evaluator's reductions
def test_evaluator_summarize_on_given_labels():
    sizes = [5, 3, 1, 1]
    labels = np.array([0, 0, 1, -1, 3, 0, -1, 1])
    r = evaluate.RmsdClusterEvaluator.summarize(sizes, 10, labels, samples_nonfinite=2, refs_nonfinite=1)
    assert r["n_clusters"] == 4.0 and r["populations_ref"] == [0.5, 0.3, 0.1, 0.1]
    assert r["populations_samples"] == [3 / 8, 2 / 8, 0.0, 1 / 8] and r["unassigned_share"] == 2 / 8
    assert r["largest_cluster_share_ref"] == 0.5 and r["largest_cluster_share_samples"] == 3 / 8
    assert r["samples_nonfinite"] == 2.0 and r["refs_nonfinite"] == 1.0
    assert r["population_js"] == pytest.approx(evaluate.js_divergence(np.array([5.0, 3, 1, 1, 0]), np.array([3.0, 2, 0, 1, 2])))
    # min_size = 2: the two singletons of the reference and the sample in one of them fall into the unassigned bin
    r = evaluate.RmsdClusterEvaluator.summarize(sizes, 10, labels, min_size=2)
    assert r["n_clusters"] == 2.0 and r["populations_ref"] == [0.5, 0.3] and r["populations_samples"] == [3 / 8, 2 / 8]
    assert r["unassigned_share"] == 3 / 8
    assert r["population_js"] == pytest.approx(evaluate.js_divergence(np.array([5.0, 3, 2]), np.array([3.0, 2, 3])))
    # identical populations: zero divergence; no samples: NaN shares
    same = evaluate.RmsdClusterEvaluator.summarize([2, 1], 3, np.array([0, 1, 0, 0, 1, 0]))
    assert same["population_js"] == pytest.approx(0.0, abs=1e-12) and same["unassigned_share"] == 0.0
    none = evaluate.RmsdClusterEvaluator.summarize([2, 1], 3, np.array([], np.int64))
    assert math.isnan(none["population_js"]) and math.isnan(none["unassigned_share"]) and none["populations_ref"] == [2 / 3, 1 / 3]


def test_evaluator_and_cluster_rmsd_check_their_arguments(monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    ref = torch.zeros((3, 4, 3))
    for kw in (dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(min_size=0)):
        with pytest.raises(ValueError, match="cutoff|min_size"):
            evaluate.RmsdClusterEvaluator(ref, **kw, device="cpu")
    for kw, what in ((dict(stride=0), "stride"), (dict(steps_per_sync=0), "steps_per_sync"), (dict(max_clusters=0), "max_clusters")):
        with pytest.raises(ValueError, match=what):
            evaluate.cluster_rmsd(ref, 1.0, **kw, device="cpu")
    with pytest.raises(ValueError):
        evaluate.cluster_rmsd(torch.zeros((7, 12)), 1.0, device="cpu")
    res = evaluate.cluster_rmsd(torch.zeros((0, 4, 3)), 1.5, stride=3, device="cpu")      # nothing to cluster: no device call
    assert res.n_clusters == 0 and res.labels.shape == (0,) and res.cutoff == 1.5 and res.stride == 3


def test_evaluator_raises_without_library(monkeypatch):
    def missing(*a, **k):
        raise binding.DffLibraryError("libdff_amd.so not found")
    monkeypatch.setattr(binding, "load_library", missing)
    with pytest.raises(binding.DffLibraryError):
        evaluate.RmsdClusterEvaluator(torch.zeros((3, 4, 3)), device="cpu")


# ---------------------------------------------------------------- the package and the tool
def test_package_reexports():
    assert dff_amd.cluster_rmsd is evaluate.cluster_rmsd
    assert dff_amd.RmsdClusterEvaluator is evaluate.RmsdClusterEvaluator
    assert "cluster_rmsd" in dff_amd.__all__ and "RmsdClusterEvaluator" in dff_amd.__all__


def test_cluster_arguments():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    a = ap.parse_args(["s.pt", "chignolin", "refs"])
    assert a.clusters is None and a.cluster_cutoff == 2.0 and a.cluster_stride == 1
    a = ap.parse_args(["s.pt", "chignolin", "refs", "--clusters", "heldout.pt", "--cluster-cutoff", "1.5", "--cluster-stride", "4"])
    assert a.clusters == "heldout.pt" and a.cluster_cutoff == 1.5 and a.cluster_stride == 4
    for bad in ("x", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            ap.parse_args(["s.pt", "chignolin", "refs", "--clusters", "h.pt", "--cluster-cutoff", bad])
