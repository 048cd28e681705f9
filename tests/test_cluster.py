"""dff_rmsd_neighbors and dff_gromos_steps on the GPU.

What is compared how -- nothing here has a tolerance:
- the bit matrix against the existing kernel: adj[s, r] == (dff_rmsd_matrix(x, x)[min(s, r), max(s, r)] <= cutoff), the
  cutoffs taken from the matrix's own values (so that `<=` is met with equality), symmetric, the diagonal set, the padding
  zero, degree = the row popcount;
- against the float64 oracle (oracle/cluster.py) at cutoffs in the middle of a gap of the pair RMSDs that is, on the
  oracle alone, at least 8 times the bar the RMSD kernels are held to (RMSD_ATOL + RMSD_RTOL cutoff, tests/support.py)
  away from every pair: no pair can change sides, so adjacency, labels, centres and sizes must equal the oracle's exactly;
- the greedy loop alone on uploaded bit matrices against the oracle's loop.
"""
import numpy as np
import pytest
import torch

from oracle import cluster as co
from oracle.frames import integer_walks, noisy_ensemble, walks
from fence import COMBINATIONS, fenced
from stream_gate import N_FRAMES, Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import RMSD_ATOL, RMSD_RTOL, B, dev, ev, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

BEADS = [4, 5, 10, 35, 64]


# ---------------------------------------------------------------- helpers
def neighbors_gpu(x, cutoff):
    """-> (bits bool (n, 64 W) with the padding, degree (n,)) of binding.rmsd_neighbors"""
    xd = x if isinstance(x, torch.Tensor) else to_dev(np.asarray(x, np.float32))
    adj, deg = B().rmsd_neighbors(xd, cutoff)
    n = len(xd)
    assert adj.shape == (n, (n + 63) // 64) and adj.dtype == torch.int64 and deg.shape == (n,) and deg.dtype == torch.int32
    return co.unpack(adj.cpu().numpy(), n), deg.cpu().numpy()


def run_loop(A, max_clusters=None, steps=None, adj=None):
    """the greedy loop on the boolean matrix A (uploaded as bits), `steps` iterations per call until nothing is left
    -> (labels, centers, sizes, progress) as numpy, and the number of calls"""
    b = B()
    n = len(A)
    adj = to_dev(co.pack(A)) if adj is None else adj
    kmax = n if max_clusters is None else max_clusters
    st = b.gromos_state(adj, kmax)
    calls = 0
    while True:
        b.gromos_steps(adj, st, n if steps is None else steps)
        calls += 1
        k, left = st["progress"].cpu().tolist()
        if left <= 0 or k >= kmax:
            break
        assert calls <= n + 1, "the loop does not end"
    return out_of(st), calls


def out_of(st):
    k = int(st["progress"][0])
    return (st["labels"].cpu().numpy().astype(np.int64), st["centers"][:k].cpu().numpy().astype(np.int64),
            st["sizes"][:k].cpu().numpy().astype(np.int64), st["progress"].cpu().numpy())


def assert_clustering(got, want, what):
    for g, w, name in zip(got, want, ("labels", "centers", "sizes")):
        assert np.array_equal(g, w), f"{what}: {name} differ: {g[:12]} ... against the oracle's {w[:12]} ..."


def mixed_ensemble(n, N, seed):
    """noisy copies of four templates (close pairs) and random walks (far ones), shuffled"""
    rng = np.random.default_rng(seed)
    k = n // 5
    parts = [noisy_ensemble(rng, t.astype(np.float64), k, 0.5) for t in walks(rng, 4, N)] + [walks(rng, n - 4 * k, N)]
    x = np.concatenate(parts)
    return np.ascontiguousarray(x[rng.permutation(n)])


# ---------------------------------------------------------------- 1. bit-exact against the existing kernel
@pytest.mark.parametrize("n,N", [(200, N) for N in BEADS] + [(2100, 5)])
def test_bits_equal_the_thresholded_matrix(dev, n, N):
    x = mixed_ensemble(n, N, 100 * n + N)
    x[[7, n - 2], 1, 2] = [np.nan, np.inf]
    xd = to_dev(x)
    M = B().rmsd_matrix(xd, xd).cpu().numpy()
    iu = np.triu_indices(n, 1)
    U = np.full((n, n), np.nan, np.float32)
    U[iu] = M[iu]                                               # the value of a pair: the lower index is the query
    U.T[iu] = M[iu]
    fin = np.isfinite(x).all((1, 2))
    vals = np.sort(M[iu][np.isfinite(M[iu])])
    for q in (0.02, 0.25, 0.8):
        cutoff = float(vals[int(q * (len(vals) - 1))])          # a value of the matrix itself: d == cutoff is a neighbour
        bits, deg = neighbors_gpu(xd, cutoff)
        want = co.neighbors(U, np.float32(cutoff), fin)
        A = bits[:, :n]
        bad = np.argwhere(A != want)
        assert not len(bad), f"N={N} n={n} cutoff {cutoff}: {len(bad)} bits differ, first (s, r) = {bad[0]}, d = {U[tuple(bad[0])]!r}"
        assert np.array_equal(A, A.T) and np.array_equal(np.diag(A), fin)
        assert not bits[:, n:].any(), "padding bits set"
        assert np.array_equal(deg, A.sum(1))
        assert not A[~fin].any() and not A[:, ~fin].any()
        print(f"[cluster] N={N} n={n} cutoff {cutoff:.4f} (quantile {q}): {int(np.triu(A, 1).sum())} neighbour pairs, max degree {deg.max()}")
    assert np.triu(A, 1).sum() > 0.5 * len(vals)                # the last cutoff sets most bits, the first few


# ---------------------------------------------------------------- 2. against the fp64 oracle
@pytest.fixture(scope="module")
def oracle_sets():
    """N -> (frames, float64 distances): computed once; a test that changes frames works on a copy"""
    out = {}
    for N in BEADS:
        x = co.ensemble(N, 1000 + N)
        D = co.distances(x)
        out[N] = (x, D)
    return out


def oracle_cutoff(D, N, factor):
    """the cutoff in the window 0.9 - 1.1 x factor x BASE (N = 64: widened until pair RMSDs fall inside) and the condition
    on the oracle alone that makes exact equality a fair demand"""
    if N == 64:
        cutoff, half = co.pick_cutoff_widening(D, factor)
    else:
        cutoff, half = co.pick_cutoff(D, 0.9 * factor * co.BASE, 1.1 * factor * co.BASE)
    margin = RMSD_ATOL + RMSD_RTOL * cutoff
    assert half >= 8 * margin, f"N={N} factor {factor}: half gap {half:.3e} below 8 x {margin:.3e}"
    return cutoff, half / margin


@pytest.mark.parametrize("factor", [1.0, 1.6])
@pytest.mark.parametrize("N", BEADS)
def test_clustering_equals_the_oracle(dev, oracle_sets, N, factor):
    x, D = oracle_sets[N]
    cutoff, clear = oracle_cutoff(D, N, factor)
    want_A = co.neighbors(D, cutoff)
    want = co.gromos(want_A)
    bits, deg = neighbors_gpu(x, cutoff)
    assert np.array_equal(bits[:, :len(x)], want_A) and not bits[:, len(x):].any() and np.array_equal(deg, want_A.sum(1))
    res = ev().cluster_rmsd(x, cutoff, steps_per_sync=7)
    print(f"[cluster] N={N} cutoff {cutoff:.4f} (half gap {clear:.0f} x the bar): {len(want[1])} clusters, sizes {want[2][:6].tolist()}, "
          f"{co.top_ties(want_A)} frames tied for the top degree")
    assert_clustering((res.labels, res.centers, res.sizes), want, f"N={N} factor {factor}")
    assert res.cutoff == cutoff and np.all(np.diff(res.sizes) <= 0) and res.sizes.sum() == len(x)
    # a stride: the clustering of the strided frames, indices in the strided numbering
    sub = co.gromos(want_A[::3, ::3])
    res3 = ev().cluster_rmsd(torch.from_numpy(x), cutoff, stride=3)
    assert_clustering((res3.labels, res3.centers, res3.sizes), sub, f"N={N} factor {factor} stride 3")


# ---------------------------------------------------------------- 3. the greedy loop on its own
def random_graph(n, p, seed, dead=0.05):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((n, n)) < p, 1)
    A = A | A.T
    fin = rng.random(n) >= dead if n > 1 else np.ones(n, bool)
    A &= fin[:, None] & fin[None, :]
    A[np.arange(n), np.arange(n)] = fin
    return A


def hand_built():
    """two cliques joined by a bridge, a tie, a pair with a singleton tail (the graphs of test_cluster_host.py, side by side)"""
    A = np.zeros((24, 24), bool)
    for nodes in ([0, 1, 2, 3, 4], [5, 6, 7, 8], [12, 13, 14], [16, 17, 18]):
        for a in nodes:
            A[a, nodes] = True
    for a, b in ((4, 9), (9, 5), (20, 22)):
        A[a, b] = A[b, a] = True
    np.fill_diagonal(A, True)
    A[23] = A[:, 23] = False                                    # a frame that does not take part
    return A


GRAPHS = [("hand", hand_built)] + [(f"n={n} p={p}", lambda n=n, p=p: random_graph(n, p, 31 * n + int(100 * p)))
                                   for n in (1, 63, 64, 65, 200, 1000) for p in (0.02, 0.3)]


@pytest.mark.parametrize("name,make", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_greedy_loop_equals_the_oracle(dev, name, make):
    A = make()
    n = len(A)
    want = co.gromos(A)
    K = len(want[1])
    adj = to_dev(co.pack(A))
    # one call with many steps (more than are needed: the rest are no-ops decided on the device)
    (l, c, s, prog), calls = run_loop(A, adj=adj)
    assert calls == 1 and prog.tolist() == [K, 0]
    assert_clustering((l, c, s), want, f"{name}, one call")
    assert s.sum() == A.diagonal().sum() and np.all(np.diff(s) <= 0)
    # one step per call
    (l1, c1, s1, prog1), calls1 = run_loop(A, steps=1, adj=adj)
    assert_clustering((l1, c1, s1), want, f"{name}, one step per call")
    iterations = int((want[2] > 1).sum()) + int((want[2] == 1).any())       # the singleton tail is ONE iteration
    assert calls1 == max(iterations, 1), f"{name}: {calls1} calls of one step for {iterations} iterations"
    # a cap below the cluster count: the first `cap` clusters, everybody else -1
    for cap in sorted({1, max(K // 2, 1), max(K - 1, 1)}):
        wl, wc, ws = co.gromos(A, max_clusters=cap)
        (gl, gc, gs, gp), _ = run_loop(A, max_clusters=cap, steps=3, adj=adj)
        assert_clustering((gl, gc, gs), (wl, wc, ws), f"{name}, max_clusters {cap}")
        assert gp[0] == min(cap, K) and gp[1] == A.diagonal().sum() - ws.sum()
    # steps after the end change nothing; a restart on a used state starts over
    b = B()
    st = b.gromos_state(adj, n)
    b.gromos_steps(adj, st, n)
    before = out_of(st)
    b.gromos_steps(adj, st, 5)
    for g, w in zip(out_of(st), before):
        assert np.array_equal(g, w)
    b.gromos_steps(adj, st, 0, restart=True)
    l0, c0, s0, p0 = out_of(st)
    assert (l0 == -1).all() and len(c0) == 0 and p0.tolist() == [0, int(A.diagonal().sum())]
    assert (st["centers"].cpu().numpy() == -1).all() and (st["sizes"].cpu().numpy() == 0).all()
    b.gromos_steps(adj, st, 2)
    b.gromos_steps(adj, st, n)
    assert_clustering(out_of(st)[:3], want, f"{name}, after a restart, 2 + n steps")


# ---------------------------------------------------------------- 4. reproducibility, duplicates
def test_two_calls_are_bit_identical_and_duplicates_share_a_cluster(dev, oracle_sets):
    N = 10
    x0, D0 = oracle_sets[N]
    cutoff0, _ = oracle_cutoff(D0, N, 1.6)
    top = int(co.gromos(co.neighbors(D0, cutoff0))[1][0])
    x = x0.copy()
    copies = sorted({5, 77, 150, top})
    x[copies] = x0[top]                                         # exact duplicates of the most connected frame
    D = co.distances(x)
    cutoff, _ = oracle_cutoff(D, N, 1.6)
    xd = to_dev(x)
    adj1, deg1 = B().rmsd_neighbors(xd, cutoff)
    adj2, deg2 = B().rmsd_neighbors(xd.clone(), cutoff)
    assert torch.equal(adj1, adj2) and torch.equal(deg1, deg2)
    r1, r2 = ev().cluster_rmsd(xd, cutoff), ev().cluster_rmsd(xd, cutoff, steps_per_sync=1)
    for k in ("labels", "centers", "sizes"):
        assert np.array_equal(getattr(r1, k), getattr(r2, k)), k
    assert_clustering((r1.labels, r1.centers, r1.sizes), co.gromos(co.neighbors(D, cutoff)), "duplicates")
    bits = co.unpack(adj1.cpu().numpy(), len(x))[:, :len(x)]
    for c in copies[1:]:
        assert np.array_equal(bits[c], bits[copies[0]]), "duplicates with different neighbours"
    lab = set(r1.labels[copies].tolist())
    assert len(lab) == 1 and -1 not in lab
    # the copies have one degree: where one of them is the centre, it is the lowest-index copy (test_edge_sizes has the
    # case in which it must be)
    assert r1.centers[r1.labels[copies[0]]] not in copies[1:]


# ---------------------------------------------------------------- 5. non-finite frames
def test_non_finite_frames(dev, oracle_sets):
    N = 10
    x0, _ = oracle_sets[N]
    n = len(x0)
    x = x0.copy()
    bad = [0, 63, 64, n - 1]
    x[0, 0, 0] = np.nan
    x[63, N - 1, 2] = np.inf
    x[64, 3, 1] = -np.inf
    x[n - 1] = np.nan
    D = co.distances(x)
    cutoff, _ = oracle_cutoff(D, N, 1.6)
    fin = np.isfinite(x).all((1, 2))
    assert np.flatnonzero(~fin).tolist() == bad
    bits, deg = neighbors_gpu(x, cutoff)
    A = bits[:, :n]
    assert not A[bad].any() and not A[:, bad].any() and (deg[bad] == 0).all()
    want_A = co.neighbors(D, cutoff, fin)
    assert np.array_equal(A, want_A)
    adj = to_dev(co.pack(A))
    st = B().gromos_state(adj, n)
    B().gromos_steps(adj, st, 0)                                 # the restart alone
    assert st["progress"].cpu().tolist() == [0, n - len(bad)]    # not counted
    B().gromos_steps(adj, st, n)
    l, c, s, p = out_of(st)
    assert (l[bad] == -1).all() and (l[fin] >= 0).all() and p.tolist() == [len(c), 0] and s.sum() == n - len(bad)
    assert_clustering((l, c, s), co.gromos(want_A), "non-finite frames")


# ---------------------------------------------------------------- 6. edge sizes
def test_edge_sizes(dev):
    b = B()
    N = 8
    # n = 0: no-ops
    adj, deg = b.rmsd_neighbors(torch.empty((0, N, 3), device=dev), 1.0)
    assert adj.shape == (0, 0) and deg.shape == (0,)
    st = b.gromos_state(adj, 5)
    st["progress"].fill_(77)
    b.gromos_steps(adj, st, 3)
    assert st["progress"].cpu().tolist() == [0, 0]
    assert ev().cluster_rmsd(torch.empty((0, N, 3)), 1.0).n_clusters == 0
    # n = 1: its own cluster; a non-finite one: none
    one = integer_walks(np.random.default_rng(1), 1, N)
    bits, deg = neighbors_gpu(one, 0.0)
    assert bits[0, 0] and bits.sum() == 1 and deg.tolist() == [1]
    r = ev().cluster_rmsd(one, 0.0)
    assert r.labels.tolist() == [0] and r.centers.tolist() == [0] and r.sizes.tolist() == [1]
    r = ev().cluster_rmsd(one * np.float32("nan"), 1.0)
    assert r.labels.tolist() == [-1] and r.n_clusters == 0
    # cutoff = 0: exact duplicates are neighbours, nothing else.  Integer coordinates with 8 beads: centroids, centred
    # coordinates and every sum of products are exact in fp64, so the RMSD of a frame to its copy is exactly 0.
    x = integer_walks(np.random.default_rng(2), 70, N)
    x[[3, 40, 69]] = x[11]
    groups = np.arange(70)
    groups[[3, 40, 69]] = 11
    want_A = groups[:, None] == groups[None, :]
    xd = to_dev(x)
    M = b.rmsd_matrix(xd, xd).cpu().numpy()
    assert np.array_equal(np.triu(M == 0, 1), np.triu(want_A, 1)), "the existing kernel's zeros are not the duplicates"
    bits, deg = neighbors_gpu(xd, 0.0)
    assert np.array_equal(bits[:, :70], want_A) and deg.tolist() == want_A.sum(1).tolist()
    r = ev().cluster_rmsd(xd, 0.0)
    assert_clustering((r.labels, r.centers, r.sizes), co.gromos(want_A), "cutoff 0")
    assert r.centers[0] == 3 and r.sizes.tolist() == [4] + [1] * 66
    # a cutoff above every distance: one cluster around frame 0 (all tie)
    big = float(np.nanmax(M)) * 1.01
    bits, deg = neighbors_gpu(xd, big)
    assert bits[:, :70].all() and not bits[:, 70:].any() and (deg == 70).all()
    r = ev().cluster_rmsd(xd, big)
    assert r.centers.tolist() == [0] and r.sizes.tolist() == [70] and (r.labels == 0).all()


# ---------------------------------------------------------------- 7. stream order
SPEC_CUTOFF = 1.6 * co.BASE      # copies of one template (0.5 A noise per coordinate) are neighbours, random walks nobody's


def neighbors_spec(N):
    n, W = N_FRAMES, (N_FRAMES + 63) // 64
    cutoff = SPEC_CUTOFF

    def wrap(_, bufs):
        adj, deg = B().rmsd_neighbors(bufs["x"], cutoff)
        return {"adj": adj, "degree": deg}
    return Spec("dff_rmsd_neighbors", {"x": (to_dev(mixed_ensemble(n, N, 61)), float("nan"))},
                {"adj": ((n, W), torch.int64), "degree": ((n,), torch.int32)},
                lambda _, bufs: raw("dff_rmsd_neighbors", 0, ptr(bufs["x"]), n, N, cutoff, ptr(bufs["adj"]), ptr(bufs["degree"]),
                                    stream_of(bufs["x"])), wrap=wrap)


def gromos_spec(N):
    b = B()
    n, kmax, steps = N_FRAMES, 64, 40
    adj, _ = b.rmsd_neighbors(to_dev(mixed_ensemble(n, N, 61)), SPEC_CUTOFF)
    torch.cuda.synchronize()
    ws = torch.empty(b.gromos_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    i32 = torch.int32
    return Spec("dff_gromos_steps", {"adj": (adj, 0)},
                {"labels": ((n,), i32), "centers": ((kmax,), i32), "sizes": ((kmax,), i32), "progress": ((2,), i32)},
                lambda _, bufs: raw("dff_gromos_steps", 0, ptr(bufs["adj"]), n, 1, steps, kmax, ptr(bufs["labels"]),
                                    ptr(bufs["centers"]), ptr(bufs["sizes"]), ptr(bufs["progress"]), ptr(bufs["ws"]),
                                    bufs["ws"].numel(), stream_of(bufs["adj"])), work={"ws": ws})


@pytest.mark.parametrize("N", [10, 35])
def test_stream_order(N, gate, side):  # noqa: F811
    ref = analysis_call(neighbors_spec(N), gate, side)
    deg = ref["degree"].cpu().numpy()
    assert deg.min() >= 1 and 1 < deg.max() < N_FRAMES             # a matrix with something in it
    ref = analysis_call(gromos_spec(N), gate, side)
    k, left = ref["progress"].cpu().tolist()
    assert k >= 2 and int(ref["sizes"][0]) > 1 and int((ref["labels"] >= 0).sum()) == N_FRAMES - left


@pytest.mark.parametrize("N", [10, 35, 61])
@pytest.mark.parametrize("make", [neighbors_spec, gromos_spec], ids=["neighbors", "gromos"])
def test_fence(make, N):
    """The memory contract (tests/fence.py): 1000 frames = 15 full words and one of 40 bits per row of the bit-matrix; the alive
    mask and the key of the greedy loop at exactly dff_gromos_workspace_bytes (restart = 1: the call initialises them)."""
    spec = make(N)
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)


# ---------------------------------------------------------------- 8. the evaluator
def test_evaluator_matches_numpy_on_the_oracle_labels(dev, oracle_sets):
    N = 10
    x, D = oracle_sets[N]
    cutoff, _ = oracle_cutoff(D, N, 1.6)
    labels, centers, sizes = co.gromos(co.neighbors(D, cutoff))
    assert sizes[:3].tolist() == [90, 60, 30]
    e = ev().RmsdClusterEvaluator(x, "synthetic", cutoff=cutoff, min_size=2)
    assert np.array_equal(e.clusters.labels, labels) and np.array_equal(e.clusters.centers, centers)
    # samples: fresh noisy copies of the centres of the two largest clusters only, and far outliers.  The cutoff sits in a
    # gap of the REFERENCE's pair RMSDs; the samples' distances to the centres are checked against it in float64 below.
    rng = np.random.default_rng(8)
    n_a, n_b, n_out = 50, 30, 20
    samples = np.concatenate([noisy_ensemble(rng, x[centers[0]].astype(np.float64), n_a, 0.2),
                              noisy_ensemble(rng, x[centers[1]].astype(np.float64), n_b, 0.2), walks(rng, n_out, N)])
    samples[4, 2, 1] = np.nan
    from oracle.struct_metric import kabsch_matrix
    d = kabsch_matrix(samples, x[centers])
    fin = np.isfinite(samples).all((1, 2))
    near, dmin = np.nanargmin(np.where(fin[:, None], d, 0.0), 1), np.nanmin(np.where(fin[:, None], d, 0.0), 1)
    assert np.abs(dmin[fin] - cutoff).min() > 8 * (RMSD_ATOL + RMSD_RTOL * cutoff), "a sample too close to the cutoff"
    lab = np.where(dmin <= cutoff, near, -1)[fin]
    want = ev().RmsdClusterEvaluator.summarize(sizes, len(x), lab, min_size=2, samples_nonfinite=1)
    got = e.eval(samples)
    assert set(got) == {"n_clusters", "populations_ref", "populations_samples", "population_js", "unassigned_share",
                        "largest_cluster_share_ref", "largest_cluster_share_samples", "samples_nonfinite", "refs_nonfinite"}
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k
    # the same reductions by hand
    assert got["n_clusters"] == 3.0 and got["populations_ref"] == [0.45, 0.3, 0.15]
    assert got["populations_samples"] == [(n_a - 1) / 99, n_b / 99, 0.0]           # nothing in the third cluster
    assert got["unassigned_share"] == n_out / 99 and got["samples_nonfinite"] == 1.0 and got["refs_nonfinite"] == 0.0
    assert got["largest_cluster_share_ref"] == 0.45 and got["largest_cluster_share_samples"] == (n_a - 1) / 99
    assert got["population_js"] == pytest.approx(ev().js_divergence(np.array([90.0, 60, 30, 20]), np.array([49.0, 30, 0, 20])))
