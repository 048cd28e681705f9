#!/usr/bin/env python3
"""Time of RMSD clustering on the GPU (csrc/dff_cluster.hip): the neighbour bit-matrix dff_rmsd_neighbors and the greedy
loop dff_gromos_steps, at evaluation sizes with a cutoff of 2 A, against what the library had before:

  nearest   dff_rmsd_nearest(x, x, self_first=0) on the same ensemble: the existing kernel, which computes the same pairs
            twice (the full square) and keeps one minimum per frame
  matrix    where n <= 16 384 (the 2^28-entry cap of the dense matrix), the only previous route to a neighbour matrix:
            dff_rmsd_matrix plus a torch threshold

The ensemble: CLUSTERS random-walk templates (3.8 A bonds) with populations falling off as 1 / rank, every frame its
template plus Gaussian noise of 0.5 A per coordinate (two copies are ~1.2 A apart: neighbours at 2 A), and 10 % random
walks that are nobody's neighbour (the singleton tail), in a seeded random order.  HIP events around the enqueued work,
one warm-up call, the median of REPS; the greedy loop is timed as a whole (restart to the last cluster, rounds of
STEPS iterations with the two-integer read-back between them, as evaluate.cluster_rmsd runs it).  One JSON line per shape."""
import json
import statistics
import sys

import torch

import dff_amd
from dff_amd import binding

SHAPES = [(10240, 10), (50000, 10), (50000, 35), (20000, 56)]
CUTOFF = 2.0
CLUSTERS = 200
REPS = 5
STEPS = 64
MATRIX_CAP = 1 << 14


def walks(n, N, gen):
    step = torch.randn((n, N, 3), device="cuda", generator=gen)
    step = step * (3.8 / step.norm(dim=-1, keepdim=True))
    return step.cumsum(1).contiguous()


def ensemble(n, N, gen):
    w = 1.0 / torch.arange(1, CLUSTERS + 1, device="cuda", dtype=torch.float64)
    n_out = n // 10
    which = torch.multinomial(w, n - n_out, replacement=True, generator=gen)
    x = walks(CLUSTERS, N, gen)[which] + 0.5 * torch.randn((n - n_out, N, 3), device="cuda", generator=gen)
    x = torch.cat([x, walks(n_out, N, gen)])
    return x[torch.randperm(n, device="cuda", generator=gen)].contiguous()


def ev_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def greedy(adj, state):
    """the whole loop on a fresh state -> (clusters, iterations enqueued)"""
    state["fresh"] = True
    done = 0
    while True:
        binding.gromos_steps(adj, state, STEPS)
        done += STEPS
        k, left = (int(v) for v in state["progress"].cpu())
        if left <= 0:
            return k, done


def main():
    dff_amd.load_library()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for n, N in SHAPES:
        x = ensemble(n, N, gen)
        t_nb = ev_times(lambda: binding.rmsd_neighbors(x, CUTOFF), REPS)
        ws = torch.empty(binding.rmsd_nearest_workspace_bytes(n, n, N), dtype=torch.uint8, device="cuda")
        t_nn = ev_times(lambda: binding.rmsd_nearest(x, x, self_first=0, workspace=ws), REPS)
        adj, deg = binding.rmsd_neighbors(x, CUTOFF)
        state = binding.gromos_state(adj, n)
        k, enq = greedy(adj, state)
        sizes = state["sizes"][:k].cpu()
        iters = int((sizes > 1).sum()) + int(bool((sizes == 1).any()))       # the singleton tail is one iteration
        t_gr = ev_times(lambda: greedy(adj, state), REPS)
        t_it = ev_times(lambda: binding.gromos_steps(adj, state, STEPS, restart=True), REPS)   # STEPS iterations from the start
        nb, nn, gr = statistics.median(t_nb), statistics.median(t_nn), statistics.median(t_gr)
        pairs = n * (n - 1) // 2
        row = {"n": n, "n_beads": N, "cutoff": CUTOFF, "neighbors_ms": nb, "neighbors_ms_min": min(t_nb),
               "neighbors_ms_max": max(t_nb), "pairs_per_s": pairs / (nb * 1e-3), "nearest_self_ms": nn,
               "nearest_self_ms_min": min(t_nn), "nearest_self_ms_max": max(t_nn), "neighbors_over_nearest": nb / nn,
               "mean_degree": float(deg.double().mean()), "clusters": k, "clusters_over_1": int((sizes > 1).sum()),
               "largest": int(sizes.max()), "greedy_iterations": iters, "greedy_iterations_enqueued": enq,
               "greedy_total_ms": gr, "greedy_us_per_enqueued_iteration": gr * 1e3 / enq,
               "greedy_first_round_us_per_iteration": statistics.median(t_it) * 1e3 / STEPS}
        if n <= MATRIX_CAP:
            t_mx = ev_times(lambda: binding.rmsd_matrix(x, x) <= CUTOFF, REPS)
            row["matrix_threshold_ms"] = statistics.median(t_mx)
            row["neighbors_over_matrix"] = nb / row["matrix_threshold_ms"]
        print(json.dumps(row))
        sys.stdout.flush()
        del adj, deg, state, x, ws


if __name__ == "__main__":
    main()
