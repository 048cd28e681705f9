#!/usr/bin/env python3
"""Timing of dff_path_states at the four shapes of tools_bench_kinetics.py, on the same breathing-chain series (its native Q),
in the same way: HIP events, the minimum of five windows of 20 calls, max / min spread shown.

Timed: the call with every output, with the per-frame outputs only, and with the path table only.  Next to it on the same series
  core_states   dff_core_states, the forward half of the scan and all there was before;
  torch chain   the only previous device route to both halves: where / cummax / gather forwards, and the same on the flipped
                series for the backward half (torch_path_states below), checked equal to the kernel before it is timed.
Algorithmic bytes of the full call: n * (4 + 4) read (the reduce and the apply pass both read cv) + n * 19 written (three int8 and
two int64 arrays) + 17 bytes per path.  Trajectories: 80 of equal length.  Prints one JSON line per config."""
import json
import sys

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate
from tools_bench_kinetics import CASES, HI, LO, PEAK_HBM, TRAJECTORIES, timed


def torch_half(core_or_bad, kind, boundary):
    """the kind and the frame of the latest decisive frame (in a core, non-finite, or at `boundary`) by cummax and gather"""
    n = kind.numel()
    decisive = core_or_bad.clone()
    decisive[boundary] = True
    idx = torch.arange(n, device=kind.device)
    last = torch.cummax(torch.where(decisive, idx, torch.full_like(idx, -1)), 0).values
    k = torch.gather(kind, 0, last)
    return k, torch.where(k >= 0, last, torch.full_like(last, -1))


def torch_path_states(cv, starts, lo, hi):
    """prev, next, t_prev, t_next of dff_path_states as a chain of torch ops; starts: the first frames of the (equal-length)
    trajectories, which are also the first frames of the flipped series' trajectories"""
    n = cv.numel()
    fin = torch.isfinite(cv)
    kind = torch.where(fin & (cv <= lo), 0, torch.where(fin & (cv >= hi), 1, -1))
    core_or_bad = ~fin | (kind >= 0)
    prev, t_prev = torch_half(core_or_bad, kind, starts)
    nxt, t_next = torch_half(core_or_bad.flip(0), kind.flip(0), starts)
    return (prev.to(torch.int8), nxt.flip(0).to(torch.int8), t_prev,
            torch.where(t_next >= 0, n - 1 - t_next, torch.full_like(t_next, -1)).flip(0))


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    for name, N, n in CASES:
        # the series of tools_bench_kinetics.py: the native Q of a chain with 3.8 A bonds that breathes
        step = torch.randn((n, N, 3), device="cuda")
        step = step / step.norm(dim=-1, keepdim=True) * 3.8
        x = (torch.cumsum(step, 1) * torch.rand((n, 1, 1), device="cuda")).contiguous()
        x[0] = torch.cumsum(step[0], 0) * 0.6
        pairs, r0 = evaluate.native_pairs(x[0].cpu().numpy().astype(np.float64))
        cv = binding.struct_native_q(x, torch.from_numpy(pairs).cuda(), torch.from_numpy(r0).cuda())
        del x, step
        lengths = [n // TRAJECTORIES] * TRAJECTORIES
        starts = torch.arange(0, n, n // TRAJECTORIES, device="cuda")
        ws = torch.empty(binding.path_states_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        kws = torch.empty(binding.kinetics_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        res = binding.path_states(cv, lengths, LO, HI, workspace=ws)
        k = int(res["n_paths"].cpu())
        chain = torch_path_states(cv, starts, LO, HI)
        same = all(bool(torch.equal(res[key], c)) for key, c in zip(("prev", "next", "t_prev", "t_next"), chain))
        same = same and bool(torch.equal(res["prev"].to(torch.int32), binding.core_states(cv, lengths, LO, HI, workspace=kws)))
        row = {"workload": name, "n": n, "trajectories": len(lengths), "n_paths": k, "torch_chain_equal": same,
               "class_share": [float((res["cls"] == v).float().mean()) for v in range(-1, 6)]}
        for tag, kw in (("all", {}), ("frames", dict(paths=False)), ("table", dict(frames=False, times=False))):
            row[f"path_states_{tag}_ms"], row[f"path_states_{tag}_spread"] = timed(
                lambda: binding.path_states(cv, lengths, LO, HI, workspace=ws, **kw))
        row["core_states_ms"], row["core_states_spread"] = timed(lambda: binding.core_states(cv, lengths, LO, HI, workspace=kws))
        row["torch_chain_ms"], row["torch_chain_spread"] = timed(lambda: torch_path_states(cv, starts, LO, HI))
        row.update({"path_states_over_core_states": row["path_states_all_ms"] / row["core_states_ms"],
                    "path_states_over_torch_chain": row["path_states_all_ms"] / row["torch_chain_ms"],
                    "path_states_frac_hbm": (n * 27 + k * 17) / (row["path_states_all_ms"] * 1e-3) / PEAK_HBM})
        print(json.dumps(row))
        sys.stdout.flush()
        if not same:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
