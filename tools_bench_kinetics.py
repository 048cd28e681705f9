#!/usr/bin/env python3
"""Timing of the folding-kinetics calls (dff_struct_native_q / dff_core_states / dff_label_runs) at the output sizes of
BASELINE.json's configs, as tools_bench_states.py does for the state kernels (HIP events, the minimum of five repeats of 20
calls, max / min spread shown).

Next to each call its baseline on the same data:
  native_q      dff_struct_contacts on the same frames (it reads the same bytes; Q does P fp64 exp per frame on top), with the
                native pair list of the first frame (cutoff 10 A, offset 3) and with all N (N - 1) / 2 pairs
  core_states   the only previous device route, a torch chain of where / cummax / gather on the same tensor (torch_core_states
                below), checked equal to the kernel before it is timed
  label_runs    on the labels core_states wrote
Algorithmic bytes per pass: n * N * 12 for Q, n * (4 + 4) for core_states (cv in, labels out; the apply pass reads cv again),
n * 4 for label_runs plus 21 bytes per run.  Trajectories: 80 of equal length.  Prints one JSON line per config."""
import json
import sys

import numpy as np
import torch

import dff_amd
from dff_amd import binding, evaluate

PEAK_HBM = 8.0e12
CASES = [("chignolin config 2 (10240 x 10)", 10, 10240), ("chignolin iid config 3 (100000 x 10)", 10, 100000),
         ("villin config 4 (819200 x 35)", 35, 819200), ("protein G config 5 (409600 x 56)", 56, 409600)]
REPEATS = 5
LO, HI = 0.3, 0.7
TRAJECTORIES = 80          # divides every n of CASES


def ev_time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def timed(fn):
    """(minimum in ms, max / min) over REPEATS windows"""
    t = [ev_time(fn) for _ in range(REPEATS)]
    return min(t) * 1e3, max(t) / min(t)


def torch_core_states(cv, starts, lo, hi):
    """dff_core_states as a chain of torch ops: the index of the latest decisive frame by cummax, then its kind by gather"""
    n = cv.numel()
    fin = torch.isfinite(cv)
    kind = torch.where(fin & (cv <= lo), 0, torch.where(fin & (cv >= hi), 1, -1)).to(torch.int32)
    decisive = ~fin | (kind >= 0)
    decisive[starts] = True
    idx = torch.arange(n, device=cv.device)
    last = torch.cummax(torch.where(decisive, idx, torch.full_like(idx, -1)), 0).values
    return torch.gather(kind, 0, last)


def main():
    dff_amd.load_library()
    torch.manual_seed(0)
    for name, N, n in CASES:
        # a chain with 3.8 A bonds that breathes: Q of its first frame's contacts spreads over 0 .. 1
        step = torch.randn((n, N, 3), device="cuda")
        step = step / step.norm(dim=-1, keepdim=True) * 3.8
        x = (torch.cumsum(step, 1) * torch.rand((n, 1, 1), device="cuda")).contiguous()
        x[0] = torch.cumsum(step[0], 0) * 0.6
        folded = x[0].cpu().numpy().astype(np.float64)
        row = {"workload": name, "n": n, "n_beads": N}
        contacts = torch.from_numpy(np.linalg.norm(folded[:, None] - folded[None], axis=-1) < 10.0).to("cuda", torch.uint8)
        row["struct_contacts_ms"], row["struct_contacts_spread"] = timed(lambda: binding.struct_contacts(x, 10.0, contacts, 3))
        for tag, (pairs, r0) in (("native", evaluate.native_pairs(folded)), ("all", evaluate.native_pairs(folded, 1e9, 1))):
            pd, rd = torch.from_numpy(pairs).cuda(), torch.from_numpy(r0).cuda()
            q = binding.struct_native_q(x, pd, rd)
            ms, spread = timed(lambda: binding.struct_native_q(x, pd, rd))
            row.update({f"native_q_{tag}_pairs": len(pairs), f"native_q_{tag}_ms": ms, f"native_q_{tag}_spread": spread,
                        f"native_q_{tag}_over_contacts": ms / row["struct_contacts_ms"],
                        f"native_q_{tag}_frac_hbm": n * N * 12 / (ms * 1e-3) / PEAK_HBM,
                        f"native_q_{tag}_exp_per_s": n * len(pairs) / (ms * 1e-3)})
            if tag == "native":
                cv = q
        lengths = [n // TRAJECTORIES] * TRAJECTORIES
        starts = torch.arange(0, n, n // TRAJECTORIES, device="cuda")
        ws = torch.empty(binding.kinetics_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        labels = binding.core_states(cv, lengths, LO, HI, workspace=ws)
        same = bool(torch.equal(labels, torch_core_states(cv, starts, LO, HI)))
        row["core_states_ms"], row["core_states_spread"] = timed(lambda: binding.core_states(cv, lengths, LO, HI, workspace=ws))
        row["torch_chain_ms"], row["torch_chain_spread"] = timed(lambda: torch_core_states(cv, starts, LO, HI))
        row.update({"torch_chain_equal": same, "core_states_over_torch_chain": row["core_states_ms"] / row["torch_chain_ms"],
                    "core_states_frac_hbm": n * 8 / (row["core_states_ms"] * 1e-3) / PEAK_HBM,
                    "label_share": [float((labels == v).float().mean()) for v in (-1, 0, 1)]})
        runs = binding.label_runs(labels, lengths, workspace=ws)
        k = int(runs["n_runs"].cpu())
        row["label_runs_ms"], row["label_runs_spread"] = timed(lambda: binding.label_runs(labels, lengths, workspace=ws))
        row.update({"n_runs": k, "label_runs_frac_hbm": (n * 4 + k * 21) / (row["label_runs_ms"] * 1e-3) / PEAK_HBM,
                    "trajectories": len(lengths)})
        print(json.dumps(row))
        sys.stdout.flush()
        if not same:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
