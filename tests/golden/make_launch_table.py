#!/usr/bin/env python3
"""Recorder of tests/golden/launch_table.json: which kernel the library launches, for every model, knob setting,
sampler mode and batch that the selection rules name (tests/test_launch_plan.py pins the host-only plan to it).

Run on an MI355X, on the commit whose selection is to be recorded:  python tests/golden/make_launch_table.py [out.json]
It uses only Model, the debug knobs and last_launch(): one real launch per case (timesteps = 4 and one step per call --
selection depends on neither), and what last_launch() reports afterwards.  A case the library refuses records the
refusal's message instead.

File layout: `models` (name -> config), `knobs` (name -> {"calls": debug calls made on the model, "env_create":
environment at model creation, "env_launch": environment at the launch}), `kernels` (names), `n_cus`, `timesteps`, and
`records`, one per case: [model, knob, mode, batch, kernel index, grid, lds bytes], or [model, knob, mode, batch, message].
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TIMESTEPS = 4
MODES = (0, 1, 2)   # score, Langevin, DDPM
BATCHES = (1, 32, 100, 128, 129, 256, 257, 512, 768, 2049)


def configs():
    """name -> dff_config fields: the shipped six, hidden 256, every non-shipped input branch, one force-head model."""
    import synth_weights as synth
    keys = ("n_beads", "hidden", "n_layers", "use_intrinsic_coords", "use_distances", "use_abs_coords", "conservative")
    out = OrderedDict((name, dict(zip(keys, (N, H, L, 1, 0, 0, 1)))) for name, (_, N, H, L) in synth.SHIPPED_CONFIGS.items())
    out["hidden256"] = dict(zip(keys, (10, 256, 2, 1, 0, 0, 1)))
    for intr, dist, ab in ((0, 1, 1), (1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0)):
        out[f"gen{intr}{dist}{ab}"] = dict(zip(keys, (10, 64, 3, intr, dist, ab, 1)))
    out["force_head"] = dict(zip(keys, (10, 64, 3, 1, 0, 0, 0)))
    return out


KNOBS = OrderedDict([
    ("default", {}),
    ("force_generic", {"calls": {"force_generic": 1}}),
    ("small_waves4", {"calls": {"small_waves": 4}}),
    ("small_waves8", {"calls": {"small_waves": 8}}),
    ("group1", {"calls": {"set_group": 1}}),
    ("group2", {"calls": {"set_group": 2}}),
    ("group3", {"calls": {"set_group": 3}}),
    ("pair_off", {"calls": {"pair": 0}}),
    ("max_workgroups3", {"calls": {"max_workgroups": 3}}),
    ("l0_off", {"calls": {"l0_table": 0}}),
    ("split_off", {"env_create": {"DFF_SPLIT_BF16": "0"}}),
    ("fold_off", {"env_create": {"DFF_FOLD_KV": "0"}}),
    ("small_pair", {"env_launch": {"DFF_SMALL_PAIR": "1"}}),
])
RESET = {"force_generic": 0, "small_waves": 0, "set_group": 0, "pair": 1, "max_workgroups": 2048, "l0_table": 1}


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_model(c):
    import synth_weights as synth
    from dff_amd import binding, weights
    N, H, L = c["n_beads"], c["hidden"], c["n_layers"]
    intr, dist, ab, cons = c["use_intrinsic_coords"], c["use_distances"], c["use_abs_coords"], c["conservative"]
    params = synth.synth_gnn_params(N, H, L, decoder_scale=1e-2, decoder_out=1 if cons else 3, node_in=N + 1 + 3 * ab,
                                    edge_in=(3 * intr + dist) or 1)
    flat = weights.flatten_gnn_params(params, N, H, L, bool(cons), bool(intr), bool(dist), bool(ab))
    return binding.Model(N, H, L, flat, timesteps=TIMESTEPS, use_intrinsic_coords=intr, use_distances=dist,
                         use_abs_coords=ab, conservative=cons)


def launch(model, mode, B):
    import torch
    from dff_amd import binding
    N = model.n_beads
    x = torch.zeros(B, N, 3, device="cuda")
    x[:, :, 0] = torch.arange(N, device="cuda", dtype=torch.float32)[None, :] * 0.3
    if mode == 0:
        model.score(x, torch.full((B,), 0.25, device="cuda"))
    elif mode == 1:
        p = binding.DffLangevinParams(t_norm=0.25, force_scale=1.0, dt=1e-3, vscale=0.9, noisescale=0.4, beta=1.0,
                                      dtau=0.0, overdamped=0)
        for i in range(N):
            p.masses[i] = 12.0
        model.langevin_run(p, x, torch.zeros_like(x), 1, 1, seed=1)
    else:
        model.ddpm_run(x, 1, 1, seed=1)


def main(out_path):
    import torch
    from dff_amd import binding
    lib = binding.load_library()
    cfgs = configs()
    kernels, records = [], []
    for mname, c in cfgs.items():
        by_env = {}
        for kname, knob in KNOBS.items():
            env_create = knob.get("env_create", {})
            key = tuple(sorted(env_create.items()))
            if key not in by_env:
                with _Env(env_create):
                    by_env[key] = make_model(c)
            model = by_env[key]
            for call, arg in {**RESET, **knob.get("calls", {})}.items():
                getattr(model, call)(arg)
            with _Env(knob.get("env_launch", {})):
                for mode in MODES:
                    for B in BATCHES:
                        try:
                            launch(model, mode, B)
                        except ValueError:
                            records.append([mname, kname, mode, B, lib.dff_last_error().decode()])
                            continue
                        name, grid, lds = model.last_launch()
                        if name not in kernels:
                            kernels.append(name)
                        records.append([mname, kname, mode, B, kernels.index(name), grid, lds])
            torch.cuda.synchronize()
        for model in by_env.values():
            torch.cuda.synchronize()
            st = model.status()   # read only now: a word the host has seen changes the selection
            if st:
                print(f"WARNING: {mname}: sticky status {st:#x} (a two-workgroups launch lost its partner)", flush=True)
            model.close()
        print(f"{mname}: {len(records)} records", flush=True)
    table = OrderedDict(version=lib.dff_version().decode(), device=torch.cuda.get_device_name(0),
                        n_cus=torch.cuda.get_device_properties(0).multi_processor_count, timesteps=TIMESTEPS,
                        models=cfgs, knobs=KNOBS, kernels=kernels)
    head = json.dumps(table, indent=1)
    body = ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in records)
    with open(out_path, "w") as f:
        f.write(head[:-2] + ',\n "records": [\n' + body + "\n ]\n}\n")
    print(f"wrote {out_path}: {len(records)} records, {len(kernels)} kernels")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_table.json"))
