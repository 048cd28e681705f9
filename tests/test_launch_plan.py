"""Kernel selection without a GPU: the host-only launch plan (dff_debug_plan_launch, the function every launch goes
through) against tests/golden/launch_table.json -- what the library really launched on an MI355X, one launch per case,
recorded by tests/golden/make_launch_table.py before selection became one function -- and the properties the selection
rules promise.  One GPU test holds the plan to what a launch then reports."""
import json
import math
import os

import numpy as np
import pytest

from dff_amd import binding
from oracle import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
with open(os.path.join(ROOT, "tests", "golden", "launch_table.json")) as f:
    TABLE = json.load(f)
LDS_MAX = 160 * 1024
# debug call of a knob setting -> (dff_dispatch field, value written)
KNOB_FIELD = {"force_generic": ("force_generic", lambda a: int(a != 0)), "small_waves": ("small_waves", int),
              "set_group": ("group_override", int), "pair": ("pair_off", lambda a: int(a == 0)),
              "max_workgroups": ("max_wgs", int), "l0_table": ("l0_off", lambda a: int(a == 0))}


def config_of(model):
    c = TABLE["models"][model]
    return binding.DffConfig(c["n_beads"], c["hidden"], c["n_layers"], TABLE["timesteps"], c["use_intrinsic_coords"],
                             c["use_distances"], c["use_abs_coords"], c["conservative"])


def dispatch_of(model, knob, n_cus=None):
    """The dff_dispatch of a recorded case.  The engine flags are what dff_model_create derives for the recorder's
    synthetic weights, which pass the fp16 range guard (the GPU test below reads split == 1 back from live models):
    split unless DFF_SPLIT_BF16=0; the k / v fold for hidden 64 up to 3 layers unless DFF_FOLD_KV=0; a split <= 16-row
    kernel exists for hidden 64 (its only split shape, csrc/dff_small.hip) up to 10 beads."""
    c, k = TABLE["models"][model], TABLE["knobs"][knob]
    env = {**k.get("env_create", {}), **k.get("env_launch", {})}
    split = int(env.get("DFF_SPLIT_BF16") != "0")
    d = dict(split=split, small_split=int(split and c["hidden"] == 64 and c["n_beads"] <= 10),
             fold_kv=int(c["hidden"] == 64 and c["n_layers"] <= 3 and env.get("DFF_FOLD_KV") != "0"),
             n_cus=TABLE["n_cus"] if n_cus is None else n_cus, max_wgs=2048, small_pair=int(env.get("DFF_SMALL_PAIR") == "1"))
    for call, arg in k.get("calls", {}).items():
        field, conv = KNOB_FIELD[call]
        d[field] = conv(arg)
    return d


def planned_cases(**override):
    """(record, config, dispatch, plan) of every recorded case that was launched, the dispatch modified by `override`."""
    for r in TABLE["records"]:
        if len(r) == 7:
            cfg, d = config_of(r[0]), {**dispatch_of(r[0], r[1]), **override}
            yield r, cfg, d, binding.plan_launch(cfg, d, r[2], r[3])


def test_fixture_covers_the_cases_the_rules_name():
    assert len(TABLE["models"]) == 14 and set(synth.SHIPPED_CONFIGS) <= set(TABLE["models"])
    assert len(TABLE["knobs"]) == 13
    cases = {(r[0], r[1], r[2], r[3]) for r in TABLE["records"]}
    assert len(cases) == len(TABLE["records"]) == 14 * 13 * 3 * 10
    assert {r[3] for r in TABLE["records"]} == {1, 32, 100, 128, 129, 256, 257, 512, 768, 2049}
    assert any("pair" in k for k in TABLE["kernels"]) and any("dff_small_kernel" in k for k in TABLE["kernels"])


@pytest.mark.parametrize("model", list(TABLE["models"]))
def test_plan_is_what_the_library_launched(model):
    """Kernel name, LDS bytes and the grid of the last launch of every recorded case; the refusal's message where the
    library refused."""
    cfg, n = config_of(model), 0
    for r in TABLE["records"]:
        if r[0] != model:
            continue
        n += 1
        d = dispatch_of(model, r[1])
        if len(r) == 5:
            with pytest.raises(ValueError) as e:
                binding.plan_launch(cfg, d, r[2], r[3])
            assert str(e.value) == "dff_debug_plan_launch: " + r[4], r
            continue
        p = binding.plan_launch(cfg, d, r[2], r[3])
        assert (p["kernel"], p["last_grid"], p["lds_bytes"]) == (TABLE["kernels"][r[4]], r[5], r[6]), (r, p)
    assert n == 13 * 3 * 10


def test_plan_properties():
    """No plan exceeds the LDS or the 64 bead rows of a workgroup; the launches tile the workgroups as run() does."""
    for r, cfg, d, p in planned_cases():
        assert p["lds_bytes"] <= LDS_MAX, (r, p)
        assert p["G"] >= 1 and p["G"] * cfg.n_beads <= 64, (r, p)
        total = p["workgroups"]
        assert total == (2 * 8 * math.ceil(math.ceil(r[3] / p["G"]) / 8) if p["pair"] else math.ceil(r[3] / p["G"])), (r, p)
        assert p["last_grid"] == total - (total - 1) // d["max_wgs"] * d["max_wgs"], (r, p)
        assert p["launches"] == (total - 1) // d["max_wgs"] + 1, (r, p)
        assert p["pair"] == int("pair" in p["kernel"]) and p["table"] == (0 if d.get("l0_off") or cfg.use_abs_coords else r[2]), (r, p)


def test_a_seen_failure_word_means_no_pair_kernels():
    """With a sticky word the host has seen, the plan is the plan of dff_debug_pair(m, 0)."""
    n_pair = 0
    for r, cfg, d, p in planned_cases():
        n_pair += p["pair"]
        off = binding.plan_launch(cfg, {**d, "pair_off": 1}, r[2], r[3])
        assert not off["pair"] and binding.plan_launch(cfg, {**d, "sticky": 1}, r[2], r[3]) == off, (r, p)
    assert n_pair > 100   # the property was exercised


@pytest.mark.parametrize("n_cus", [64, 128])
def test_pair_kernels_only_where_every_pair_is_resident(n_cus):
    """On a smaller (partitioned, CU-masked) device a PAIR kernel is chosen only where its whole grid -- 16 workgroups
    per 8 groups of G proteins -- fits the CUs, one workgroup each, in one launch."""
    n_pair = 0
    for r, cfg, d, p in planned_cases(n_cus=n_cus):
        if p["pair"]:
            n_pair += 1
            assert 2 * 8 * math.ceil(math.ceil(r[3] / p["G"]) / 8) <= min(n_cus, d["max_wgs"]), (r, p)
    assert n_pair > 50


@pytest.mark.gpu
def test_launch_runs_its_plan():
    """plan_launch(cfg, model.dispatch(), mode, B) taken BEFORE a call is what last_launch() reports after it."""
    import torch
    from dff_amd import weights
    want_split = int(not os.environ.get("DFF_SPLIT_BF16", "").startswith("0"))
    for name in ("chignolin", "ala2", "trp_cage"):
        _, N, H, L = synth.SHIPPED_CONFIGS[name]
        model = binding.Model(N, H, L, weights.flatten_gnn_params(synth.synth_gnn_params(N, H, L, decoder_scale=1e-2), N, H, L))
        assert model.dispatch()["split"] == want_split and model.dispatch()["n_cus"] == torch.cuda.get_device_properties(0).multi_processor_count
        lp = binding.DffLangevinParams(t_norm=0.02, force_scale=1.0, dt=1e-3, vscale=0.9, noisescale=0.4, beta=1.0)
        lp.masses[:N] = [12.0] * N
        for B in (1, 100, 300):
            x = torch.from_numpy(synth.normal((B, N, 3), 1, 1).astype(np.float32)).cuda()
            for mode in (0, 1):
                p = binding.plan_launch(model.cfg, model.dispatch(), mode, B)
                if mode == 0:
                    model.score(x, torch.full((B,), 0.02, device="cuda"))
                else:
                    model.langevin_run(lp, x, torch.zeros_like(x), 1, 1, seed=1)
                assert model.last_launch() == (p["kernel"], p["last_grid"], p["lds_bytes"]), (name, B, mode, p)
        torch.cuda.synchronize()
        assert model.status() == 0
        model.close()
