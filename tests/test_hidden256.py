"""hidden_nf = 256: not a shipped checkpoint size, but the size of the reference's own smoke test
(models/graph_transformer.py:332-359: num_beads 10, hidden_nf 256, n_layers 5, conservative False).  Round 4: the <= 64-row
kernel has fp32-engine variants for it (up to 32 beads).  Golden vectors: tests/golden/make_golden_r04.py (reference
classes, seeded synthetic weights): that exact architecture (force head) and a conservative 20-bead, 2-layer model."""
import numpy as np
import pytest
import torch

from oracle import cpu_repro
from oracle import reference_twin as twin
from oracle import synth
from support import assert_energy, rel, twin_energies

SHAPES = {"smoke": (10, 256, 5, False), "cons": (20, 256, 2, True)}   # N, H, L, conservative


def params_for(name, decoder_scale=1.0):
    N, H, L, cons = SHAPES[name]
    return synth.synth_gnn_params(N, H, L, seed=2560 + N, decoder_scale=decoder_scale, decoder_out=1 if cons else 3)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", list(SHAPES))
def test_twin_matches_reference(name, golden):
    g = golden(f"score_h256_{name}.npz")
    N, H, L, cons = SHAPES[name]
    p = params_for(name)
    # host-independent float32 arithmetic (oracle/cpu_repro.py), as the golden vectors were recorded
    f = cpu_repro.call(twin.score, twin.to_torch(p), torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), L, conservative=cons).numpy()
    assert np.array_equal(f, g["forces32"])
    f64 = twin.score(twin.to_torch(p, torch.float64), torch.from_numpy(g["x"]).double(), torch.from_numpy(g["t"]).double(),
                     L, conservative=cons).numpy()
    assert np.abs(f64 - g["forces64"]).max() < 1e-11


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def _model(name, decoder_scale=1.0):
    from dff_amd.score import GraphTransformer
    N, H, L, cons = SHAPES[name]
    return GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                            use_distances=False, conservative=cons, state_dict=params_for(name, decoder_scale))


@gpu
def test_config_limits_are_reported():
    """hidden sizes without a kernel variant, and bead counts a hidden size cannot hold, are refused with a message --
    not silently mis-run (the reference itself accepts any hidden_nf)."""
    from dff_amd import binding
    lib = binding.load_library()
    for n_beads, hidden, ok in ((10, 256, True), (32, 256, True), (33, 256, False), (10, 192, False), (56, 128, True), (61, 128, True),
                                (62, 128, False)):
        cfg = binding.DffConfig(n_beads, hidden, 2, 1000, 1, 0, 0, 1)
        n = lib.dff_weight_count(cfg)
        w = np.zeros(n, np.float32)
        handle = binding.C.c_void_p()
        rc = lib.dff_model_create(binding.C.byref(cfg), w.ctypes.data_as(binding.C.c_void_p), n, 0,
                                  binding.C.byref(handle))
        assert (rc == 0) == ok, (n_beads, hidden, rc, lib.dff_last_error())
        if rc == 0:
            lib.dff_model_destroy(handle)


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_score_vs_reference(name, golden):
    g = golden(f"score_h256_{name}.npz")
    N, H, L, cons = SHAPES[name]
    model = _model(name)
    x, t = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["t"]).cuda()
    if cons:
        f, e = model.native.score(x, t, return_energy=True)
        np.testing.assert_allclose(e.cpu().numpy()[..., None], g["energy32"], rtol=0, atol=5e-5)
        # ... and the bar of tests/test_score_energy.py: the golden holds no float64 energies, the twin gives them (same seeded weights)
        _, e64 = twin_energies(params_for(name), g["x"], g["t"], L)
        assert_energy(e.cpu().numpy(), g["energy32"], e64, model.native.last_launch()[0], f"h256 {name}")
    else:
        f = model.native.score(x, t)
    f = f.cpu().numpy()
    kname = model.native.last_launch()[0]
    assert kname.startswith("dff_fused_kernel<256,"), kname
    r64, r32 = rel(f, g["forces64"]), rel(g["forces32"], g["forces64"])
    print(f"h256 {name}: {kname} rel(hip,ref64)={r64:.3e} rel(ref32,ref64)={r32:.3e}")
    assert r64 <= 1e-5 and r64 <= 2.5 * max(r32, 4e-7)
    assert np.abs(f - g["forces32"]).max() <= 1e-4 * np.abs(g["forces32"]).max()
    # ragged batch + grouping: the same rows again inside a larger batch
    xb = torch.cat([x, x[:2] + 0.25, x]), torch.cat([t, t[:2], t])
    fb = model.native.score(*xb).cpu().numpy()
    assert rel(fb[:3], f) <= 2e-6 and rel(fb[5:], f) <= 2e-6


@gpu
def test_fused_langevin_vs_reference(golden):
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.langevin import LangevinDiffusion
    g = golden("langevin_h256_cons.npz")
    N = SHAPES["cons"][0]
    model = _model("cons", decoder_scale=1e-2)
    diff = GaussianDiffusion(model, num_atoms=N, timesteps=1000, norm_factor=3.0)
    K, si = int(g["K"]), int(g["save_interval"])
    ld = LangevinDiffusion(diff, torch.from_numpy(g["x0"]), K, save_interval=si, t=20, temp_data=340, temp_sim=340, dt=None,
                           masses=[12.0] * N, friction=1.0, verbose=False)
    traj = ld.sample(noises=torch.from_numpy(g["noise"])).numpy()
    err = np.abs(traj - g["frames"]).max() / np.abs(g["frames"]).max()
    print(f"h256 Langevin K={K}: rel err {err:.3e}")
    assert err <= 5e-6 * K
