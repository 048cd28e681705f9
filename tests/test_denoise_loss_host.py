"""Host side of the denoising loss (no GPU): the ABI symbols, the p2_loss_weight tables against the reference's, the KL check
of forward() and the Philox step reserved for the forward process."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import cpu_repro
from oracle import noise
from oracle import reference_twin as twin

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# golden key -> arguments of ddpm.p2_loss_weight_table (tests/golden/make_golden_ploss.py: TABLES)
TABLES = {"ones_g0.5_k1": ("ones", 1000, 0.5, 1), "score_matching": ("score_matching", 1000),
          "higheruntil_100": ("higheruntil_100", 1000), "lower_bound_10_5": ("lower_bound_10_5", 1000)}


def test_library_exports_the_forward_process_abi():
    import dff_amd
    from dff_amd import binding
    lib = ctypes.CDLL(binding.LIB_PATH)
    for name in ("dff_q_sample", "dff_denoise_workspace_bytes", "dff_denoise_loss"):
        assert hasattr(lib, name), name
        assert name in binding.SYMBOLS
    assert callable(dff_amd.eval_loss) and callable(dff_amd.loss_profile)
    # bad arguments are refused on the host, before a device is touched
    typed = dff_amd.load_library()
    assert typed.dff_denoise_workspace_bytes(None, 4) == -1
    assert typed.dff_q_sample(None, None, None, 1, None, 0, 0, 0, None, None, None) == 1   # DFF_EINVAL
    assert typed.dff_denoise_loss(None, None, None, 1, None, 0, 0, 0, 2, None, None, None, None, None, 0, None) == 1


def test_p2_loss_weight_tables_equal_the_reference_bit_for_bit(golden):
    """All four families at T = 1000, computed under the arithmetic pin the golden vectors were recorded under."""
    from dff_amd import ddpm
    g = golden("ploss_tables.npz")
    got = cpu_repro.call(ddpm.p2_loss_weight_tables, [TABLES[k] for k in TABLES])
    for k, w in zip(TABLES, got):
        assert w.dtype == np.float32 and w.shape == (1000,)
        assert np.array_equal(w, g[k]), (k, np.abs(w - g[k]).max())
    # gamma = 0 ("ones" as every shipped config trains): the uniform distribution over the levels
    assert torch.equal(ddpm.p2_loss_weight_table("ones", 1000), torch.ones(1000))


@pytest.mark.parametrize("bad", ["bogus", "", "Ones", "higher_until_100"])
def test_unknown_loss_weights_raise_the_reference_exception(bad):
    from dff_amd import ddpm
    with pytest.raises(Exception, match=f"Wrong loss_weights: {bad}"):
        ddpm.p2_loss_weight_table(bad)


def _diffusion_without_a_model():
    """assert_normal_kl reads three schedule buffers and nothing else: an object with just those (the constructor needs
    a model on a GPU)."""
    from dff_amd.ddpm import GaussianDiffusion
    d = object.__new__(GaussianDiffusion)
    sched = twin.make_schedule()
    for k in ("sqrt_alphas_cumprod", "alphas_cumprod", "log_one_minus_alphas_cumprod"):
        setattr(d, k, sched[k])
    d.num_timesteps = 1000
    return d


def test_assert_normal_kl_passes_on_unit_scale_data_and_refuses_a_blown_up_molecule():
    d = _diffusion_without_a_model()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 10, 3, generator=g)
    x = x - x.mean(1, keepdim=True)
    t = torch.full((6,), 999, dtype=torch.long)
    d.assert_normal_kl(x, t)
    with pytest.raises(AssertionError, match="Normal KL check at T failed"):
        d.assert_normal_kl(x * 1e4, t)       # un-normalised data of that size is not noise at T - 1
    with pytest.raises(AssertionError, match="Normal KL check at T failed"):
        d.assert_normal_kl(x, torch.full((6,), 500, dtype=torch.long))
    with pytest.raises(AssertionError, match="Center not at zero"):
        d.assert_normal_kl(x + 1.0, t)


def test_forward_step_constant_is_the_documented_counter_word():
    from dff_amd import binding
    assert binding.FORWARD_STEP == 0xFFFFFFFE00000000
    seed = (0x9E3779B9 << 32) | 0x2545F491
    for draw in (0, 5, 2 ** 32 - 1):
        _, c = noise.counters(seed, (7 << 32) | 9, binding.FORWARD_STEP | draw, 11)
        assert [int(v) for v in c] == [9, 7 ^ (11 << 8), draw, 0xFFFFFFFE]
    # distinct from every step the samplers use: DDPM levels, the prior, Langevin steps below the reserved word
    steps = np.array([0, 999, noise.PRIOR_STEP, 2 ** 32, binding.FORWARD_STEP - 1, binding.FORWARD_STEP, binding.FORWARD_STEP | 5],
                     dtype=np.uint64)
    _, c = noise.counters(seed, 3, steps, 0)
    assert len(np.unique(c, axis=0)) == len(steps)
    with open(os.path.join(ROOT, "include", "dff.h")) as f:
        assert "0xFFFFFFFE00000000 | draw" in f.read()
