"""The forward process and its loss on the GPU (dff_q_sample, dff_denoise_loss, GaussianDiffusion.q_sample / p_losses / forward,
losses.loss_profile, tools_eval_loss.py).  Run with ``-m gpu``.

Shapes: ala2 (5 beads) and chignolin (10) on the <= 16-row kernel, trp_cage (20) on the <= 64-row kernel, the chignolin
force-head model; batches of 1, 7 and 11, the last with dff_debug_max_workgroups(4) (three launches of the score).

Bounds, all from the arithmetic (EPS = 2^-24, one float32 rounding):
  q_sample, per element      (2 N + 6) EPS (max|x0| + 2 max|z|): two N-term float32 means and a handful of roundings
  an in-kernel draw          M_DRAW x E32 of tests/test_noise_stream.py (E32 = max |normals32_plain - normals64| over the very
                             draws under test), through the centring (|P|_inf <= 2) plus the q_sample roundings
  loss arithmetic            relative (3 N + 8) EPS against float64 on the kernel's own x_t, model output and the noise
  against the reference      the score bar of tests/test_gpu_parity.py, rel(gpu, ref64) <= guard_for(kernel) rel(ref32, ref64);
                             sample b's share of it is E_b = guard rel(ref32, ref64) |out64_b| (the shares' squares add up
                             to the bar's), and with r = center_zero(out64_b) - center_zero(z_b):
                               l2: |loss - loss64| <= (2 E_b |r| + E_b^2) / (3 N)      l1: <= sqrt(3 N) E_b / (3 N)
                             plus EPS loss64, the rounding of the float32 the ABI returns the loss in (the synthetic models'
                             output is ~1e-2 of the noise, so the score bar alone is BELOW one float32 rounding of the loss).
"""
import json
import math

import numpy as np
import pytest
import torch

from oracle import noise
from oracle import synth
from support import guard_for, rel, write_model_dir

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
M_DRAW = 4.0          # tests/test_noise_stream.py: |kernel draw - normals64| <= M_DRAW * E32
LIPSCHITZ = 10.0      # tests/test_noise_stream.py: assumed bound of |d eps / d x| of the synthetic networks
HI = 2 ** 32
SEED = (0x9E3779B9 << 32) | 0x2545F491
T = 1000

# name -> (config, conservative, weight seed); the conservative ones are the models the golden vectors were recorded with
MODELS = {"ala2": ("ala2", True, 1234), "chignolin": ("chignolin", True, 1234), "trp_cage": ("trp_cage", True, 1234),
          "chignolin_nc": ("chignolin", False, 4321)}
KERNEL = {"ala2": "dff_small_kernel<", "chignolin": "dff_small_kernel<", "trp_cage": "dff_fused_kernel<",
          "chignolin_nc": "dff_small_kernel<"}
_models = {}


def get_model(name):
    if name not in _models:
        from dff_amd.score import GraphTransformer
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        cfg, cons, wseed = MODELS[name]
        _, N, H, L = synth.SHIPPED_CONFIGS[cfg]
        p = synth.synth_gnn_params(N, H, L, seed=wseed, decoder_out=1 if cons else 3)
        m = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                             use_distances=False, conservative=cons, state_dict=p)
        if name == "ala2":
            m.native.small_waves(8)     # (hidden 96 defaults to the <= 64-row kernel: keep ala2 on the <= 16-row one)
        _models[name] = m
    return _models[name]


def n_beads(name):
    return synth.SHIPPED_CONFIGS[MODELS[name][0]][1]


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def centre(a):
    return a - a.mean(axis=1, keepdims=True)


def inputs(name, B, stream):
    """Un-centred x0, un-centred normals and levels that mix 0, 1, 500, T - 1."""
    N = n_beads(name)
    x0 = (synth.normal((B, N, 3), 9090, stream) + np.array([0.4, -0.3, 0.2])).astype(np.float32)
    z = synth.normal((B, N, 3), 9090, stream + 50).astype(np.float32)
    t = np.array([0, T - 1, 1, 500], np.int64)[np.arange(B) % 4]
    return x0, z, t


def q_sample64(nat, x0, z, t):
    a = nat.schedule("sqrt_alphas_cumprod").astype(np.float64)[t][:, None, None]
    s = nat.schedule("sqrt_one_minus_alphas_cumprod").astype(np.float64)[t][:, None, None]
    return centre(a * x0.astype(np.float64) + s * centre(z.astype(np.float64)))


def q_bound(N, x0, z):
    return (2 * N + 6) * EPS * (np.abs(x0).max() + 2 * np.abs(z).max())


CASES = [(m, B) for m in MODELS for B in (1, 7, 11)]
case_param = pytest.mark.parametrize("name,B", CASES, ids=[f"{m}-{B}" for m, B in CASES])


class knobs:
    """Batch 11 runs with four workgroups per launch (three launches of the score)."""
    def __init__(self, nat, B):
        self.nat, self.n = nat, 4 if B == 11 else 2048

    def __enter__(self):
        self.nat.max_workgroups(self.n)
        return self.nat

    def __exit__(self, *exc):
        self.nat.max_workgroups(2048)


# ------------------------------------------------------------------------------------------------ 1: q_sample, supplied noise
@case_param
def test_q_sample_with_supplied_noise(name, B):
    nat, N = get_model(name).native, n_beads(name)
    x0, z, t = inputs(name, B, 1)
    xt, tn = nat.q_sample(cuda(x0), cuda(t), noise=cuda(z), return_tnorm=True)
    xt, tn = xt.cpu().numpy(), tn.cpu().numpy()
    err, bound = np.abs(xt - q_sample64(nat, x0, z, t)).max(), q_bound(N, x0, z)
    print(f"[ploss] q_sample {name} B={B}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert np.array_equal(tn, t.astype(np.float32) / np.float32(T))
    assert np.abs(xt.mean(1)).max() <= bound


@pytest.mark.parametrize("cfg", ["ala2", "chignolin", "trp_cage"])
def test_q_sample_equals_the_reference(cfg, golden):
    g = golden(f"ploss_{cfg}.npz")
    nat, N = get_model(cfg).native, n_beads(cfg)
    xt, tn = nat.q_sample(cuda(g["x0"]), cuda(g["t"]), noise=cuda(g["noise"]), return_tnorm=True)
    err, bound = np.abs(xt.cpu().numpy() - g["xt"]).max(), q_bound(N, g["x0"], g["noise"])
    print(f"[ploss] q_sample vs reference {cfg}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound and np.abs(centre(g["q_sample"].astype(np.float64)) - xt.cpu().numpy()).max() <= bound
    assert np.array_equal(tn.cpu().numpy(), g["tnorm"])
    # ... and through GaussianDiffusion.q_sample
    from dff_amd.ddpm import GaussianDiffusion
    d = GaussianDiffusion(get_model(cfg), num_atoms=N, timesteps=T)
    assert torch.equal(d.q_sample(torch.from_numpy(g["x0"]), torch.from_numpy(g["t"]), torch.from_numpy(g["noise"])), xt)


@pytest.mark.parametrize("name", ["chignolin", "trp_cage"])
def test_out_of_range_level_gives_nan_for_that_sample_only(name):
    nat = get_model(name).native
    x0, z, _ = inputs(name, 6, 2)
    t_ok = np.array([5, 7, 999, 3, 0, 500], np.int64)
    t_bad = t_ok.copy()
    t_bad[[1, 2, 4]] = (-1, T, 2 ** 31 - 1)
    ok = nat.q_sample(cuda(x0), cuda(t_ok), noise=cuda(z)).cpu().numpy()
    bad, tn = nat.q_sample(cuda(x0), cuda(t_bad), noise=cuda(z), return_tnorm=True)
    bad, tn = bad.cpu().numpy(), tn.cpu().numpy()
    assert np.isnan(bad[[1, 2, 4]]).all() and np.isnan(tn[[1, 2, 4]]).all()
    assert np.array_equal(bad[[0, 3, 5]], ok[[0, 3, 5]]) and np.isfinite(tn[[0, 3, 5]]).all()
    loss = nat.denoise_loss(cuda(x0), cuda(t_bad), noise=cuda(z)).cpu().numpy()
    assert np.isnan(loss[[1, 2, 4]]).all() and np.isfinite(loss[[0, 3, 5]]).all()


# ------------------------------------------------------------------------------------------------ 2: in-kernel noise
def draw_bound(e32, N, zmax, s):
    """Centred draws read out of x_t at x0 = 0: the draw's own error through the centring, and q_sample's roundings / s."""
    return 2 * M_DRAW * e32 + (2 * N + 6) * EPS * 2 * zmax / s


def kernel_draws(nat, N, B, offset, draw):
    """x_t / sqrt_one_minus_alphas_cumprod[T - 1] at x0 = 0, t = T - 1: center_zero of the kernel's draws (float32 x_t too)."""
    s = float(nat.schedule("sqrt_one_minus_alphas_cumprod")[T - 1])
    xt = nat.q_sample(torch.zeros((B, N, 3), device="cuda"), torch.full((B,), T - 1, device="cuda"), seed=SEED,
                      sample_offset=offset, draw=draw).cpu().numpy()
    return xt.astype(np.float64) / s, xt, s


@pytest.mark.parametrize("name", ["ala2", "chignolin", "trp_cage"])
@pytest.mark.parametrize("offset,draw", [(HI - 3, 0), (0, 5), (HI - 3, 5)])
def test_in_kernel_noise_is_the_documented_stream(name, offset, draw):
    from dff_amd import binding
    nat, N, B = get_model(name).native, n_beads(name), 7
    items = np.arange(B, dtype=np.uint64) + np.uint64(offset)
    step = binding.FORWARD_STEP | draw
    z64 = noise.normals64(SEED, items, step, N)
    e32 = float(np.abs(noise.normals32_plain(SEED, items, step, N).astype(np.float64) - z64).max())
    got, xt, s = kernel_draws(nat, N, B, offset, draw)
    err, bound = np.abs(got - centre(z64)).max(), draw_bound(e32, N, np.abs(z64).max(), s)
    print(f"[ploss] draws {name} offset={offset} draw={draw}: max err {err:.3e} (bound {bound:.3e}, E32 {e32:.3e})")
    assert err <= bound
    # the stream does not depend on how the batch is cut into calls
    parts = [nat.q_sample(torch.zeros((n, N, 3), device="cuda"), torch.full((n,), T - 1, device="cuda"), seed=SEED,
                          sample_offset=offset + lo, draw=draw).cpu().numpy() for lo, n in ((0, 3), (3, 4))]
    assert np.array_equal(np.concatenate(parts), xt)
    # another draw index: other normals
    other, _, _ = kernel_draws(nat, N, B, offset, draw + 1)
    assert np.abs(other - got).max() > 0.1


def test_item_range_ends_at_two_to_the_forty():
    nat, N, B, lim = get_model("chignolin").native, 10, 6, 1 << 40
    x0, t = torch.zeros((B, N, 3), device="cuda"), torch.full((B,), 10, device="cuda")
    nat.q_sample(x0, t, seed=SEED, sample_offset=lim - B)
    nat.denoise_loss(x0, t, seed=SEED, sample_offset=lim - B)
    for off in (lim - B + 1, lim, 2 ** 64 - 1):
        with pytest.raises(ValueError, match=r"2\^40"):
            nat.q_sample(x0, t, seed=SEED, sample_offset=off)
        with pytest.raises(ValueError, match=r"2\^40"):
            nat.denoise_loss(x0, t, seed=SEED, sample_offset=off)
    nat.q_sample(x0, t, noise=torch.zeros_like(x0), sample_offset=lim)      # supplied noise does not use the offset
    with pytest.raises(ValueError):
        nat.denoise_loss(x0, t, loss_type="huber")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3: the loss arithmetic
def loss64(out, z, kind):
    d = centre(out.astype(np.float64)) - centre(z.astype(np.float64))
    return (np.abs(d) if kind == "l1" else d * d).reshape(len(d), -1).mean(1)


def check_arithmetic(nat, N, x0, z, t, tag):
    B = len(x0)
    for kind in ("l1", "l2"):
        total = torch.zeros(2, dtype=torch.float64, device="cuda")
        loss, xt, out = nat.denoise_loss(cuda(x0), cuda(t), noise=cuda(z), loss_type=kind, total=total, return_xt=True,
                                         return_model_out=True)
        loss, xt, out, tot = loss.cpu().numpy(), xt.cpu().numpy(), out.cpu().numpy(), total.cpu().numpy()
        ref = loss64(out, z, kind)
        rel = np.abs(loss - ref) / ref
        print(f"[ploss] arithmetic {tag} {kind}: max rel err {rel.max():.3e} (bound {(3 * N + 8) * EPS:.3e}), kernel {nat.last_launch()}")
        assert np.isfinite(out).all() and (rel <= (3 * N + 8) * EPS).all()
        assert np.abs(xt - q_sample64(nat, x0, z, t)).max() <= q_bound(N, x0, z)
        exact = math.fsum(float(v) for v in loss)
        assert abs(tot[0] - exact) <= B * 2.0 ** -52 * exact and tot[1] == B
        yield kind, loss, tot, total


@case_param
def test_loss_arithmetic_and_deterministic_total(name, B):
    model, N = get_model(name), n_beads(name)
    x0, z, t = inputs(name, B, 3)
    # The score's two-workgroups-per-protein variants (trp_cage at these batches) need their whole grid in ONE launch, so the
    # workgroup limit also decides whether dff_score may pick them -- and they add in another order (include/dff.h, NOTE at
    # dff_model_status).  That choice belongs to the score path, not to this call: it is held fixed here (one workgroup per
    # protein), and what is compared across limits is the cutting into launches.  The other tests run the default choice.
    model.native.pair(False)
    try:
        _loss_arithmetic_and_total(model, name, N, B, x0, z, t)
    finally:
        model.native.pair(True)


def _loss_arithmetic_and_total(model, name, N, B, x0, z, t):
    with knobs(model.native, B) as nat:
        first = {k: (loss, tot) for k, loss, tot, _ in check_arithmetic(nat, N, x0, z, t, f"{name} B={B}")}
        assert KERNEL[name] in nat.last_launch()[0]
        for kind, loss, tot, total in check_arithmetic(nat, N, x0, z, t, f"{name} B={B} again"):
            assert np.array_equal(tot, first[kind][1]) and np.array_equal(loss, first[kind][0])
            # the call ADDS to total
            nat.denoise_loss(cuda(x0), cuda(t), noise=cuda(z), loss_type=kind, total=total)
            assert np.array_equal(total.cpu().numpy(), [tot[0] + tot[0], 2 * B])
    # ... and the workgroup limit changes nothing
    nat = model.native
    nat.max_workgroups(2048 if B == 11 else 3)
    try:
        for kind, loss, tot, _ in check_arithmetic(nat, N, x0, z, t, f"{name} B={B} other limit"):
            assert np.array_equal(tot, first[kind][1]) and np.array_equal(loss, first[kind][0])
    finally:
        nat.max_workgroups(2048)


def test_a_batch_beyond_one_pass_of_the_workspace():
    """16384 samples per pass: 16384 + 3 run as two passes over the same workspace, whose size stops growing there."""
    nat, N = get_model("ala2").native, 5
    B = 16384 + 3
    assert nat.denoise_workspace_bytes(B) == nat.denoise_workspace_bytes(16384) == nat.denoise_workspace_bytes(10 ** 6)
    assert nat.denoise_workspace_bytes(7) < nat.denoise_workspace_bytes(8) < nat.denoise_workspace_bytes(16384)
    x0, z, t = inputs("ala2", B, 4)
    for _ in check_arithmetic(nat, N, x0, z, t, f"ala2 B={B}"):
        pass


@pytest.mark.parametrize("name", list(MODELS))
def test_regenerated_target_equals_supplied_draws(name):
    """noise_dev = NULL against noise_dev = the kernel's own (centred) draws, read out of x_t at x0 = 0.  The two runs' targets
    and x_t differ per element by at most D = draw_bound (the read-out's error); the model output follows x_t with at most
    LIPSCHITZ D: d changes by at most (1 + LIPSCHITZ) D per element, so l1 by that and l2 by 2 (1 + L) D mean|d| + ((1 + L) D)^2."""
    from dff_amd import binding
    nat, N, B = get_model(name).native, n_beads(name), 7
    zc, _, s = kernel_draws(nat, N, B, HI - 3, 2)
    items = np.arange(B, dtype=np.uint64) + np.uint64(HI - 3)
    z64 = noise.normals64(SEED, items, binding.FORWARD_STEP | 2, N)
    e32 = float(np.abs(noise.normals32_plain(SEED, items, binding.FORWARD_STEP | 2, N).astype(np.float64) - z64).max())
    D = (1 + LIPSCHITZ) * draw_bound(e32, N, np.abs(z64).max(), s)
    x0, t = torch.zeros((B, N, 3), device="cuda"), torch.full((B,), T - 1, device="cuda")
    for kind in ("l1", "l2"):
        a, out = nat.denoise_loss(x0, t, seed=SEED, sample_offset=HI - 3, draw=2, loss_type=kind, return_model_out=True)
        b = nat.denoise_loss(x0, t, noise=cuda(zc.astype(np.float32)), loss_type=kind)
        a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        mean_abs_d = np.abs(centre(out.cpu().numpy().astype(np.float64)) - zc).reshape(B, -1).mean(1)
        bound = D if kind == "l1" else 2 * D * mean_abs_d + D * D
        print(f"[ploss] regenerated target {name} {kind}: max diff {np.abs(a - b).max():.3e} (bound {np.min(bound):.3e})")
        assert np.isfinite(a).all() and (np.abs(a - b) <= bound + 2 * EPS * a).all()


# ------------------------------------------------------------------------------------------------ 4: against the reference
def reference_bounds(g, kname, out64, z, fwd=False):
    """Per-sample (l1, l2) bounds from the score bar (module docstring)."""
    o32 = g["fwd_out32" if fwd else "out32"]
    bar = guard_for(kname) * rel(o32, out64)
    B, N = out64.shape[:2]
    E = bar * np.linalg.norm(out64.reshape(B, -1), axis=1)
    r = np.linalg.norm((centre(out64) - centre(z.astype(np.float64))).reshape(B, -1), axis=1)
    return {"l1": math.sqrt(3 * N) * E / (3 * N), "l2": (2 * E * r + E * E) / (3 * N)}, bar


@pytest.mark.parametrize("cfg", ["ala2", "chignolin", "trp_cage"])
def test_losses_against_the_reference(cfg, golden):
    from dff_amd.ddpm import GaussianDiffusion
    g = golden(f"ploss_{cfg}.npz")
    model, N = get_model(cfg), n_beads(cfg)
    nat = model.native
    out = nat.score(cuda(g["xt"]), cuda(g["tnorm"])).cpu().numpy()
    kname = nat.last_launch()[0]
    bounds, bar = reference_bounds(g, kname, g["out64"], g["noise"])
    print(f"[ploss] {cfg}: rel(gpu, ref64) = {rel(out, g['out64']):.3e}, bar {bar:.3e}, kernel {kname}")
    assert rel(out, g["out64"]) <= bar
    x0, t, z = cuda(g["x0"]), cuda(g["t"]), cuda(g["noise"])
    d = GaussianDiffusion(model, num_atoms=N, timesteps=T, norm_factor=float(g["norm_factor"]), loss_weights="higheruntil_100")
    for kind in ("l1", "l2"):
        loss = nat.denoise_loss(x0, t, noise=z, loss_type=kind).cpu().numpy().astype(np.float64)
        ref = g[f"{kind}_64"]
        tol = bounds[kind] + EPS * ref
        print(f"[ploss] {cfg} {kind}: |loss - loss64| / tol = {np.abs(loss - ref) / tol}, vs the float32 reference "
              f"{np.abs(loss - g[kind + '_32']).max():.3e}")
        assert (np.abs(loss - ref) <= tol).all()
        # GaussianDiffusion.p_losses: the float32 mean of those (B + 1 more roundings)
        d.loss_type = kind
        mean = d.p_losses(torch.from_numpy(g["x0"]), torch.from_numpy(g["t"]), torch.from_numpy(g["noise"]))
        assert mean.dim() == 0 and mean.dtype == torch.float32
        mref = float(g[f"{kind}_mean64"])
        assert abs(float(mean) - mref) <= tol.mean() + (len(ref) + 1) * EPS * mref
    # forward(): Angstrom input, the recorded multinomial draw injected, the recorded randn_like draw passed through
    d.loss_type = "l2"
    fb, _ = reference_bounds(g, kname, g["fwd_out64"], g["fwd_noise"], fwd=True)
    real = torch.multinomial
    seen = {}

    def recorded(w, n, replacement=False):
        seen["w"], seen["n"], seen["replacement"] = w, n, replacement
        return torch.from_numpy(g["fwd_t"]).to(w.device)
    torch.multinomial = recorded
    try:
        val = d(torch.from_numpy(g["fwd_mol"]), noise=torch.from_numpy(g["fwd_noise"]), t_diff_range=(0, 10))
    finally:
        torch.multinomial = real
    assert seen["w"] is d.p2_loss_weight and seen["n"] == 7 and seen["replacement"] is True
    fref = float(g["fwd_loss64"])
    tol = fb["l2"].mean() + EPS * fref + (7 + 1) * EPS * fref
    # (forward's own centring and division by norm_factor are float32 operations on the input: 3 roundings of |x0| <= 4 through
    # q_sample and the network, LIPSCHITZ at most -- below the score bar by an order of magnitude, inside EPS * loss here)
    print(f"[ploss] {cfg} forward: {float(val):.7f} vs {fref:.7f} (tol {tol:.3e}; float32 reference {float(g['fwd_loss32']):.7f})")
    assert abs(float(val) - fref) <= tol
    t_drawn = torch.multinomial(d.p2_loss_weight, 64, replacement=True)
    assert t_drawn.min() >= 0 and t_drawn.max() < T
    with pytest.raises(AssertionError, match="Normal KL check"):
        d(torch.from_numpy(g["fwd_mol"]) * 1e3)


# ------------------------------------------------------------------------------------------------ 5: the profile and the CLI
def test_loss_profile_equals_explicit_p_losses():
    from dff_amd import losses
    from dff_amd.ddpm import GaussianDiffusion, center_zero
    model, N, norm = get_model("chignolin"), 10, 3.113133430480957
    d = GaussianDiffusion(model, num_atoms=N, timesteps=T, norm_factor=norm, seed=11)
    data = torch.from_numpy((synth.normal((9, N, 3), 555, 1) * norm + 2.0).astype(np.float32))
    levels, draws, bs = [0, 20, 999], 2, 4
    prof = losses.loss_profile(d, data, levels, draws=draws, batch_size=bs)
    assert list(prof["levels"]) == levels and list(prof["count"]) == [9 * draws] * 3 and prof["loss"].dtype == np.float64
    x = center_zero(data.cuda()) / norm
    for k, level in enumerate(levels):
        acc = 0.0
        for lo in range(0, 9, bs):
            xb = x[lo:lo + bs].contiguous()
            for dr in range(draws):
                m = d.p_losses(xb, torch.full((len(xb),), level, device="cuda"), sample_offset=lo, draw=dr)
                acc += float(m) * len(xb)
        want = acc / (9 * draws)
        print(f"[ploss] profile level {level}: {prof['loss'][k]:.8f} vs {want:.8f}")
        assert abs(prof["loss"][k] - want) <= (bs + 2) * EPS * want      # (the explicit means are float32: bs + 1 roundings each)
    # the keys do not depend on the batch size (the sums are taken in another order: not bit for bit)
    assert np.allclose(losses.loss_profile(d, data, levels, draws=draws, batch_size=9)["loss"], prof["loss"], rtol=1e-6, atol=0)
    # p_losses without keys advances the object's counter; seed() rewinds it
    d.seed(11)
    t = torch.full((9,), 20, device="cuda")
    a, b = float(d.p_losses(x, t)), float(d.p_losses(x, t))
    d.seed(11)
    a2 = float(d.p_losses(x, t))
    assert a == a2 and a != b
    d.seed(12)
    assert float(d.p_losses(x, t)) != a
    ev = losses.eval_loss(d, [(data,), (data,)], 2)
    assert ev.dim() == 0 and torch.isfinite(ev)


def test_tools_eval_loss_end_to_end(tmp_path, capsys):
    import tools_eval_loss
    params, (N, H, L) = write_model_dir(tmp_path, "chignolin")
    data = (synth.normal((12, N, 3), 556, 1) * 3.113133430480957).astype(np.float32)
    np.save(tmp_path / "val.npy", data)
    out = tools_eval_loss.main(["--model_path", str(tmp_path), "--data", str(tmp_path / "val.npy"), "--levels", "0:60:20",
                                "--draws", "2", "--batch_size", "8", "--seed", "4"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.loads(json.dumps(out))
    assert [p["level"] for p in out["profile"]] == [0, 20, 40] and all(p["count"] == 24 for p in out["profile"])
    assert all(math.isfinite(p["loss"]) and p["loss"] > 0 for p in out["profile"]) and math.isfinite(out["forward_loss"])
    torch.save(torch.from_numpy(data), tmp_path / "val.pt")
    out2 = tools_eval_loss.main(["--model_path", str(tmp_path), "--data", str(tmp_path / "val.pt"), "--levels", "0,20,40",
                                 "--draws", "2", "--batch_size", "8", "--seed", "4", "--loss_type", "l1"])
    assert out2["loss_type"] == "l1" and [p["level"] for p in out2["profile"]] == [0, 20, 40]
    assert all(a["loss"] != b["loss"] for a, b in zip(out["profile"], out2["profile"]))
