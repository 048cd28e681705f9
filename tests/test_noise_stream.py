"""The in-kernel noise stream (noise_dev == NULL: Philox4x32-10 + Box-Muller on the hardware transcendentals, csrc/dff_device.h)
against the host reference oracle/noise.py, draw by draw, for every kernel variant that draws.

CPU: the Random123 known-answer vectors of Philox4x32-10, the edge words of the float32 uniforms, distinct counters inside the
documented range.  GPU (-m gpu): (a) one Langevin step arranged so that v_out is the draw times a power of two -- an exact
read-out of every draw; (b) 1, 2 and 7 Langevin steps with force_scale = 0 against the float64 recurrence on the reference's
draws, in one launch and chunked; (c) the reverse-DDPM steps and the prior against the same launch on supplied noise
float32(normals64); (d) the 2^40 limit of offset + count.  CASES is the variant matrix: each case asserts the kernel that ran,
so a dispatch change cannot empty it, and says whether the <= 16-row kernel's idle last wave pre-draws the normals (xi_pre).

Tolerance of a draw.  The uniforms are exact, so a draw differs from normals64 only by the error of v_log_f32, v_sqrt_f32,
v_sin_f32 / v_cos_f32.  The yardstick is NOT the kernel: E32 = max |normals32_plain - normals64| over the very draws under test
(the same Box-Muller in plain numpy float32; 1.6e-6 over 2e5 random words, 0.8 - 1.0e-6 over 600 draws), and every draw must lie
within M_DRAW * E32 of normals64.  A wrong counter, word, step or item gives an unrelated normal -- an O(1) error -- so the
factor only guards the accuracy claim.
MEASURED on the MI355X: worst draw 4.3e-7 = 0.65 x E32 (docstring of test_langevin_one_step_reads_out_every_draw).
"""
import numpy as np
import pytest

from oracle import noise
from oracle import synth
from support import EPS, M_DRAW, e32_of as _e32
from variants import CASES, HI, MODELS, Case, get_native

SEED = (0x9E3779B9 << 32) | 0x2545F491      # non-zero high word


# ------------------------------------------------------------------------------------------------ CPU: the host reference
@pytest.mark.parametrize("key,ctr,out", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 2, (0xFFFFFFFF,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(key, ctr, out):
    """The three known-answer vectors Random123 ships for philox4x32_10 (kat_vectors)."""
    w = noise.philox4x32_10(np.array(key), np.array(ctr))
    assert w.dtype == np.uint32 and " ".join(f"{int(v):08x}" for v in w) == out
    # vectorised: the same block inside a batch of different ones
    keys = np.array([(1, 2), key, (3, 4)], dtype=np.uint64)
    ctrs = np.array([(5, 6, 7, 8), ctr, (0, 0, 0, 1)], dtype=np.uint64)
    assert " ".join(f"{int(v):08x}" for v in noise.philox4x32_10(keys, ctrs)[1]) == out


def test_uniform_edge_words():
    """w = 0 -> 2^-33 (the largest |z|: sqrt(66 ln 2) = 6.7637); w >= 2^32 - 128 -> u = 1, r = 0; never 0, never above 1."""
    w = np.array([0, 1, 2, 255, 256, 2 ** 24, 2 ** 24 + 1, 2 ** 31, HI - 257, HI - 256, HI - 129, HI - 128, HI - 127, HI - 1], np.uint32)
    u = noise.uniforms(w)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32)
    assert (u[-3:] == 1.0).all() and (u[:-3] < 1.0).all() and (u > 0).all() and (u <= 1.0).all()
    assert np.all(np.diff(u.astype(np.float64)) >= 0)
    rng = np.random.default_rng(11)
    ur = noise.uniforms(rng.integers(0, HI, size=200000, dtype=np.uint32))
    assert ur.min() > 0 and ur.max() <= 1.0
    # through the Box-Muller: the extreme draws
    for box in (lambda ww: noise._box_muller(ww, np.float64, np.float64(2 * np.pi)),
                lambda ww: noise._box_muller(ww, np.float32, np.float32(2 * np.pi))):
        z = box(np.array([[0, HI - 1, 0, HI - 1], [HI - 128, 12345, HI - 1, 999]], np.uint32))
        assert abs(z[0, 0] - 6.7637056) < 1e-5 and abs(z[0, 2] - 6.7637056) < 1e-5 and abs(z[0, 1]) < 1e-5
        assert (z[1] == 0).all() and np.isfinite(z).all()


def test_plain_float32_yardstick_is_of_the_expected_size():
    """E32 over 2e5 random word quadruples + the edge words: about 1.6e-6, dominated by the rounding of 2 pi u at large r."""
    rng = np.random.default_rng(5)
    w = rng.integers(0, HI, size=(200000, 4), dtype=np.uint32)
    w[:8] = np.array([0, 1, HI - 1, HI - 128, HI - 129, 2 ** 31, 2 ** 30, 3 * 2 ** 30], np.uint32)[:, None]
    w[8:16, 1] = w[:8, 0]
    e32 = np.abs(noise._box_muller(w, np.float32, np.float32(2 * np.pi)).astype(np.float64)
                 - noise._box_muller(w, np.float64, np.float64(2 * np.pi))).max()
    assert 5e-7 < e32 < 3e-6, e32


def test_counters_are_distinct_inside_the_supported_range():
    items = [0, 1, 2, 255, 256, HI - 2, HI - 1, HI, HI + 1, (1 << 40) - 2, (1 << 40) - 1]
    steps = [0, 1, 2, 999, HI - 2, HI - 1, HI, HI + 1, (1 << 63) + 5]
    it, st, bd = np.meshgrid(np.array(items, np.uint64), np.array(steps, np.uint64), np.arange(64, dtype=np.uint64), indexing="ij")
    key, ctr = noise.counters(SEED, it, st, bd)
    assert (key[..., 0] == (SEED & 0xFFFFFFFF)).all() and (key[..., 1] == (SEED >> 32)).all()
    flat = ctr.reshape(-1, 4)
    assert len(np.unique(flat, axis=0)) == len(flat)
    out = noise.philox4x32_10(key, ctr).reshape(-1, 4)
    assert len(np.unique(out, axis=0)) == len(out)            # (a bijection of the counter for a fixed key)
    # the documented layout, word by word
    k, c = noise.counters(SEED, (7 << 32) | 9, (3 << 32) | 5, 11)
    assert [int(v) for v in c] == [9, 7 ^ (11 << 8), 5, 3] and [int(v) for v in k] == [SEED & 0xFFFFFFFF, SEED >> 32]
    assert [int(v) for v in noise.counters(SEED, 3, noise.PRIOR_STEP, 0)[1]] == [3, 0, 0xFFFFFFFF, 0]
    # ... and why the range ends at 2^40: bit 40 of the item is bit 0 of the bead
    with pytest.raises(ValueError):
        noise.counters(SEED, 1 << 40, 0, 0)
    assert noise.ITEM_LIMIT == 1 << 40 and (((1 << 40) >> 32) ^ (0 << 8)) == ((0 >> 32) ^ (1 << 8))


def test_normals_shapes_and_components():
    z = noise.normals64(SEED, np.arange(3) + HI - 2, np.array([[0], [HI + 1]]), 4)
    assert z.shape == (2, 3, 4, 3) and z.dtype == np.float64
    w = noise.philox4x32_10(*noise.counters(SEED, HI - 1, HI + 1, 2))
    u = noise.uniforms(w).astype(np.float64)
    r0, r2 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    exp = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r2 * np.cos(2 * np.pi * u[3])]
    assert np.array_equal(z[1, 1, 2], np.array(exp))
    z32 = noise.normals32_plain(SEED, np.arange(3) + HI - 2, np.array([[0], [HI + 1]]), 4)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 3e-6


# ------------------------------------------------------------------------------------------------ GPU: the kernels' draws
gpu = pytest.mark.gpu

case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])


def _state(case, stream):
    """Centred O(1) coordinates for the case's batch, float32."""
    x = synth.normal((case.B, case.N, 3), 20261, stream)
    return (x - x.mean(1, keepdims=True)).astype(np.float32)


def _items(case):
    return np.arange(case.B, dtype=np.uint64) + np.uint64(case.offset)


# Langevin parameters of (a) and (b): beta = 1 and masses 4^-k make noise_sigma = sqrt(1 / (beta m)) = 2^k exactly, a different
# one per bead; noisescale is a power of two; vscale is arbitrary.
SIGMAS = np.array([1.0, 2.0, 0.5, 0.25, 4.0])
NOISESCALE, VSCALE, DT = 0.5, 0.7, 0.5


def _langevin_params(N, force_scale=0.0):
    from dff_amd import binding
    p = binding.DffLangevinParams()
    p.t_norm, p.force_scale, p.dt, p.vscale, p.noisescale, p.beta, p.dtau, p.overdamped = 0.02, force_scale, DT, VSCALE, NOISESCALE, 1.0, 0.0, 0
    sig = SIGMAS[np.arange(N) % len(SIGMAS)]
    for i in range(N):
        p.masses[i] = float(1.0 / sig[i] ** 2)
    return p, sig


def _run_langevin(nat, p, x, v, n_steps, seed, offset, step_offset):
    import torch
    xd, vd = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    nat.langevin_run(p, xd, vd, n_steps, n_steps, seed=seed, traj_offset=offset, step_offset=step_offset)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), vd.cpu().numpy()


def _report(tag, err, z64, e32, extra=""):
    """Print the worst draw's error, its ratio to E32 and where it sits (radius, angle) before anything is asserted."""
    k = np.unravel_index(np.nanargmax(np.where(np.isfinite(err), err, np.inf)), err.shape)
    print(f"[noise] {tag}: max |kernel - normals64| = {err[k]:.3e} = {err[k] / e32:.2f} x E32 ({e32:.3e}) over {err.size} draws; "
          f"worst at {tuple(int(i) for i in k)} z = {z64[k]:+.4f}{extra}")


@gpu
@case_param
def test_langevin_one_step_reads_out_every_draw(case):
    """(a) force_scale = 0, v = 0, noisescale and noise_sigma powers of two: v_out = noisescale * (noise_sigma * xi) without a
    rounding, so v_out / (noisescale noise_sigma) IS the kernel's draw; the network runs (real weights) but contributes f = 0 --
    a non-finite force would turn v_out into NaN and fail here.  Every draw of the batch is compared.
    MEASURED on the MI355X (first run, all 24 cases, 90 .. 2400 draws each): max |kernel - normals64| per case 1.7e-7 .. 4.3e-7
    against E32 = 4.5e-7 .. 1.3e-6 of the same draws -- ratio 0.26 .. 0.65, worst draw 4.26e-7 at z = +3.80 (0.64 x E32): the
    hardware Box-Muller is CLOSER to float64 than numpy's float32 one (v_sin_f32 / v_cos_f32 take the angle in revolutions and
    skip the rounding of 2 pi u).  M_DRAW = 4 leaves a factor of six."""
    p, sig = _langevin_params(case.N)
    x, v0 = _state(case, 1), np.zeros((case.B, case.N, 3), np.float32)
    with case.knobs() as nat:
        _, v1 = _run_langevin(nat, p, x, v0, 1, SEED, case.offset, case.step_offset)
        name = case.check_launch(nat)
    e32, z64 = _e32(SEED, _items(case), case.step_offset, case.N)
    draws = v1.astype(np.float64) / (NOISESCALE * sig)[None, :, None]
    err = np.abs(draws - z64)
    _report(f"(a) {case.id} {name}", err, z64, e32)
    assert np.isfinite(v1).all(), "non-finite velocities: the forces of this state are not finite"
    assert (err <= M_DRAW * e32).all()


def _langevin_oracle(x, v, z64, sig):
    """float64 recurrence of the BAOAB step with f = 0 (csrc: centre; x += v dt / 2; v = v vscale + noisescale sigma xi;
    x += v dt / 2) on the reference's draws z64 (n, B, N, 3).  Returns x, v and the largest |x|, |v| on the way."""
    x, v = x.astype(np.float64), v.astype(np.float64)
    vs, ns, dt = float(np.float32(VSCALE)), float(np.float32(NOISESCALE)), float(np.float32(DT))
    xmax, vmax = np.abs(x).max(), np.abs(v).max()
    for z in z64:
        x = x - x.mean(1, keepdims=True)
        x = x + v * dt / 2
        v = v * vs + ns * (sig[None, :, None] * z)
        x = x + v * dt / 2
        xmax, vmax = max(xmax, np.abs(x).max()), max(vmax, np.abs(v).max())
    return x, v, xmax, vmax


@gpu
@case_param
@pytest.mark.parametrize("n_steps", [1, 2, 7])
def test_langevin_steps_follow_the_reference_draws(case, n_steps):
    """(b) force_scale = 0: the dynamics are linear in the draws.  Bound: with d = M_DRAW E32 per draw, after s steps
        |dv_s| <= Dv_s = vscale Dv_{s-1} + noisescale sigma_max d + 3 EPS vmax,  Dv_0 = 0        (<= 3 roundings of v per step)
        |dx_n| <= 2 sum_s [ dt / 2 (Dv_s + Dv_{s+1}) + (N + 6) EPS xmax ]
    (a step adds v dt / 2 twice and rounds the bead mean -- N roundings of partial sums -- and five more operations; the centring
    is a projection P, P P = P, |P|_inf <= 2, so the accumulated error is projected once, not once per step).
    In one launch and as two chunks (step_offset advanced): the velocities, a function of the draws alone, agree bit for bit."""
    p, sig = _langevin_params(case.N)
    x0 = _state(case, 2)
    v0 = (0.25 * synth.normal((case.B, case.N, 3), 20261, 3)).astype(np.float32)
    steps = np.arange(n_steps, dtype=np.uint64) + np.uint64(case.step_offset)
    e32, z64 = _e32(SEED, _items(case)[None, :], steps[:, None], case.N)
    xr, vr, xmax, vmax = _langevin_oracle(x0, v0, z64, sig)
    d = M_DRAW * e32
    dv = [0.0]
    for s in range(1, n_steps + 1):
        dv.append(float(np.float32(VSCALE)) * dv[-1] + NOISESCALE * sig.max() * d + 3 * EPS * vmax)
    dx = 2 * sum(DT / 2 * (dv[s] + dv[s + 1]) + (case.N + 6) * EPS * xmax for s in range(n_steps))
    with case.knobs() as nat:
        x1, v1 = _run_langevin(nat, p, x0, v0, n_steps, SEED, case.offset, case.step_offset)
        case.check_launch(nat)
        k = n_steps // 2
        if k:
            xa, va = _run_langevin(nat, p, x0, v0, k, SEED, case.offset, case.step_offset)
            x2, v2 = _run_langevin(nat, p, xa, va, n_steps - k, SEED, case.offset, case.step_offset + k)
            case.check_launch(nat)
    ev, ex = np.abs(v1 - vr).max(), np.abs(x1 - xr).max()
    print(f"[noise] (b) {case.id} n={n_steps}: |dv| = {ev:.3e} (bound {dv[-1]:.3e}), |dx| = {ex:.3e} (bound {dx:.3e}), E32 = {e32:.3e}")
    assert np.isfinite(v1).all() and np.isfinite(x1).all()
    assert (np.abs(v1 - vr) <= dv[-1]).all() and (np.abs(x1 - xr) <= dx).all()
    if k:
        assert np.array_equal(v2, v1)
        assert (np.abs(x2 - xr) <= dx).all()


def _ddpm(nat, x, t_start, t_end, noise_=None, offset=0, init_prior=False):
    import torch
    xd = torch.from_numpy(x).cuda()
    nd = torch.from_numpy(np.ascontiguousarray(noise_, np.float32)).cuda() if noise_ is not None else None
    nat.ddpm_run(xd, t_start, t_end, noise=nd, seed=SEED, sample_offset=offset, init_prior=init_prior)
    torch.cuda.synchronize()
    return xd.cpu().numpy()


LIPSCHITZ = 10.0     # assumed bound of |d eps / d x| of the synthetic networks (their forces are O(1) for O(1) inputs); it enters
                     # only through c1 sqrt_recipm1 = 4.4e-3 (levels 500 .. 497) and 6.4e-3 (level 0): 4 - 6 % of the bound


def _level_terms(nat, t):
    s = {k: float(nat.schedule(k)[t]) for k in ("posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
                                                "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")}
    sigma = float(np.exp(0.5 * s["posterior_log_variance_clipped"])) if t > 0 else 0.0
    amp = abs(s["posterior_mean_coef1"] * s["sqrt_recip_alphas_cumprod"] + s["posterior_mean_coef2"]) \
        + abs(s["posterior_mean_coef1"] * s["sqrt_recipm1_alphas_cumprod"]) * LIPSCHITZ
    return sigma, amp


def _centred_noise_bound(e32, N, zmax):
    """Two runs whose normals differ by at most  M_DRAW E32 (the draw) + 2^-22 (float32 rounding of the supplied |z| < 8):
    after subtracting the bead mean (|P|_inf <= 2; N + 1 roundings that may fall differently in the two runs)."""
    return 2 * (M_DRAW * e32 + 2.0 ** -22) + 2 * (N + 1) * EPS * zmax


def _level_bound(sigma, cn, N, ymax):
    """x_new = mean + sigma xi_c, then centred: the means are bit-identical in the two runs (same x, same deterministic kernel),
    so the outputs differ by sigma (difference of the centred normals) + 3 roundings of magnitude ymax, projected (x 2), plus the
    N + 1 roundings of the last bead mean."""
    return 2 * (sigma * cn + 3 * EPS * ymax) + 2 * (N + 1) * EPS * ymax


@gpu
@case_param
def test_ddpm_steps_equal_the_same_launch_on_reference_noise(case):
    """(c) dff_ddpm_run(noise = NULL) against dff_ddpm_run(noise = float32(normals64)): same model, input, levels, kernel.
    One level per launch at t = 999, 500, 1, 0 (bit-identical at 0: the noise is masked) and levels 500 .. 497 fused, where a
    difference made at one level passes through the later ones amplified by at most
    A_t = |c1 sqrt_recip + c2| + |c1 sqrt_recipm1| LIPSCHITZ per level (schedule tables)."""
    x = _state(case, 4)
    items, N = _items(case), case.N
    with case.knobs() as nat:
        for t in (999, 500, 1, 0):
            e32, z64 = _e32(SEED, items, t, N)
            ya = _ddpm(nat, x, t, t, None, case.offset)
            name = case.check_launch(nat)
            yb = _ddpm(nat, x, t, t, z64[None], case.offset)
            case.check_launch(nat)
            sigma, _ = _level_terms(nat, t)
            bound = _level_bound(sigma, _centred_noise_bound(e32, N, np.abs(z64).max()), N, np.abs(yb).max())
            diff = np.abs(ya - yb).max()
            print(f"[noise] (c) {case.id} {name} t={t}: |y_philox - y_supplied| = {diff:.3e} (bound {bound:.3e}, sigma_t {sigma:.3e})")
            assert np.isfinite(ya).all() and np.isfinite(yb).all()
            if t == 0:
                assert np.array_equal(ya, yb)
            else:
                assert (np.abs(ya - yb) <= bound).all()
        levels = np.array([500, 499, 498, 497], dtype=np.uint64)
        e32, z64 = _e32(SEED, items[None, :], levels[:, None], N)
        ya = _ddpm(nat, x, 500, 497, None, case.offset)
        case.check_launch(nat)
        yb = _ddpm(nat, x, 500, 497, z64, case.offset)
        cn = _centred_noise_bound(e32, N, np.abs(z64).max())
        bound = 0.0
        for t in (500, 499, 498, 497):
            sigma, amp = _level_terms(nat, t)
            bound = bound * amp + _level_bound(sigma, cn, N, np.abs(yb).max())
        diff = np.abs(ya - yb).max()
        print(f"[noise] (c) {case.id} t=500..497 fused: |y_philox - y_supplied| = {diff:.3e} (bound {bound:.3e})")
        assert np.isfinite(ya).all() and (np.abs(ya - yb) <= bound).all()


@gpu
@case_param
def test_ddpm_prior_equals_the_reference_prior(case):
    """init_prior = 1 with in-kernel noise against the same launch (level 0) started from center_zero(float32(normals64(step =
    0xFFFFFFFF))) on supplied noise.  The two starting points differ by the centred-draw bound; level 0 passes that on amplified
    by A_0 and adds its own roundings (its noise is masked)."""
    items, N = _items(case), case.N
    e32, z64 = _e32(SEED, items, noise.PRIOR_STEP, N)
    x_ref = z64.astype(np.float32)
    x_ref = x_ref - x_ref.mean(1, keepdims=True, dtype=np.float32)
    z0 = noise.normals64(SEED, items, 0, N)
    with case.knobs() as nat:
        ya = _ddpm(nat, np.full((case.B, N, 3), 123.0, np.float32), 0, 0, None, case.offset, init_prior=True)   # (x is overwritten)
        name = case.check_launch(nat)
        yb = _ddpm(nat, x_ref, 0, 0, z0[None], case.offset)
        _, amp = _level_terms(nat, 0)
    ymax = max(np.abs(yb).max(), np.abs(x_ref).max())
    bound = amp * _centred_noise_bound(e32, N, np.abs(z64).max()) * 2 + _level_bound(0.0, 0.0, N, ymax)
    diff = np.abs(ya - yb).max()
    print(f"[noise] prior {case.id} {name}: |y_philox - y_reference| = {diff:.3e} (bound {bound:.3e}, E32 {e32:.3e})")
    assert np.isfinite(ya).all() and (np.abs(ya - yb) <= bound).all()


@gpu
@pytest.mark.parametrize("cid", ["chignolin-g1", "ala2-g3-4waves-ragged", "trp-cage-one", "trp-cage-pair"])
def test_two_shards_equal_one_call(cid):
    """Two halves of a batch as separate calls with offsets o and o + B / 2 == the one call, bit for bit: three Langevin steps
    with force_scale = 0 (the draws alone), and two reverse-DDPM levels through the network."""
    case = next(c for c in CASES if c.id == cid)
    B = case.B - case.B % 2
    p, _ = _langevin_params(case.N)
    x0 = _state(case, 5)[:B]
    v0 = (0.25 * synth.normal((B, case.N, 3), 20261, 6)).astype(np.float32)
    h = B // 2
    with case.knobs() as nat:
        x1, v1 = _run_langevin(nat, p, x0, v0, 3, SEED, case.offset, case.step_offset)
        xa, va = _run_langevin(nat, p, x0[:h].copy(), v0[:h].copy(), 3, SEED, case.offset, case.step_offset)
        xb, vb = _run_langevin(nat, p, x0[h:].copy(), v0[h:].copy(), 3, SEED, case.offset + h, case.step_offset)
        case.check_launch(nat)
        # (with the network in play the halves must be whole groups: a protein's rounding depends on its rows' place in the tile)
        g = max(case.group, 1)
        hd = g * max(1, h // g)
        xd = x0[:2 * hd]
        ya = _ddpm(nat, xd.copy(), 500, 499, None, case.offset)
        yh = np.concatenate([_ddpm(nat, xd[:hd].copy(), 500, 499, None, case.offset),
                             _ddpm(nat, xd[hd:].copy(), 500, 499, None, case.offset + hd)])
    assert np.array_equal(np.concatenate([va, vb]), v1) and np.array_equal(np.concatenate([xa, xb]), x1)
    assert np.array_equal(ya, yh)


@gpu
@pytest.mark.parametrize("model", ["chignolin", "trp_cage"])
def test_item_range_ends_at_two_to_the_forty(model):
    """(d) offset + count may reach 2^40 but not pass it: beyond, bits 40.. of the item would alias the bead field of counter
    word 1.  The refusal happens on the host, before anything is enqueued (state buffers untouched); the last admissible
    offset still draws what the reference draws."""
    import torch
    nat = get_native(model)
    N, B, lim = MODELS[model][0], 6, 1 << 40
    case = Case("edge", model, B, (), offset=lim - B)
    p, sig = _langevin_params(N)
    x, v0 = _state(case, 7), np.zeros((B, N, 3), np.float32)
    # accepted and correct
    _, v1 = _run_langevin(nat, p, x, v0, 1, SEED, lim - B, 5)
    e32, z64 = _e32(SEED, _items(case), 5, N)
    err = np.abs(v1.astype(np.float64) / (NOISESCALE * sig)[None, :, None] - z64)
    _report(f"(d) {model} offset 2^40 - {B}", err, z64, e32)
    assert (err <= M_DRAW * e32).all()
    ya = _ddpm(nat, x, 500, 500, None, lim - B)
    e32, z64 = _e32(SEED, _items(case), 500, N)
    yb = _ddpm(nat, x, 500, 500, z64[None], lim - B)
    sigma, _ = _level_terms(nat, 500)
    assert (np.abs(ya - yb) <= _level_bound(sigma, _centred_noise_bound(e32, N, np.abs(z64).max()), N, np.abs(yb).max())).all()
    # refused: one past, far past, and an offset whose sum wraps around 2^64
    xd, vd = torch.from_numpy(x).cuda(), torch.from_numpy(v0 + 0.5).cuda()
    for off in (lim - B + 1, lim, lim + 12345, 2 ** 64 - 1):
        with pytest.raises(ValueError, match=r"2\^40"):
            nat.langevin_run(p, xd, vd, 1, 1, seed=SEED, traj_offset=off, step_offset=0)
        with pytest.raises(ValueError, match=r"2\^40"):
            nat.ddpm_run(xd, 500, 500, seed=SEED, sample_offset=off)
        with pytest.raises(ValueError, match=r"2\^40"):
            nat.ddpm_run(xd, 0, 0, seed=SEED, sample_offset=off, init_prior=True)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(vd.cpu().numpy(), v0 + 0.5)
    # supplied noise does not use the offset: not refused
    nz = torch.zeros((1, B, N, 3), device="cuda")
    nat.ddpm_run(xd, 0, 0, noise=nz, seed=SEED, sample_offset=lim)
    torch.cuda.synchronize()
