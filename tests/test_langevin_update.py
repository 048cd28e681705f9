"""The Langevin update WITH a live force -- v += dt f / m_i, the two half drifts, the friction and noise terms, the Brownian
x += f dtau + sqrt(2 dtau / beta) xi, the frame / kinetic-energy / noise indexing -- against the float64 oracle twin
(oracle/reference_twin.simulate on the same weights, inputs and noise) on every kernel variant of variants.CASES, under both
integrators.  The frames comparisons of test_gpu_parity.py (STEP_TOL x K relative to the largest coordinate) cannot see the
force: a step moves a bead by 1e-3 of its coordinate (that module's docstring has the numbers).  Here the velocities, the
kinetic energies and, under Brownian dynamics, the frames are held to bars a lost tenth of the force misses by a factor of 20
and more -- and (a), a test of the reference alone, says so for every case before a kernel runs.

Set-up.  Full decoder scale (variants.MODELS), per-bead masses 12 (1 + ((7 i) mod 5) / 8) = 12, 15, 18, 13.5, 16.5, ... (exact
in float32, no two neighbours equal), constants from twin.langevin_constants at norm 3.0, noise level 20, 340 K; K steps,
save_interval 2, supplied noise, a non-zero v0, un-centred x0.  The oracle runs on a subset of the batch (_subset): first, last,
both sides of every launch boundary and of the group boundary nearest the middle of the batch.

Bars of (b), per quantity q:  guard_for(kernel) x d32_q + R_q,  absolute, on max |kernel - twin64| over the subset.
d32_q = max |twin float32 - twin float64| of q on the same inputs: the reference's own float32 distance, as for the forces.
R_q allows for the roundings of the update itself, which the kernel need not make where the twin's float32 run makes them:
  v:   N_V EPS vmax per step, N_V = 10: the eight float32 operations of the velocity update (dxs force_scale, dt f, / m_i, v +,
       v vscale, noise_sigma_i xi, noisescale nz, v +), each on a value of at most vmax, one for the rounding of vscale to
       float32 (it multiplies vmax), and one for the five roundings of the other constants (force_scale, dt, noisescale, and
       the two of sqrtf(inv_beta / m_i)) together: they scale the kick and the noise term, under a tenth of vmax each.  The
       errors of earlier steps are carried on multiplied by vscale < 1: K steps add up to at most K times one step's.
  x:   2 K (N + 6) EPS xmax, the count test_noise_stream.py derives for a step of the same update (the bead mean: N roundings;
       subtracting it and the two drifts: five more operations and a spare; the centring is a projection of norm <= 2 that
       acts on the accumulated error once), plus the velocity allowance carried into x by the drifts, K dt R_v.  The Brownian
       step has N + 4 roundings at xmax (the mean, / N, the subtraction, two additions) and three at the size of its two
       increments, far under xmax: the same N + 6 covers it.
  ke:  (3 N + 2) EPS ke_max: 3 N products m_i v^2 summed, the square and the final halving.
vmax, xmax and ke_max are the largest |v|, |x|, ke of the float64 oracle over v0 / x0, the frames and the final state (the
velocities change by a few per cent over K steps: the end points stand for the path).

MEASURED on the MI355X (worst err / bar over the 24 cases; every case prints its own):
  (b) test_update_follows_the_oracle, BAOAB: v_out 0.062 (trp-cage-pair / -one; 0.036 - 0.062 over the cases), ke 0.20
      (ala2-g5-ragged), frames and x_out 0.024 (ala2-g2-8waves-ragged).  Brownian: frames and x_out 0.017 (chignolin-g1; 0.004 - 0.017 over the cases).
  (c) test_brownian_reads_out_every_draw: 0.125 (ala2-g3-4waves-ragged: 4.5e-7 against E32 = 5.3e-7); 3 + 4 steps == 7 bit for bit.
  (d) test_update_invariants: last ke against 0.5 sum m v^2 of v_out: 2.6e-7 relative (protein-g-one) where the bar is 1.0e-5.
  (e), (f): exact.  No case above 1: no defect found in the update of either kernel.
  Mutation check (scratch builds): force x 0.9 in the BAOAB update of dff_kernels.hip -> v_out of its 13 cases at 77 - 1040
  bars; mass_i read from bead 0 in dff_small.hip -> v_out of its 11 cases at 300 - 15000 bars, ke at 190 - 14600; f * a.dtau
  dropped from the Brownian branch of both kernels -> frames of all 24 cases at 430 - 11500 bars.
"""
import numpy as np
import pytest
import torch

from oracle import reference_twin as twin
from oracle import synth
from support import EPS, GUARD_FP32, M_DRAW, e32_of, guard_for
from variants import CASES, MODELS, get_native, params, subset as _subset

gpu = pytest.mark.gpu
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
integ_param = pytest.mark.parametrize("integ", ["baoab", "brownian"])

NORM, TLEV, TEMP, SAVE = 3.0, 20, 340.0, 2
N_V = 10                  # float32 roundings of one velocity update, each at most EPS vmax (module docstring)
VISIBLE = 20.0            # (a): a probe must differ from the oracle by at least this many bars
SEED = (0x9E3779B9 << 32) | 0x2545F491
# (K, dt) per integrator; dt None: the derived one of langevin_constants (7.2e-4 here).  Chosen so that (a) holds for every
# case -- a condition on the reference alone: at the derived dt a Brownian step moves a bead by f dtau = 1e-3 of its
# coordinate and a tenth of that is 7 (56 beads) to 35 (5 beads) bars; at dt = 4e-3 it is 40 and more.  The `gen` models
# (absolute coordinates among the node features) have forces 10 - 50 x larger: they keep the derived dt, where they are
# 220 / 1400 bars away -- at 4e-3 chignolin's Brownian trajectory runs away (|x| 2 -> 11 in six steps) and its float32 run
# is 1e-3 from its float64 one: no yardstick.
RUN = {"baoab": (6, None), "brownian": (6, 4e-3)}
RUN_OF = {("chignolin_gen", "brownian"): (6, None), ("trp_cage_gen", "brownian"): (6, None)}


def masses_of(N):
    return [12.0 * (1.0 + ((7 * i) % 5) / 8.0) for i in range(N)]


def _run_of(model, integ):
    return RUN_OF.get((model, integ), RUN[integ])


def _constants(model, integ):
    K, dt = _run_of(model, integ)
    return twin.langevin_constants(NORM, TLEV, twin.make_schedule(), TEMP, TEMP, masses_of(MODELS[model][0]),
                                   1.0 if integ == "baoab" else None, dt)


def _inputs(model, B, K):
    """x0 (B, N, 3) un-centred, v0 (B, N, 3), noises (K, B, N, 3), float32.  Trajectory b's numbers depend on (model, b, K) alone,
    not on B: cases of one model share their leading trajectories, and with them the oracle's runs."""
    N, wseed = MODELS[model][0], MODELS[model][5]
    x0 = synth.normal((B, N, 3), wseed + 101, 1) + 0.25 * synth.normal((B, 1, 3), wseed + 101, 2)
    v0 = 0.5 * synth.normal((B, N, 3), wseed + 101, 3)
    nz = synth.normal((B, K, N, 3), wseed + 101, 4).transpose(1, 0, 2, 3)
    return x0.astype(np.float32), v0.astype(np.float32), np.ascontiguousarray(nz, np.float32)


_oracle_cache = {}


def _oracle(model, integ, idx, dtype=torch.float64, force_factor=1.0, rotate=False):
    """twin.simulate on trajectories idx of the model's inputs -> (frames (n, K / SAVE, N, 3), ke (n, K / SAVE) or None, x, v or
    None) as float64 numpy.  Cached: the tests of a case, and the cases of a model with the same subset, share a run."""
    key = (model, integ, idx, dtype, force_factor, rotate)
    if key not in _oracle_cache:
        N, H, L, flags, cons, _ = MODELS[model]
        K, _ = _run_of(model, integ)
        x0, v0, nz = _inputs(model, max(idx) + 1, K)
        sel = list(idx)
        m = masses_of(N)
        if rotate:
            m = m[-1:] + m[:-1]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        fr, ke, x, v = twin.simulate(twin.to_torch(params(model), dtype), t(x0[sel]), t(nz[:, sel]), m, _constants(model, integ), L, SAVE,
                                     v0=t(v0[sel]), conservative=cons, flags=tuple(bool(f) for f in flags), force_factor=force_factor)
        n64 = lambda a: None if a is None else a.double().numpy()  # noqa: E731
        _oracle_cache[key] = tuple(n64(a) for a in (fr, ke, x, v))
    return _oracle_cache[key]


QUANTITIES = {"baoab": ("v_out", "ke", "frames", "x_out"), "brownian": ("frames", "x_out")}


def _as_dict(res):
    fr, ke, x, v = res
    return {"frames": fr, "ke": ke, "x_out": x, "v_out": v}


def _allowances(case, integ, ref):
    """R_q of the module docstring from the float64 oracle's magnitudes."""
    K, _ = _run_of(case.model, integ)
    c = _constants(case.model, integ)
    x0, v0, _ = _inputs(case.model, case.B, K)
    sel = list(_subset(case))
    xc = x0[sel].astype(np.float64)
    xmax = max(np.abs(xc - xc.mean(1, keepdims=True)).max(), np.abs(ref["frames"]).max(), np.abs(ref["x_out"]).max())
    rx = 2 * K * (case.N + 6) * EPS * xmax
    if integ == "brownian":
        return {"frames": rx, "x_out": rx}
    rv = N_V * K * EPS * max(np.abs(v0[sel]).max(), np.abs(ref["v_out"]).max())
    rx += K * c["dt"] * rv
    return {"v_out": rv, "ke": (3 * case.N + 2) * EPS * ref["ke"].max(), "frames": rx, "x_out": rx}


def _bars(case, integ, guard):
    idx = _subset(case)
    ref = _as_dict(_oracle(case.model, integ, idx))
    r32 = _as_dict(_oracle(case.model, integ, idx, torch.float32))
    R = _allowances(case, integ, ref)
    return ref, {q: guard * np.abs(r32[q] - ref[q]).max() + R[q] for q in QUANTITIES[integ]}


# ------------------------------------------------------------------------------------------------ (a) CPU: the reference alone
@case_param
@integ_param
def test_probes_are_visible(case, integ):
    """(a) A condition on the reference, no kernel: the float64 oracle with the force scaled by 0.9 and, under BAOAB, with the mass
    list rotated by one bead must each lie at least VISIBLE = 20 bars of (b) from the oracle itself -- force probe: v_out (BAOAB),
    frames (Brownian); mass probe: v_out and ke -- with the bars taken at the larger guard (GUARD_FP32).  So a kernel that loses a
    tenth of the force, or reads a neighbour's mass, cannot pass (b) on any case."""
    idx = _subset(case)
    ref, bars = _bars(case, integ, GUARD_FP32)
    probes = [("force x 0.9", _as_dict(_oracle(case.model, integ, idx, force_factor=0.9)), ("v_out",) if integ == "baoab" else ("frames",))]
    if integ == "baoab":
        probes.append(("masses rotated", _as_dict(_oracle(case.model, integ, idx, rotate=True)), ("v_out", "ke")))
    ok = True
    for what, res, qs in probes:
        for q in qs:
            d = np.abs(res[q] - ref[q]).max()
            print(f"[update] (a) {case.id} {integ} {what} -> {q}: {d:.3e} = {d / bars[q]:.0f} bars ({bars[q]:.3e})")
            ok = ok and d >= VISIBLE * bars[q]
    assert ok


# ------------------------------------------------------------------------------------------------ GPU
def _params_of(model, integ, c=None):
    from dff_amd import binding
    c = _constants(model, integ) if c is None else c
    p = binding.DffLangevinParams()
    p.t_norm, p.force_scale, p.dt, p.beta = c["t_norm"], 1.0 / (c["kbt_inv"] * c["sigma_t"]), c["dt"], c["beta"]
    if integ == "baoab":
        p.vscale, p.noisescale, p.overdamped, p.dtau = c["vscale"], c["noisescale"], 0, 0.0
    else:
        p.vscale, p.noisescale, p.overdamped, p.dtau = 0.0, 0.0, 1, c["dtau"]
    for i, m in enumerate(masses_of(MODELS[model][0])):
        p.masses[i] = m
    return p


def _gpu_run(nat, case, integ, frames=True, ke=True):
    """K steps of the case's batch through binding.Model.langevin_run on supplied noise -> dict of numpy arrays laid out as
    the oracle's (frames (B, K / SAVE, N, 3), ke (B, K / SAVE)).  The output buffers start as NaN: an entry the kernel does not
    write stays one."""
    K, _ = _run_of(case.model, integ)
    x0, v0, nz = _inputs(case.model, case.B, K)
    xd, nd = torch.from_numpy(x0).cuda(), torch.from_numpy(nz).cuda()
    vd = torch.from_numpy(v0).cuda() if integ == "baoab" else None
    fd = torch.full((K // SAVE, case.B, case.N, 3), float("nan"), device="cuda") if frames else None
    kd = torch.full((K // SAVE, case.B), float("nan"), device="cuda") if ke and integ == "baoab" else None
    nat.langevin_run(_params_of(case.model, integ), xd, vd, K, SAVE, noise=nd, seed=SEED, traj_offset=case.offset,
                     step_offset=case.step_offset, frames=fd, ke=kd)
    torch.cuda.synchronize()
    n = lambda a: None if a is None else a.cpu().numpy()  # noqa: E731
    return {"frames": None if fd is None else n(fd).transpose(1, 0, 2, 3), "ke": None if kd is None else n(kd).T, "x_out": n(xd), "v_out": n(vd)}


@gpu
@case_param
@integ_param
def test_update_follows_the_oracle(case, integ):
    """(b) K steps under the case's knobs against the float64 oracle on the subset: v_out, every ke frame, every frame and x_out
    (BAOAB); every frame and x_out (Brownian).  Bars: module docstring.  err / bar is printed per quantity before anything is
    asserted; a ratio above 1 is a finding about the kernel, not about the bar."""
    from dff_amd import binding
    with case.knobs() as nat:
        plan = binding.plan_launch(nat.cfg, nat.dispatch(), 1, case.B)
        got = _gpu_run(nat, case, integ)
        name = case.check_launch(nat)
    G = case.group if case.group else 1
    assert plan["G"] == G and plan["launches"] == -(-plan["workgroups"] // case.max_wgs), (case.id, plan)   # what _subset assumes
    ref, bars = _bars(case, integ, guard_for(name))
    sel, ok = list(_subset(case)), True
    for q in QUANTITIES[integ]:
        assert np.isfinite(got[q]).all(), (case.id, q, "not finite, or a frame the kernel did not write")
        err = np.abs(got[q][sel] - ref[q]).max()
        print(f"[update] (b) {case.id} {integ} {name} {q}: err {err:.3e} / bar {bars[q]:.3e} = {err / bars[q]:.3f}")
        ok = ok and err <= bars[q]
    assert ok


def _brownian_readout_params(N):
    from dff_amd import binding
    p = binding.DffLangevinParams()
    p.t_norm, p.force_scale, p.dt, p.vscale, p.noisescale, p.beta, p.dtau, p.overdamped = 0.02, 0.0, 0.5, 0.0, 0.0, 1.0, 0.5, 1
    for i, m in enumerate(masses_of(N)):
        p.masses[i] = m
    return p


def _brownian(nat, p, x, n_steps, offset, step_offset):
    xd = torch.from_numpy(x).cuda()
    nat.langevin_run(p, xd, None, n_steps, n_steps, seed=SEED, traj_offset=offset, step_offset=step_offset)
    torch.cuda.synchronize()
    return xd.cpu().numpy()


@gpu
@case_param
def test_brownian_reads_out_every_draw(case):
    """(c) The Brownian branch on in-kernel noise: overdamped = 1, v_dev = NULL, noise_dev = NULL, force_scale = 0, dtau = 0.5,
    beta = 1, so brown_sigma = sqrt(2 dtau / beta) = 1 exactly and one step gives x_out = centre(x_0) + xi.  With the centring
    redone in float64 on the host, x_out - centre(x_0) is the draw up to the N + 1 roundings of the kernel's centring and the one
    of the addition: every draw of the batch within M_DRAW E32 + (N + 2) EPS xmax of noise.normals64 at the case's offset and
    step_offset.  Then 7 steps in one launch == 3 + 4 steps with step_offset advanced, bit for bit in x."""
    p = _brownian_readout_params(case.N)
    x0, _, _ = _inputs(case.model, case.B, 1)
    with case.knobs() as nat:
        x1 = _brownian(nat, p, x0, 1, case.offset, case.step_offset)
        name = case.check_launch(nat)
        x7 = _brownian(nat, p, x0, 7, case.offset, case.step_offset)
        xa = _brownian(nat, p, x0, 3, case.offset, case.step_offset)
        xb = _brownian(nat, p, xa, 4, case.offset, case.step_offset + 3)
        case.check_launch(nat)
    items = np.arange(case.B, dtype=np.uint64) + np.uint64(case.offset)
    e32, z64 = e32_of(SEED, items, case.step_offset, case.N)
    xc = x0.astype(np.float64)
    xc -= xc.mean(1, keepdims=True)
    assert np.isfinite(x1).all() and np.isfinite(x7).all()
    err = np.abs(x1.astype(np.float64) - xc - z64)
    bar = M_DRAW * e32 + (case.N + 2) * EPS * max(np.abs(xc).max(), np.abs(x1).max())
    print(f"[update] (c) {case.id} {name}: max |draw - normals64| = {err.max():.3e} / bar {bar:.3e} = {err.max() / bar:.3f} "
          f"over {err.size} draws (E32 {e32:.3e})")
    assert (err <= bar).all()
    assert np.array_equal(xb, x7)


@gpu
@case_param
@integ_param
def test_update_invariants(case, integ):
    """(d) Every trajectory of the batch, exact unless stated: K is a multiple of save_interval, so the last saved frame IS
    x_out; the last ke frame is 0.5 sum m_i v_i^2 of v_out (float64 on the host) within (3 N + 2) EPS ke; frames_dev = NULL,
    ke_dev = NULL and both NULL leave x_out and v_out bit for bit what they are with both buffers."""
    with case.knobs() as nat:
        full = _gpu_run(nat, case, integ)
        case.check_launch(nat)
        others = [_gpu_run(nat, case, integ, frames=False)]
        if integ == "baoab":
            others += [_gpu_run(nat, case, integ, ke=False), _gpu_run(nat, case, integ, frames=False, ke=False)]
        case.check_launch(nat)
    assert np.isfinite(full["frames"]).all() and np.isfinite(full["x_out"]).all()
    assert np.array_equal(full["frames"][:, -1], full["x_out"])
    for o in others:
        assert np.array_equal(o["x_out"], full["x_out"])
        if integ == "baoab":
            assert np.array_equal(o["v_out"], full["v_out"])
    if integ == "baoab":
        assert np.isfinite(full["ke"]).all() and others[1]["ke"] is None and np.array_equal(others[0]["ke"], full["ke"])
        m = np.array(masses_of(case.N))
        ke = 0.5 * (m[None, :, None] * full["v_out"].astype(np.float64) ** 2).sum((1, 2))
        err = np.abs(full["ke"][:, -1] - ke) / ke
        print(f"[update] (d) {case.id}: ke worst relative error {err.max():.3e} / bar {(3 * case.N + 2) * EPS:.3e}")
        assert (err <= (3 * case.N + 2) * EPS).all()


@gpu
def test_argument_contract():
    """(e) Refusals of dff_langevin_run, made on the host before anything is enqueued (the state buffers stay as they were):
    v_dev = NULL or a mass <= 0 with overdamped = 0; n_steps no multiple of save_interval with frames requested.  The first two
    are accepted with overdamped = 1, where neither is read."""
    nat = get_native("chignolin")
    N, B = 10, 3
    x0, v0, nz = _inputs("chignolin", B, 3)
    xd, vd, nd = torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda(), torch.from_numpy(nz).cuda()
    frames = torch.zeros((1, B, N, 3), device="cuda")
    for bad in (0.0, -12.0, float("nan")):
        p = _params_of("chignolin", "baoab")
        p.masses[N - 1] = bad
        with pytest.raises(ValueError, match="masses must be positive"):
            nat.langevin_run(p, xd, vd, 1, 1, noise=nd[:1])
    with pytest.raises(ValueError, match="v_dev required"):
        nat.langevin_run(_params_of("chignolin", "baoab"), xd, None, 1, 1, noise=nd[:1])
    for integ in ("baoab", "brownian"):
        with pytest.raises(ValueError, match="save_interval must be a factor"):
            nat.langevin_run(_params_of("chignolin", integ), xd, vd if integ == "baoab" else None, 3, 2, noise=nd, frames=frames)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x0) and np.array_equal(vd.cpu().numpy(), v0) and not frames.any()
    # accepted under Brownian dynamics, and the bad mass changes nothing there
    p = _params_of("chignolin", "brownian")
    nat.langevin_run(p, xd, None, 1, 1, noise=nd[:1])
    p.masses[N - 1] = 0.0
    x2 = torch.from_numpy(x0).cuda()
    nat.langevin_run(p, x2, None, 1, 1, noise=nd[:1])
    torch.cuda.synchronize()
    assert torch.isfinite(xd).all() and torch.equal(xd, x2) and not np.array_equal(xd.cpu().numpy(), x0)
    assert nat.status() == 0


@gpu
@pytest.mark.parametrize("friction", [1.0, None])
def test_sampler_class_passes_the_oracle_constants(friction):
    """(f) LangevinDiffusion(...).sample(noises=...) with the per-bead masses (chignolin) == the direct binding call with the
    scalars of twin.langevin_constants, bit for bit: dt derived from masses[0], dtau = dt / masses[0] when friction is None."""
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.langevin import LangevinDiffusion
    from dff_amd.score import GraphTransformer
    model, integ = "chignolin", "baoab" if friction is not None else "brownian"
    N, H, L, _, _, _ = MODELS[model]
    K, B = 6, 5
    gt = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False, use_distances=False,
                          conservative=True, state_dict=params(model))
    diff = GaussianDiffusion(gt, num_atoms=N, timesteps=1000, norm_factor=NORM)
    x0, _, nz = _inputs(model, B, K)
    init = torch.from_numpy(x0) * NORM
    ld = LangevinDiffusion(diff, init, K, save_interval=SAVE, t=TLEV, diffusion_steps=1000, temp_data=TEMP, temp_sim=TEMP, dt=None,
                           masses=masses_of(N), friction=friction, kb="consistent", verbose=False)
    traj = ld.sample(noises=torch.from_numpy(nz))
    c = twin.langevin_constants(NORM, TLEV, twin.make_schedule(), TEMP, TEMP, masses_of(N), friction, None)
    assert c["dt"] == ld.dt and (friction is not None or c["dtau"] == c["dt"] / masses_of(N)[0])
    xd = (init / NORM).cuda().contiguous()
    vd = torch.zeros_like(xd) if friction is not None else None
    fd = torch.full((K // SAVE, B, N, 3), float("nan"), device="cuda")
    kd = torch.full((K // SAVE, B), float("nan"), device="cuda") if friction is not None else None
    gt.native.langevin_run(_params_of(model, integ, c), xd, vd, K, SAVE, noise=torch.from_numpy(nz).cuda(), frames=fd, ke=kd)
    torch.cuda.synchronize()
    want = fd.permute(1, 0, 2, 3).cpu().reshape(-1, N, 3) * NORM
    assert torch.isfinite(want).all() and torch.equal(traj, want) and torch.equal(ld.x, xd)
    if friction is not None:
        assert torch.equal(ld.v, vd) and np.array_equal(ld.kinetic_energies, kd.permute(1, 0).cpu().numpy())
    else:
        assert ld.kinetic_energies is None
