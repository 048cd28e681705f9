"""The reverse-DDPM update -- centred eps, the x0 estimate sqrt_recip x - sqrt_recipm1 eps, its centring, the posterior mean
c1 x0 + c2 x, sigma_t times the centred noise (masked at level 0), the +-1000 clamp, the last centring, the schedule lookup and
the noise indexing -- against the float64 oracle twin (oracle/reference_twin.p_sample_loop on the same weights, inputs and noise)
on every kernel variant of variants.CASES.  The update lives in a branch of its own in each kernel (dff_small.hip: one register
column per thread with four masked 16-slot means; dff_kernels.hip: stage by stage with four bead_mean calls) that shares no code
with the other kernel or with the Langevin update.  The chain comparisons of test_gpu_parity.py (STEP_TOL x K relative to the
largest coordinate) see the model term only where a chain touches level 999 (that module's docstring has the numbers), and
test_noise_stream.py (c) compares the kernel with itself.  Here a lost tenth of eps misses the bars by a factor of 20 and more
-- and (a), a test of the reference alone, says so for every case before a kernel runs.

Set-up.  Full decoder scale (variants.MODELS); x0 ~ N(0, 1) seeded per (model, sample), centred in float32 (the ABI uses x as it
comes, the network centres its own input, the reference asserts a centred x); supplied noise unless stated; the case's `offset`
is the sample_offset; every launch gets a zeroed flag word and x_out is checked for finiteness.  The oracle runs on a subset of
the batch (variants.subset): first, last, both sides of every launch boundary and of the group boundary nearest the middle.

Level windows, chosen from the reference alone.  HIGH = 996 .. 991, six fused levels just below the top, where the step applies
eps with c1 sqrt_recipm1 = 0.58 .. 0.24 (ordinary levels: 3 - 6e-3): the intrinsic-input models, energy and force head.  LOW =
3 .. 0, every model; it ends on level 0, whose noise is masked.  The two `gen` models (absolute coordinates among the node
features, |eps| of about 2) run LOW only: at HIGH their float32 and float64 runs are 5e-4 to 3e-3 apart relative, so the
reference has no yardstick there (the reasoning test_langevin_update.py records for its RUN_OF); at LOW they are 1e-7 apart and
a tenth of eps is 23 / 175 bars.  For the other models a tenth of eps at LOW is 0.8 - 11 bars: printed by (a), not required.
LOW holds the state, the noise indexing, the schedule lookup and the level-0 mask; HIGH holds the model term.

Bars of (b) and (d), per window:  guard_for(kernel) x d32 + R,  absolute, on max |kernel - twin64| over the subset.
d32 = max |twin float32 - twin float64| on the same inputs: the reference's own float32 distance, as for the forces.
R allows for the float32 roundings of the update itself, which the kernel need not make where the twin's float32 run makes them,
counted from the step's operations and sized by the float64 oracle's own magnitudes at that step (the twin's `report`): E =
max |eps|, Z = max |noise| (0 at level 0), X0 = max |x0 estimate|, X = max |x| before the clamp, ymax = the largest |x| of the run
(inputs included).  A bead mean is N roundings (N - 1 additions, each on a partial sum whose share of the mean is at most the
largest term, and the division) and the subtraction one more.  With ae = c1 sqrt_recipm1 and sigma = exp(lv / 2), one step makes
  eps:    mean and subtraction, N + 1 roundings at E, carried into x by ae ......................... (N + 1) ae E
  noise:  mean and subtraction N + 1; expf within 2 ulp (lv / 2 is exact) and sigma x noise: 3 ...... (N + 4) sigma Z
  x0:     two products and a difference 3; mean and subtraction N + 1; c1 x x0 1; c2 x x 1 (at c2 ymax);
          their sum 1 (at most c1 X0 + c2 ymax) ................................................... (N + 6) c1 X0 + 2 c2 ymax
  + sigma noise: 1 at X ........................................................................... X
and then the last centring: a projection of norm <= 2 (test_noise_stream.py's factor) on everything above, plus its own N + 1
roundings at min(X, 1000).  So   r_t = EPS (2 [(N + 1) ae E + (N + 4) sigma Z + (N + 6) c1 X0 + 2 c2 ymax + X] + (N + 1) min(X, 1000)),
and a later level passes an earlier one's error on multiplied by A_t = c1 sqrt_recip + c2 = 1 / sqrt(alpha_t) (1.33 at level 996,
1.13 at 991, 1.00 at LOW, 31.6 at 999):  R = sum_k r_k prod_{j > k} A_j.  (What the network adds to A_t is ae |d eps / d x|, a few
per cent of it at HIGH for networks whose |eps| is 1e-2 of |x|; the reference's own float32 errors travel the same way inside
d32.)  R is a worst-case count, none of it fitted to the kernel: it comes to 0.6 - 5.6e-4 at HIGH (ymax 6.7 - 13: the state
grows by A_t per level) and 1.0e-5 - 1.2e-4 at LOW, about 30 - 200 x d32, and within a few per cent of the 2 K (N + 6) EPS ymax the
other two modules use (which puts every step at the window's ymax; this count sizes each step by its own magnitudes and carries
it on by A_t).  (a) holds at the windows above with this R; no window had to move.

(c) is the check on WHICH LEVEL THE NETWORK SEES from the second fused step on.  No comparison with the oracle can see that at
these windows (measured on the CPU at the bars above, GUARD_FP32): the float64 oracle with the network fed level t + 1 from the
second step on lies 0.16 - 0.71 bars from itself at HIGH and 0.01 - 0.03 at LOW on the intrinsic models, 0.11 / 0.23 at LOW on
trp-cage-gen / chignolin-gen (the time column of the node embedding is one input among N + 1, and a level is 1e-3 of it).
It is 20 and more float32 ulps of the largest coordinate at HIGH (1 - 10 at LOW), so a bit comparison of the fused loop with chained
single-level launches catches it.  The state crosses a launch
boundary as the very float32 values the fused loop keeps in LDS (x_io is written from xst and read back into it), and the step
the fused path of dff_small.hip adds -- `centre()` after the update, and on the layer-0 table the next level's LayerNorm rows
taken during stage E (`hoistA`) -- is the arithmetic a fresh launch does at its top: bit equality is asserted, no allowance.

MEASURED on the MI355X (worst err / bar over the 24 cases; every case prints its own):
  (b) test_update_follows_the_oracle: HIGH 0.023 (chignolin-g1, chignolin-4waves; 0.005 - 0.023 over the 22 cases), LOW 0.033
      (chignolin-force-head; 0.005 - 0.033 over the 24).  The error is the reference's own d32 to within a factor of 1.6.
  (c) test_fused_equals_chained: bit-identical on all 24 cases, both windows, supplied and in-kernel noise (92 comparisons).
  (d) test_clamp: 0.25 (chignolin-gen; trp-cage-gen 0.24: at |x| up to 60 their d32 is 5e-3 / 6e-2 and the kernel is inside
      it; 0.007 - 0.043 over the other 22); flag word 1, 0 at |x| <= 1, clamp_flag = NULL bit-identical, on every case.
  (e) test_update_invariants: |bead mean| 0.066 of (N + 1) EPS ymax (ala2-g3-3-launches); the split launches exact.
  (f): as stated.  Bit 1 of the flag word stayed clear in every run.  No case above 1: no defect found in either kernel's update.
  (a) on the CPU, (i) eps x 0.9: 41 (protein G) - 156 bars at HIGH on the energy models, 243 / 507 on the force heads, 175 / 23 at
      LOW on chignolin-gen / trp-cage-gen; (ii) >= 3500 at HIGH, >= 119 at LOW; (iii) >= 8600 at HIGH, >= 170 at LOW.
  Mutation check (scratch builds, each run once through (b) and (d)).  eps x 0.9 in the DDPM branch of dff_small.hip and of
  dff_kernels.hip (one build: a case runs one kernel or the other): all 24 cases of (b) fail -- the 11 of dff_small.hip at 99 -
  511 bars (HIGH; chignolin-gen 176 at LOW), the 13 of dff_kernels.hip at 41 - 242 (trp-cage-gen 23 at LOW) -- and all 24 of (d),
  at 84 - 2300 bars.  post_c2[t_int - 1] (clipped at 0) in both kernels: all 24 cases of (b) fail, at 2700 - 13700 bars (HIGH)
  and 19000 - 111000 (LOW), and all 24 of (d), at 111 - 5700.  For contrast, the 67 earlier tests that run a reverse step (the
  golden, odd-size and full-size chains, the input-branch, force-head and hidden-256 modules, test_noise_stream.py) under the
  first mutation: 9 fail, all of them chains of test_gpu_parity.py at default dispatch (the golden loop, the single steps, the
  odd bead counts, the full-size subset: a tenth of eps is about one of their bars); the other 58 -- every per-variant one
  among them -- pass.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_twin as twin
from oracle import synth
from support import EPS, GUARD_FP32, guard_for
from variants import CASES, MODELS, get_native, params, subset

gpu = pytest.mark.gpu
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])

T = 1000
HIGH, LOW, TOP = (996, 991), (3, 0), (999, 999)      # (t_start, t_end); TOP: the one step of (d)
KMAX = 6                  # noise rows 0 .. KMAX are made for every sample: a window uses its first K (the oracle's probe (iii) one more)
VISIBLE = 20.0            # (a): a probe must differ from the oracle by at least this many bars
SEED = (0x9E3779B9 << 32) | 0x2545F491
CLAMP_SCALES = (16.0, 17.0, 18.0, 19.0, 20.0, 22.0, 24.0)     # (d): the first that meets the conditions on the reference
CLAMP_MARGIN = 1e-4
SCHED = twin.make_schedule()


def _is_gen(model):
    return not MODELS[model][3][0]


def _windows(model):
    return (LOW,) if _is_gen(model) else (HIGH, LOW)


def _levels(win):
    return list(range(win[0], win[1] - 1, -1))


def _inputs(model, B):
    """x0 (B, N, 3) centred in float32, noises (KMAX + 1, B, N, 3), float32.  Sample b's numbers depend on (model, b) alone, not on
    B: cases of one model share their leading samples."""
    N, wseed = MODELS[model][0], MODELS[model][5]
    x0 = synth.normal((B, N, 3), wseed + 202, 1).astype(np.float32)
    x0 = x0 - x0.mean(1, keepdims=True, dtype=np.float32)
    nz = synth.normal((B, KMAX + 1, N, 3), wseed + 202, 2).transpose(1, 0, 2, 3)
    return x0, np.ascontiguousarray(nz, np.float32)


def _clamp_x0(model, B, scale):
    """(d): even samples times `scale` (they reach the clamp at level 999), odd samples times scale / 8 (they do not)."""
    x0, _ = _inputs(model, B)
    s = np.where(np.arange(B) % 2 == 0, scale, scale / 8.0).astype(np.float32)
    return x0 * s[:, None, None]


def _unit_x0(model, B):
    x0, _ = _inputs(model, B)
    return x0 / np.abs(x0).max()


_oracle_cache = {}


def _oracle(model, win, idx, dtype=torch.float64, probe=None, scale=None):
    """twin.p_sample_loop over the window on samples idx of the model's inputs (of _clamp_x0 at `scale`) -> (x_out (n, N, 3) as
    float64 numpy, the twin's report).  Cached: the tests of a case, and the cases of a model with the same subset, share a run."""
    key = (model, win, idx, dtype, tuple(sorted((probe or {}).items())), scale)
    if key not in _oracle_cache:
        N, H, L, flags, cons, _ = MODELS[model]
        x0, nz = _inputs(model, max(idx) + 1)
        if scale is not None:
            x0 = _clamp_x0(model, max(idx) + 1, scale)
        sel = list(idx)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        assert np.abs(x0[sel].astype(np.float64).mean(1)).max() < 1e-3     # (the reference's own entry check, ddpm.py:242)
        rep = {}
        out = twin.p_sample_loop(twin.to_torch(params(model), dtype), SCHED, t(x0[sel]), t(nz[:, sel]), win[0], L, T, t_end=win[1],
                                 conservative=cons, flags=tuple(bool(f) for f in flags), probe=probe, report=rep)
        rep["pre_clamp"] = [a.double().numpy() for a in rep["pre_clamp"]]
        rep["clamped"] = rep["clamped"].numpy()
        rep["x_in_max"] = float(np.abs(x0[sel]).max())
        _oracle_cache[key] = (out.double().numpy(), rep)
    return _oracle_cache[key]


def _allowance(N, win, rep):
    """R of the module docstring from the schedule and the float64 oracle's magnitudes -> (R, ymax)."""
    g = lambda name, t: float(SCHED[name][t])  # noqa: E731
    ymax = max([rep["x_in_max"]] + [float(np.abs(a).max()) for a in rep["pre_clamp"]])
    R = 0.0
    for k, t in enumerate(_levels(win)):
        c1, c2 = g("posterior_mean_coef1", t), g("posterior_mean_coef2", t)
        sr, srm1 = g("sqrt_recip_alphas_cumprod", t), g("sqrt_recipm1_alphas_cumprod", t)
        sig = 0.0 if t == 0 else float(np.exp(0.5 * g("posterior_log_variance_clipped", t)))
        E, Z, X0 = rep["eps_max"][k], rep["noise_max"][k], rep["x0_max"][k]
        X = float(np.abs(rep["pre_clamp"][k]).max())
        pre = (N + 1) * c1 * srm1 * E + (N + 4) * sig * Z + (N + 6) * c1 * X0 + 2 * c2 * ymax + X
        R = R * (c1 * sr + c2) + EPS * (2 * pre + (N + 1) * min(X, 1000.0))
    return R, ymax


def _bars(case, win, guard, scale=None):
    """-> (float64 oracle on the subset, its report, bar, (d32, R, ymax))"""
    idx = subset(case)
    ref, rep = _oracle(case.model, win, idx, scale=scale)
    r32, _ = _oracle(case.model, win, idx, torch.float32, scale=scale)
    d32 = np.abs(r32 - ref).max()
    R, ymax = _allowance(case.N, win, rep)
    return ref, rep, guard * d32 + R, (d32, R, ymax)


def _clamp_scale(case):
    """(d): the first of CLAMP_SCALES at which, in the float64 oracle on the subset, some samples clamp and others do not and no
    coordinate before the clamp lies within 1000 (1 +- CLAMP_MARGIN) -- a choice made from the reference alone."""
    for s in CLAMP_SCALES:
        _, rep = _oracle(case.model, TOP, subset(case), scale=s)
        v = np.abs(rep["pre_clamp"][0])
        if rep["clamped"].any() and not rep["clamped"].all() and (np.abs(v - 1000.0) > 1000.0 * CLAMP_MARGIN).all():
            return s
    raise AssertionError((case.id, "no scale of CLAMP_SCALES meets the conditions of (d)"))


# ------------------------------------------------------------------------------------------------ (a) CPU: the reference alone
@case_param
def test_probes_are_visible(case):
    """(a) A condition on the reference, no kernel: the float64 oracle with (i) the network output scaled by 0.9, (ii) every
    schedule table read at level t - 1, (iii) noise row k + 1 used at step k must each lie at least VISIBLE = 20 bars of (b) from
    the oracle itself, the bars taken at the larger guard (GUARD_FP32).  (i) is required at HIGH (LOW for the `gen` models) and
    only printed at LOW for the others: there a tenth of the model term is 1 - 4 bars (module docstring); LOW holds the state,
    the noise indexing, the schedule lookup and the level-0 mask, HIGH the model term.  (ii) and (iii) are required at every
    window.  Then the conditions of (d) on its inputs."""
    idx, ok = subset(case), True
    for win in _windows(case.model):
        ref, _, bar, (d32, R, ymax) = _bars(case, win, GUARD_FP32)
        eps_required = win == HIGH or _is_gen(case.model)
        for what, probe, required in (("(i) eps x 0.9", {"eps_factor": 0.9}, eps_required), ("(ii) schedule row t - 1", {"sched_shift": -1}, True),
                                      ("(iii) noise row k + 1", {"noise_shift": 1}, True)):
            d = np.abs(_oracle(case.model, win, idx, probe=probe)[0] - ref).max()
            print(f"[ddpm] (a) {case.id} t={win[0]}..{win[1]} {what}: {d:.3e} = {d / bar:.1f} bars ({bar:.3e}: d32 {d32:.3e}, R {R:.3e}, "
                  f"ymax {ymax:.2f}){'' if required else ' (not required)'}")
            ok = ok and (d >= VISIBLE * bar or not required)
    s = _clamp_scale(case)
    _, rep = _oracle(case.model, TOP, idx, scale=s)
    print(f"[ddpm] (a) {case.id} clamp scale {s}: samples {[i for i, c in zip(idx, rep['clamped']) if c]} of {idx} clamp, "
          f"largest coordinate before the clamp {np.abs(rep['pre_clamp'][0]).max():.0f}")
    assert ok


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_run(nat, case, win, x0=None, supplied=True, flag=True, first_row=0):
    """The window in one launch of binding.Model.ddpm_run on the case's batch (x0: the inputs of _inputs unless given), on noise
    rows first_row .. or on in-kernel noise -> (x_out numpy, flag word or None).  The flag word starts as 0."""
    K = win[0] - win[1] + 1
    xin, nz = _inputs(case.model, case.B)
    xd = torch.from_numpy(np.ascontiguousarray(xin if x0 is None else x0, np.float32)).cuda()
    nd = torch.from_numpy(nz[first_row:first_row + K]).cuda() if supplied else None
    fd = torch.zeros(1, dtype=torch.int32, device="cuda") if flag else None
    nat.ddpm_run(xd, win[0], win[1], noise=nd, seed=SEED, sample_offset=case.offset, clamp_flag=fd)
    torch.cuda.synchronize()
    out = xd.cpu().numpy()
    assert np.isfinite(out).all(), (case.id, win, "x_out is not finite")
    return out, None if fd is None else int(fd.item())


def _check_plan(nat, case):
    from dff_amd import binding
    plan = binding.plan_launch(nat.cfg, nat.dispatch(), 1, case.B)
    G = case.group if case.group else 1
    assert plan["G"] == G and plan["launches"] == -(-plan["workgroups"] // case.max_wgs), (case.id, plan)   # what subset() assumes


@gpu
@case_param
def test_update_follows_the_oracle(case):
    """(b) Each window of the case in one fused launch under the case's knobs, on supplied noise, against the float64 oracle on
    the subset.  Bars: module docstring.  err / bar is printed before anything is asserted; a ratio above 1 is a finding about
    the kernel, not about the bar.  The flag word stays 0."""
    got = {}
    with case.knobs() as nat:
        _check_plan(nat, case)
        for win in _windows(case.model):
            got[win] = _gpu_run(nat, case, win)
            name = case.check_launch(nat)
    sel, ok = list(subset(case)), True
    for win, (x, flag) in got.items():
        ref, _, bar, (d32, R, ymax) = _bars(case, win, guard_for(name))
        err = np.abs(x[sel] - ref).max()
        print(f"[ddpm] (b) {case.id} {name} t={win[0]}..{win[1]}: err {err:.3e} / bar {bar:.3e} = {err / bar:.3f} (d32 {d32:.3e}, R {R:.3e}, flag {flag})")
        ok = ok and err <= bar and flag == 0
    assert ok


@gpu
@case_param
def test_fused_equals_chained(case):
    """(c) The whole batch, every window: the K-level launch == K single-level launches from the same x0 with the matching noise
    rows, bit for bit, on supplied noise and on in-kernel noise (keyed by the level: the same draws).  The state crosses a launch
    boundary as the float32 values the fused loop keeps in LDS, and neither kernel's fused path makes an arithmetic step a fresh
    launch does not (module docstring).  This is the check on WHICH LEVEL THE NETWORK SEES from the second fused step on."""
    with case.knobs() as nat:
        for win in _windows(case.model):
            for supplied in (True, False):
                fused, flag = _gpu_run(nat, case, win, supplied=supplied)
                case.check_launch(nat)
                x, flags = None, []
                for k, t in enumerate(_levels(win)):
                    x, f = _gpu_run(nat, case, (t, t), x0=x, supplied=supplied, first_row=k)
                    flags.append(f)
                case.check_launch(nat)
                same = np.array_equal(x, fused)
                print(f"[ddpm] (c) {case.id} t={win[0]}..{win[1]} {'supplied' if supplied else 'in-kernel'} noise: "
                      f"{'bit-identical' if same else 'max |fused - chained| = %.3e' % np.abs(x - fused).max()}")
                assert same and flag == 0 and not any(flags)


@gpu
@case_param
def test_clamp(case):
    """(d) One step at level 999 (it multiplies x by 31.6) from the inputs of _clamp_x0 at the scale _clamp_scale chose on the
    reference: in the float64 oracle some samples of the subset clamp, others do not, and no coordinate before the clamp lies
    within 1000 (1 +- 1e-4).  x_out of the subset within the bars (taken on these inputs); the flag word exactly 1 (bit 1, a
    centre off by 1e-3, clear); the same inputs scaled to |x| <= 1 give flag word 0; clamp_flag = NULL gives the same x_out bit
    for bit."""
    s, idx = _clamp_scale(case), subset(case)
    x0 = _clamp_x0(case.model, case.B, s)
    with case.knobs() as nat:
        x, flag = _gpu_run(nat, case, TOP, x0=x0)
        name = case.check_launch(nat)
        x_null, none = _gpu_run(nat, case, TOP, x0=x0, flag=False)
        _, flag_unit = _gpu_run(nat, case, TOP, x0=_unit_x0(case.model, case.B))
        case.check_launch(nat)
    ref, rep, bar, (d32, R, ymax) = _bars(case, TOP, guard_for(name), scale=s)
    assert rep["clamped"].any() and not rep["clamped"].all(), (case.id, rep["clamped"])
    assert (np.abs(np.abs(rep["pre_clamp"][0]) - 1000.0) > 1000.0 * CLAMP_MARGIN).all()
    err = np.abs(x[list(idx)] - ref).max()
    print(f"[ddpm] (d) {case.id} {name} scale {s}: err {err:.3e} / bar {bar:.3e} = {err / bar:.3f} (d32 {d32:.3e}, R {R:.3e}, ymax {ymax:.0f}), "
          f"flag {flag}, at |x| <= 1 {flag_unit}")
    assert err <= bar
    assert flag == 1 and flag_unit == 0 and none is None
    assert np.array_equal(x_null, x)


@gpu
@case_param
def test_update_invariants(case):
    """(e) Every sample of the batch: |bead mean| of x_out at most (N + 1) EPS ymax (the N roundings of the kernel's float32 mean,
    each on a partial sum of at most N ymax, divided by N, and the one of the subtraction; ymax the largest |x| going in or
    coming out).  Cases whose last group is ragged: HIGH (LOW for a `gen` model) as two launches, its first half and its second,
    == the one launch bit for bit."""
    G = case.group if case.group else 1
    with case.knobs() as nat:
        outs = {win: _gpu_run(nat, case, win) for win in _windows(case.model)}
        case.check_launch(nat)
        win = _windows(case.model)[0]
        if case.B % G:
            m = (win[0] + win[1] + 1) // 2
            xa, fa = _gpu_run(nat, case, (win[0], m))
            xb, fb = _gpu_run(nat, case, (m - 1, win[1]), x0=xa, first_row=win[0] - m + 1)
            case.check_launch(nat)
    x0, _ = _inputs(case.model, case.B)
    for w, (x, flag) in outs.items():
        mean = np.abs(x.astype(np.float64).mean(1)).max()
        bar = (case.N + 1) * EPS * max(np.abs(x0).max(), np.abs(x).max())
        print(f"[ddpm] (e) {case.id} t={w[0]}..{w[1]}: largest |bead mean| {mean:.3e} / bar {bar:.3e} = {mean / bar:.3f}")
        assert mean <= bar and flag == 0
    if case.B % G:
        assert np.array_equal(xb, outs[win][0]) and fa == 0 and fb == 0


@gpu
def test_argument_contract():
    """(f) Refusals of dff_ddpm_run, made on the host before anything is enqueued (x and the flag word stay as they were):
    t_start >= T, t_end < 0, t_end > t_start, a negative batch.  A batch of 0 is accepted and does nothing."""
    nat = get_native("chignolin")
    N, B = MODELS["chignolin"][0], 3
    x0, nz = _inputs("chignolin", B)
    xd, nd = torch.from_numpy(x0).cuda(), torch.from_numpy(nz).cuda()
    fd = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t_start, t_end in ((T, T), (T + 5, T - 1), (3, -1), (-1, -1), (2, 3), (0, 1)):
        with pytest.raises(ValueError, match="bad timestep range"):
            nat.ddpm_run(xd, t_start, t_end, seed=SEED, clamp_flag=fd)
    raw = lambda b: nat.lib.dff_ddpm_run(nat.handle, b, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(nd.data_ptr()), 0, 0, 3, 3, 0,  # noqa: E731
                                         ctypes.c_void_p(fd.data_ptr()), nat._stream())
    assert raw(-1) == 1 and b"negative batch" in nat.lib.dff_last_error()       # DFF_EINVAL
    assert raw(-2 ** 31) == 1
    assert raw(0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x0) and int(fd.item()) == 0
    assert nat.status() == 0
