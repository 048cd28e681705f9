"""The two-piece fp16 split engine (split_f16 kernels) against operands chosen to hurt it, and against the fp32-MFMA
engine as a sampler.  `-m gpu`; every call goes through the C ABI.

An fp32 operand of a weight GEMM is carried as h + l'/2048 (two fp16 pieces rounded to nearest: 2^-22 per operand where
fp32 is exact) and a product keeps three of the four piece products.  On i.i.d. operands the piece roundings cancel along
a dot product (tests/test_gpu_parity.py, tests/fuzz_shapes.py: synthetic uniform weights).  Here:

* `test_fp16_engine_on_structured_operands`: weights on a bf16 grid, on an int8-dequantised grid, with same-sign
  residuals (w = fp16(w) (1 + 2^-12): every low piece has the sign of its high piece), LayerNorm rows with one entry of
  1e2 among entries of 1e-3 (the pieces are cut of the activations "as they are": 2^-35 absolute), energy heads of 1e-6
  and 1e4, and coordinates at the +-1000 clamp of models/ddpm.py:248-250 -- both engines against the twin in float64 at
  the bars of tests/test_gpu_parity.py, on the six shipped architectures and a hidden-128 model at 16 rows.  The
  low-magnitude structures (every GEMM weight of the blocks x 1e-5 / 1e-6, one matrix x 1e-6 per kind, LayerNorm gains and
  biases of 1e-5, coordinates of 1e-4 sigma) sit where a piece's 2^-36 absolute floor, not its 2^-22 relative step, decides:
  before the low-end guard of dff_model_create the split engine's forces on the decayed model were 0.9 - 1.0 from float64
  and the folded q' = W_k^T W_q of a tiny W_kv was 2.7e-4 off relative to itself
  (`test_stash_intermediates_relative_on_low_magnitude_models`).  Those models now run the fp32 engine
  (`test_fp16_engine_steps_aside_for_models_below_its_range`); x_tiny cannot be bounded on the host and keeps the split
  engine: measured 0.7 - 1.8e-6 from float64 where the reference's own float32 run is 1.1 - 2.8e-6.
* `test_engines_agree_statistically`: 20 000 Langevin steps x 256 trajectories with the in-kernel Philox noise on either
  engine; the pairwise-distance histograms of the two ensembles (the library's own dff_pwd_hist) are no
  further apart -- Jensen-Shannon, evaluate/evaluators.py:251-270 -- than two seeds of ONE engine, and both thermostats
  hold equipartition (dynamics/langevin_cgnet.py:538-542).
* `test_engines_agree_statistically_iid`: the same comparison for the other sampler of the hot path -- reverse-DDPM chains
  (models/ddpm.py:195-254) over the last 300 noise levels, 4096 chains per engine and seed.
"""
import numpy as np
import pytest
import torch

from oracle import reference_twin as twin
from oracle import synth
from support import GUARD, GUARD_FP32, rel

pytestmark = pytest.mark.gpu

NORM_STD = {"chignolin": 3.113133430480957, "villin": 6.082900047302246}
TEMP = {"chignolin": 340, "villin": 360}


@pytest.fixture(scope="module")
def dff():
    import dff_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dff_amd.load_library()
    return dff_amd


def bf16_grid(w):
    """float32 -> nearest bfloat16 (ties to even), as float32"""
    u = w.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# one matrix kind of the low-magnitude structures: state-dict key suffix (scaled in layer 1 only)
ONE_MATRIX = {"W_q": "0.0.fn.to_q.weight", "W_kv": "0.0.fn.to_kv.weight", "W_o": "0.0.fn.to_out.weight",
              "W1": "1.0.fn.0.weight", "W2": "1.0.fn.2.weight"}


def structured(params, kind):
    """The synthetic state dict with its Linear weights / LayerNorm affine parameters moved onto a structure."""
    out, ln = {}, 0
    for k, v in params.items():
        v = v.copy()
        linear = v.ndim == 2 and "proj" not in k          # (the gates' 1 x 3H projections are row-stage VALU work, not GEMMs)
        if kind.startswith("all_linear_"):                # the uniformly decayed model: every GEMM weight of the blocks x s, the
            s = float(kind[len("all_linear_"):])          # energy head x 1/s (the embeddings are folded on the host, not GEMMs:
            if k == "node_decoder.weight":                # scaling them too leaves forces of 1e-21 the float32 reference cannot
                v = (v / s).astype(np.float32)            # resolve at all)
            elif linear and k.startswith("graphtransformer."):
                v = (v * s).astype(np.float32)
        elif kind.startswith("one_matrix_"):              # one_matrix_1e-6[W_o]: exactly one tiny matrix (layer 1's)
            s, which = kind[len("one_matrix_"):-1].split("[")
            if k == "graphtransformer.layers.1." + ONE_MATRIX[which]:
                v = (v * float(s)).astype(np.float32)
        elif kind == "ln_gain_tiny" and (k.endswith("norm.weight") or k.endswith("norm.bias")):
            v = (v * 1e-5).astype(np.float32)             # every LayerNorm row (a forward GEMM input) is O(1e-5)
        elif kind == "bf16_grid" and linear:
            v = bf16_grid(v)
        elif kind == "int8_grid" and linear:              # symmetric per-tensor int8, dequantised
            s = np.abs(v).max() / 127.0
            v = (np.round(v / s) * s).astype(np.float32)
        elif kind == "same_sign_residual" and linear:     # h (1 + 2^-12): exact in fp32; w - fp16(w) has the sign of w everywhere
            h = v.astype(np.float16).astype(np.float32)
            v = (h * np.float32(1.0 + 2.0 ** -12)).astype(np.float32)
        elif kind == "ln_outlier" and k.endswith("norm.weight"):
            g = np.full_like(v, 1e-3)
            g[1::2] *= -1
            g[(7 * ln + 3) % v.size] = 100.0              # (1e3 would put sqrt(H) |gain| |W1 row|_1 past the engine's range guard:
            ln += 1                                       #  test_fp16_engine_steps_aside_for_models_out_of_its_range covers that side)
            v = g
        elif kind == "ln_outlier" and k.endswith("norm.bias"):
            v = (v * 1e-2).astype(np.float32)
        out[k] = v
    return out


STRUCTURES = ["bf16_grid", "int8_grid", "same_sign_residual", "ln_outlier", "decoder_1e-6", "decoder_1e4", "x_at_clamp"]
# uniformly small operands: a fp16 piece resolves 2^-36 absolutely (its subnormal spacing, / 2^11), so below ~2^-14 the split's
# error stops being relative (a decayed / pruned checkpoint; LayerNorm's eps = 1e-5 does not rescue rows of variance << 1e-5)
LOW_MAGNITUDE = (["all_linear_1e-5", "all_linear_1e-6"] + [f"one_matrix_1e-6[{w}]" for w in ONE_MATRIX]
                 + ["ln_gain_tiny", "x_tiny"])
# the ill-conditioned structures are held to the relative bar only: logits of 1e2 .. 1e3 (ln_outlier, x_at_clamp: the
# reference's own float32 run is 1e-5 .. 2e-3 from its float64 one), and the decayed model (forces of 1e-11 .. 1e-12 out of
# bias-dominated values: the softmax gradient cancels, and the reference's float32 run is 5e-5 .. 1e-4 from its float64 one)
ILL_CONDITIONED = ("ln_outlier", "x_at_clamp", "all_linear_1e-5", "all_linear_1e-6")
# ... those the library gives to the fp32 engine at dff_model_create (a weight matrix or a LayerNorm row bound below 2^-12:
# test_fp16_engine_steps_aside_for_models_below_its_range); x_tiny cannot be bounded on the host and keeps the split engine
BELOW_RANGE = set(LOW_MAGNITUDE) - {"x_tiny"}
# the six shipped architectures and a hidden-128 model at <= 16 rows (the generic kernel's split variants, not the <= 16-row
# kernel's: hidden 96 / 128 have none there)
ARCHS = dict(synth.SHIPPED_CONFIGS, h128_n16=("-", 16, 128, 3))


def structured_case(cfg, kind):
    """(params, x, t, L) of one structured-operand case"""
    _, N, H, L = ARCHS[cfg]
    dec = {"decoder_1e-6": 1e-6, "decoder_1e4": 1e4}.get(kind, 1e-2)
    params = structured(synth.synth_gnn_params(N, H, L, seed=777, decoder_scale=dec), kind)
    x = synth.normal((5, N, 3), 21, 3)
    if kind == "x_at_clamp":                               # every coordinate on the clamp; one sample spread inside it
        x = np.sign(x) * 1000.0
        x[0] = np.clip(synth.normal((N, 3), 22, 3) * 300.0, -1000.0, 1000.0)
    if kind == "x_tiny":                                   # coordinates of 1e-4 sigma: every relative position is tiny
        x = x * 1e-4
    x = (x - x.mean(1, keepdims=True)).astype(np.float32)
    t = np.array([0.0, 0.02, 0.3, 0.7, 0.999], np.float32)
    return params, x, t, L


def twin_forces(params, x, t, L):
    f32ref = twin.score(twin.to_torch(params), torch.from_numpy(x), torch.from_numpy(t), L).numpy()
    f64 = twin.score(twin.to_torch(params, torch.float64), torch.from_numpy(x).double(), torch.from_numpy(t).double(), L).numpy()
    return f32ref, f64


@pytest.mark.parametrize("cfg", list(ARCHS))
@pytest.mark.parametrize("kind", STRUCTURES + LOW_MAGNITUDE)
def test_fp16_engine_on_structured_operands(dff, cfg, kind, monkeypatch):
    from dff_amd.score import GraphTransformer
    _, N, H, L = ARCHS[cfg]
    params, x, t, L = structured_case(cfg, kind)
    f32ref, f64 = twin_forces(params, x, t, L)
    r32 = rel(f32ref, f64)
    absbar = 5e-6 if kind not in ILL_CONDITIONED else np.inf
    got, knames = {}, {}
    for split in (True, False):
        monkeypatch.setenv("DFF_SPLIT_BF16", "1" if split else "0")
        model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                                 use_distances=False, conservative=True, state_dict=params)
        f = model.native.score(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).cpu().numpy()
        knames[split] = model.native.last_launch()[0]
        assert np.isfinite(f).all() and model.native.status() == 0
        got[split] = rel(f, f64)
    print(f"{cfg} {kind}: rel(split_f16, f64)={got[True]:.3e} rel(fp32 MFMA, f64)={got[False]:.3e} rel(ref32, ref64)={r32:.3e} "
          f"|F|max={np.abs(f64).max():.3e} kernels={knames[True]} | {knames[False]}")
    assert got[True] <= absbar and got[True] <= GUARD * max(r32, 4e-7)
    assert got[False] <= absbar and got[False] <= GUARD_FP32 * max(r32, 4e-7)
    assert ("split_f16" in knames[True]) == (kind not in BELOW_RANGE), knames[True]
    assert "split_" not in knames[False], knames[False]


# every kernel family with a split variant, and how to select it: (architecture, DFF_FOLD_KV, dff_debug_force_generic, kernel
# name of the split engine must contain, ... must not contain)
SPLIT_FAMILIES = {
    "fold_le16": ("chignolin", "1", False, ("dff_small_kernel<", "split_f16", "fold_kv"), ()),
    "unfolded_le16": ("chignolin", "0", False, ("dff_small_kernel<", "split_f16"), ("fold_kv",)),
    "le64": ("chignolin", "1", True, ("dff_fused_kernel<64,", "split_f16"), ("pair",)),
    "generic_h128": ("h128_n16", "1", False, ("dff_fused_kernel<128,", "split_f16"), ()),
    "pair": ("protein_g", "1", False, ("dff_fused_kernel<128,", "split_f16", "pair"), ()),
}


@pytest.mark.parametrize("family", list(SPLIT_FAMILIES))
@pytest.mark.parametrize("kind", ["x_tiny", "all_linear_1e-6", "one_matrix_1e-6[W_o]", "ln_gain_tiny"])
def test_fp16_engine_low_magnitude_on_every_split_family(dff, family, kind, monkeypatch):
    """The low-magnitude structures on every kernel family that has a split variant (the <= 16-row kernel folded and unfolded,
    the <= 64-row kernel, the generic hidden-128 variant, two workgroups per protein).  The synthetic model itself runs the
    split variant of the family (asserted from last_launch()); a low-magnitude model runs it too, or -- below the engine's range --
    the fp32 engine; either way at the bars of test_fp16_engine_on_structured_operands."""
    from dff_amd.score import GraphTransformer
    cfg, fold, generic, has, hasnt = SPLIT_FAMILIES[family]
    _, N, H, L = ARCHS[cfg]
    monkeypatch.setenv("DFF_FOLD_KV", fold)
    monkeypatch.setenv("DFF_SPLIT_BF16", "1")
    params, x, t, L = structured_case(cfg, kind)
    f32ref, f64 = twin_forces(params, x, t, L)
    r32 = rel(f32ref, f64)
    names = {}
    for what, p in (("synthetic", synth.synth_gnn_params(N, H, L, seed=777, decoder_scale=1e-2)), (kind, params)):
        model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                                 use_distances=False, conservative=True, state_dict=p)
        model.native.force_generic(generic)
        f = model.native.score(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).cpu().numpy()
        names[what] = model.native.last_launch()[0]
        assert np.isfinite(f).all() and model.native.status() == 0
    err = rel(f, f64)
    print(f"{family} {kind}: rel({names[kind]}, f64)={err:.3e} rel(ref32, ref64)={r32:.3e} (synthetic model: {names['synthetic']})")
    assert all(h in names["synthetic"] for h in has) and not any(h in names["synthetic"] for h in hasnt), names
    if kind in BELOW_RANGE:
        assert "split_" not in names[kind], names
    else:
        assert all(h in names[kind] for h in has) and not any(h in names[kind] for h in hasnt), names
    assert err <= (5e-6 if kind not in ILL_CONDITIONED else np.inf)
    assert err <= (GUARD if "split_f16" in names[kind] else GUARD_FP32) * max(r32, 4e-7)


@pytest.mark.parametrize("cfg,steps", [("chignolin", 20000), ("villin", 20000)])
def test_engines_agree_statistically(dff, cfg, steps, monkeypatch, tmp_path):
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.evaluate import PwdEvaluator
    from dff_amd.langevin import LangevinDiffusion
    from dff_amd.score import GraphTransformer
    _, N, H, L = synth.SHIPPED_CONFIGS[cfg]
    P, save, burn = 256, 250, 20
    params = synth.synth_gnn_params(N, H, L, decoder_scale=1e-2)
    init = torch.from_numpy(synth.normal((P, N, 3), 11, 4).astype(np.float32)) * NORM_STD[cfg]
    init = init - init.mean(1, keepdim=True)
    c = twin.langevin_constants(NORM_STD[cfg], 20, twin.make_schedule(), TEMP[cfg], TEMP[cfg], [12.0] * N, 1.0, None)
    expect_ke = 1.5 * N / c["beta"]
    runs = {}
    for split, seed in ((True, 101), (True, 202), (False, 101), (False, 202)):
        monkeypatch.setenv("DFF_SPLIT_BF16", "1" if split else "0")
        model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                                 use_distances=False, conservative=True, state_dict=params)
        diff = GaussianDiffusion(model, num_atoms=N, timesteps=1000, norm_factor=NORM_STD[cfg])
        ld = LangevinDiffusion(diff, init, n_timesteps=steps, save_interval=save, t=20, temp_data=TEMP[cfg], temp_sim=TEMP[cfg],
                               dt=None, masses=[12.0] * N, friction=1.0, verbose=False, seed=seed)
        traj = ld.sample()
        kname = model.native.last_launch()[0]
        assert ("split_f16" in kname) == split, kname
        nf = steps // save
        assert traj.shape == (P * nf, N, 3) and torch.isfinite(traj).all() and model.native.status() == 0
        ke = np.asarray(ld.kinetic_energies)                  # (P, nf)
        late = ke[:, burn:]
        # equipartition of the BAOAB thermostat: <KE> = 3 N / (2 beta) whatever the forces are (P x 60 frames: +-0.4 % at 1 sigma)
        assert abs(late.mean() / expect_ke - 1.0) < 0.03, (split, seed, late.mean(), expect_ke)
        runs[(split, seed)] = (traj.reshape(P, nf, N, 3)[:, burn:].reshape(-1, N, 3).contiguous(), late.mean() / expect_ke)
    js = {}
    for a, b in (((True, 101), (True, 202)), ((False, 101), (False, 202)), ((True, 101), (False, 101)), ((True, 202), (False, 202)),
                 ((True, 101), (False, 202))):
        ev = PwdEvaluator(runs[a][0], mol_name=cfg, offset=3, saved_ref=str(tmp_path / f"ref_{a[0]}_{a[1]}.pickle"))
        js[(a, b)] = float(ev.eval(runs[b][0]))
    same = [js[((True, 101), (True, 202))], js[((False, 101), (False, 202))]]
    cross = [js[((True, 101), (False, 101))], js[((True, 202), (False, 202))], js[((True, 101), (False, 202))]]
    print(f"{cfg}: JS(two seeds, split_f16)={same[0]:.3e} JS(two seeds, fp32 MFMA)={same[1]:.3e} JS(split_f16 vs fp32 MFMA)="
          + " ".join(f"{v:.3e}" for v in cross) + " KE/expected=" + " ".join(f"{runs[k][1]:.4f}" for k in runs))
    # two engines are two samples of one ensemble: no further apart than two seeds of one engine (each JS is an estimate from
    # 256 x 60 correlated frames: a quarter of slack)
    assert max(cross) <= 1.25 * max(same), (cross, same)


@pytest.mark.parametrize("cfg", ["chignolin", "villin"])
def test_engines_agree_statistically_iid(dff, cfg, monkeypatch, tmp_path):
    """The reverse-DDPM sampler (models/ddpm.py:195-254, in-kernel Philox noise) on either engine: 4096 chains per run over the last
    300 noise levels (a random-weight network is no denoiser: from t = T its chains run into the +-1000 clamp, from t = 300 they stay
    O(1)); the pairwise-distance histograms are no further apart between the engines than between two seeds of one."""
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.evaluate import PwdEvaluator
    from dff_amd.score import GraphTransformer
    _, N, H, L = synth.SHIPPED_CONFIGS[cfg]
    B, rounds, t0 = 256, 16, 300
    params = synth.synth_gnn_params(N, H, L, decoder_scale=1e-2)
    inits = []
    for r in range(rounds):
        x = torch.from_numpy(synth.normal((B, N, 3), 300 + r, 5).astype(np.float32))
        inits.append(x - x.mean(1, keepdim=True))
    runs = {}
    for split, seed in ((True, 11), (True, 22), (False, 11), (False, 22)):
        monkeypatch.setenv("DFF_SPLIT_BF16", "1" if split else "0")
        model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                                 use_distances=False, conservative=True, state_dict=params)
        diff = GaussianDiffusion(model, num_atoms=N, timesteps=1000, norm_factor=NORM_STD[cfg])
        outs = []
        for r in range(rounds):
            diff.seed(1000 * seed + r)
            outs.append(diff.p_sample_loop_from(inits[r], t0, 0).cpu() * NORM_STD[cfg])
        out = torch.cat(outs)
        kname = model.native.last_launch()[0]
        assert ("split_f16" in kname) == split, kname
        assert out.shape == (B * rounds, N, 3) and torch.isfinite(out).all() and model.native.status() == 0
        assert float(out.abs().max()) < 50.0 * NORM_STD[cfg] and not diff.last_clamped
        assert float(out.mean(1).abs().max()) < 1e-3 * NORM_STD[cfg]          # centred chains (models/ddpm.py:251-252)
        runs[(split, seed)] = out.contiguous()
    assert not torch.equal(runs[(True, 11)], runs[(True, 22)])                 # (the seed reaches the kernel's Philox key)
    js = {}
    for a, b in (((True, 11), (True, 22)), ((False, 11), (False, 22)), ((True, 11), (False, 11)), ((True, 22), (False, 22)),
                 ((True, 11), (False, 22))):
        ev = PwdEvaluator(runs[a], mol_name=cfg, offset=3, saved_ref=str(tmp_path / f"iid_ref_{a[0]}_{a[1]}.pickle"))
        js[(a, b)] = float(ev.eval(runs[b]))
    same = [js[((True, 11), (True, 22))], js[((False, 11), (False, 22))]]
    cross = [js[((True, 11), (False, 11))], js[((True, 22), (False, 22))], js[((True, 11), (False, 22))]]
    print(f"{cfg} iid: JS(two seeds, split_f16)={same[0]:.3e} JS(two seeds, fp32 MFMA)={same[1]:.3e} JS(split_f16 vs fp32 MFMA)="
          + " ".join(f"{v:.3e}" for v in cross))
    # same seed, two engines: the same draws, so the ensembles nearly coincide; different seeds: the sampling noise of 4096 chains
    # either way -- no pair of engines further apart than two seeds of one (a quarter of slack)
    assert max(cross) <= 1.25 * max(same), (cross, same)


@pytest.mark.parametrize("cfg", ["chignolin", "villin"])
@pytest.mark.parametrize("kind", sorted(BELOW_RANGE))
def test_fp16_engine_steps_aside_for_models_below_its_range(dff, cfg, kind, capfd):
    """The mirror of test_fp16_engine_steps_aside_for_models_out_of_its_range (tests/test_gpu_parity.py): a weight matrix whose
    largest entry is below 2^-12, or LayerNorm rows bounded below 2^-12 by their gains and biases, would leave the fp16 pieces'
    2^-22 relative accuracy (a piece resolves 2^-36 absolutely).  dff_model_create gives such a model the fp32-MFMA engine, says
    so in one line on stderr, and its forces are the reference's (twin, float64)."""
    from dff_amd.score import GraphTransformer
    _, N, H, L = ARCHS[cfg]
    params, x, t, L = structured_case(cfg, kind)
    capfd.readouterr()
    model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                             use_distances=False, conservative=True, state_dict=params)
    err = capfd.readouterr().err
    f = model.native.score(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).cpu().numpy()
    kname = model.native.last_launch()[0]
    f32ref, f64 = twin_forces(params, x, t, L)
    r32, r = rel(f32ref, f64), rel(f, f64)
    print(f"{cfg} {kind}: {kname} rel(hip, f64)={r:.3e} rel(ref32, ref64)={r32:.3e}")
    assert "split_" not in kname, kname
    assert "below the fp16 split engine's range, weight GEMMs run on the fp32 matrix pipe" in err, err
    assert np.isfinite(f).all() and r <= GUARD_FP32 * max(r32, 4e-7), (r, r32)
    assert kind in ILL_CONDITIONED or r <= 5e-6, (r, r32)


@pytest.mark.parametrize("path", ["fold_le16", "le64"])
@pytest.mark.parametrize("kind", [f"one_matrix_1e-6[{w}]" for w in ONE_MATRIX] + ["ln_gain_tiny"])
def test_stash_intermediates_relative_on_low_magnitude_models(dff, path, kind, monkeypatch):
    """Stage-level companion of the force checks: a tiny matrix inside a residual branch can hide in the forces while that branch
    is wrong.  Every stashed forward stage (q, k, v, P, attn_out, ff, u) of chignolin's kernel -- the <= 16-row FOLD kernel, and
    the <= 64-row kernel -- against the float64 kernel model (oracle/kernel_model.py), each measured RELATIVE TO ITS OWN
    magnitude (test_stash_intermediates_vs_kernel_model divides by max(1, |ref|max): an absolute bar for tiny stages), and held to
    a small multiple of the same stage's error in the float32 kernel model."""
    from oracle import kernel_model as km
    from dff_amd.score import GraphTransformer
    monkeypatch.setenv("DFF_SPLIT_BF16", "1")
    monkeypatch.setenv("DFF_FOLD_KV", "1")
    cfg = "chignolin"
    _, N, H, L = ARCHS[cfg]
    params, x, t, L = structured_case(cfg, kind)
    x, t = x[:2].copy(), t[1:3].copy()
    model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                             use_distances=False, conservative=True, state_dict=params)
    model.native.force_generic(path == "le64")
    model.native.score(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda())
    torch.cuda.synchronize()
    kname = model.native.last_launch()[0]
    assert ("dff_small_kernel<" in kname) == (path == "fold_le16"), kname
    fw = km.fold_kv(km.fold_weights(params, L))            # hidden == head dimension: the library folds W_k / W_v away
    xc = x.astype(np.float64) - x.astype(np.float64).mean(1, keepdims=True)
    _, st64 = km.forward(fw, xc, t)
    _, st32 = km.forward(km.cast(fw, np.float32), xc, t)

    def stages(st, b):
        return dict(q=st["q"][b].transpose(1, 0, 2).reshape(N, 512), k=st["k"][b].transpose(1, 0, 2).reshape(N, 512),
                    v=st["v"][b].transpose(1, 0, 2).reshape(N, 512), P=st["P"][b], attn_out=st["attn_out"][b], ff=st["ff"][b],
                    u=st["u"][b].transpose(1, 0, 2).reshape(N, 24))
    worst, worst32 = {}, {}
    for b in range(2):
        for l in range(L):
            ref, ref32 = stages(st64[l], b), stages(st32[l], b)
            for name in ref:
                if name in ("k", "v") and "fold_kv" in kname:
                    continue   # keys and values ARE the LayerNorm rows there: never projected, never stashed
                got = model.native.debug_stash(b, l, name)
                if name == "u":
                    got = got[:, :24]
                scale = np.abs(ref[name]).max()
                key = f"l{l}.{name}"
                worst[key] = max(worst.get(key, 0.0), np.abs(got - ref[name]).max() / scale)
                worst32[key] = max(worst32.get(key, 0.0), np.abs(ref32[name] - ref[name]).max() / scale)
    print(f"{kind} {kname}: stage error / own magnitude (kernel | float32 kernel model): "
          + " ".join(f"{k}={worst[k]:.1e}|{worst32[k]:.1e}" for k in worst))
    for key in worst:
        assert worst[key] <= 16.0 * max(worst32[key], 1e-7), (key, worst[key], worst32[key])


def test_fp16_engine_fused_samplers_on_decayed_model(dff):
    """The sampler level: a short fused Langevin run and a short fused reverse-DDPM run of the uniformly decayed chignolin model
    (all_linear_1e-6) on supplied noise, against the twin's simulate / p_sample_loop at tests/test_gpu_parity.py's STEP_TOL x K."""
    from dff_amd.ddpm import GaussianDiffusion
    from dff_amd.langevin import LangevinDiffusion
    from dff_amd.score import GraphTransformer
    STEP_TOL = 5e-6                                       # tests/test_gpu_parity.py
    cfg, kind, K, P, tlev = "chignolin", "all_linear_1e-6", 6, 5, 20
    _, N, H, L = ARCHS[cfg]
    params, _, _, L = structured_case(cfg, kind)
    norm, temp, masses = NORM_STD[cfg], TEMP[cfg], [12.0] * N
    model = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                             use_distances=False, conservative=True, state_dict=params)
    diff = GaussianDiffusion(model, num_atoms=N, timesteps=1000, norm_factor=norm)
    x0 = synth.normal((P, N, 3), 43, 7).astype(np.float32)
    x0 = (x0 - x0.mean(1, keepdims=True)) * norm
    noises = synth.normal((K, P, N, 3), 44, 7).astype(np.float32)
    ld = LangevinDiffusion(diff, torch.from_numpy(x0), K, save_interval=2, t=tlev, diffusion_steps=1000, temp_data=temp,
                           temp_sim=temp, dt=None, masses=masses, friction=1.0, kb="consistent", verbose=False)
    traj = ld.sample(noises=torch.from_numpy(noises)).numpy().reshape(P, K // 2, N, 3)
    kl = model.native.last_launch()[0]
    c = twin.langevin_constants(norm, tlev, twin.make_schedule(), temp, temp, masses, 1.0, None)
    fr, _, _, _ = twin.simulate(twin.to_torch(params), torch.from_numpy(x0) / norm, torch.from_numpy(noises), masses, c, L, 2)
    ref = (fr * norm).numpy()
    err_l = np.abs(traj - ref).max() / np.abs(ref).max()
    xd = synth.normal((P, N, 3), 45, 7).astype(np.float32)
    xd = (xd - xd.mean(1, keepdims=True)) * 0.6
    nd = synth.normal((K, P, N, 3), 46, 7).astype(np.float32)
    y = diff.p_sample_loop_from(torch.from_numpy(xd), K - 1, 0, noises=torch.from_numpy(nd)).cpu().numpy()
    kd = model.native.last_launch()[0]
    refd = twin.p_sample_loop(twin.to_torch(params), twin.make_schedule(), torch.from_numpy(xd), torch.from_numpy(nd), K - 1, L).numpy()
    err_d = np.abs(y - refd).max() / np.abs(refd).max()
    print(f"{kind}: {K}-step Langevin ({kl}) rel err {err_l:.3e}; {K} reverse steps ({kd}) rel err {err_d:.3e}")
    assert err_l <= STEP_TOL * K and err_d <= STEP_TOL * K, (err_l, err_d)
    assert ("split_" in kl) == (kind not in BELOW_RANGE) and ("split_" in kd) == (kind not in BELOW_RANGE), (kl, kd)
    assert model.native.status() == 0
