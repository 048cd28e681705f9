#!/usr/bin/env python3
"""Golden vectors of the forward process and its loss (models/ddpm.py:100-138, 164-193, 265-337), by running the
REFERENCE classes on the CPU:

    python tests/golden/make_golden_ploss.py <path to a checkout of microsoft/two-for-one-diffusion>

Writes ploss_<cfg>.npz for ala2, chignolin and trp_cage (synthetic weights of oracle/synth.py, seed 1234, full decoder
scale: the models tests/test_gpu_parity.py builds) and ploss_tables.npz.  Data only.  Per config, batch 7 with
t = 0 and t = T - 1 among the levels:
  x0, t, noise                     un-centred x0 in normalised units, int64 levels, un-centred standard normals
  q_sample, xt                     the reference's q_sample(x0, t, center_zero(noise)) and its center_zero (p_losses' x), float32
  tnorm                            1.0 * t / T as p_losses passes it (float32)
  out32, out64                     the score network at (xt, tnorm): float32 modules, and the same modules in float64
                                   on the SAME float32 xt, tnorm (what a float32 implementation is measured against)
  l1_32, l2_32, l1_64, l2_64       per-sample losses: the mean of each row of the reference's reduce(loss, "b ... -> b (...)", "mean")
                                   (the float64 ones from out64 and the noise centred in float64)
  l1_mean32, l2_mean32, ...64      p_losses' return value (float32: the reference's own call; float64: mean of the above)
  fwd_mol, fwd_t, fwd_noise,       one forward(mol) (Angstrom input, loss_type l2): the multinomial draw and the randn_like
  fwd_loss32, fwd_loss64,          draw replayed from the same generator state, the value, and its float64 counterpart
  fwd_out32, fwd_out64             with the model outputs of that call
ploss_tables.npz: the four p2_loss_weight tables at T = 1000 ("ones" with gamma 0.5, k 1; "score_matching";
"higheruntil_100"; "lower_bound_10_5").
"""
import os
import sys
import types

import numpy as np
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, REPO)
from oracle import cpu_repro  # noqa: E402
cpu_repro.pin()
import torch  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DFF_REFERENCE_DIR", "")
assert os.path.isdir(os.path.join(REF, "models")), "usage: make_golden_ploss.py <reference checkout>"
sys.modules["mdtraj"] = types.ModuleType("mdtraj")
sys.path.insert(0, REF)
sys.path.insert(1, REPO)

from einops import reduce  # noqa: E402
from models.graph_transformer import GraphTransformer  # noqa: E402  (reference)
from models.ddpm import GaussianDiffusion  # noqa: E402  (reference)
from utils import center_zero  # noqa: E402  (reference)

from oracle import synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NORM_STD = {"chignolin": 3.113133430480957, "ala2": 0.9449278712272644, "trp_cage": 5.08211088180542}
T = 1000
LEVELS = np.array([0, T - 1, 1, 500, 20, 250, T - 2], np.int64)
TABLES = {"ones_g0.5_k1": dict(loss_weights="ones", p2_loss_weight_gamma=0.5, p2_loss_weight_k=1),
          "score_matching": dict(loss_weights="score_matching"),
          "higheruntil_100": dict(loss_weights="higheruntil_100"),
          "lower_bound_10_5": dict(loss_weights="lower_bound_10_5")}


def build(cfg, dtype=torch.float32, loss_type="l2", **kw):
    _, N, H, L = synth.SHIPPED_CONFIGS[cfg]
    gnn = GraphTransformer(N, hidden_nf=H, device="cpu", n_layers=L, use_intrinsic_coords=True, use_abs_coords=False,
                           use_distances=False, conservative=True)
    params = synth.synth_gnn_params(N, H, L, seed=1234)
    res = gnn.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    kw.setdefault("loss_weights", "higheruntil_100")
    ddpm = GaussianDiffusion(model=gnn, features=torch.eye(N), num_atoms=N, timesteps=T, norm_factor=NORM_STD[cfg],
                             loss_type=loss_type, **kw)
    ddpm.eval()
    return (ddpm.double() if dtype == torch.float64 else ddpm), N


def chain(ddpm, x0, t, noise, xt=None, tn=None):
    """p_losses step by step with the reference's own pieces; per-sample l1 / l2 and the model output."""
    nz = center_zero(noise)
    q = ddpm.q_sample(x_start=x0, t=t, noise=nz)
    if xt is None:
        xt = center_zero(q)
        tn = 1.0 * t / ddpm.num_timesteps
    out = ddpm.model(xt, ddpm.h, tn, alphas=ddpm.sqrt_alphas_cumprod[t].pow(2)).detach()
    oc = center_zero(out)
    # (the reference's reduce only flattens each sample to a row of 3 N entries -- nothing is named to reduce over -- and
    # p_losses takes the mean of everything; the per-sample loss is the mean of a row)
    per = {k: reduce(f(oc, nz, reduction="none"), "b ... -> b (...)", "mean").mean(dim=1)
           for k, f in (("l1", torch.nn.functional.l1_loss), ("l2", torch.nn.functional.mse_loss))}
    return q, xt, tn, out, per


def main():
    np.savez(os.path.join(OUT, "ploss_tables.npz"),
             **{k: build("ala2", **kw)[0].p2_loss_weight.numpy() for k, kw in TABLES.items()})
    for cfg in ("ala2", "chignolin", "trp_cage"):
        ddpm, N = build(cfg)
        ddpm64, _ = build(cfg, torch.float64)
        ddpm64.h = ddpm64.h.double()
        x0 = (synth.normal((7, N, 3), 4242, 1) + np.array([0.3, -0.2, 0.1])).astype(np.float32)
        noise = synth.normal((7, N, 3), 4242, 2).astype(np.float32)
        x0t, tt, nzt = torch.from_numpy(x0), torch.from_numpy(LEVELS), torch.from_numpy(noise)
        q, xt, tn, out32, per32 = chain(ddpm, x0t, tt, nzt)
        assert tn.dtype == torch.float32
        _, _, _, out64, per64 = chain(ddpm64, x0t.double(), tt, nzt.double(), xt.double(), tn.double())
        rec = dict(x0=x0, t=LEVELS, noise=noise, q_sample=q.numpy(), xt=xt.numpy(), tnorm=tn.numpy(), out32=out32.numpy(),
                   out64=out64.numpy())
        for k in ("l1", "l2"):
            ddpm.loss_type = k
            mean32 = ddpm.p_losses(x0t, tt, noise=nzt).detach()
            assert abs(float(mean32) - float(per32[k].mean())) <= 2.0 ** -22 * float(mean32), (cfg, k)
            rec.update({f"{k}_32": per32[k].numpy(), f"{k}_64": per64[k].numpy(), f"{k}_mean32": mean32.numpy(),
                        f"{k}_mean64": per64[k].mean().numpy()})
        # one forward(): Angstrom input, t from the multinomial, noise from randn_like, both replayed
        ddpm.loss_type = "l2"
        mol = torch.from_numpy(synth.normal((7, N, 3), 4242, 3).astype(np.float32) * np.float32(NORM_STD[cfg]) + np.float32(1.5))
        torch.manual_seed(31)
        val = ddpm(mol).detach()
        torch.manual_seed(31)
        ft = torch.multinomial(ddpm.p2_loss_weight, 7, replacement=True).long()
        fn = torch.randn_like(mol)
        m32 = center_zero(mol) / ddpm.norm_factor
        _, fxt, ftn, fout32, fper32 = chain(ddpm, m32, ft, fn)
        assert abs(float(val) - float(fper32["l2"].mean())) <= 2.0 ** -22 * float(val), cfg
        _, _, _, fout64, fper64 = chain(ddpm64, m32.double(), ft, fn.double(), fxt.double(), ftn.double())
        rec.update(fwd_out32=fout32.numpy(), fwd_out64=fout64.numpy(), fwd_mol=mol.numpy(), fwd_t=ft.numpy(), fwd_noise=fn.numpy(), fwd_loss32=val.numpy(),
                   fwd_loss64=fper64["l2"].mean().numpy(), norm_factor=np.float64(NORM_STD[cfg]))
        np.savez(os.path.join(OUT, f"ploss_{cfg}.npz"), **rec)
        r = np.linalg.norm(rec["out32"] - rec["out64"]) / np.linalg.norm(rec["out64"])
        print(f"{cfg}: rel(out32, out64) = {r:.3e}  |out| rms = {np.sqrt((rec['out64'] ** 2).mean()):.3f}  l2 = {rec['l2_64']}  "
              f"fwd t = {rec['fwd_t']} loss = {float(val):.6f}")
    print("done")


if __name__ == "__main__":
    main()
