"""What the test modules share that is not an oracle (those are in oracle/): the device fixture and the lazy accessors of
the package, the upload helpers, the constants and bars that more than one file holds a kernel to, and the assertions on
top of them (refused, same_bits among them).  The host stand-ins that go behind evaluate's seams are in tests/standins.py.  Fixtures are imported by name (`from support import dev  # noqa: F401`).  Pytest does not rewrite the
asserts of this module, so each of them carries the values it compares in its message."""
import argparse
import os
import pickle
import re

import numpy as np
import pytest
import torch

from oracle import noise
from oracle import reference_twin as twin
from oracle import synth

MOLS = ["chignolin", "trp_cage", "bba", "villin", "protein_g"]
N_BEADS = {"chignolin": 10, "trp_cage": 20, "bba": 28, "villin": 35, "protein_g": 56}
RMSD_ATOL, RMSD_RTOL = 1e-5, 1e-6          # the bar of test_struct_metrics.py::test_rmsd_vs_kabsch
MIRROR = np.array([-1.0, 1.0, 1.0])
GAP_MIN = 1e-2            # strict superposition comparisons run on frames with (l1 - l2) / (l1 - l4) >= GAP_MIN
MAX_EXCLUDED = 0.02       # at most this share of a data set may fall below it
GUARD = 2.0        # rel(hip, ref64) <= GUARD * rel(ref32, ref64): the split engine (every shipped architecture's default path)
GUARD_FP32 = 2.5   # ... the fp32-MFMA engine (DFF_SPLIT_BF16=0, `gen` branches, hidden 256)
M_DRAW = 4.0       # |kernel draw - normals64| <= M_DRAW * E32 (test_noise_stream.py derives it)
EPS = 2.0 ** -24   # relative error of one float32 rounding


# ---------------------------------------------------------------- the package and the device
@pytest.fixture(scope="module")
def dev():
    import dff_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dff_amd.load_library()
    return torch.device("cuda:0")


def B():
    from dff_amd import binding
    return binding


def ev():
    from dff_amd import evaluate
    return evaluate


def hmm_chunk():
    """frames of a chain per chunk of the hidden-Markov-model kernels, read from the library"""
    return B().hmm_chunk()


ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "two-for-one-diffusion_amd", "csrc")


def build_units():
    """the translation units build.sh compiles and links, {unit: its source file in csrc/}, from its one list (UNITS)"""
    units = re.search(r'(?m)^UNITS="([^"]+)"$', open(os.path.join(ROOT, "build.sh")).read()).group(1).split()
    assert len(units) == len(set(units)), units
    return {u: re.sub(r"^dff_small_m\d$", "dff_small", u) + ".hip" for u in units}   # the <= 16-row kernel: once per sampler mode


def owning_unit(kernel_file):
    """The text of the unit that compiles csrc/<kernel_file> into the library: of the units build.sh lists, the ONE whose
    source includes the file by name."""
    texts = {src: open(os.path.join(CSRC, src)).read() for src in set(build_units().values())}
    owners = [src for src, text in sorted(texts.items()) if '#include "%s"' % kernel_file in text]
    assert len(owners) == 1, (kernel_file, owners)
    return texts[owners[0]]


def refused(lib, rc, what):
    """the ABI call returned DFF_EINVAL and dff_last_error() says `what`"""
    assert rc == 1, (rc, what)
    assert what in lib.dff_last_error().decode(), (what, lib.dff_last_error().decode())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def up(a, dev):
    """a copy of the host frames on the device (the shared sets are read-only)"""
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def on_device(x, dev, vec4):
    """x on the device at a 16-byte aligned address (vec4) or 4 bytes past one (the kernels' scalar tile loads)"""
    flat = torch.empty(x.size + 4, dtype=torch.float32, device=dev)
    off = 0 if vec4 else 1
    assert flat.data_ptr() % 16 == 0, f"a fresh allocation at {flat.data_ptr():#x} is not 16-byte aligned"
    t = flat[off:off + x.size].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert x.size == 0 or (t.data_ptr() % 16 == 0) == vec4, f"vec4 {vec4} but the view is at {t.data_ptr():#x}"
    return t


# ---------------------------------------------------------------- golden frames
def x_rmsd(g):
    x = g["x"].copy()
    x[tuple(g["nonfinite_at"].T)] = g["nonfinite_val"]
    return x


def golden_frames(golden, mol):
    """(frames with the golden's injected non-finite coordinates, folded structure float32)"""
    f = golden("struct_folded.npz")[mol].astype(np.float32)
    x = golden("struct_ref_ala2.npz")["x"] if mol == "ala2" else x_rmsd(golden(f"struct_ref_{mol}.npz"))
    return x, f


# ---------------------------------------------------------------- bars
def assert_rmsd(got, ref, what=""):
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (f"{what}: NaN at frames {np.flatnonzero(np.isnan(got))[:8]}, "
                                                           f"the oracle's at {np.flatnonzero(np.isnan(ref))[:8]}")
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    bad = err > RMSD_ATOL + RMSD_RTOL * ref[ok]
    assert not bad.any(), (f"{what}: {bad.sum()} of {ok.sum()} frames off, worst |err| {err.max():.3e} A "
                           f"at rmsd {ref[ok][np.argmax(err)]:.3e}")


def assert_close(got, want, what=""):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the oracle's {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {np.isnan(got).sum()} NaN, the oracle has {np.isnan(want).sum()}"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bad = err > RMSD_ATOL + RMSD_RTOL * want[ok]
    worst = err.max() if err.size else 0.0
    print(f"{what}: {ok.sum()} pairs, worst |err| {worst:.3e} A")
    assert not bad.any(), f"{what}: {bad.sum()} of {ok.sum()} pairs off, worst |err| {worst:.3e} A"


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def e32_of(seed, items, steps, N):
    """E32 of the draws under test and normals64 of them."""
    z64 = noise.normals64(seed, items, steps, N)
    return float(np.abs(noise.normals32_plain(seed, items, steps, N).astype(np.float64) - z64).max()), z64


def guard_for(kname):
    """The bar that goes with the kernel that ran (its name says which engine multiplied the weights)."""
    return GUARD if "split_" in kname else GUARD_FP32


# ---------------------------------------------------------------- the energies of dff_score (tests/test_score_energy.py)
R32_FLOOR = 4e-7   # the floor under the twin's own float32 distance: the forces' floor (test_fp16_engine_over_gradient_magnitudes)
K_E = 2.5          # rel(e_hip, e64) <= K_E * max(rel(e32, e64), R32_FLOOR), batch and every single protein: the split engine
K_E_FP32 = 4.0     # ... the fp32-MFMA engine (tests/test_score_energy.py, MEASURED and THE CHOICE OF K_E)


def k_energy(kname):
    """K_E of the kernel that ran (its name says which engine multiplied the weights, as for guard_for)."""
    return K_E if "split_" in kname else K_E_FP32


def twin_energies(params, x, t, L, flags=(True, False, False)):
    """(e32, e64): the twin's per-bead energies (B, N) of numpy (x, t) in float32 and in float64, same weights."""
    e32 = twin.score(twin.to_torch(params), torch.from_numpy(x), torch.from_numpy(t), L, return_energy=True, flags=flags)[1]
    e64 = twin.score(twin.to_torch(params, torch.float64), torch.from_numpy(x).double(), torch.from_numpy(t).double(), L,
                     return_energy=True, flags=flags)[1]
    return e32.numpy()[..., 0], e64.numpy()[..., 0]


def energy_distance(e, e32, e64):
    """How dff_score's energies are compared with the float64 oracle, as numbers: (r, r32e, worst) with
    r = ||e - e64|| / ||e64|| over the whole (B, N) output, r32e the same distance of the twin's float32 run (the yardstick),
    worst = (r_b, b) of the protein whose own rows are furthest, relative to its own norm."""
    e, e32, e64 = (np.asarray(a, np.float64).reshape(np.shape(e64)[0], -1) for a in (e, e32, e64))
    per = [rel(e[b], e64[b]) for b in range(e64.shape[0])]
    b = int(np.argmax(per))
    return rel(e, e64), rel(e32, e64), (per[b], b)


def assert_energy(e, e32, e64, kname, what):
    """The energy bar: r <= 1e-5 and r <= K_E(kernel) x max(r32e, R32_FLOOR) over the batch, and the same for every protein
    on its own against the batch's yardstick.  Prints the figures before it asserts; returns r / max(r32e, R32_FLOOR)."""
    r, r32e, (rb, b) = energy_distance(e, e32, e64)
    yard, k = max(r32e, R32_FLOOR), k_energy(kname)
    print(f"[energy] {what} {kname}: r={r:.3e} r32e={r32e:.3e} ratio={r / yard:.2f} worst protein {b}: r_b={rb:.3e} ratio={rb / yard:.2f} "
          f"K_E={k}")
    assert np.isfinite(np.asarray(e)).all(), f"{what}: non-finite energies"
    assert r <= 1e-5 and r <= k * yard, f"{what} {kname}: energies r={r:.3e}, bar {min(1e-5, k * yard):.3e} (r32e={r32e:.3e}, K_E={k})"
    assert rb <= 1e-5 and rb <= k * yard, (f"{what} {kname}: energies of protein {b} r_b={rb:.3e}, bar {min(1e-5, k * yard):.3e} "
                                           f"(r32e={r32e:.3e}, K_E={k})")
    return r / yard


# ---------------------------------------------------------------- a model on disk
def write_model_dir(path, cfg, decoder_scale=1e-2):
    """A saved_models/<mol>-style directory in the reference's format: args.pickle (argparse
    Namespace that also pickles an nn.Module, as the shipped ones do) + model-best.pt whose
    ["ema"] entry is an EMA(GaussianDiffusion) state-dict (trainer.py:181-206, sample.py:154-167)."""
    mol, N, H, L = synth.SHIPPED_CONFIGS[cfg]
    ns = argparse.Namespace(mol=mol, mean0=True, fold=1, shuffle_data_before_splitting=True, scale_data=True,
                            backbone_network="graph-transformer", hidden_features_gnn=H, num_layers_gnn=L,
                            use_intrinsic_coords=True, use_abs_coords=False, use_distances=False, conservative=True,
                            diffusion_steps=1000, loss_weights="higheruntil_100", activation=torch.nn.Tanh())
    with open(path / "args.pickle", "wb") as f:
        pickle.dump(ns, f)
    params = synth.synth_gnn_params(N, H, L, decoder_scale=decoder_scale)
    gd = {k: v.clone() for k, v in twin.make_schedule().items()}
    gd["p2_loss_weight"] = torch.ones(1000)
    gd.update({"model." + k: torch.from_numpy(v) for k, v in params.items()})
    ema = {"initted": torch.tensor([True]), "step": torch.tensor([123])}
    ema.update({"ema_model." + k: v for k, v in gd.items()})
    ema.update({"online_model." + k: torch.zeros_like(v) for k, v in gd.items()})
    torch.save({"step": 123, "model": {k: torch.zeros_like(v) for k, v in gd.items()}, "ema": ema}, path / "model-best.pt")
    return params, (N, H, L)
