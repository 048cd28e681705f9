"""Every ABI call is ordered on the caller's stream, and only on it, by the protocol of tests/stream_gate.py (the gate, the
poison, the sentinel and what is asserted are described there): the harness's own controls, the model calls, the forward
process, the analysis calls, and two calls on two streams at once.  (dff_superpose: tests/test_superpose.py.)

The model calls run on the kernel variants of tests/test_noise_stream.py (same synthetic models, same knobs; every case asserts
the kernel that ran).  A fresh model's first call ("cold") allocates, builds the layer-0 table and synchronises the stream:
only its results are asserted; the identical second call ("warm") on the same model and stream must not block.

Next to each stream test, test_fence_* runs the same Spec through the fence protocol of tests/fence.py: all buffers of the call in
one arena between guard bands, workspaces at exactly their *_workspace_bytes, both fill patterns at both placements.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.frames import splitmix_labels, synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import BLOCKING, GATE_MIN_MS, N_FRAMES, Run, Spec, analysis_call, gated, ptr, raw, reference, stream_of
from stream_gate import gate, side  # noqa: F401  (fixtures)
from support import to_dev

pytestmark = pytest.mark.gpu

SEED = (0x9E3779B9 << 32) | 0x2545F491
HI = 2 ** 32
T = 1000


# ------------------------------------------------------------------------------------------------ the harness itself
def test_control_a_default_stream_op_does_not_wait_for_the_gate(gate, side):
    """No library call: with the gate queued on the side stream, y = x * 2 on the DEFAULT stream sees the poison (it ran during
    the gate), the same operation on the side stream sees the real value.  If side streams ever blocked the null stream here,
    the first assertion fails: this file cannot pass without testing anything."""
    assert gate.ms >= GATE_MIN_MS, f"gate too short: {gate.ms:.1f} ms"
    real = torch.arange(1024, dtype=torch.float32, device="cuda") + 1.0
    x = torch.full_like(real, -7.0)
    torch.cuda.synchronize()
    ev_gate = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(gate.cycles)
        ev_gate.record()
        x.copy_(real)
    y_default = x * 2                                  # default stream: not ordered after the gate
    torch.cuda.default_stream().synchronize()
    still_gated = not ev_gate.query()
    y_default_host = y_default.cpu()
    with torch.cuda.stream(side):
        y_side = x * 2
    side.synchronize()
    assert still_gated, "the default stream waited for the side stream's gate: side streams block the null stream here"
    assert torch.equal(y_default_host, torch.full((1024,), -14.0)), "the default-stream op saw the value queued behind the gate"
    assert torch.equal(y_side.cpu(), real.cpu() * 2)


def test_control_the_protocol_catches_a_call_on_the_wrong_stream(gate, side):
    """The protocol on a stand-in `call` (plain torch): enqueued on the default stream instead of the current one it must fail
    the bit-equality, and one that synchronises must fail the non-blocking check."""
    real = torch.arange(256, dtype=torch.float32, device="cuda") * 0.5 + 0.25      # (x + 1 is never the sentinel)

    def good(_, b):
        torch.add(b["x"], 1.0, out=b["y"])

    def misplaced(_, b):
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.add(b["x"], 1.0, out=b["y"])

    def blocking(_, b):
        torch.cuda.current_stream().synchronize()
        torch.add(b["x"], 1.0, out=b["y"])

    def spec(fn):
        return Spec("control", {"x": (real, float("nan"))}, {"y": ((256,), torch.float32)}, fn)
    ref = reference(spec(good))
    gated(spec(good), side, gate, ref)
    with pytest.raises(AssertionError, match="differs from the default-stream result"):
        gated(spec(misplaced), side, gate, ref)
    side.synchronize()
    with pytest.raises(AssertionError, match="it synchronised"):
        gated(spec(blocking), side, gate, ref)
    side.synchronize()


def test_control_the_fence_sees_a_stray_device_write():
    """The fence protocol (tests/fence.py; its controls run on the CPU in tests/test_fence.py) once on the device: a stand-in
    `call` that also writes the one byte after its output -- inside the arena, so nothing is harmed -- fails the band check; on
    the separate allocations of the reference run that byte is the allocator's padding and the stand-in leaves it alone."""
    real = torch.arange(256, dtype=torch.float32, device="cuda") * 0.5 + 0.25

    def good(_, b):
        torch.add(b["x"], 1.0, out=b["y"])

    def stray(_, b):
        good(_, b)
        yb = b["y"].view(torch.uint8)
        o = yb.storage_offset() + yb.numel()
        if o < yb.untyped_storage().nbytes():
            torch.as_strided(yb, (1,), (1,), o).fill_(1)

    def spec(fn):
        return Spec("control", {"x": (real, float("nan"))}, {"y": ((256,), torch.float32)}, fn)
    for pattern, placement in COMBINATIONS:
        fenced(spec(good), pattern=pattern, placement=placement)
        with pytest.raises(AssertionError, match=r"guard band damaged: 1 byte\(s\), the first 1 byte\(s\) past the end of y"):
            fenced(spec(stray), pattern=pattern, placement=placement)


# ------------------------------------------------------------------------------------------------ the model calls
# name ->(N, H, L, flags (intrinsic, distances, abs), conservative, weight seed): tests/test_noise_stream.py
MODELS = {
    "ala2": (5, 96, 2, (1, 0, 0), True, 1234),
    "chignolin": (10, 64, 3, (1, 0, 0), True, 1234),
    "trp_cage": (20, 128, 3, (1, 0, 0), True, 1234),
    "protein_g": (56, 128, 3, (1, 0, 0), True, 1234),
}
_params, _shared = {}, {}


def new_native(name):
    """A fresh model (nothing warmed).  Synchronises (uploads): never behind a gate."""
    from dff_amd.score import GraphTransformer
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    N, H, L, (intr, dist, ab), cons, wseed = MODELS[name]
    if name not in _params:
        _params[name] = synth.synth_gnn_params(N, H, L, seed=wseed, decoder_out=1 if cons else 3, node_in=N + 1 + 3 * ab,
                                               edge_in=(3 * intr + dist) or 1)
    return GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=bool(intr), use_abs_coords=bool(ab),
                            use_distances=bool(dist), conservative=cons, state_dict=_params[name]).native


def shared_native(name):
    if name not in _shared:
        _shared[name] = new_native(name)
    return _shared[name]


class Case:
    def __init__(self, cid, model, B, has, lacks=(), group=0, waves=0, pair=True, max_wgs=2048, last_grid=None, offset=0,
                 step_offset=0):
        self.id, self.model, self.B, self.has, self.lacks = cid, model, B, has, lacks
        self.group, self.waves, self.pair, self.max_wgs, self.last_grid = group, waves, pair, max_wgs, last_grid
        self.offset, self.step_offset = offset, step_offset
        self.N = MODELS[model][0]

    @contextlib.contextmanager
    def knobs(self, nat):
        """(dff_debug_pair(0) synchronises the device: the knobs are set before any gate is queued)"""
        try:
            nat.set_group(self.group); nat.small_waves(self.waves); nat.force_generic(False)
            nat.pair(self.pair); nat.max_workgroups(self.max_wgs)
            yield nat
        finally:
            nat.set_group(0); nat.small_waves(0); nat.force_generic(False); nat.pair(True); nat.max_workgroups(2048)

    def check_launch(self, nat):
        name, grid, _ = nat.last_launch()
        assert all(h in name for h in self.has) and not any(l in name for l in self.lacks), (self.id, name)
        if self.last_grid is not None:
            assert grid == self.last_grid, (self.id, grid)
        return name


S16, S64 = "dff_small_kernel<", "dff_fused_kernel<"
CASES = [
    Case("chignolin-8waves", "chignolin", 12, (S16 + "64,8",), offset=HI - 3, step_offset=HI + 1),
    Case("ala2-g3-4waves-ragged", "ala2", 10, (S16 + "96,4",), waves=4, group=3, offset=HI - 3, step_offset=HI - 2),
    Case("chignolin-3-launches", "chignolin", 40, (S16 + "64,8",), max_wgs=16, last_grid=8, offset=HI - 17, step_offset=0),
    Case("trp-cage-pair", "trp_cage", 6, (S64 + "128,2,", "pair"), offset=HI - 3, step_offset=HI - 2),
    Case("trp-cage-one", "trp_cage", 6, (S64 + "128,2,",), ("pair",), pair=False, offset=7, step_offset=0),
    Case("protein-g-pair", "protein_g", 4, (S64 + "128,4,", "pair"), offset=HI - 3, step_offset=0),
]
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
noise_param = pytest.mark.parametrize("supplied", [False, True], ids=["philox", "supplied-noise"])


def _centred(B, N, stream):
    x = synth.normal((B, N, 3), 20261, stream)
    return (x - x.mean(1, keepdims=True)).astype(np.float32)


def score_spec(case):
    B, N = case.B, case.N
    from dff_amd import binding

    def fn(nat, b):
        binding._check(nat.lib, nat.lib.dff_score(nat.handle, binding._ptr(b["x"]), binding._ptr(b["tnorm"]), B,
                                                  binding._ptr(b["force"]), binding._ptr(b["energy"]), nat._stream()), "dff_score")

    def wrap(nat, b):
        f, e = nat.score(b["x"], b["tnorm"], return_energy=True)
        return {"force": f, "energy": e}
    tn = (0.02 + 0.9 * np.arange(B) / B).astype(np.float32)
    return Spec("dff_score", {"x": (to_dev(_centred(B, N, 11) + np.float32(0.25)), float("nan")), "tnorm": (to_dev(tn), float("nan"))},
                {"force": ((B, N, 3), torch.float32), "energy": ((B, N), torch.float32)}, fn, wrap=wrap)


N_STEPS, SAVE = 6, 3


def _langevin_params(N):
    from dff_amd import binding
    p = binding.DffLangevinParams()
    p.t_norm, p.force_scale, p.dt, p.vscale, p.noisescale, p.beta, p.dtau, p.overdamped = 0.02, 0.01, 0.5, 0.7, 0.5, 1.0, 0.0, 0
    for i in range(N):
        p.masses[i] = float(4.0 ** -(i % 3))
    return p


def langevin_spec(case, supplied):
    B, N = case.B, case.N
    p = _langevin_params(N)
    ins = {"x": (to_dev(_centred(B, N, 12)), float("nan")),
           "v": (to_dev((0.25 * synth.normal((B, N, 3), 20261, 13)).astype(np.float32)), float("nan"))}
    if supplied:
        ins["noise"] = (to_dev(synth.normal((N_STEPS, B, N, 3), 20261, 14).astype(np.float32)), float("nan"))

    def fn(nat, b):
        nat.langevin_run(p, b["x"], b["v"], N_STEPS, SAVE, noise=b.get("noise"), seed=SEED, traj_offset=case.offset,
                         step_offset=case.step_offset, frames=b["frames"], ke=b["ke"])
    return Spec("dff_langevin_run", ins, {"frames": ((N_STEPS // SAVE, B, N, 3), torch.float32), "ke": ((N_STEPS // SAVE, B), torch.float32)},
                fn, inout=("x", "v"))


T_START, T_END = 3, 0


def ddpm_spec(case, supplied):
    """Levels 3 .. 0 from the in-kernel prior: x is an output (sentinel); the clamp flag is only ever SET, so it is an input too
    (real 0, poison 1)."""
    B, N = case.B, case.N
    ins = {"clamp_flag": (torch.zeros(1, dtype=torch.int32, device="cuda"), 1)}
    if supplied:
        ins["noise"] = (to_dev(synth.normal((T_START - T_END + 1, B, N, 3), 20261, 15).astype(np.float32)), float("nan"))

    def fn(nat, b):
        nat.ddpm_run(b["x"], T_START, T_END, noise=b.get("noise"), seed=SEED, sample_offset=case.offset, init_prior=True,
                     clamp_flag=b["clamp_flag"])
    return Spec("dff_ddpm_run", ins, {"x": ((B, N, 3), torch.float32)}, fn, inout=("clamp_flag",))


def _model_call(case, spec, gate, side):
    """Reference on the shared model (default stream); then a FRESH model: the cold call behind a gate (results only), the
    identical warm call on the same model and stream (results, and it may not block)."""
    assert (spec.name, "warm") not in BLOCKING
    A = shared_native(case.model)
    with case.knobs(A):
        ref = reference(spec, A)
        name = case.check_launch(A)
    assert all(bool(torch.isfinite(ref[k].float()).all()) for k in spec.results), f"{spec.name}: the reference result is not finite"
    Bm = new_native(case.model)
    try:
        with case.knobs(Bm):
            torch.cuda.synchronize()
            gated(spec, side, gate, ref, Bm, nonblocking=(spec.name, "cold") not in BLOCKING, tag=f" [{case.id}, cold, {name}]")
            assert case.check_launch(Bm) == name
            gated(spec, side, gate, ref, Bm, nonblocking=True, tag=f" [{case.id}, warm, {name}]")
            assert case.check_launch(Bm) == name
            assert Bm.status() == 0
    finally:
        torch.cuda.synchronize()
        Bm.close()


@case_param
def test_score(case, gate, side):
    _model_call(case, score_spec(case), gate, side)


@case_param
@noise_param
def test_langevin_run(case, supplied, gate, side):
    _model_call(case, langevin_spec(case, supplied), gate, side)


@case_param
@noise_param
def test_ddpm_run(case, supplied, gate, side):
    _model_call(case, ddpm_spec(case, supplied), gate, side)


def _model_fence(case, spec):
    """The memory contract (tests/fence.py) on the caller's buffers of a model call -- the model's own scratch is out of reach --
    on the shared model, warmed by the reference call as in the stream test; every fenced call runs the kernel the case names."""
    A = shared_native(case.model)
    with case.knobs(A):
        ref = reference(spec, A)
        name = case.check_launch(A)
        for pattern, placement in COMBINATIONS:
            fenced(spec, A, pattern=pattern, placement=placement, ref=ref)
            assert case.check_launch(A) == name
        assert A.status() == 0


@case_param
def test_fence_score(case):
    _model_fence(case, score_spec(case))


@case_param
@noise_param
def test_fence_langevin_run(case, supplied):
    _model_fence(case, langevin_spec(case, supplied))


@case_param
@noise_param
def test_fence_ddpm_run(case, supplied):
    _model_fence(case, ddpm_spec(case, supplied))


# ------------------------------------------------------------------------------------------------ the forward process
FAMILY = {"chignolin": S16, "trp_cage": S64}


def _forward_inputs(model, B, supplied):
    N = MODELS[model][0]
    x0 = (synth.normal((B, N, 3), 9090, 21) + np.array([0.4, -0.3, 0.2])).astype(np.float32)
    t = np.array([0, T - 1, 1, 500], np.int32)[np.arange(B) % 4]
    ins = {"x0": (to_dev(x0), float("nan")), "t": (to_dev(t), 0)}
    if supplied:
        ins["noise"] = (to_dev(synth.normal((B, N, 3), 9090, 71).astype(np.float32)), float("nan"))
    return N, ins


def q_sample_spec(model, B, supplied):
    from dff_amd import binding
    N, ins = _forward_inputs(model, B, supplied)

    def fn(nat, b):
        binding._check(nat.lib, nat.lib.dff_q_sample(nat.handle, binding._ptr(b["x0"]), binding._ptr(b["t"]), B,
                                                     binding._ptr(b.get("noise")), SEED, HI - 3, 5, binding._ptr(b["xt"]),
                                                     binding._ptr(b["tnorm"]), nat._stream()), "dff_q_sample")

    def wrap(nat, b):
        xt, tn = nat.q_sample(b["x0"], b["t"], noise=b.get("noise"), seed=SEED, sample_offset=HI - 3, draw=5, return_tnorm=True)
        return {"xt": xt, "tnorm": tn}
    return Spec("dff_q_sample", ins, {"xt": ((B, N, 3), torch.float32), "tnorm": ((B,), torch.float32)}, fn, wrap=wrap)


def denoise_loss_spec(nat, model, B, supplied, loss_type="l2", wrapper=True):
    from dff_amd import binding
    N, ins = _forward_inputs(model, B, supplied)
    ins["total"] = (torch.tensor([0.25, 3.0], dtype=torch.float64, device="cuda"), float("nan"))
    ws = torch.empty(nat.denoise_workspace_bytes(B), dtype=torch.uint8, device="cuda")

    def fn(nat_, b):
        binding._check(nat_.lib, nat_.lib.dff_denoise_loss(
            nat_.handle, binding._ptr(b["x0"]), binding._ptr(b["t"]), B, binding._ptr(b.get("noise")), SEED, HI - 3, 5,
            binding.LOSS_TYPES[loss_type], binding._ptr(b["loss"]), binding._ptr(b["total"]), binding._ptr(b["xt"]),
            binding._ptr(b["model_out"]), binding._ptr(b["ws"]), b["ws"].numel(), nat_._stream()), "dff_denoise_loss")

    def wrap(nat_, b):
        loss, xt, out = nat_.denoise_loss(b["x0"], b["t"], noise=b.get("noise"), seed=SEED, sample_offset=HI - 3, draw=5,
                                          loss_type=loss_type, return_xt=True, return_model_out=True)
        return {"loss": loss, "xt": xt, "model_out": out}
    return Spec("dff_denoise_loss", ins, {"loss": ((B,), torch.float32), "xt": ((B, N, 3), torch.float32),
                                          "model_out": ((B, N, 3), torch.float32)}, fn, inout=("total",), work={"ws": ws},
                wrap=wrap if wrapper else None)


def _forward_call(model, spec, gate, side):
    nat = shared_native(model)
    ref = reference(spec, nat)
    if spec.name == "dff_denoise_loss":
        assert FAMILY[model] in nat.last_launch()[0]
        assert float(ref["total"][1]) == 3.0 + ref["loss"].numel()
    assert all(bool(torch.isfinite(ref[k].double()).all()) for k in spec.results)
    gated(spec, side, gate, ref, nat, nonblocking=(spec.name, "warm") not in BLOCKING, tag=f" [{model}]")
    assert nat.status() == 0


@pytest.mark.parametrize("model,B", [("chignolin", 11), ("trp_cage", 5)])
@noise_param
def test_q_sample(model, B, supplied, gate, side):
    _forward_call(model, q_sample_spec(model, B, supplied), gate, side)


@pytest.mark.parametrize("model,B", [("chignolin", 11), ("trp_cage", 5)])
@noise_param
def test_denoise_loss(model, B, supplied, gate, side):
    _forward_call(model, denoise_loss_spec(shared_native(model), model, B, supplied), gate, side)


def _forward_fence(model, spec):
    nat = shared_native(model)
    ref = reference(spec, nat)
    for pattern, placement in COMBINATIONS:
        fenced(spec, nat, pattern=pattern, placement=placement, ref=ref)
    assert nat.status() == 0


@pytest.mark.parametrize("model,B", [("chignolin", 11), ("trp_cage", 5)])
@noise_param
def test_fence_q_sample(model, B, supplied):
    _forward_fence(model, q_sample_spec(model, B, supplied))


@pytest.mark.parametrize("model,B", [("chignolin", 11), ("trp_cage", 5)])
@noise_param
def test_fence_denoise_loss(model, B, supplied):
    """(the workspace holds x_t, tnorm, the model output and the partial sums: at exactly dff_denoise_workspace_bytes)"""
    _forward_fence(model, denoise_loss_spec(shared_native(model), model, B, supplied))


def test_denoise_loss_two_passes_over_one_workspace(gate, side):
    """16384 + 3 samples: two passes whose q_sample, score, loss and copy-out all reuse one workspace -- the second pass must
    be ordered after the first pass's copies."""
    nat = shared_native("chignolin")
    B = 16384 + 3
    assert nat.denoise_workspace_bytes(B) == nat.denoise_workspace_bytes(16384)
    _forward_call("chignolin", denoise_loss_spec(nat, "chignolin", B, True, loss_type="l1", wrapper=False), gate, side)


# ------------------------------------------------------------------------------------------------ the analysis calls
beads_param = pytest.mark.parametrize("N", [10, 35])


def pwd_max_spec(N):
    from dff_amd import binding
    off = 3
    npairs = binding.pwd_num_pairs(N, off)
    return Spec("dff_pwd_max", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 31)), float("nan"))}, {"max": ((npairs,), torch.float32)},
                lambda _, b: raw("dff_pwd_max", 0, ptr(b["x"]), N_FRAMES, N, off, ptr(b["max"]), stream_of(b["x"])),
                wrap=lambda _, b: {"max": binding.pwd_max(b["x"], off)})


def pwd_hist_spec(N):
    """(raw call only: the wrapper reads the bin counts back)"""
    from dff_amd import binding
    off = 3
    npairs = binding.pwd_num_pairs(N, off)
    nbins = (5 + np.arange(npairs) % 17).astype(np.int32)
    hmax = (12.0 + 0.37 * (np.arange(npairs) % 29)).astype(np.float32)
    mb = int(nbins.max())
    return Spec("dff_pwd_hist", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 32)), float("nan")), "nbins": (to_dev(nbins), 1), "hmax": (to_dev(hmax), 1.0)},
                {"hist": ((npairs, mb + 2), torch.int32)},
                lambda _, b: raw("dff_pwd_hist", 0, ptr(b["x"]), N_FRAMES, N, off, ptr(b["nbins"]), ptr(b["hmax"]), mb, mb + 2,
                                 ptr(b["hist"]), stream_of(b["x"])))


def struct_rmsd_spec(N):
    from dff_amd import binding
    ref = synth_chain_frames(1, N, 33)[0]
    return Spec("dff_struct_rmsd", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 34)), float("nan")), "ref": (to_dev(ref), to_dev(ref * 0.5 + 1.0))},
                {"rmsd": ((N_FRAMES,), torch.float32)},
                lambda _, b: raw("dff_struct_rmsd", 0, ptr(b["x"]), N_FRAMES, N, ptr(b["ref"]), ptr(b["rmsd"]), stream_of(b["x"])),
                wrap=lambda _, b: {"rmsd": binding.struct_rmsd(b["x"], b["ref"])})


def struct_dihedrals_spec(N):
    from dff_amd import binding
    return Spec("dff_struct_dihedrals", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 35)), float("nan"))}, {"dih": ((N_FRAMES, N - 3), torch.float32)},
                lambda _, b: raw("dff_struct_dihedrals", 0, ptr(b["x"]), N_FRAMES, N, ptr(b["dih"]), stream_of(b["x"])),
                wrap=lambda _, b: {"dih": binding.struct_dihedrals(b["x"])})


def _tic_model(N, k=2):
    from dff_amd import binding
    F = binding.struct_tic_num_features(N)
    mean = synth.uniform((F,), 778, 1, 0.0, 10.0)
    coeff = synth.uniform((F, k), 778, 2, -0.1, 0.1)
    return F, k, to_dev(mean), to_dev(coeff)


def struct_tic_spec(N):
    from dff_amd import binding
    F, k, mean, coeff = _tic_model(N)
    return Spec("dff_struct_tic", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 36)), float("nan")), "mean": (mean, 1.0), "coeff": (coeff, 0.5)},
                {"proj": ((N_FRAMES, k), torch.float64)},
                lambda _, b: raw("dff_struct_tic", 0, ptr(b["x"]), N_FRAMES, N, ptr(b["mean"]), ptr(b["coeff"]), k, ptr(b["proj"]),
                                 stream_of(b["x"])),
                wrap=lambda _, b: {"proj": binding.struct_tic(b["x"], b["mean"], b["coeff"])})


def struct_contacts_spec(N):
    folded = (synth.uniform((N, N), 779, 1) > 0).astype(np.uint8)
    return Spec("dff_struct_contacts", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 37)), float("nan")), "folded": (to_dev(folded), 0)},
                {"counts": ((N, N), torch.int32), "mismatch": ((N_FRAMES,), torch.int32)},
                lambda _, b: raw("dff_struct_contacts", 0, ptr(b["x"]), N_FRAMES, N, 8.0, ptr(b["folded"]), 3, ptr(b["counts"]),
                                 ptr(b["mismatch"]), stream_of(b["x"])))


def struct_tic_features_spec(N):
    from dff_amd import binding
    F = binding.struct_tic_num_features(N)
    return Spec("dff_struct_tic_features", {"x": (to_dev(synth_chain_frames(N_FRAMES, N, 38)), float("nan"))}, {"feat": ((N_FRAMES, F), torch.float32)},
                lambda _, b: raw("dff_struct_tic_features", 0, ptr(b["x"]), N_FRAMES, N, ptr(b["feat"]), stream_of(b["x"])),
                wrap=lambda _, b: {"feat": binding.struct_tic_features(b["x"])})


def struct_tic_assign_spec(N):
    from dff_amd import binding
    F, k, mean, coeff = _tic_model(N)
    K = 4
    x = to_dev(synth_chain_frames(N_FRAMES, N, 39))
    proj = binding.struct_tic(x, mean, coeff)
    torch.cuda.synchronize()
    centers = proj[[3, 250, 600, 901]].clone()                       # four of the projections: every state is populated
    return Spec("dff_struct_tic_assign", {"x": (x, float("nan")), "mean": (mean, 1.0), "coeff": (coeff, 0.5), "centers": (centers, 0.0)},
                {"labels": ((N_FRAMES,), torch.int32), "proj": ((N_FRAMES, k), torch.float64), "dist2": ((N_FRAMES,), torch.float64)},
                lambda _, b: raw("dff_struct_tic_assign", 0, ptr(b["x"]), N_FRAMES, N, ptr(b["mean"]), ptr(b["coeff"]), k,
                                 ptr(b["centers"]), K, ptr(b["labels"]), ptr(b["proj"]), ptr(b["dist2"]), stream_of(b["x"])),
                wrap=lambda _, b: dict(zip(("labels", "proj", "dist2"),
                                           binding.struct_tic_assign(b["x"], b["mean"], b["coeff"], b["centers"], True, True))))


def kmeans_step_spec():
    from dff_amd import binding
    n, d, K = N_FRAMES, 2, 4
    pts = synth.normal((n, d), 780, 1) + np.array([[2.0, -1.0]]) * (np.arange(n) % 4)[:, None]
    centers = pts[[1, 2, 3, 4]].copy()
    ws = torch.empty(max(binding.kmeans_workspace_bytes(n, d, K), 1), dtype=torch.uint8, device="cuda")
    return Spec("dff_kmeans_step", {"pts": (to_dev(pts), float("nan")), "centers": (to_dev(centers), 0.5)},
                {"labels": ((n,), torch.int32), "dist2": ((n,), torch.float64), "sums": ((K, d), torch.float64),
                 "counts": ((K,), torch.int64), "inertia": ((1,), torch.float64)},
                lambda _, b: raw("dff_kmeans_step", 0, ptr(b["pts"]), n, d, ptr(b["centers"]), K, ptr(b["labels"]), ptr(b["dist2"]),
                                 ptr(b["sums"]), ptr(b["counts"]), ptr(b["inertia"]), ptr(b["ws"]), b["ws"].numel(), stream_of(b["pts"])),
                work={"ws": ws})


def transition_counts_spec():
    K, lags, lengths = 4, np.array([1, 7], np.int32), np.array([400, 250, 350], np.int64)
    labels = (splitmix_labels(N_FRAMES, K))
    return Spec("dff_transition_counts", {"labels": (to_dev(labels), 0)}, {"counts": ((2, K, K), torch.int64)},
                lambda _, b: raw("dff_transition_counts", 0, ptr(b["labels"]), N_FRAMES, lengths.ctypes.data_as(C.c_void_p), 3,
                                 lags.ctypes.data_as(C.c_void_p), 2, K, ptr(b["counts"]), stream_of(b["labels"])))


def tica_moments_spec(N, lengths, lag):
    """The accumulators are ADDED to: inputs as well as outputs (real: small non-zero values; poison NaN)."""
    from dff_amd import binding
    n = int(sum(lengths))
    F = binding.struct_tic_num_features(N)
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    x = to_dev(synth_chain_frames(n, N, 40))
    feat0 = binding.struct_tic_features(x[:1]).double().reshape(F).clone()
    torch.cuda.synchronize()
    ws = torch.empty(binding.tica_workspace_bytes(N, n, lag), dtype=torch.uint8, device="cuda")
    acc = {"sx": torch.full((F,), 0.5, dtype=torch.float64, device="cuda"), "sy": torch.full((F,), -0.25, dtype=torch.float64, device="cuda"),
           "m0": torch.full((F, F), 0.125, dtype=torch.float64, device="cuda"), "mt": torch.full((F, F), 2.0, dtype=torch.float64, device="cuda")}
    ins = {"x": (x, float("nan")), "shift": (feat0, 0.0)}
    ins.update({k: (v, float("nan")) for k, v in acc.items()})
    return Spec("dff_tica_moments", ins, {},
                lambda _, b: raw("dff_tica_moments", 0, ptr(b["x"]), n, N, ln.ctypes.data_as(C.c_void_p), int(ln.size), lag,
                                 ptr(b["shift"]), ptr(b["ws"]), b["ws"].numel(), ptr(b["sx"]), ptr(b["sy"]), ptr(b["m0"]), ptr(b["mt"]),
                                 stream_of(b["x"])),
                inout=("sx", "sy", "m0", "mt"), work={"ws": ws})


N_ENS = 257


def rmsd_matrix_spec(N):
    from dff_amd import binding
    return Spec("dff_rmsd_matrix", {"x": (to_dev(synth_chain_frames(N_ENS, N, 41)), float("nan")), "y": (to_dev(synth_chain_frames(N_ENS, N, 42)), float("nan"))},
                {"out": ((N_ENS, N_ENS), torch.float32)},
                lambda _, b: raw("dff_rmsd_matrix", 0, ptr(b["x"]), N_ENS, ptr(b["y"]), N_ENS, N, ptr(b["out"]), stream_of(b["x"])),
                wrap=lambda _, b: {"out": binding.rmsd_matrix(b["x"], b["y"])})


def rmsd_nearest_spec(N, exclude_self):
    """exclude_self: the candidates ARE the queries (self_first = 0) -- without the exclusion every query would find itself."""
    from dff_amd import binding
    x = synth_chain_frames(N_ENS, N, 41)
    y = x if exclude_self else synth_chain_frames(N_ENS, N, 42)
    sf = 0 if exclude_self else -1
    ws = torch.empty(max(binding.rmsd_nearest_workspace_bytes(N_ENS, N_ENS, N), 1), dtype=torch.uint8, device="cuda")

    def wrap(_, b):
        r, i = binding.rmsd_nearest(b["x"], b["y"], self_first=sf)
        return {"rmsd": r, "index": i}
    return Spec("dff_rmsd_nearest", {"x": (to_dev(x), float("nan")), "y": (to_dev(y), float("nan"))},
                {"rmsd": ((N_ENS,), torch.float32), "index": ((N_ENS,), torch.int64)},
                lambda _, b: raw("dff_rmsd_nearest", 0, ptr(b["x"]), N_ENS, ptr(b["y"]), N_ENS, N, sf, ptr(b["rmsd"]), ptr(b["index"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["x"])),
                work={"ws": ws}, wrap=wrap)


@beads_param
@pytest.mark.parametrize("make", [pwd_max_spec, pwd_hist_spec, struct_rmsd_spec, struct_dihedrals_spec, struct_tic_spec,
                                  struct_contacts_spec, struct_tic_features_spec, struct_tic_assign_spec, rmsd_matrix_spec],
                         ids=lambda f: f.__name__[:-5])
def test_analysis_call(make, N, gate, side):
    ref = analysis_call(make(N), gate, side)
    if make is pwd_hist_spec:          # every structure lands in a bin of every pair (or beyond hmax): the real input was read
        assert 0 < int(ref["hist"].sum()) <= N_FRAMES * ref["hist"].shape[0]
        assert int(ref["hist"][:, -2:].abs().sum()) == 0            # the columns between max_bins and ld are zeroed too
    if make is struct_tic_assign_spec:
        assert sorted(ref["labels"].unique().tolist()) == [0, 1, 2, 3]


@beads_param
@pytest.mark.parametrize("exclude_self", [False, True], ids=["all-candidates", "exclude-self"])
def test_rmsd_nearest(N, exclude_self, gate, side):
    ref = analysis_call(rmsd_nearest_spec(N, exclude_self), gate, side)
    idx = ref["index"].cpu().numpy()
    assert (idx >= 0).all() and (idx < N_ENS).all()
    if exclude_self:
        assert (idx != np.arange(N_ENS)).all() and float(ref["rmsd"].min()) > 0


def test_kmeans_step(gate, side):
    ref = analysis_call(kmeans_step_spec(), gate, side)
    assert int(ref["counts"].sum()) == N_FRAMES


def test_transition_counts(gate, side):
    ref = analysis_call(transition_counts_spec(), gate, side)
    assert 0 < int(ref["counts"][0].sum()) < N_FRAMES - 3


@pytest.mark.parametrize("N,lengths,lag,chunks", [
    (56, [1000] + [50] * 1000 + [1000], 100, 2),        # the smaller multi-chunk case of tests/test_tica_fit.py: C = 42 112
    (10, [600, 400], 10, 1),
], ids=["two-chunks", "one-chunk"])
def test_tica_moments(N, lengths, lag, chunks, gate, side):
    from dff_amd import binding
    k = len(np.unique(binding.tica_debug_plan(N, lengths, lag)[:, 0]))
    assert k >= 2 if chunks == 2 else k == 1
    analysis_call(tica_moments_spec(N, lengths, lag), gate, side)


# ------------------------------------------------------------------------------------------------ the analysis calls, fenced
def _fence(spec):
    """Both patterns at both placements (tests/fence.py) against one reference."""
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)
    return ref


fence_beads_param = pytest.mark.parametrize("N", [10, 35, 61])       # 61: 183 floats per frame, a partial quad at every tile's end


@fence_beads_param
@pytest.mark.parametrize("make", [pwd_max_spec, pwd_hist_spec, struct_rmsd_spec, struct_dihedrals_spec, struct_tic_spec,
                                  struct_contacts_spec, struct_tic_features_spec, struct_tic_assign_spec, rmsd_matrix_spec],
                         ids=lambda f: f.__name__[:-5])
def test_fence_analysis_call(make, N):
    """1000 frames against 64-frame tiles (257 structures for the RMSD matrix).  Under "tight" the coordinates sit at 4 mod 16:
    the tile loads take their scalar path, under "natural" the 16-byte one -- the same bits."""
    _fence(make(N))


@fence_beads_param
@pytest.mark.parametrize("exclude_self", [False, True], ids=["all-candidates", "exclude-self"])
def test_fence_rmsd_nearest(N, exclude_self):
    _fence(rmsd_nearest_spec(N, exclude_self))


def test_fence_kmeans_step():
    _fence(kmeans_step_spec())


def test_fence_transition_counts():
    _fence(transition_counts_spec())


@pytest.mark.parametrize("N,lengths,lag,chunks", [
    (56, [1000] + [50] * 1000 + [1000], 100, 2),
    (10, [600, 400], 10, 1),
], ids=["two-chunks", "one-chunk"])
def test_fence_tica_moments(N, lengths, lag, chunks):
    """The workspace (features of a chunk, the slices' partial matrices and sums) at exactly dff_tica_workspace_bytes; the
    accumulators are added to, so they are results as well."""
    _fence(tica_moments_spec(N, lengths, lag))


# ------------------------------------------------------------------------------------------------ two streams at once
def _two_at_once(specs, nats, gate, tag):
    """Two calls issued back to back on two side streams, each behind its own gate, nothing synchronised in between: each equals
    its serial result (no hidden process-wide device state)."""
    refs = [reference(sp, nat) for sp, nat in zip(specs, nats)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = [Run(sp, nat) for sp, nat in zip(specs, nats)]
    torch.cuda.synchronize()
    for run, st in zip(runs, streams):
        run.enqueue(st, gate)
    both_gated = not runs[0].ev_gate.query() and not runs[1].ev_gate.query()
    for run, st, ref in zip(runs, streams, refs):
        run.check(st, ref, True, tag)
    assert both_gated, "the second call was issued only after the first stream's gate had finished"


def test_two_stateless_calls_on_two_streams(gate):
    _two_at_once([struct_rmsd_spec(10), pwd_hist_spec(35)], [None, None], gate, " [two streams]")


def test_two_models_on_two_streams(gate):
    cases = [CASES[0], CASES[3]]                         # chignolin (<= 16-row kernel), trp-cage (two workgroups per protein)
    nats = [shared_native(c.model) for c in cases]
    specs = [langevin_spec(c, False) for c in cases]
    for sp, nat in zip(specs, nats):                      # warm both (default knobs)
        reference(sp, nat)
    _two_at_once(specs, nats, gate, " [two models]")
    assert S16 in nats[0].last_launch()[0] and "pair" in nats[1].last_launch()[0]
    assert nats[0].status() == 0 and nats[1].status() == 0
