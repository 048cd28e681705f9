"""The kernel-variant matrix the GPU tests of the sampler updates share (a helper, not a test): the synthetic models, one
live native model per name, the subset of a batch the oracles run on, and CASES -- every kernel variant that runs an update (both kernels, 4 and 8 waves, groups with
a ragged tail, batches cut into three launches, one and two workgroups per protein, the general-input branch, the force
head, hidden 256), each with the knobs that select it and the assertion that it is the kernel that ran.  A score call selects the
same kernels (selection does not depend on the mode): tests/test_score_energy.py runs the matrix on dff_score's energies.  Also the
three lists of odd sizes that the force and the energy tests of dff_score share."""
import contextlib

from oracle import synth

HI = 2 ** 32

# name -> (N, H, L, flags (intrinsic, distances, abs), conservative, weight seed)
MODELS = {
    "ala2": (5, 96, 2, (1, 0, 0), True, 1234),
    "chignolin": (10, 64, 3, (1, 0, 0), True, 1234),
    "n14": (14, 64, 2, (1, 0, 0), True, 1414),             # 14 rows on four waves: no idle wave, the update draws in line
    "trp_cage": (20, 128, 3, (1, 0, 0), True, 1234),
    "villin": (35, 128, 3, (1, 0, 0), True, 1234),
    "protein_g": (56, 128, 3, (1, 0, 0), True, 1234),
    "h256": (20, 256, 2, (1, 0, 0), True, 2580),
    "chignolin_gen": (10, 64, 3, (0, 1, 1), True, 2468),
    "trp_cage_gen": (20, 128, 3, (0, 1, 1), True, 2468),
    "chignolin_nc": (10, 64, 3, (1, 0, 0), False, 4321),
    "trp_cage_nc": (20, 128, 3, (1, 0, 0), False, 4321),
}
_models, _params = {}, {}


def params(name):
    """The synthetic parameter dict of a model (no GPU needed): what get_native loads, for the twin to run the same weights."""
    if name not in _params:
        N, H, L, (intr, dist, ab), cons, wseed = MODELS[name]
        # real (seeded) weights at full decoder scale: the production kernel variants run, the fp16 engine stays engaged
        _params[name] = synth.synth_gnn_params(N, H, L, seed=wseed, decoder_out=1 if cons else 3, node_in=N + 1 + 3 * ab,
                                               edge_in=(3 * intr + dist) or 1)
    return _params[name]


def get_native(name):
    import torch
    if name not in _models:
        from dff_amd.score import GraphTransformer
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        N, H, L, (intr, dist, ab), cons, wseed = MODELS[name]
        _models[name] = GraphTransformer(N, H, device="cuda:0", n_layers=L, use_intrinsic_coords=bool(intr), use_abs_coords=bool(ab),
                                         use_distances=bool(dist), conservative=cons, state_dict=params(name))
    return _models[name].native


class Case:
    def __init__(self, cid, model, B, has, lacks=(), xi_pre=None, group=0, waves=0, generic=False, pair=True, max_wgs=2048,
                 last_grid=None, offset=0, step_offset=0):
        self.id, self.model, self.B, self.has, self.lacks, self.xi_pre = cid, model, B, has, lacks, xi_pre
        self.group, self.waves, self.generic, self.pair, self.max_wgs, self.last_grid = group, waves, generic, pair, max_wgs, last_grid
        self.offset, self.step_offset = offset, step_offset
        self.N = MODELS[model][0]

    @contextlib.contextmanager
    def knobs(self):
        nat = get_native(self.model)
        try:
            nat.set_group(self.group); nat.small_waves(self.waves); nat.force_generic(self.generic)
            nat.pair(self.pair); nat.max_workgroups(self.max_wgs)
            yield nat
        finally:
            nat.set_group(0); nat.small_waves(0); nat.force_generic(False); nat.pair(True); nat.max_workgroups(2048)

    def check_launch(self, nat):
        """The kernel this case exists for did run (and, for a batch cut into launches, the last launch's grid)."""
        name, grid, _ = nat.last_launch()
        assert all(h in name for h in self.has) and not any(l in name for l in self.lacks), (self.id, name)
        if self.xi_pre is not None:     # the <= 16-row kernel pre-draws iff  rows * lanes-per-row <= (waves - 1) * 64  (dff_small.hip)
            assert "dff_small_kernel<" in name
            nw = 4 if ("pair" in name or name.split(",")[1].rstrip(">") == "4") else 8
            G = self.group if self.group else 1
            assert (min(G, self.B) * self.N * (32 if nw == 8 else 16) <= (nw - 1) * 64) == self.xi_pre, (self.id, name)
        if self.last_grid is not None:
            assert grid == self.last_grid, (self.id, grid)
        return name


def subset(case):
    """The trajectories of a case's batch an oracle runs on: first and last, both sides of every launch boundary (max_wgs G),
    and both sides of the group boundary nearest the middle of the batch (which serves as the trajectory in the middle); the
    middle one of a one-group batch."""
    B, G = case.B, case.group if case.group else 1
    idx = {0, B - 1}
    for b in range(case.max_wgs * G, B, case.max_wgs * G):
        idx |= {b - 1, b}
    n_groups = -(-B // G)
    if n_groups > 1:
        k = G * min(max(int(round(B / 2 / G)), 1), n_groups - 1)
        idx |= {k - 1, k}
    else:
        idx.add(B // 2)
    idx = tuple(sorted(idx))
    assert len(idx) <= (4 if case.N >= 35 else 8), (case.id, idx)
    return idx


# ---- the odd sizes: the smallest shapes at which tile tails, pad rows and group offsets exist (the forces:
# tests/test_gpu_parity.py, the energies: tests/test_score_energy.py)
ODD_FOUR_ROW_TILES = [49, 53, 56, 57, 60, 61]                                  # N at hidden 128, two layers
ODD_TWO_AND_THREE_ROW_TILES = [(128, 17), (128, 23), (128, 32), (128, 33), (128, 41), (128, 45), (128, 48), (96, 17), (96, 26),
                               (96, 32), (64, 17), (64, 31)]                   # (H, N)
ODD_SMALL_MODELS = [(64, 2, 1), (64, 3, 5), (64, 7, 2), (64, 11, 1), (64, 13, 1), (64, 16, 1), (96, 2, 8), (96, 9, 1), (96, 16, 1),
                    (128, 4, 4), (128, 10, 1), (128, 15, 1), (256, 2, 1), (256, 16, 1), (256, 17, 1), (256, 32, 1)]   # (H, N, G)


def odd_params(H, N, which):
    """The seeded weights of an odd-size model (decoder scale 1): `which` 4 = the four-row-tile list, 2 = two and three row
    tiles, 1 = the small models -- the seeds tests/test_gpu_parity.py has always used for them."""
    return synth.synth_gnn_params(N, H, 2, seed={4: 4000 + N, 2: 5000 + N + H, 1: 6000 + N + H}[which])


S16, S64 = "dff_small_kernel<", "dff_fused_kernel<"
CASES = [
    # ---- the <= 16-row kernel: both sides of the xi_pre condition, 4 and 8 waves, groups, a ragged last group
    Case("chignolin-g1", "chignolin", 12, (S16 + "64,8",), xi_pre=True, offset=0, step_offset=0),
    Case("chignolin-8waves", "chignolin", 5, (S16 + "64,8",), xi_pre=True, waves=8, offset=HI - 3, step_offset=HI + 1),
    Case("chignolin-4waves", "chignolin", 7, (S16 + "64,4",), xi_pre=True, waves=4, offset=7, step_offset=HI - 2),
    Case("n14-fills-the-last-wave", "n14", 9, (S16 + "64,4",), xi_pre=False, offset=HI + 5, step_offset=HI - 2),
    Case("ala2-g1-8waves", "ala2", 6, (S16 + "96,8",), xi_pre=True, waves=8, offset=HI - 3, step_offset=0),
    Case("ala2-g2-8waves-ragged", "ala2", 7, (S16 + "96,8",), xi_pre=True, waves=8, group=2, offset=7, step_offset=HI + 1),
    Case("ala2-g3-4waves-ragged", "ala2", 10, (S16 + "96,4",), xi_pre=False, waves=4, group=3, offset=HI - 3, step_offset=HI - 2),
    Case("chignolin-gen", "chignolin_gen", 6, (S16 + "64,8", "gen"), xi_pre=True, offset=HI + 5, step_offset=0),
    Case("chignolin-force-head", "chignolin_nc", 6, (S16 + "64,8",), xi_pre=True, offset=7, step_offset=HI + 1),
    Case("chignolin-3-launches", "chignolin", 40, (S16 + "64,8",), xi_pre=True, max_wgs=16, last_grid=8, offset=HI - 17, step_offset=0),
    Case("ala2-g3-3-launches", "ala2", 40, (S16 + "96,4",), xi_pre=False, waves=4, group=3, max_wgs=5, last_grid=4, offset=HI - 17,
         step_offset=HI + 1),
    # ---- the <= 64-row kernel: one and two workgroups per protein, the generic kernel on a small config, groups of ala2,
    # hidden 256, a general-input branch, the force head
    Case("ala2-default", "ala2", 9, (S64 + "96,1,",), offset=HI + 5, step_offset=HI - 2),
    Case("ala2-g5-ragged", "ala2", 12, (S64 + "96,2,",), ("pair",), group=5, pair=False, offset=HI - 3, step_offset=0),
    Case("chignolin-generic", "chignolin", 6, (S64 + "64,1,",), ("pair",), generic=True, pair=False, offset=HI - 3, step_offset=HI + 1),
    Case("trp-cage-pair", "trp_cage", 6, (S64 + "128,2,", "pair"), offset=HI - 3, step_offset=HI - 2),
    Case("trp-cage-one", "trp_cage", 6, (S64 + "128,2,",), ("pair",), pair=False, offset=7, step_offset=0),
    Case("villin-pair", "villin", 5, (S64 + "128,3,", "pair"), offset=HI + 5, step_offset=HI + 1),
    Case("villin-one", "villin", 5, (S64 + "128,3,",), ("pair",), pair=False, offset=HI - 3, step_offset=HI - 2),
    Case("protein-g-pair", "protein_g", 4, (S64 + "128,4,", "pair"), offset=HI - 3, step_offset=0),
    Case("protein-g-one", "protein_g", 4, (S64 + "128,4,",), ("pair",), pair=False, offset=0, step_offset=HI + 1),
    Case("hidden-256", "h256", 5, (S64 + "256,",), pair=False, offset=HI - 3, step_offset=HI - 2),
    Case("trp-cage-gen", "trp_cage_gen", 5, (S64 + "128,2,", "gen"), ("pair",), offset=HI - 3, step_offset=HI + 1),
    Case("trp-cage-force-head", "trp_cage_nc", 5, (S64 + "128,2,",), ("pair",), offset=HI + 5, step_offset=0),
    Case("trp-cage-3-launches", "trp_cage", 40, (S64 + "128,2,",), ("pair",), pair=False, max_wgs=16, last_grid=8, offset=HI - 17,
         step_offset=HI - 2),
]
