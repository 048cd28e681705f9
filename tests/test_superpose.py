"""dff_superpose on the GPU against the float64 oracle superpose64 of oracle/struct_metric.py (batched Kabsch by SVD with the
reflection fix; the eigenvalues of Horn's key matrix by numpy.linalg.eigvalsh).

What is compared how:
- STRICT, on frames whose relative eigenvalue gap (l1 - l2) / (l1 - l4) is >= 1e-2 (below it the rotation itself is
  ill-conditioned; at most 2 % of a data set may be excluded, asserted):
    aligned  |got - oracle| <= 2^-23 max |oracle value of that frame|: one fp32 rounding (2^-24 relative) with a factor 2;
             the fp64 rotation error at that gap is ~ 2^-52 / 1e-2 and negligible
    rot      <= 1e-9 per entry, four orders above that estimate
- on EVERY finite frame, degenerate ones included:
    rot      |R^T R - I| <= 1e-12 and |det R - 1| <= 1e-12
    rmsd     RMSD_ATOL, RMSD_RTOL of tests/support.py against the oracle
    the plain, unrotated fp64 RMSD of the returned aligned frame to the reference is the oracle's minimal RMSD within that
    same bar plus 2^-23 max |coordinate| (the fp32 rounding of the frame)
- dsum, dsq <= 1e-10 sum_frames |term| on data sets without an excluded frame (fp64 summation, n 2^-53 at n <= 2^19, and the
  rotation error are both below 1e-12 of that); count exact.
"""
import numpy as np
import pytest
import torch

from oracle.frames import gaussian, half_turn, noisy_ensemble, rand_rot, synth_chain_frames
from oracle.struct_metric import stats64, superpose64
from fence import COMBINATIONS, fenced
from stream_gate import N_FRAMES, Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import GAP_MIN, MAX_EXCLUDED, MIRROR, RMSD_ATOL, RMSD_RTOL, B, dev, golden_frames, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def run(x, ref, **kw):
    """binding.superpose with every output -> dict of host arrays"""
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda")
    res = B().superpose(xd, np.asarray(ref, np.float32), rot=True, rmsd=True, stats=True, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def check(got, x, ref, what, strict_all=False, stats=False):
    """the comparisons of the module docstring; strict_all: no frame may fall below the gap; stats: compare dsum / dsq"""
    o = superpose64(x, ref)
    fin, N = o["finite"], np.asarray(x).shape[1]
    r64 = np.asarray(ref, np.float32).astype(np.float64)
    # non-finite frames: NaN rows, not counted
    for k in ("aligned", "rot", "rmsd"):
        assert np.isnan(got[k][~fin]).all(), f"{what}: {k} of a non-finite frame is not NaN"
        assert np.isfinite(got[k][fin]).all(), f"{what}: {k} of a finite frame is not finite"
    assert int(got["count"][0]) == int(fin.sum()), what
    if not fin.any():
        return o
    R, al = got["rot"][fin], got["aligned"][fin].astype(np.float64)
    # every finite frame: a proper rotation, the minimal RMSD, and an aligned frame that reaches it
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max()
    det = np.abs(np.linalg.det(R) - 1).max()
    want = o["rmsd"][fin]
    e_rmsd = np.abs(got["rmsd"][fin] - want)
    bar = RMSD_ATOL + RMSD_RTOL * want
    plain = np.sqrt(((al - r64) ** 2).sum((1, 2)) / N)
    e_plain = np.abs(plain - want)
    bar_plain = bar + EPS32 * np.abs(o["aligned"][fin]).max((1, 2))
    print(f"[superpose] {what}: {fin.sum()} finite frames, |R^T R - I| {orth:.2e}, |det - 1| {det:.2e}, rmsd err {e_rmsd.max():.2e}, "
          f"plain-RMSD err {e_plain.max():.2e} (bar {bar_plain.min():.2e})")
    assert orth <= 1e-12 and det <= 1e-12, what
    assert np.all(e_rmsd <= bar), f"{what}: rmsd off by {e_rmsd.max():.3e}"
    assert np.all(e_plain <= bar_plain), f"{what}: the aligned frame misses the minimal RMSD by {e_plain.max():.3e}"
    # strict, on well-conditioned frames
    ok = o["gap"][fin] >= GAP_MIN
    excluded = 1.0 - ok.mean()
    assert excluded <= MAX_EXCLUDED, f"{what}: {excluded:.2%} of the frames below the gap"
    if strict_all:
        assert ok.all(), f"{what}: {(~ok).sum()} frames below the gap"
    if ok.any():
        e_rot = np.abs(R[ok] - o["R"][fin][ok]).max()
        e_al = np.abs(al[ok] - o["aligned"][fin][ok]).max((1, 2))
        bar_al = EPS32 * np.abs(o["aligned"][fin][ok]).max((1, 2))
        print(f"[superpose] {what}: {ok.sum()} strict frames ({excluded:.3%} excluded), rot err {e_rot:.2e}, "
              f"aligned err / bar {np.max(e_al / bar_al):.3f}")
        assert e_rot <= 1e-9, f"{what}: rot off by {e_rot:.3e}"
        assert np.all(e_al <= bar_al), f"{what}: aligned off by {np.max(e_al / bar_al):.3f} bars"
    if stats:
        assert ok.all(), f"{what}: statistics are compared on sets without an excluded frame"
        dsum, dsq, _, dabs = stats64(o, ref)
        e1, e2 = np.abs(got["dsum"] - dsum) / dabs, np.abs(got["dsq"] - dsq) / dsq
        print(f"[superpose] {what}: dsum err / sum |d| {e1.max():.2e}, dsq err / dsq {e2.max():.2e}")
        assert e1.max() <= 1e-10 and e2.max() <= 1e-10, what
    return o


# ---------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("mol", ["chignolin", "villin", "protein_g", "ala2"])
def test_goldens(dev, golden, mol):
    x, f = golden_frames(golden, mol)
    o = check(run(x, f), x, f, mol, strict_all=mol != "ala2", stats=mol != "ala2")
    if mol != "ala2":
        assert (~o["finite"]).sum() > 0             # the goldens' injected non-finite frames came back as NaN rows


# ---------------------------------------------------------------- 2. bead counts and frame counts
@pytest.mark.parametrize("N", [4, 64])
def test_bead_count_limits_and_ragged_tiles(dev, N):
    rng = np.random.default_rng(4000 + N)
    x, ref = gaussian(rng, 3000, N)
    check(run(x, ref), x, ref, f"N={N} gaussian")
    for n in (1, 63, 64, 65, 129):
        got = run(x[:n], ref)
        o = superpose64(x[:n], ref)
        assert int(got["count"][0]) == n
        ok = o["gap"] >= GAP_MIN
        assert np.all(np.abs(got["aligned"] - o["aligned"])[ok] <= EPS32 * np.abs(o["aligned"][ok]).max((1, 2))[:, None, None]), n
        assert np.abs(got["rot"] - o["R"])[ok].max() <= 1e-9 and np.all(np.abs(got["rmsd"] - o["rmsd"]) <= RMSD_ATOL + RMSD_RTOL * o["rmsd"])
        # one lane computes one frame: its value does not depend on the tile or the lane that handles it
        full = run(x[:200], ref)
        for k in ("aligned", "rot", "rmsd"):
            assert np.array_equal(got[k], full[k][:n]), (n, k)


def test_grid_stride(dev, golden):
    """more tiles than workgroups (the cap follows from the size of the workspace: one slice of 4 N + 1 doubles per
    workgroup), the last tile ragged; a well-conditioned ensemble, so that the statistics are compared as well"""
    b = B()
    N = 10
    cap = b.superpose_workspace_bytes(1 << 36, N) // (8 * (4 * N + 1))
    assert b.superpose_workspace_bytes(64 * cap, N) == b.superpose_workspace_bytes(64 * (cap + 1), N)
    n = 64 * (cap + 2) + 37
    rng = np.random.default_rng(77)
    f = golden("struct_folded.npz")["chignolin"].astype(np.float64)
    x = (f + rng.standard_normal((n, N, 3))).astype(np.float32)
    x = np.einsum("nij,nbj->nbi", np.stack([rand_rot(rng) for _ in range(64)])[rng.integers(64, size=n)], x).astype(np.float32)
    x[[5, 64 * cap + 3, n - 1], 2, 1] = np.nan
    xd = torch.from_numpy(x).to(dev)
    got = run(xd, f)
    check(got, x, f, f"grid stride, {n} frames on {cap} workgroups", strict_all=True, stats=True)
    for sl in (slice(0, 64 * 11 + 13), slice(n - 64 * 11 - 29, n)):
        sub = run(xd[sl].clone(), f)
        for k in ("aligned", "rot", "rmsd"):
            assert np.array_equal(sub[k], got[k][sl], equal_nan=True), k


@pytest.mark.parametrize("N", [3, 65])
def test_bead_count_out_of_range_refused(dev, N):
    x = torch.ones((70, N, 3), device=dev)
    with pytest.raises(ValueError, match="n_beads"):
        B().superpose(x, np.zeros((N, 3), np.float32))
    with pytest.raises(ValueError, match="n_beads"):
        B().superpose_workspace_bytes(70, N)


# ---------------------------------------------------------------- 3. exact rotations
@pytest.mark.parametrize("mol", ["chignolin", "protein_g"])
def test_exact_rotations(dev, golden, mol):
    f = golden("struct_folded.npz")[mol].astype(np.float32)
    f64 = f.astype(np.float64)
    rng = np.random.default_rng(len(f))
    shift = np.array([3.0, -2.0, 7.0])
    Rs = [half_turn(a) for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1], rng.standard_normal(3))] + [np.eye(3), rand_rot(rng)]
    x = np.stack([f64 @ R.T + (0.0 if i == 4 else shift) for i, R in enumerate(Rs)]).astype(np.float32)
    got = run(x, f)
    o = check(got, x, f, f"{mol} exact rotations", strict_all=True)          # half turns (q0 = 0) are well-conditioned
    # the frames are R_s f: the rotation back is R_s^T (to the fp32 rounding of the frames: 2^-24 relative per coordinate)
    for s, R in enumerate(Rs):
        assert np.abs(got["rot"][s] - R.T).max() <= 1e-5, s
    assert np.abs(got["rot"][4] - np.eye(3)).max() <= 1e-9 and got["rmsd"][4] <= RMSD_ATOL
    assert np.all(got["rmsd"] <= RMSD_ATOL + 1e-6 * np.abs(f).max() * 4)     # rigid copies, fp32-rounded


# ---------------------------------------------------------------- 4. degenerate frames: invariants only
@pytest.mark.parametrize("N", [4, 10, 64])
def test_degenerate_frames(dev, N):
    rng = np.random.default_rng(6000 + N)
    ref = (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    chain = np.stack([(np.arange(N) - (N - 1) / 2) * 3.8, np.zeros(N), np.zeros(N)], 1)
    plane = rng.standard_normal((N, 3)) * 5 * np.array([1.0, 1.0, 0.0])
    point = np.tile(np.array([[1.5, -2.0, 3.25]]), (N, 1))
    frames = [chain, chain @ rand_rot(rng).T + 3.0, plane, plane @ rand_rot(rng).T, point, ref * MIRROR,
              (ref * MIRROR) @ rand_rot(rng).T, ref + 1e4, ref @ rand_rot(rng).T + 1e4]
    x = np.stack(frames).astype(np.float32)
    for r, name in ((ref, "compact"), (chain.astype(np.float32), "straight-chain"), (point.astype(np.float32), "coincident")):
        got = run(x, r)
        o = superpose64(x, r)
        fin = np.ones(len(x), bool)
        # invariants of check() without the gap filter's share (these sets are degenerate on purpose)
        R, al = got["rot"], got["aligned"].astype(np.float64)
        assert np.isfinite(R).all() and np.isfinite(al).all() and int(got["count"][0]) == len(x)
        assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 1e-12
        assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
        bar = RMSD_ATOL + RMSD_RTOL * o["rmsd"]
        assert np.all(np.abs(got["rmsd"] - o["rmsd"]) <= bar), (name, np.abs(got["rmsd"] - o["rmsd"]).max())
        plain = np.sqrt(((al - r.astype(np.float64)) ** 2).sum((1, 2)) / N)
        e = np.abs(plain - o["rmsd"])
        print(f"[superpose] N={N} {name} reference: plain-RMSD err {e.max():.2e}, rmsd {o['rmsd'].round(3)}")
        assert np.all(e <= bar + EPS32 * np.abs(o["aligned"]).max((1, 2))), (name, e.max())
        assert fin.all()
    # the mirror image stays a mirror image: a proper rotation cannot match it
    got = run(x[5:7], ref)
    assert np.all(got["rmsd"] > 0.5) and np.all(np.linalg.det(got["rot"]) > 0)


# ---------------------------------------------------------------- 5. memory paths
@pytest.mark.parametrize("N", [4, 10, 13, 64])
def test_in_place_and_unaligned_views_bit_equal(dev, N):
    b = B()
    rng = np.random.default_rng(7000 + N)
    ref = (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    for n in (1, 63, 129, 1000):
        flat = torch.from_numpy((rng.standard_normal(n * 3 * N + 4) * 5).astype(np.float32)).to(dev)
        al = flat[:n * 3 * N].view(n, N, 3).clone()
        want = b.superpose(al, ref, rot=True, rmsd=True, stats=True)
        # in place: aligned_dev == x_dev
        x2 = al.clone()
        res = b.superpose(x2, ref, out=x2)
        assert res["aligned"].data_ptr() == x2.data_ptr() and torch.equal(x2, want["aligned"]), (n, "in place")
        # an unaligned contiguous view, as input and as output: the scalar tile-load / tile-store paths
        for k in (1, 2, 3):
            src = torch.empty(n * 3 * N + 4, device=dev)
            v = src[k:k + n * 3 * N].view(n, N, 3)
            v.copy_(al)
            out = torch.empty(n * 3 * N + 4, device=dev)[k:k + n * 3 * N].view(n, N, 3)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k and out.data_ptr() % 16 == 4 * k
            got = b.superpose(v, ref, rot=True, rmsd=True, stats=True, out=out)
            for key in want:
                assert torch.equal(got[key], want[key]), (n, k, key)
            b.superpose(v, ref, out=v)
            assert torch.equal(v, want["aligned"]), (n, k, "in place, unaligned")


# ---------------------------------------------------------------- 6. optional outputs
def superpose_raw(x, n, N, ref, aligned=None, rot=None, rmsd=None, dsum=None, dsq=None, count=None, ws=None, ws_bytes=None):
    raw("dff_superpose", 0, ptr(x), n, N, ptr(ref), ptr(aligned), ptr(rot), ptr(rmsd), ptr(dsum), ptr(dsq), ptr(count), ptr(ws),
        (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes, stream_of(ref))


def test_optional_outputs(dev):
    b = B()
    rng = np.random.default_rng(8000)
    n, N = 333, 35
    x, ref = gaussian(rng, n, N)
    x[17, 3, 0] = np.inf
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    want = b.superpose(xd, rd, rot=True, rmsd=True, stats=True)
    need = b.superpose_workspace_bytes(n, N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def fresh():
        return {"aligned": torch.full((n, N, 3), 123.0, device=dev), "rot": torch.full((n, 3, 3), 123.0, dtype=torch.float64, device=dev),
                "rmsd": torch.full((n,), 123.0, device=dev), "dsum": torch.full((N, 3), 123.0, dtype=torch.float64, device=dev),
                "dsq": torch.full((N,), 123.0, dtype=torch.float64, device=dev),
                "count": torch.full((1,), 123, dtype=torch.int64, device=dev)}
    # each output alone (the statistics need the workspace), statistics without aligned frames, everything
    for keys in (["aligned"], ["rot"], ["rmsd"], ["dsum"], ["dsq"], ["count"], ["dsum", "dsq", "count"], list(want)):
        bufs = fresh()
        st = any(k in keys for k in ("dsum", "dsq", "count"))
        superpose_raw(xd, n, N, rd, ws=ws if st else None, **{k: bufs[k] for k in keys})
        for k, v in bufs.items():
            if k in keys:
                assert torch.equal(v, want[k]) or (torch.equal(torch.isnan(v), torch.isnan(want[k])) and
                                                   torch.equal(torch.nan_to_num(v), torch.nan_to_num(want[k]))), (keys, k)
            else:
                assert bool((v == 123).all()), (keys, k)
    assert int(want["count"]) == n - 1 and torch.isnan(want["aligned"][17]).all() and torch.isnan(want["rmsd"][17])
    # no output at all: a no-op
    superpose_raw(xd, n, N, rd)
    # n == 0 zeroes the statistics (and needs no workspace)
    bufs = fresh()
    superpose_raw(xd, 0, N, rd, dsum=bufs["dsum"], dsq=bufs["dsq"], count=bufs["count"])
    assert not bufs["dsum"].any() and not bufs["dsq"].any() and int(bufs["count"]) == 0
    # a workspace one byte too small, or none, is refused; the outputs stay untouched
    bufs = fresh()
    for kw in (dict(ws=ws, ws_bytes=need - 1), dict(ws=None)):
        with pytest.raises(ValueError, match="workspace"):
            superpose_raw(xd, n, N, rd, dsum=bufs["dsum"], **kw)
    torch.cuda.synchronize()
    assert bool((bufs["dsum"] == 123).all())
    # two identical calls, the workspace dirty from other work in between: bit-identical statistics
    ws.fill_(0x7B)
    again = b.superpose(xd, rd, aligned=False, stats=True, workspace=ws)
    for k in ("dsum", "dsq", "count"):
        assert torch.equal(again[k], want[k]), k
    # a non-finite reference makes every frame a non-finite frame
    bad = rd.clone()
    bad[N - 1, 2] = float("nan")
    res = b.superpose(xd, bad, rot=True, rmsd=True, stats=True)
    assert torch.isnan(res["aligned"]).all() and torch.isnan(res["rot"]).all() and torch.isnan(res["rmsd"]).all()
    assert int(res["count"]) == 0 and not res["dsum"].any() and not res["dsq"].any()


def test_rmsd_is_the_quantity_of_struct_rmsd(dev, golden):
    x, f = golden_frames(golden, "villin")
    xd = torch.from_numpy(x).to(dev)
    a = B().superpose(xd, f, aligned=False, rmsd=True)["rmsd"].cpu().numpy().astype(np.float64)
    s = B().struct_rmsd(xd, f).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(s))
    ok = ~np.isnan(s)
    assert np.all(np.abs(a[ok] - s[ok]) <= RMSD_ATOL + RMSD_RTOL * s[ok])


# ---------------------------------------------------------------- 7. the Python layer
def test_evaluate_superpose_chunked(dev, golden):
    from dff_amd import evaluate
    x, f = golden_frames(golden, "villin")
    whole, rot = evaluate.superpose(x, f, return_rotations=True)
    assert whole.shape == x.shape and whole.dtype == torch.float32 and rot.shape == (len(x), 3, 3)
    for chunk in (100, 257, 1023):
        part, prot = evaluate.superpose(torch.from_numpy(x), f, return_rotations=True, chunk=chunk)
        assert torch.equal(torch.nan_to_num(part), torch.nan_to_num(whole)) and torch.equal(torch.isnan(part), torch.isnan(whole))
        assert torch.equal(torch.nan_to_num(prot), torch.nan_to_num(rot))
    o = superpose64(x, f)
    dsum, dsq, count, dabs = stats64(o, f)
    for chunk in (None, 300):
        g1, g2, c = evaluate.superpose_stats(x, f, chunk=chunk)
        assert c == count
        assert (np.abs(g1 - dsum) / dabs).max() <= 1e-10 and (np.abs(g2 - dsq) / dsq).max() <= 1e-10, chunk


@pytest.mark.parametrize("mol", ["chignolin", "protein_g"])
def test_rmsf_and_flexibility_evaluator(dev, golden, mol):
    from dff_amd import evaluate
    x, f = golden_frames(golden, mol)
    samples, refs = x[: len(x) // 2], x[len(x) // 2:]
    prof = {}
    for name, part in (("samples", samples), ("refs", refs)):
        o = superpose64(part, f)
        dsum, dsq, count, _ = stats64(o, f)
        prof[name] = (evaluate.rmsf_from_sums(dsum, dsq, count), f.astype(np.float64) + dsum / count)
        got = evaluate.rmsf(part, f)
        print(f"[superpose] {mol} {name}: rmsf err {np.abs(got - prof[name][0]).max():.2e} A")
        assert np.abs(got - prof[name][0]).max() <= 1e-6
    ev = evaluate.FlexibilityEvaluator(refs, mol, folded=f)
    r = ev.eval(samples)
    want = evaluate.FlexibilityEvaluator.summarize(prof["samples"][0], prof["refs"][0], prof["samples"][1], prof["refs"][1],
                                                   int((~np.isfinite(samples).all((1, 2))).sum()),
                                                   int((~np.isfinite(refs).all((1, 2))).sum()))
    assert set(r) == set(want)
    for k in want:
        assert r[k] == pytest.approx(want[k], abs=1e-6), k
    assert np.abs(ev.profiles["samples"]["rmsf"] - prof["samples"][0]).max() <= 1e-6
    assert np.abs(ev.profiles["refs"]["mean"] - prof["refs"][1]).max() <= 1e-6
    # without a folded structure both ensembles are aligned on the reference data's mean structure
    ev2 = evaluate.FlexibilityEvaluator(refs, mol)
    assert evaluate.kabsch_rmsd64(ev2.align_on, prof["refs"][1]) < 1.0 and np.isfinite(list(ev2.eval(samples).values())).all()


def test_mean_structure_on_a_synthetic_ensemble(dev):
    """the assertion of test_superpose_host.py::test_mean_structure_converges_to_the_template, on the GPU"""
    from dff_amd import evaluate
    sigma, n = 0.3, 2048
    rng = np.random.default_rng(2048)
    template = rng.standard_normal((10, 3)) * 4
    x = noisy_ensemble(rng, template, n, sigma)
    mean, n_iter = evaluate.mean_structure(x)
    d = evaluate.kabsch_rmsd64(mean, template)
    print(f"[superpose] mean structure after {n_iter} passes: {d / sigma:.4f} sigma from the template")
    assert 1 <= n_iter <= 10 and d <= 0.1 * sigma
    prof = evaluate.rmsf(x, "mean")
    assert prof.shape == (10,) and np.all(prof > 0.6 * sigma * np.sqrt(3)) and np.all(prof < 1.1 * sigma * np.sqrt(3))


# ---------------------------------------------------------------- 8. stream order
def superpose_spec(N):
    b = B()
    n = N_FRAMES
    ref = synth_chain_frames(1, N, 51)[0]
    ws = torch.empty(b.superpose_workspace_bytes(n, N), dtype=torch.uint8, device="cuda")

    def wrap(_, bufs):
        return b.superpose(bufs["x"], bufs["ref"], rot=True, rmsd=True, stats=True)
    return Spec("dff_superpose", {"x": (to_dev(synth_chain_frames(n, N, 52)), float("nan")), "ref": (to_dev(ref), to_dev(ref * 0.5 + 1.0))},
                {"aligned": ((n, N, 3), torch.float32), "rot": ((n, 3, 3), torch.float64), "rmsd": ((n,), torch.float32),
                 "dsum": ((N, 3), torch.float64), "dsq": ((N,), torch.float64), "count": ((1,), torch.int64)},
                lambda _, bufs: raw("dff_superpose", 0, ptr(bufs["x"]), n, N, ptr(bufs["ref"]), ptr(bufs["aligned"]), ptr(bufs["rot"]),
                                    ptr(bufs["rmsd"]), ptr(bufs["dsum"]), ptr(bufs["dsq"]), ptr(bufs["count"]), ptr(bufs["ws"]),
                                    bufs["ws"].numel(), stream_of(bufs["x"])),
                work={"ws": ws}, wrap=wrap)


@pytest.mark.parametrize("N", [10, 35])
def test_stream_order(N, gate, side):  # noqa: F811
    ref = analysis_call(superpose_spec(N), gate, side)
    assert int(ref["count"]) == N_FRAMES and bool(torch.isfinite(ref["aligned"]).all())


@pytest.mark.parametrize("N", [10, 35, 61])
def test_fence(N):
    """The memory contract (tests/fence.py): all nine buffers in one arena, the workspace at exactly
    dff_superpose_workspace_bytes.  Under "tight" x and aligned sit at 4 mod 16: the tile load and the tile store take their
    scalar paths (N = 61: 183 floats per frame, a partial quad at every tile's end under "natural")."""
    spec = superpose_spec(N)
    ref = reference(spec)
    for pattern, placement in COMBINATIONS:
        fenced(spec, pattern=pattern, placement=placement, ref=ref)
