"""dff_msm_propagate on the GPU (csrc/dff_msm_propagate.hip) and evaluate.msm_propagate / msm_autocorrelation / metastable_sets /
chapman_kolmogorov on top of it.  tests/propagate_cases.py holds the matrices, the longdouble truth, the measure E(s) and its
bar (8 x numpy's own fp64 chain on the same case, floored at one unit, capped by (s + 2) K); the kernel is never its own
reference.

Every size runs all kinds of propagate_cases.kinds in one call with M = 3, R = 4, S = 64, on each path that takes the size; the
figures are printed per case.

MEASURED on the MI355X, worst E over the steps and the kinds of a size, in units, LDS path / streamed path (numpy's fp64 chain on
the same cases), L = 120 the LDS limit; the bar is 8 units or more everywhere except where the cap (s + 2) K is lower:
  K      E LDS / streamed (numpy)
  1      0.00 / 0.00 (0.00)
  2      2.52 / 2.52 (2.52)
  3      12.02 / 12.02 (12.02)
  5      2.09 / 2.09 (2.09)
  16     1.18 / 1.18 (1.35)
  17     0.77 / 0.77 (0.58)
  33     0.51 / 0.51 (0.50)
  64     0.57 / 0.57 (0.53)
  65     1.46 / 1.46 (1.46)
  120    1.40 / 1.40 (1.40)
  121       - / 0.76 (0.76)
  257       - / 0.45 (0.49)
  1024      - / 0.16 (0.10)   (S = 8)
The two paths run the same chains of fused multiply-adds and agree bit for bit.  The kernel sits at numpy's own error.  (K = 3: 12.02 is the signed matrix at s = 64, kernel and numpy alike;
its bar is 8 x 12.02.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import propagate_cases as pc
from oracle import msm as oracle
from oracle import msm_bootstrap as boot
from oracle.frames import synth_chain_frames
from fence import COMBINATIONS, fenced
from stream_gate import Spec, analysis_call, gate, ptr, raw, reference, side, stream_of  # noqa: F401  (gate, side: fixtures)
from support import B, dev, ev, same_bits, to_dev  # noqa: F401  (dev)

pytestmark = pytest.mark.gpu

BY_SIZE, LDS, STREAMED = 0, 1, 2


def limit():
    return B().msm_propagate_lds_limit()


def paths_of(K):
    return [LDS, STREAMED] if K <= limit() else [STREAMED]


def pack(mats, w0s, obss, Kmax=None, fill=np.nan):
    """compact slots, `fill` (NaN) wherever a problem does not reach"""
    ks = np.array([len(T) for T in mats], np.int32)
    Kmax = Kmax or int(ks.max())
    t = np.full((len(mats), Kmax * Kmax), fill)
    for p, T in enumerate(mats):
        t[p, :T.size] = np.asarray(T).reshape(-1)
    P, M, R = len(w0s), w0s[0].shape[0], obss[0].shape[0]
    w0, obs = np.full((P, M, Kmax), fill), np.full((P, R, Kmax), fill)
    for p in range(P):
        K = w0s[p].shape[1]
        w0[p, :, :K], obs[p, :, :K] = w0s[p], obss[p]
    return t.reshape(len(mats), Kmax, Kmax), ks, w0, obs


def propagate(mats, w0s, obss, S, path=BY_SIZE, mat_of=None, Kmax=None, want_last=True, fill=0xFF, extra=0):
    """-> (out (P, S + 1, M, R), w_last (P, M, Kmax) | None, status (P,), the workspace's bytes after the call).  mats: one matrix
    per problem, or with mat_of the shared ones."""
    t, km, w0, obs = pack(mats, w0s, obss, Kmax)
    ks = km if mat_of is None else km[np.asarray(mat_of)]
    P = len(w0s)
    need = B().msm_propagate_workspace_bytes(P, t.shape[1], w0.shape[1], obs.shape[1])
    ws = torch.full((need + extra,), fill, dtype=torch.uint8, device="cuda")
    B().debug_msm_propagate_path(path)
    try:
        out, last, status = B().msm_propagate(to_dev(t), mat_of, ks, to_dev(w0), to_dev(obs), S, want_last=want_last, workspace=ws)
    finally:
        B().debug_msm_propagate_path(BY_SIZE)
    out, status = out.cpu().numpy(), status.cpu().numpy()
    last = last.cpu().numpy() if last is not None else None
    for p, K in enumerate(ks):
        assert status[p] != 0 or not np.isnan(out[p]).any(), f"problem {p}: NaN in out with status 0"
        if last is not None:
            assert np.isnan(last[p, :, K:]).all(), f"problem {p}: w_last is written from K_p = {K} on"
            assert status[p] != 0 or not np.isnan(last[p, :, :K]).any(), f"problem {p}: NaN in w_last with status 0"
    return out, last, status, ws.cpu().numpy()


# ---------------------------------------------------------------- 1. accuracy over sizes, kinds and paths
def check_size(K, names=None, S=pc.STEPS):
    kinds = pc.kinds(K)
    names = names or list(kinds)
    w0, obs = pc.vectors(K)
    for path in paths_of(K):
        out, last, status, _ = propagate([kinds[n] for n in names], [w0] * len(names), [obs] * len(names), S, path)
        for p, n in enumerate(names):
            assert status[p] == 0, (K, n, path, status[p])
            truth, unit, e_np = pc.reference(K, n, S)
            e, bar = pc.measure(out[p], truth, unit), pc.bar_of(e_np, K)
            print(f"[prop] K {K:4d} path {path} {n:14s} E {e.max():6.2f} (numpy {e_np.max():5.2f}, bar {bar.max():5.1f}, at s = 0: "
                  f"{e[0]:5.2f} of {bar[0]:5.1f})")
            assert (e <= bar).all(), (K, n, path, int(np.argmax(e - bar)), e.max(), bar.max())
            if n in ("metastable", "nonreversible", "identity", "cyclic", "all_equal", "scaled_down", "scaled_up"):
                assert (last[p, :, :K] >= 0).all(), f"K = {K} {n}: a negative w_last from non-negative T and w0"


@pytest.mark.parametrize("K", pc.SIZES)
def test_measure_under_its_bar(K, dev):
    check_size(K)


def test_measure_around_the_lds_limit_and_above(dev):
    L = limit()
    for K in (L, L + 1, 257):
        check_size(K)


def test_one_problem_of_1024_states(dev):
    check_size(1024, ["metastable"], S=8)


def mixed():
    """five problems of mixed sizes on both sides of the limit: (matrices, start vectors, observables)"""
    L = limit()
    sizes = (3, L + 1, 1, 64, 17)
    names = ("metastable", "signed", "nonreversible", "nonreversible", "signed")
    return ([pc.kinds(K)[n] for K, n in zip(sizes, names)], [pc.vectors(K)[0] for K in sizes], [pc.vectors(K)[1] for K in sizes])


def test_mixed_sizes_in_one_call_under_a_larger_kmax(dev):
    mats, w0s, obss = mixed()
    Kmax = limit() + 9
    out, last, status, ws = propagate(mats, w0s, obss, 20, Kmax=Kmax, fill=0xAB, extra=4096)
    assert not status.any()
    assert (ws[-4096:] == 0xAB).all(), "the call wrote beyond the workspace it asked for"
    for p, T in enumerate(mats):
        truth, _ = pc.chain(T, w0s[p], obss[p], 20, np.longdouble)
        unit = pc.units(T, w0s[p], obss[p], 20)
        mine, _ = pc.chain(T, w0s[p], obss[p], 20, np.float64)
        e, bar = pc.measure(out[p], truth, unit), pc.bar_of(pc.measure(mine, truth, unit), len(T))
        assert (e <= bar).all(), (p, e.max(), bar.max())


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("path", [LDS, STREAMED], ids=["lds", "streamed"])
def test_exact_cases(path, dev):
    K, S = 37, 50
    w0, obs = pc.vectors(K)
    kinds = pc.kinds(K)
    out, last, status, _ = propagate([kinds["identity"]], [w0], [obs], S, path)
    assert not status.any() and all(same_bits(out[0, s], out[0, 0]) for s in range(S + 1)), "identity: out[s] != out[0]"
    assert same_bits(last[0, :, :K], w0)
    onehot = np.eye(K)[[0, 5, 36]]                                   # observable r = the indicator of state (0, 5, 36)[r]
    out, _, status, _ = propagate([kinds["cyclic"]], [w0], [onehot], S, path)
    for s in range(S + 1):
        for r, state in enumerate((0, 5, 36)):
            assert same_bits(out[0, s, :, r], w0[:, (state - s) % K]), f"cyclic shift: step {s}, state {state} (w T, not T w)"
    plain, _, _, _ = propagate([kinds["metastable"]], [w0], [obs], S, path)
    for name, e in (("scaled_down", -3), ("scaled_up", 3)):
        out, _, status, _ = propagate([kinds[name]], [w0], [obs], S, path)
        scaled = plain[0] * (2.0 ** (e * np.arange(S + 1)))[:, None, None]
        assert not status.any() and same_bits(out[0], scaled), f"{name}: out[s] != out[s] 2^({e} s)"
    out, last, status, _ = propagate([kinds["metastable"]], [w0], [obs], 0, path)               # S = 0
    ref = np.array([[pc.chain(kinds["metastable"], w0[m:m + 1], obs[r:r + 1], 0, np.longdouble)[0][0, 0, 0] for r in range(4)]
                    for m in range(3)])
    assert out.shape == (1, 1, 3, 4) and same_bits(last[0, :, :K], w0)
    assert (np.abs(out[0, 0] - ref) <= 2.0 * K * pc.EPS * np.abs(w0).sum(axis=1)[:, None] * np.abs(obs).max(axis=1)[None, :]).all()
    out, last, status, _ = propagate([np.array([[0.5]])], [np.array([[3.0], [-1.0]])], [np.array([[2.0]])], 4, path)   # K = 1
    assert same_bits(out[0, :, :, 0], np.array([[6.0, -2.0], [3.0, -1.0], [1.5, -0.5], [0.75, -0.25], [0.375, -0.125]]))
    assert same_bits(last[0, :, 0], np.array([3.0 / 16, -1.0 / 16]))


@pytest.mark.parametrize("path", [LDS, STREAMED], ids=["lds", "streamed"])
def test_two_state_chain_against_its_closed_form(path, dev):
    a, b, S = 0.03, 0.11, 64
    T = np.array([[1 - a, a], [b, 1 - b]])
    p0, obs = np.array([[1.0, 0.0], [0.25, 0.75]]), np.eye(2)
    out, _, status, _ = propagate([T], [p0], [obs], S, path)
    la, lb = np.longdouble(a), np.longdouble(b)
    pi = np.array([lb, la]) / (la + lb)
    closed = pi[None, None, :] + (p0.astype(np.longdouble) - pi)[None, :, :] * ((1 - la - lb) ** np.arange(S + 1))[:, None, None]
    unit = pc.units(T, p0, obs, S)
    mine, _ = pc.chain(T, p0, obs, S, np.float64)
    e, bar = pc.measure(out[0], closed, unit), pc.bar_of(pc.measure(mine, closed, unit), 2)
    print(f"[prop] two states path {path}: E {e.max():.2f}, bar {bar.max():.1f}")
    assert not status.any() and (e <= bar).all(), (e.max(), bar.max())


# ---------------------------------------------------------------- 3. invariance, bit for bit
@pytest.mark.parametrize("path", [BY_SIZE, LDS, STREAMED], ids=["by-size", "lds", "streamed"])
def test_batch_invariance(path, dev):
    mats, w0s, obss = mixed()
    if path == LDS:
        mats, w0s, obss = mats[:1] + mats[2:], w0s[:1] + w0s[2:], obss[:1] + obss[2:]
    n, S, Kmax = len(mats), 12, limit() + 1
    out, last, status, _ = propagate(mats, w0s, obss, S, path, Kmax=Kmax, fill=0xFF)
    again = propagate(mats, w0s, obss, S, path, Kmax=Kmax, fill=0xFF)
    assert all(same_bits(x, y) for x, y in zip((out, last, status), again)), "two calls differ"
    order = list(range(n))[::-1]
    po, pl, ps, _ = propagate([mats[i] for i in order], [w0s[i] for i in order], [obss[i] for i in order], S, path, Kmax=Kmax, fill=0x00)
    for at, i in enumerate(order):
        assert same_bits(out[i], po[at]) and same_bits(last[i], pl[at]) and status[i] == ps[at], f"problem {i} permuted, workspace 0x00"
    nolast = propagate(mats, w0s, obss, S, path, Kmax=Kmax, want_last=False)
    assert nolast[1] is None and same_bits(out, nolast[0]), "out differs without w_last"
    longer, _, _, _ = propagate(mats, w0s, obss, S + 9, path, Kmax=Kmax)
    assert same_bits(longer[:, :S + 1], out), "the first steps of a longer run differ"
    i = n - 2
    crowd = [i] * 17 + [0] + [i] * 22                                 # the same problem among 40, sharing one matrix or not
    co, cl, _, _ = propagate([mats[i], mats[0]], [w0s[j] for j in crowd], [obss[j] for j in crowd], S, path,
                             mat_of=[0] * 17 + [1] + [0] * 22, Kmax=Kmax)
    one = propagate([mats[i]], [w0s[i]], [obss[i]], S, path, Kmax=Kmax)
    for at in (0, 16, 18, 39):
        assert same_bits(co[at], one[0][0]) and same_bits(cl[at], one[1][0]), f"P = 1 against place {at} of 40 on a shared matrix"
    assert same_bits(co[17], out[0]) and same_bits(out[i], one[0][0])
    for m in range(3):                                               # M = 3 against three M = 1 problems on the shared matrix
        so, sl, _, _ = propagate([mats[i]], [w0s[i][m:m + 1]] * 2, [obss[i]] * 2, S, path, mat_of=[0, 0], Kmax=Kmax)
        assert same_bits(so[1, :, 0], out[i, :, m]) and same_bits(sl[1, 0], last[i, m]), f"start row {m} alone"
    for r in range(4):                                               # R = 4 against the observables one by one
        so, sl, _, _ = propagate([mats[i]], [w0s[i]], [obss[i][r:r + 1]], S, path, Kmax=Kmax)
        assert same_bits(so[0, :, :, 0], out[i, :, :, r]) and same_bits(sl[0], last[i]), f"observable {r} alone"


def test_sixteen_rows_and_observables_on_both_paths(dev):
    K = 100
    w0, obs = pc.vectors(K, 16, 16)
    T = pc.kinds(K)["signed"]
    a = propagate([T], [w0], [obs], 10, LDS)
    b = propagate([T], [w0], [obs], 10, STREAMED)
    truth, _ = pc.chain(T, w0, obs, 10, np.longdouble)
    assert (pc.measure(a[0][0], truth, pc.units(T, w0, obs, 10)) <= 8.0).all()
    one = propagate([T], [w0[11:12]], [obs[7:8]], 10, STREAMED)
    assert same_bits(one[0][0, :, 0, 0], b[0][0, :, 11, 7]) and same_bits(one[1][0, 0], b[1][0, 11])
    assert same_bits(a[0], b[0]), "the two paths run the same chains"


# ---------------------------------------------------------------- 4. failures stay local
@pytest.mark.parametrize("path", [BY_SIZE, STREAMED], ids=["by-size", "streamed"])
def test_non_finite_entries_fail_their_problem_alone(path, dev):
    mats, w0s, obss = mixed()
    S = 6
    clean = propagate(mats, w0s, obss, S, path)
    for where in ("T", "w0", "obs"):
        for bad in (np.nan, np.inf):
            m2, w2, o2 = [np.array(x) for x in mats], [np.array(x) for x in w0s], [np.array(x) for x in obss]
            {"T": m2, "w0": w2, "obs": o2}[where][3][-1, 5] = bad
            out, last, status, _ = propagate(m2, w2, o2, S, path)
            assert list(status) == [0, 0, 0, 1, 0], (where, bad, status)
            assert np.isnan(out[3]).all() and np.isnan(last[3, :, :64]).all()
            for p in (0, 1, 2, 4):
                assert same_bits(out[p], clean[0][p]) and same_bits(last[p], clean[1][p]), (where, bad, p)
    t, ks, w0, obs = pack(mats, w0s, obss)                            # NaN beyond K_p (pack's fill) was ignored in every call above
    assert np.isnan(t[0, 0, 9]) and np.isnan(w0[0, 0, 3]) and np.isnan(obs[2, 0, 1])


def test_an_overflow_is_reported_not_returned_as_nan(dev):
    T = np.array([[1e200, -1e200], [1e200, 1e200]])
    out, last, status, _ = propagate([T, np.eye(2)], [np.ones((1, 2))] * 2, [np.ones((1, 2))] * 2, 3)
    assert list(status) == [2, 0] and np.isnan(out[0]).all() and np.isnan(last[0, :, :2]).all() and (out[1] == 2.0).all()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_carry_their_message(dev):
    lib = B().load_library()
    L = limit()

    def call(ks=(4, 3), Kmax=4, P=None, M=2, R=2, S=3, n_mat=2, mat_of=(0, 1), wsb=1 << 20, path=BY_SIZE):
        ks, mo = np.array(ks, np.int32), np.array(mat_of, np.int32)
        P = len(ks) if P is None else P
        buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        lib.dff_debug_msm_propagate_path(path)
        try:
            rc = lib.dff_msm_propagate(0, ptr(buf), n_mat, mo.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), P, Kmax, ptr(buf),
                                       M, ptr(buf), R, S, ptr(buf), None, ptr(buf), ptr(ws), wsb, None)
        finally:
            lib.dff_debug_msm_propagate_path(BY_SIZE)
        return rc, lib.dff_last_error().decode()

    for kw, text in ((dict(M=0), "start vectors must be 1..16"), (dict(M=17), "start vectors must be 1..16"),
                     (dict(R=0), "observables must be 1..16"), (dict(R=17), "observables must be 1..16"),
                     (dict(S=-1), "steps must be 0..65535"), (dict(S=65536), "steps must be 0..65535"),
                     (dict(ks=[1] * 16384, mat_of=[0] * 16384, Kmax=1, M=16, R=16, S=65535), "output values, at most"),
                     (dict(mat_of=(0, 2)), "problem 1 takes matrix 2 of 2"), (dict(mat_of=(0, -1)), "problem 1 takes matrix -1 of 2"),
                     (dict(mat_of=(0, 0)), "problem 1 reads matrix 0 with 3 states, an earlier problem with 4"),
                     (dict(ks=(4, 5)), "problem 1 has 5 states, must be 1..Kmax = 4"), (dict(ks=(0, 4)), "problem 0 has 0 states"),
                     (dict(wsb=15), "workspace of 15 bytes, 16 needed"),
                     (dict(ks=(4, L + 1), Kmax=L + 1, path=LDS), f"problem 1 has {L + 1} states, the forced LDS path takes at most {L}")):
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, msg)


# ---------------------------------------------------------------- 6. stream order
def propagate_spec():
    """five problems of 40 states on three matrices, every entry written (K_p = Kmax); poison: NaN matrices and vectors"""
    K, M, R, S = 40, 3, 2, 9
    t, ks, w0, obs = pack([pc.metastable(K, seed=s) for s in range(3)], [pc.vectors(K, M, R, seed=s)[0] for s in range(5)],
                          [pc.vectors(K, M, R, seed=s)[1] for s in range(5)])
    mat_of = np.array([0, 1, 2, 1, 0], np.int32)
    ks5 = np.full(5, K, np.int32)
    ws = torch.empty(B().msm_propagate_workspace_bytes(5, K, M, R), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    return Spec("dff_msm_propagate", {"t": (to_dev(t), nan), "w0": (to_dev(w0), nan), "obs": (to_dev(obs), nan)},
                {"out": ((5, S + 1, M, R), torch.float64), "last": ((5, M, K), torch.float64), "status": ((5,), torch.int32)},
                lambda _, b: raw("dff_msm_propagate", 0, ptr(b["t"]), 3, mat_of.ctypes.data_as(C.c_void_p), ks5.ctypes.data_as(C.c_void_p),
                                 5, K, ptr(b["w0"]), M, ptr(b["obs"]), R, S, ptr(b["out"]), ptr(b["last"]), ptr(b["status"]),
                                 ptr(b["ws"]), b["ws"].numel(), stream_of(b["t"])),
                work={"ws": ws})


@pytest.mark.parametrize("forced", [LDS, STREAMED], ids=["lds", "streamed"])
def test_the_call_is_ordered_on_its_stream(forced, gate, side):
    B().debug_msm_propagate_path(forced)
    try:
        ref = analysis_call(propagate_spec(), gate, side)
    finally:
        B().debug_msm_propagate_path(BY_SIZE)
    assert not bool(ref["status"].any()) and bool(torch.isfinite(ref["out"]).all())
    assert float((ref["last"].sum(dim=2) - 1.0).abs().max()) < 1e-12          # stochastic T: the rows keep their sum


@pytest.mark.parametrize("forced", [LDS, STREAMED], ids=["lds", "streamed"])
def test_fence(forced):
    """The memory contract (tests/fence.py) on both paths: all seven buffers in one arena, the P descriptors at exactly
    dff_msm_propagate_workspace_bytes."""
    B().debug_msm_propagate_path(forced)
    try:
        spec = propagate_spec()
        ref = reference(spec)
        for pattern, placement in COMBINATIONS:
            fenced(spec, pattern=pattern, placement=placement, ref=ref)
    finally:
        B().debug_msm_propagate_path(BY_SIZE)


# ---------------------------------------------------------------- 7. the Python layer
SETTINGS = dict(tol=1e-12, max_iter=100000, steps_per_sync=64)


def ck_by_numpy(base, tests, multiples, sets):
    """the definitions of chapman_kolmogorov on the same fitted models, in np.longdouble"""
    def rows(m):
        act, pi = np.asarray(m.active_set), m.stationary_distribution.astype(np.longdouble)
        ind = np.stack([np.isin(act, s) for s in sets]).astype(np.longdouble)
        w = ind * pi
        return w / w.sum(axis=1)[:, None], ind
    pred, est = [], []
    w, ind = rows(base)
    for k in multiples:
        pred.append(w @ np.linalg.matrix_power(base.transition_matrix.astype(np.longdouble), k) @ ind.T)
        wk, ik = rows(tests[k])
        est.append(wk @ tests[k].transition_matrix.astype(np.longdouble) @ ik.T)
    return np.array(pred), np.array(est)


def test_chapman_kolmogorov_on_a_three_well_jump_process(dev):
    labels, lengths = pc.three_well_trajectories()
    sets, mult = pc.three_well_sets(), (1, 2, 3, 4, 5)
    ck = ev().chapman_kolmogorov(labels, 2, sets, mult, lengths, 9, **SETTINGS)
    assert ck.predicted.shape == ck.estimated.shape == (5, 3, 3) and list(ck.lagtimes) == [2, 4, 6, 8, 10]
    assert same_bits(ck.predicted[0], ck.estimated[0]), "k = 1: the same model on the same path"
    pred, est = ck_by_numpy(ck.models[1], ck.models, mult, sets)
    # every entry is at most 1 = |w|_1 |T|^k |indicator|_inf: the unit is 2^-52; numpy's bar is floored at 8 units, capped (s + 2) K
    bar = np.minimum(8.0, (np.array(mult) + 2.0) * 9)[:, None, None] * pc.EPS
    assert (np.abs(ck.predicted - pred) <= bar).all() and (np.abs(ck.estimated - est) <= 8.0 * pc.EPS).all()
    assert np.abs(ck.predicted.sum(axis=2) - 1.0).max() < 1e-10 and ck.max_abs_diff < 0.1 and ck.rms_diff <= ck.max_abs_diff
    print(f"[prop] CK three wells: max |predicted - estimated| {ck.max_abs_diff:.4f}, rms {ck.rms_diff:.4f}")
    wrong = ev().chapman_kolmogorov(labels, 2, [[0, 3, 6], [1, 4, 7], [2, 5, 8]], mult, lengths, 9, **SETTINGS)
    assert same_bits(wrong.predicted[0], wrong.estimated[0])


def test_chapman_kolmogorov_bootstrap_equals_the_models_of_fit_counts(dev):
    labels, lengths = pc.three_well_trajectories()
    sets, mult, lag, nb = pc.three_well_sets(), (1, 2, 4), 2, 8
    ck = ev().chapman_kolmogorov(labels, lag, sets, mult, lengths, 9, n_resamples=nb, seed=4, **SETTINGS)
    assert ck.predicted_resamples.shape == (nb, 3, 3, 3) and 0.0 <= ck.share_inside <= 1.0
    assert (ck.estimated_lo <= ck.estimated_hi).all() and (ck.predicted_lo <= ck.predicted_hi).all()
    w = ev().bootstrap_weights(len(lengths), nb, 4)
    counts = {k: boot.weighted_counts(labels, lengths, lengths, lag * k, 9, w) for k in mult}
    for b in range(nb):
        models = {k: ev().MarkovStateModel(lag * k, **SETTINGS).fit_counts(counts[k][b]) for k in mult}
        pred, est = ev().chapman_kolmogorov_of_models([(models[1], models)], mult, sets)
        assert same_bits(pred[0], ck.predicted_resamples[b]) and same_bits(est[0], ck.estimated_resamples[b]), b
    one = ev().chapman_kolmogorov(labels, lag, sets, mult, lengths, 9, n_resamples=nb, seed=4, resample_batch=3, **SETTINGS)
    assert same_bits(one.predicted_resamples, ck.predicted_resamples) and same_bits(one.estimated_resamples, ck.estimated_resamples)


@pytest.mark.parametrize("K", [8, 40, 200])
def test_metastable_sets_of_a_four_block_model(K, dev):
    C4, blocks = pc.four_block_counts(K)
    m = ev().MarkovStateModel(1, **SETTINGS).fit_counts(C4)
    sets = ev().metastable_sets(m, 4)
    assert len(sets) == 4 and all(np.array_equal(s, b) for s, b in zip(sets, blocks)), [s.tolist() for s in sets]
    chi = ev().pcca_memberships(m, 4)
    assert chi.shape == (K, 4) and np.abs(chi.sum(axis=1) - 1.0).max() < 1e-9


def test_autocorrelation_and_relaxation_of_a_two_state_model(dev):
    S = 40
    m = ev().MarkovStateModel(3, reversible=False).fit_counts(np.array([[96.0, 4.0], [9.0, 91.0]]))   # T is the rounded row shares
    T, pi = m.transition_matrix, m.stationary_distribution
    lam = (1 - np.longdouble(T[0, 1]) - np.longdouble(T[1, 0])) ** np.arange(S + 1)
    ac = ev().msm_autocorrelation(m, [2.0, -1.0], S)
    assert list(ac.lags[:3]) == [0, 3, 6] and ac.acf[0] == 1.0 and ac.acf.shape == ac.cov.shape == (S + 1,)
    # C(s) and C(0) each within 8 units U = 2^-52 |pi a~|_1 |a~|_inf (the floor of the bar; the cap (s + 2) K is larger from s = 2
    # on), and U / C(0) <= 2 for two states (pi_0 a~_0 = -pi_1 a~_1 = g: |pi a~|_1 = 2 g, C(0) = g (|a~_0| + |a~_1|) >= g |a~|_inf):
    # 32 units of 2^-52.  The closed form itself: T's rows are rounded, so its second eigenvalue is 1 - a - b only to about two
    # roundings, which lam^s carries s times over lam = 0.87: 3 (s + 2) units.  A component of a~ along (1, 1) from pi's rounding
    # drops out of C exactly, since sum_i pi_i a~_i = 0 by construction.
    err = np.abs(ac.acf - lam)
    print(f"[prop] two-state ACF: worst error {float(err.max()):.2e}")
    assert (err <= (32.0 + 3.0 * (np.arange(S + 1) + 2.0)) * pc.EPS).all(), float(err.max())
    rel = ev().msm_relaxation(m, [1.0, 0.0], [[1.0, 0.0], [0.0, 1.0]], S)
    pil = np.array([T[1, 0], T[0, 1]], np.longdouble) / (np.longdouble(T[0, 1]) + np.longdouble(T[1, 0]))
    closed = pil[None, :] + (np.array([1.0, 0.0]) - pil)[None, :] * lam[:, None]
    assert rel.shape == (S + 1, 2) and (np.abs(rel - closed) <= (8.0 + 3.0 * (np.arange(S + 1) + 2.0))[:, None] * pc.EPS).all()
    assert ev().msm_relaxation(m, [1.0, 0.0], [1.0, 0.0], 3).shape == (4,)
    nr = ev().MarkovStateModel(1, reversible=False).fit_counts(np.array([[5.0, 3.0, 0.0], [0.0, 4.0, 2.0], [3.0, 0.0, 6.0]]))
    out = ev().msm_propagate(nr, np.eye(3), np.ones((1, 3)), 5)
    assert out.shape == (1, 6, 3, 1) and np.abs(out - 1.0).max() <= 16 * pc.EPS                 # rows of a stochastic matrix sum to 1


def test_the_evaluator_on_a_two_well_jump_process(dev):
    """Two conformations visited by a two-state jump process, which is Markovian at every lag: the test must hold (the predictions
    inside the estimates' bootstrap intervals, the differences small), the model's ACF of the first TIC must follow the measured
    one, and the reference, analysed first, defines the sets that the samples reuse."""
    beads, wells = 10, np.array([[0.97, 0.03], [0.05, 0.95]])
    base = synth_chain_frames(2, beads, 91).astype(np.float64)

    def frames(seed):
        paths = oracle.jump_process(wells, 20, 1500, seed)
        return (base[paths.reshape(-1)] + 0.05 * np.random.default_rng(seed + 1).standard_normal((paths.size, beads, 3))).astype(np.float32)
    F = B().struct_tic_num_features(beads)
    rng = np.random.default_rng(17)
    tica = (rng.uniform(0.0, 10.0, F), rng.uniform(-0.1, 0.1, (F, 2)))
    lengths = [1500] * 20
    e = ev().ChapmanKolmogorovEvaluator("chignolin", tica, n_microstates=8, lagtime=2, n_sets=2, multiples=(1, 2, 4), frame_time=0.5,
                                        ref_data=frames(31), ref_traj_lengths=lengths, n_bootstrap=20)
    sets = [s.copy() for s in e.sets]
    res = e.eval(frames(11), lengths)
    keys = set(ev().ChapmanKolmogorovEvaluator.KEYS) | {"ck_share_inside"}
    assert set(res) == keys | {k + "_ref" for k in keys} | {"ck_max_abs_diff_minus_ref"}
    assert len(sets) == 2 and all(np.array_equal(a, b) for a, b in zip(sets, e.sets)) and res["n_sets"] == 2.0
    assert sorted(np.concatenate(sets).tolist()) == sorted(e.models["refs"].active_set.tolist())
    print(f"[prop] evaluator: ck max {res['ck_max_abs_diff']:.4f} (ref {res['ck_max_abs_diff_ref']:.4f}), share inside "
          f"{res['ck_share_inside']:.2f}, acf rms {res['acf_rms_diff']:.4f}")
    assert res["ck_diagonal_predicted"][0] == res["ck_diagonal_estimated"][0] and np.array(res["ck_diagonal_predicted"]).shape == (3, 2)
    # 30 000 frames, 0.03 - 0.05 jumps per frame: the set-to-set probabilities of two estimates from the same data differ by their
    # sampling error, a few 1e-3; 0.05 and an ACF within 0.05 rms separate a Markovian process from a broken propagation
    assert res["ck_max_abs_diff"] < 0.05 and res["ck_max_abs_diff_ref"] < 0.05 and res["acf_rms_diff"] < 0.05
    assert res["ck_share_inside"] >= 0.5 and res["samples_nonfinite"] == 0.0
    assert res["ck_max_abs_diff_minus_ref"] == res["ck_max_abs_diff"] - res["ck_max_abs_diff_ref"]
