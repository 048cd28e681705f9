"""Host side of the device eigensolver: the symbols and refusals of dff_sym_eig_topk (refused on the host, before any device
call), the LDS arithmetic, MarkovStateModel.symmetrized / eigenvectors and msm_spectrum on a numpy stand-in behind
evaluate.spectral_solver (eig_cases.host_topk: np.linalg.eigh with the call's sign and padding rules), the eigensolver keyword
of bootstrap_msm / implied_timescales / implied_timescales_bootstrap / MsmEvaluator, the re-exports and the tool's arguments.
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dff_amd
import eig_cases as ec
from dff_amd import binding, evaluate
from oracle import msm as oracle
from oracle import msm_bootstrap as boot
from oracle.msm_bootstrap import five_state_case
from standins import OracleSweeps
from support import owning_unit, refused, same_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dff_sym_eig_workspace_bytes", "dff_sym_eig_lds_limit", "dff_sym_eig_topk", "dff_debug_sym_eig_path")
p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
FAKE = C.c_void_p(4096)                         # a non-null "device pointer": every call below is refused before it is used


# ---------------------------------------------------------------- symbols and refusals
def test_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "dff.h")).read()
    lib = binding.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in binding.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(binding.SYMBOLS["dff_sym_eig_topk"][1]) == 12
    assert binding.SYMBOLS["dff_sym_eig_workspace_bytes"] == (C.c_longlong, [C.c_int, C.c_int])
    assert binding.SYMBOLS["dff_sym_eig_lds_limit"] == (C.c_int, []) and binding.SYMBOLS["dff_debug_sym_eig_path"] == (C.c_int, [C.c_int])
    assert binding.SYM_EIG_MAX_BATCH == evaluate.SPECTRUM_MAX_BATCH == 16384 and binding.SYM_EIG_MAX_K == 32
    text = owning_unit("dff_sym_eig.hip")
    assert '#include "dff_sym_eig.hip"' in text
    assert "dff_sym_eig" not in open(os.path.join(ROOT, "build.sh")).read()


def test_the_lds_path_fits_a_compute_unit():
    """the packed triangle, seven vectors, the 16 groups' partial sums and the bisection's tables of the LDS path"""
    L = binding.sym_eig_lds_limit()
    assert 64 <= L < 1024
    doubles = L * (L + 1) // 2 + (7 + 16) * L + 3 * 32 + 16 + 256 // 2
    assert 8 * doubles <= 160 * 1024
    assert 8 * ((7 + 8) * 1024 + 3 * 32 + 16 + 512 // 2) <= 160 * 1024          # the workspace path's vectors at K = 1024


def test_workspace_bytes_and_refusals_before_any_device_call():
    lib = binding.load_library()
    assert binding.sym_eig_workspace_bytes(1, 1) == (1 + 4 + 1) * 8
    assert binding.sym_eig_workspace_bytes(48, 1024) == 48 * (1 + 4 + 1024 * 1024) * 8
    for bad in ((0, 4), (16385, 4), (4, 0), (4, 1025)):
        assert lib.dff_sym_eig_workspace_bytes(*bad) == -1, bad
    with pytest.raises(ValueError, match="problems must be 1..16384"):
        binding.sym_eig_workspace_bytes(0, 4)

    def call(ks=(4, 3), Kmax=4, P=None, k=2, a=FAKE, w=FAKE, v=FAKE, status=FAKE, ws=FAKE, wsb=1 << 20):
        ks = np.array(ks, np.int32)
        return lib.dff_sym_eig_topk(0, a, p(ks), len(ks) if P is None else P, Kmax, k, w, v, status, ws, wsb, None)
    refused(lib, call(P=0), "problems must be 1..16384")
    refused(lib, call(ks=[1] * 16385, Kmax=1), "problems must be 1..16384")
    refused(lib, call(Kmax=0), "states must be 1..1024")
    refused(lib, call(Kmax=1025), "states must be 1..1024")
    refused(lib, call(k=0), "eigenpairs must be 1..32")
    refused(lib, call(k=33), "eigenpairs must be 1..32")
    refused(lib, call(a=None), "null matrices")
    refused(lib, call(w=None), "null matrices")
    refused(lib, call(status=None), "null matrices")
    refused(lib, call(ks=(4, 5)), "problem 1 has 5 states, must be 1..Kmax = 4")
    refused(lib, call(ks=(0, 4)), "problem 0 has 0 states")
    need = 2 * (1 + 4 + 16) * 8
    refused(lib, call(wsb=need - 1), f"workspace of {need - 1} bytes, {need} needed")
    refused(lib, call(ws=None), f"workspace of {1 << 20} bytes, {need} needed")
    refused(lib, call(ws=C.c_void_p(4100)), "8-byte aligned")
    assert lib.dff_debug_sym_eig_path(3) == 1 and "0 (by size), 1 (LDS) or 2 (workspace)" in lib.dff_last_error().decode()
    L = binding.sym_eig_lds_limit()
    assert lib.dff_debug_sym_eig_path(1) == 0
    try:
        refused(lib, call(ks=(4, L + 1), Kmax=L + 1, wsb=1 << 30), f"problem 1 has {L + 1} states, the forced LDS path takes at most {L}")
    finally:
        assert lib.dff_debug_sym_eig_path(0) == 0
    with pytest.raises(ValueError, match="contiguous float64 CUDA tensor"):
        binding.sym_eig_topk(torch.zeros((2, 4, 4), dtype=torch.float64), [4, 4], 2)


def test_package_reexports():
    for name in ("msm_spectrum", "MsmSpectrum", "spectral_solver"):
        assert getattr(dff_amd, name) is getattr(evaluate, name) and name in dff_amd.__all__
    for name in ("sym_eig_topk", "sym_eig_workspace_bytes", "sym_eig_lds_limit", "debug_sym_eig_path"):
        assert callable(getattr(binding, name))


# ---------------------------------------------------------------- the Python layer on a stand-in
class HostSpectral:
    calls = 0

    def __init__(self, device):
        pass

    def __call__(self, a, ks, k, vectors):
        HostSpectral.calls += 1
        return ec.host_topk(np.asarray(a), ks, k, vectors)


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(evaluate, "reversible_sweeper", OracleSweeps)
    monkeypatch.setattr(evaluate, "resampled_counter", boot.Counter)
    monkeypatch.setattr(evaluate, "batched_reversible_sweeper", boot.Sweeper)
    monkeypatch.setattr(evaluate, "spectral_solver", HostSpectral)
    monkeypatch.setattr(binding, "micro_transition_counts",
                        lambda lab, lengths, lags, K: torch.from_numpy(oracle.transition_counts(lab.numpy(), lengths, lags, K)))
    HostSpectral.calls = 0


def model_of(T, lag=1, scale=1e7, pad=0, **kw):
    """a MarkovStateModel fitted on counts pi_i T_ij scale of a reversible T (the estimator returns T), `pad` unvisited states
    in front of it"""
    w, v = np.linalg.eig(T.T)
    pi = np.abs(np.real(v[:, np.argmax(np.real(w))]))
    C0 = np.zeros((len(T) + pad, len(T) + pad))
    C0[pad:, pad:] = pi[:, None] / pi.sum() * T * scale
    return evaluate.MarkovStateModel(lag, device="cpu", **kw).fit_counts(C0)


LINE = np.array([[0.9, 0.1, 0.0], [0.2, 0.7, 0.1], [0.0, 0.3, 0.7]])


def test_symmetrized_and_its_refusals(on_host):
    m = model_of(LINE, lag=2)
    M = m.symmetrized()
    assert same_bits(M, M.T)
    r = np.sqrt(m.stationary_distribution)
    assert np.allclose(M, r[:, None] * m.transition_matrix / r[None, :], rtol=1e-13)
    assert np.allclose(np.linalg.eigvalsh(M)[::-1], m.eigenvalues(), atol=1e-14)
    with pytest.raises(ValueError, match="not fitted"):
        evaluate.MarkovStateModel(1, device="cpu").symmetrized()
    plain = evaluate.MarkovStateModel(1, reversible=False, device="cpu").fit_counts(np.array([[5.0, 2.0], [1.0, 7.0]]))
    for call in (plain.symmetrized, plain.eigenvectors, lambda: evaluate.msm_spectrum(plain)):
        with pytest.raises(ValueError, match="reversible"):
            call()
    with pytest.raises(ValueError, match="side"):
        m.eigenvectors(1, side="up")
    for bad in (0, 32):
        with pytest.raises(ValueError, match="k must be 1..31"):
            evaluate.msm_spectrum(m, k=bad)


def test_eigenvectors_of_a_model(on_host):
    m = model_of(LINE, lag=2)
    T, pi = m.transition_matrix, m.stationary_distribution
    lam = m.eigenvalues()
    psi, phi = m.eigenvectors(2), m.eigenvectors(2, side="left")
    assert psi.shape == phi.shape == (3, 3)
    for j in range(3):
        assert np.abs(T @ psi[j] - lam[j] * psi[j]).max() <= 1e-14 and np.abs(phi[j] @ T - lam[j] * phi[j]).max() <= 1e-14
        assert psi[j][np.argmax(np.abs(psi[j]))] > 0
        assert np.allclose(phi[j], pi * psi[j], rtol=1e-13, atol=1e-16)
    assert np.abs(psi[0] - 1.0).max() <= 1e-14 and np.abs(phi[0] - pi).max() <= 1e-15
    assert np.abs((psi * pi) @ psi.T - np.eye(3)).max() <= 1e-14
    more = m.eigenvectors(4)                                         # k + 1 beyond the active set: NaN rows
    assert more.shape == (5, 3) and np.isnan(more[3:]).all() and same_bits(more[:3], psi)


def test_msm_spectrum_pads_short_circuits_and_batches(on_host):
    a, b = model_of(LINE, lag=2), model_of(LINE[:2, :2] / LINE[:2, :2].sum(axis=1, keepdims=True), lag=3, pad=1)
    one = evaluate.MarkovStateModel(4, device="cpu").fit_counts(np.diag([0.0, 3.0, 0.0]))
    assert list(b.active_set) == [1, 2] and len(one.active_set) == 1
    only = np.zeros(3)
    only[one.active_set] = 1.0
    sp = evaluate.msm_spectrum([a, b, one], k=2, vectors=True, device="cpu")
    assert HostSpectral.calls == 1                                   # the one-state model is not sent, the other two share a call
    assert sp.eigenvalues.shape == (3, 3) and sp.timescales.shape == (3, 2) and sp.right.shape == sp.left.shape == (3, 3, 3)
    assert not sp.status.any()
    assert np.allclose(sp.eigenvalues[0], a.eigenvalues(), atol=1e-14) and same_bits(sp.timescales[0], evaluate._timescales_of(sp.eigenvalues[0, 1:], 2, 2))
    assert np.allclose(sp.timescales[0], a.timescales(2), rtol=1e-10)
    assert np.allclose(sp.eigenvalues[1, :2], b.eigenvalues(), atol=1e-14) and np.isnan(sp.eigenvalues[1, 2])
    assert np.allclose(sp.timescales[1, 0], b.timescales(1)[0], rtol=1e-10) and np.isnan(sp.timescales[1, 1])
    assert (sp.right[1][:, 0] == 0).all() and (sp.left[1][:, 0] == 0).all()          # full index: zero outside the active set
    assert np.allclose(sp.right[1][0, 1:], 1.0, atol=1e-14) and np.allclose(sp.left[1][0, 1:], b.stationary_distribution, atol=1e-15)
    assert sp.eigenvalues[2, 0] == 1.0 and np.isnan(sp.eigenvalues[2, 1:]).all() and np.isnan(sp.timescales[2]).all()
    assert same_bits(sp.right[2][0], only) and same_bits(sp.left[2][0], only)
    for i, m in enumerate((a, b, one)):
        alone = evaluate.msm_spectrum(m, k=2, vectors=True, device="cpu")
        for name in ("eigenvalues", "timescales", "right", "left", "status"):
            assert same_bits(getattr(alone, name)[0], getattr(sp, name)[i]), (i, name)
    plain = evaluate.msm_spectrum(a, k=2, device="cpu")
    assert plain.right is None and plain.left is None and same_bits(plain.eigenvalues, sp.eigenvalues[:1])


def test_bootstrap_host_is_todays_path_and_device_goes_through_the_solver(on_host):
    labels, lengths, w = five_state_case()
    kw = dict(traj_lengths=lengths, n_states=5, weights=w, k=2, tol=1e-12, max_iter=100000, steps_per_sync=16, device="cpu")
    host = evaluate.bootstrap_msm(labels, 2, **kw)
    assert HostSpectral.calls == 0
    counts = boot.weighted_counts(labels, lengths, lengths, 2, 5, w)
    for b, Cb in enumerate(counts):                                  # eigensolver="host" (the default): bit for bit today's
        m = evaluate.MarkovStateModel(2, tol=1e-12, max_iter=100000, steps_per_sync=16, device="cpu").fit_counts(Cb)
        assert same_bits(host.timescales[b], m.timescales(2)), b
    assert same_bits(host.timescales, evaluate.bootstrap_msm(labels, 2, eigensolver="host", **kw).timescales)
    devi = evaluate.bootstrap_msm(labels, 2, eigensolver="device", resample_batch=4, **kw)
    assert HostSpectral.calls == -(-len(w) // 4)                     # one call per batch of resamples
    for name in ("stationary", "n_active", "active_count_share", "converged", "n_iter", "weights", "unit_lengths"):
        assert same_bits(getattr(host, name), getattr(devi, name)), name
    assert np.array_equal(np.isnan(host.timescales), np.isnan(devi.timescales))
    assert np.allclose(host.timescales, devi.timescales, rtol=1e-9, equal_nan=True)
    for fn in (evaluate.bootstrap_msm, evaluate.implied_timescales_bootstrap):
        with pytest.raises(ValueError, match="eigensolver must be 'host' or 'device'"):
            fn(labels, [2] if fn is evaluate.implied_timescales_bootstrap else 2, lengths, 5, eigensolver="gpu", device="cpu")


def test_implied_timescales_with_either_solver(on_host):
    labels, lengths, _ = five_state_case()
    kw = dict(k=2, steps_per_sync=16, device="cpu")
    host = evaluate.implied_timescales(labels, [1, 2, 3], lengths, 5, **kw)
    assert HostSpectral.calls == 0
    devi = evaluate.implied_timescales(labels, [1, 2, 3], lengths, 5, eigensolver="device", **kw)
    assert HostSpectral.calls == 1 and np.allclose(host, devi, rtol=1e-9, equal_nan=True)
    with pytest.raises(ValueError, match="eigensolver must be 'host' or 'device'"):
        evaluate.implied_timescales(labels, [1], lengths, 5, eigensolver="", **kw)
    with pytest.raises(ValueError, match="reversible"):
        evaluate.implied_timescales(labels, [1], lengths, 5, reversible=False, eigensolver="device", **kw)
    ph, lh, hh = evaluate.implied_timescales_bootstrap(labels, [1, 3], lengths, 5, n_resamples=5, seed=2, **kw)
    pd, ld, hd = evaluate.implied_timescales_bootstrap(labels, [1, 3], lengths, 5, n_resamples=5, seed=2, eigensolver="device", **kw)
    for x, y in ((ph, pd), (lh, ld), (hh, hd)):
        assert np.allclose(x, y, rtol=1e-9, equal_nan=True)


def test_the_evaluator_with_either_solver(on_host, monkeypatch):
    monkeypatch.setattr(binding, "load_library", lambda *a, **k: None)
    monkeypatch.setattr(evaluate, "_frames", lambda x, device: torch.as_tensor(np.asarray(x, np.float64)))
    monkeypatch.setattr(evaluate.MsmEvaluator, "project", lambda self, x: x.reshape(len(x), 1))
    monkeypatch.setattr(binding, "micro_kmeans_step",
                        lambda proj, centers, accumulate=True, workspace=None: {"labels": proj[:, 0].round().to(torch.int32)})

    def make(**kw):
        F = binding.DFF_MAX_BEADS
        return evaluate.MsmEvaluator("chignolin", (np.zeros(F), np.zeros((F, 1))), n_microstates=5, lagtime=2, n_timescales=2,
                                     frame_time=0.5, centers=np.arange(5.0).reshape(5, 1), device="cpu", **kw)
    labels, lengths, _ = five_state_case()
    frames = np.where(labels < 0, 0, labels).astype(np.float64).reshape(-1, 1, 1)
    for boots in ({}, {"n_bootstrap": 5, "bootstrap_seed": 3}):
        HostSpectral.calls = 0
        host = make(**boots).eval(frames, lengths)
        assert HostSpectral.calls == 0
        devi = make(eigensolver="device", **boots).eval(frames, lengths)
        assert HostSpectral.calls >= 1 and set(host) == set(devi)
        for key in host:
            assert np.allclose(host[key], devi[key], rtol=1e-9, equal_nan=True), key
    with pytest.raises(ValueError, match="eigensolver must be 'host' or 'device'"):
        make(eigensolver="lapack")


# ---------------------------------------------------------------- the tool
def test_spectrum_arguments_of_the_tool():
    import tools_eval_samples as tool
    ap = tool.build_parser()
    base = ["s.pt", "chignolin", "refs"]
    with_msm = base + ["--msm", "--msm-states", "9", "--msm-lag", "2"]
    assert tool.msm_spectrum_arguments(ap.parse_args(base)) == ("host", None)
    assert tool.msm_spectrum_arguments(ap.parse_args(with_msm)) == ("host", None)
    a = ap.parse_args(with_msm + ["--msm-eigensolver", "device", "--msm-eigenvectors", "3"])
    assert tool.msm_spectrum_arguments(a) == ("device", 3) and tool.msm_arguments(a) == (9, 2)
    for alone in (["--msm-eigensolver", "device"], ["--msm-eigensolver", "host"], ["--msm-eigenvectors", "2"]):
        with pytest.raises(SystemExit, match="need --msm"):
            tool.msm_spectrum_arguments(ap.parse_args(base + alone))
    for bad in (["--msm-eigensolver", "gpu"], ["--msm-eigenvectors", "0"], ["--msm-eigenvectors", "32"], ["--msm-eigenvectors", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(with_msm + bad)
