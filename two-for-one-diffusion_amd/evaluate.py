"""Host-side mirror of the reference's pairwise-distance Jensen-Shannon metric
(evaluate/evaluators.py: PwdEvaluator :195-287, js_divergence :905-915, normalize_histogram
:918-924, kl_divergence :927-931, get_pwd_triu_batch :934-948) on top of the HIP kernels
dff_pwd_max / dff_pwd_hist (csrc/dff_pwd.hip).

Same names, arguments and results as the reference, with one difference of mechanism: the
reference materialises the (n, n_pairs) distance matrix and histograms its columns with
torch.histc on the CPU; here the structures stay on the GPU, only per-pair maxima and integer
histogram counts come back, and the (n_pairs x bins) Jensen-Shannon reduction runs in numpy
exactly as the reference writes it.  There is no CPU fallback: without the HIP library the
evaluator raises DffLibraryError.
"""
from __future__ import annotations

import io
import json
import os
import pickle

import numpy as np
import torch

from . import binding


# ---- evaluators.py:905-931, verbatim semantics (float32 in, numpy reductions) ----
def normalize_histogram(hist: np.ndarray) -> np.ndarray:
    hist = np.array(hist)
    return hist / np.sum(hist)


def kl_divergence(p1: np.ndarray, p2: np.ndarray):
    return np.sum(p1 * np.log(p1 / p2))


def js_divergence(h1: np.ndarray, h2: np.ndarray):
    p1 = normalize_histogram(h1) + 1e-10
    p2 = normalize_histogram(h2) + 1e-10
    M = (p1 + p2) / 2
    return (kl_divergence(p1, M) + kl_divergence(p2, M)) / 2


def nbins_for(maxval: torch.Tensor, resolution: float) -> torch.Tensor:
    """int(torch.div(m, resolution, rounding_mode="floor") + 1) for every pair (evaluators.py:242,259)."""
    return (torch.div(maxval.float().cpu(), resolution, rounding_mode="floor") + 1).to(torch.int64)


def _to_device(x, device):
    x = torch.as_tensor(x)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise AssertionError("Shape mismatch")          # get_pwd_triu_batch's assert, evaluators.py:945
    return x.to(device=device, dtype=torch.float32).contiguous()


class PwdEvaluator:
    """Drop-in for evaluate.evaluators.PwdEvaluator (same constructor arguments and .eval()).

    val_data / all_mol are (n, N, 3) coordinate tensors in Angstrom (CPU or GPU).  `device` (extra,
    keyword-only) selects the GPU the histograms are computed on.

    Beyond the reference: frames with a non-finite coordinate are left out whole, like every evaluator here does, and
    counted in refs_nonfinite (0 when the reference histograms come from a pickle) and samples_nonfinite (of the last
    eval); no finite frame at all, or a distance the histogram kernel cannot bin, is a ValueError.
    """

    def __init__(self, val_data, plots_folder="", mol_name="", offset=0, saved_ref="none", evalset="testset",
                 *, device="cuda:0"):
        self.offset = offset
        self.plots_folder = plots_folder
        self.mol_name = mol_name.lower()
        self.resolution = 0.1
        self.device = torch.device(device)
        self.samples_nonfinite = 0
        binding.load_library()      # fail loudly now rather than at the first eval()
        if saved_ref == "none":
            saved_ref = f"./saved_references/saved_pwd_{mol_name.upper()}_{evalset}_offset_{self.offset}.pickle"
        if os.path.exists(saved_ref):
            with open(saved_ref, "rb") as f:
                data = pickle.load(f)
            self.gt_max = data["gt_max"]
            self.gt_hist = data["gt_hist"]
            self.refs_nonfinite = 0
        else:
            x, self.refs_nonfinite = self._finite_frames(val_data, "the reference structures")
            self.gt_max = binding.pwd_max(x, self.offset).cpu()
            nb = self._nbins(self.gt_max, self.resolution, x.shape[1])
            self.gt_hist = self._histograms(x, nb)
            d = os.path.dirname(saved_ref)
            if d == "" or os.path.isdir(d):
                with open(saved_ref, "wb") as f:
                    pickle.dump({"gt_max": self.gt_max, "gt_hist": self.gt_hist}, f)

    def _finite_frames(self, frames, what):
        """The frames without a non-finite coordinate, on the device, and how many were left out: a NaN in one bead would
        otherwise vanish from that bead's pairs only, and the pairs' histograms would have different totals."""
        x = _to_device(frames, self.device)
        ok = torch.isfinite(x).all(dim=2).all(dim=1)
        bad = int((~ok).sum())
        if bad:
            x = x[ok].contiguous()
        if len(x) == 0:
            raise ValueError(f"PwdEvaluator: no finite frame among {what} ({bad} with a non-finite coordinate)")
        return x, bad

    def _nbins(self, maxval, resolution, n_beads):
        """nbins_for, after refusing what the histogram kernel cannot bin: a distance of finite frames that is not finite
        (a squared difference overflows float32) or that needs more than binding.PWD_MAX_BINS bins."""
        maxval = torch.as_tensor(maxval).float().cpu()
        over = ~torch.isfinite(maxval) | (torch.div(maxval, resolution, rounding_mode="floor") + 1 > binding.PWD_MAX_BINS)
        if bool(over.any()):
            p = int(over.nonzero()[0])
            i, j = (int(t[p]) for t in torch.triu_indices(n_beads, n_beads, offset=self.offset))
            raise ValueError(f"PwdEvaluator: the distance between beads {i} and {j} (pair {p}) reaches {float(maxval[p]):g} "
                             f"Angstrom; histograms of {resolution:g} Angstrom bins hold at most "
                             f"{binding.PWD_MAX_BINS * resolution:.1f} Angstrom ({binding.PWD_MAX_BINS} bins)")
        return nbins_for(maxval, resolution)

    def _histograms(self, x, nbins):
        """list over pairs of float32 CPU tensors, what torch.histc(pwd[:, p], bins, 0, resolution*bins) returns"""
        hmax = torch.tensor([self.resolution * int(b) for b in nbins], dtype=torch.float64).float()
        counts = binding.pwd_hist(x, self.offset, nbins.to(torch.int32), hmax).cpu()
        return [counts[p, : int(b)].to(torch.float32) for p, b in enumerate(nbins)]

    def js_divergence_pwd(self, hist_gt, all_mol, gt_max, resolution):
        """Mean over pairs of JS(gt histogram, histogram of the sampled structures) (evaluators.py:251-270).
        Takes the structures (n, N, 3) where the reference takes their (n, n_pairs) distance matrix."""
        x, self.samples_nonfinite = self._finite_frames(all_mol, "the samples")
        smax = binding.pwd_max(x, self.offset).cpu()
        maxval = torch.maximum(torch.as_tensor(gt_max).float().cpu(), smax)
        nb = self._nbins(maxval, resolution, x.shape[1])
        hmax = torch.tensor([resolution * int(b) for b in nb], dtype=torch.float64).float()
        counts = binding.pwd_hist(x, self.offset, nb.to(torch.int32), hmax).cpu()
        result_js = np.empty(len(hist_gt))
        for i, (hgt, b) in enumerate(zip(hist_gt, nb)):
            b = int(b)
            hist_sampled = counts[i, :b].to(torch.float32)
            if b > len(hgt):
                hgt = torch.cat((hgt, torch.zeros(b - len(hgt))))
            result_js[i] = js_divergence(hgt.numpy(), hist_sampled.numpy())
        return result_js.mean()

    def eval(self, all_mol, plot_pwds=False, milestone=0):
        if plot_pwds:
            raise NotImplementedError("plotting (evaluators.py:289-349) is outside the hot path")
        return self.js_divergence_pwd(self.gt_hist, all_mol, self.gt_max, self.resolution)

    def unit_histograms(self, samples, unit_lengths, max_bytes=2 << 30):
        """(hist int32 CUDA (U, pairs, ld), nbins (pairs,), ref float64 (pairs, ld), units (U,)): the PWD histogram of every
        unit, one dff_pwd_hist call per unit into its slice, with the bins of the point estimate (the max over gt_max and all
        finite samples); ref is gt_hist padded with zeros.  The units are laid out on the frames as given; a frame with a
        non-finite coordinate is dropped whole, as eval does, and makes its unit shorter (units: the lengths after that)."""
        x = _to_device(samples, self.device)
        units = np.asarray(unit_lengths, np.int64).reshape(-1)
        if units.sum() != len(x) or (units < 0).any():
            raise ValueError(f"PwdEvaluator: unit lengths add up to {int(units.sum())}, not to the {len(x)} frames given")
        ok = torch.isfinite(x).all(dim=2).all(dim=1)
        self.samples_nonfinite = int((~ok).sum())
        if self.samples_nonfinite:
            kept = np.concatenate(([0], np.cumsum(ok.cpu().numpy().astype(np.int64))))
            ends = np.cumsum(units)
            units = kept[ends] - kept[ends - units]
            x = x[ok].contiguous()
        if len(x) == 0:
            raise ValueError(f"PwdEvaluator: no finite frame among the samples ({self.samples_nonfinite} with a non-finite coordinate)")
        maxval = torch.maximum(torch.as_tensor(self.gt_max).float().cpu(), binding.pwd_max(x, self.offset).cpu())
        nb = self._nbins(maxval, self.resolution, x.shape[1])
        hmax = torch.tensor([self.resolution * int(b) for b in nb], dtype=torch.float64).float()
        U, P, ld = len(units), len(nb), int(nb.max())
        if U * P * ld * 4 > max_bytes:
            raise ValueError(f"PwdEvaluator: the histograms of {U} units x {P} pairs x {ld} bins take {U * P * ld * 4} bytes, more "
                             f"than max_bytes = {max_bytes}: lower n_blocks (fewer, longer units) or raise max_bytes")
        hist = torch.empty((U, P, ld), dtype=torch.int32, device=self.device)
        nb32, hm = nb.to(torch.int32).to(self.device), hmax.to(self.device)
        start = 0
        for u, ln in enumerate(units.tolist()):
            binding.pwd_hist(x[start:start + ln], self.offset, nb32, hm, out=hist[u])
            start += ln
        ref = np.zeros((P, ld))
        for p, hgt in enumerate(self.gt_hist):
            m = min(len(hgt), ld)
            ref[p, :m] = np.asarray(hgt, np.float64)[:m]
        return hist, nb.numpy().astype(np.int32), ref, units

    def eval_bootstrap(self, samples, traj_lengths=None, block_frames=None, n_blocks=256, n_resamples=200, seed=0, *,
                       weights=None, unit_lengths=None, max_bytes=2 << 30):
        """Block bootstrap of eval(): JsBootstrap over the bead pairs (values: the mean over pairs, as eval averages them).
        Units: sample_units(n, traj_lengths, block_frames, n_blocks), or unit_lengths.  The bins per pair are the point
        estimate's, fixed for every resample."""
        units = _js_units(len(samples), traj_lengths, block_frames, n_blocks, unit_lengths)
        hist, nb, ref, units = self.unit_histograms(samples, units, max_bytes)
        return bootstrap_js(hist, nb, ref, n_resamples=n_resamples, seed=seed, weights=weights, unit_lengths=units,
                            device=self.device)


# =====================================================================================================
# Structure metrics of the reference's evaluators (evaluate/evaluators.py: Evaluator :28-111,
# DihedralEnergiesEvaluator :114-176, TicEvaluator :340-500, RmsdEvaluator :608-679, ContactEvaluator
# :735-859) on top of the HIP kernels dff_struct_* (csrc/dff_struct.hip).  Per-frame work (RMSD, dihedrals,
# TIC projections, contacts) runs on the GPU; the histogram and divergence reductions below run in numpy,
# written as the reference writes them, and are kept as functions of their own so that they can be checked
# on given per-frame values.  Plotting raises NotImplementedError; without the HIP library the evaluators
# raise DffLibraryError.
# =====================================================================================================
# PDB identifiers of the folded structures (datasets/dataset_utils_empty.py: Molecules) and the RMSD axis of
# the reference's saved free-energy curves (evaluators.py:624-633)
PROTEIN_IDS = {"chignolin": "CLN025", "trp_cage": "2JOF", "bba": "1FME", "villin": "2F4K", "protein_g": "NuG2"}
RMSD_CUTOFF_REF = {"chignolin": 10, "trp_cage": 12, "bba": 14, "villin": 14, "protein_g": 20}
RMSD_NBINS_REF = 100
# State presets of the reference's dynamics analysis (evaluate_fastfolders.ipynb, cell 21): the number of k-means
# clusters per protein and their centres in the plane of the first two TICs.  They belong to the reference's OWN saved
# TICA models (saved_TICA_*.pickle): a model fitted with evaluate.TICA has its own TIC signs and scale, and needs
# centres fitted on its own projections (StateTransitionEvaluator(fit_data=...)).  No preset exists for protein G.
STATE_COUNTS = {"chignolin": 3, "villin": 3, "trp_cage": 3, "bba": 4}
STATE_CENTERS = {
    "chignolin": ((0.69400153, -0.34598462), (-0.48732213, 0.00642035), (1.87483537, 0.06285344)),
    "trp_cage": ((-2.15921372, 0.0062795), (0.47752285, -0.38050238), (0.40182245, 2.0690773)),
    "bba": ((-0.5756589, -0.60663654), (1.7861676, -0.87717611), (0.91295128, 1.07518898), (-0.49210152, 0.40313689)),
    "villin": ((1.08971813, -0.98522752), (-2.49001353, -2.31375028), (-0.12929561, 0.53703407)),
}
K_BT_IN_KCAL_PER_MOL = 1.380650324e-23 * 300 * 6.02214076e23 / 1000 / 4.184   # evaluators_CGflowmatching.py:11-15


# ---- restricted unpickler: the reference's saved references without deeptime and without running code ----
class _Inert:
    """Stand-in for a deeptime class in a saved TICA pickle: keeps the pickled state as attributes, runs nothing."""

    def __new__(cls, *args, **kwargs):
        return object.__new__(cls)

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        else:
            self.__dict__["_state"] = state


_DEEPTIME_CLASSES = {
    ("deeptime.decomposition._tica", "TICA"),
    ("deeptime.decomposition._koopman", "CovarianceKoopmanModel"),
    ("deeptime.covariance._covariance", "WhiteningTransform"),
    ("deeptime.covariance._covariance", "CovarianceModel"),
    ("deeptime.basis._base", "Concatenation"),
    ("deeptime.basis._monomials", "Identity"),
}
_NUMPY_GLOBALS = {"ndarray", "dtype", "_reconstruct", "scalar"}


class RestrictedUnpickler(pickle.Unpickler):
    """Unpickler for the reference's saved references: numpy arrays, dtypes and scalars, and the six deeptime classes
    of a saved TICA model (mapped to inert stubs).  Any other global is refused."""

    def find_class(self, module, name):
        if (module, name) in _DEEPTIME_CLASSES:
            return type(name, (_Inert,), {"__module__": "dff_amd.evaluate.inert"})
        if module in ("numpy", "numpy.core.multiarray", "numpy._core.multiarray") and name in _NUMPY_GLOBALS:
            if name in ("ndarray", "dtype"):
                return getattr(np, name)
            core = np._core.multiarray if hasattr(np, "_core") else np.core.multiarray
            return getattr(core, name)
        raise pickle.UnpicklingError(f"saved reference names a global that is not allowed: {module}.{name}")


def restricted_load(path):
    with open(path, "rb") as f:
        return RestrictedUnpickler(io.BytesIO(f.read())).load()


def load_tica_reference(path, dim=2):
    """A saved TICA reference as plain arrays: {"mean" (F,), "coeff" (F, dim), "singular_values", "gt_prob",
    "bin_edges_x", "bin_edges_y"} (+ "cov_00" from a pickle).  `path` is the reference's own
    saved_TICA_*.pickle (read through RestrictedUnpickler) or an .npz holding those arrays.  The projection is
    (f - mean) @ coeff, coeff = the instantaneous whitening's sqrt_inv_cov[:, :dim] (kinetic-map scaling)."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            out = {k: np.asarray(z[k]) for k in z.files}
        out["coeff"] = out["coeff"][:, :dim]
        return out
    tica, gt_prob, edges_x, edges_y = restricted_load(path)
    model = tica._model
    white = model._whitening_instantaneous
    out = {"mean": np.asarray(white.mean, np.float64), "coeff": np.asarray(white.sqrt_inv_cov, np.float64)[:, :dim],
           "singular_values": np.asarray(model._singular_values, np.float64),
           "gt_prob": np.asarray(gt_prob), "bin_edges_x": np.asarray(edges_x), "bin_edges_y": np.asarray(edges_y)}
    cov = getattr(model, "_cov", None)
    if cov is not None and hasattr(cov, "_cov_00"):
        out["cov_00"] = np.asarray(cov._cov_00, np.float64)
    return out


# ---- TICA fitting: TICA(lagtime=100, dim=2).fit_transform(get_tic_features(...)) of evaluators.py:384-420 ----
# deeptime 0.4.4's estimator as the reference's pickles record it: symmetrised, mean removed, no Bessel correction
# (mean_t == mean_0, cov_tt == cov_00), kinetic-map scaling.  The sums come from the GPU (binding.tica_moments); the
# covariances and the decomposition below are float64 numpy.
TICA_MAX_DIM = 8          # components dff_struct_tic projects per call


def tica_covariances(sx, sy, m0, mt, w, shift):
    """(mean, cov_00, cov_0t) from the sums of dff_tica_moments over w frame pairs, features shifted by `shift`:
    mu' = (S_x + S_y) / 2w, mean = shift + mu', C00 = M_0 / 2w - mu' mu'^T, C0t = M_tau / 2w - mu' mu'^T.  m0 / mt
    hold upper triangles; they are mirrored."""
    w = int(w)
    if w <= 0:
        raise ValueError("TICA: no frame pairs at this lag time (every trajectory has <= lagtime frames)")
    sx, sy, shift = (np.asarray(a, np.float64) for a in (sx, sy, shift))
    mu = (sx + sy) / (2.0 * w)
    mm = np.outer(mu, mu)

    def sym(m):
        u = np.triu(np.asarray(m, np.float64))
        return u + np.triu(u, 1).T

    return shift + mu, sym(m0) / (2.0 * w) - mm, sym(mt) / (2.0 * w) - mm


def tica_from_covariances(cov_00, cov_0t, mean, dim=2, epsilon=1e-6, scaling="kinetic_map"):
    """TICA decomposition of symmetric C00 / C0t: {"mean", "coeff" (F, dim), "full_coeff" (F, rank),
    "singular_values" (rank,), "rank"}.
      1. eigh(C00), keep the eigenvalues > epsilon (their count is the rank), S = V diag(ev^-1/2);
      2. K = S^T C0t S, eigh(K), sorted by |eigenvalue| descending (the singular values, signed);
      3. kinetic-map coefficients W = S U diag(singular values).
    Column signs: the entry of largest magnitude of each column of W is positive (deeptime's signs follow no rule; a
    TIC's sign is arbitrary).  The projection is (f - mean) @ coeff."""
    if scaling != "kinetic_map":
        raise ValueError(f"TICA: only kinetic_map scaling is supported, not {scaling!r}")
    dim = int(dim)
    if not 1 <= dim <= TICA_MAX_DIM:
        raise ValueError(f"TICA: dim must be 1..{TICA_MAX_DIM}, not {dim}")
    c00 = np.asarray(cov_00, np.float64)
    c0t = np.asarray(cov_0t, np.float64)
    ev, V = np.linalg.eigh(c00)
    keep = ev > epsilon
    rank = int(keep.sum())
    if dim > rank:
        raise ValueError(f"TICA: dim = {dim} exceeds the rank {rank} of C00 at epsilon = {epsilon}")
    S = V[:, keep] / np.sqrt(ev[keep])
    K = S.T @ c0t @ S
    s, U = np.linalg.eigh((K + K.T) / 2)
    order = np.argsort(-np.abs(s), kind="stable")
    s, U = s[order], U[:, order]
    W = (S @ U) * s
    big = np.argmax(np.abs(W), axis=0)
    W = W * np.where(W[big, np.arange(W.shape[1])] < 0, -1.0, 1.0)
    return {"mean": np.asarray(mean, np.float64), "coeff": W[:, :dim].copy(), "full_coeff": W, "singular_values": s,
            "rank": rank}


def tica_timescales(singular_values, lagtime):
    """Implied timescales -lagtime / ln|s_i| (in frames)."""
    return -float(lagtime) / np.log(np.abs(np.asarray(singular_values, np.float64)))


class TICA:
    """TICA(lagtime, dim) fitted on the GPU: features and lag-tau moments by the HIP kernels (dff_tica_moments),
    covariances and decomposition in float64 numpy (tica_covariances, tica_from_covariances).

    partial_fit(traj) streams one time-ordered trajectory (n, N, 3) in Angstrom; fit(data, traj_lengths=None) starts
    afresh on an array (one trajectory, or back-to-back trajectories of `traj_lengths` frames) or a list of arrays (one
    trajectory each).  LangevinDiffusion.sample() returns its frames simulation-major: traj_lengths =
    [n_timesteps // save_interval] * parallel_sim fits the sampler's own runs.  Features are shifted by those of the
    first frame fitted, for the conditioning of the sums."""

    def __init__(self, lagtime, dim=2, epsilon=1e-6, *, device="cuda:0"):
        if int(lagtime) < 1:
            raise ValueError("TICA: lagtime must be >= 1")
        if not 1 <= int(dim) <= TICA_MAX_DIM:
            raise ValueError(f"TICA: dim must be 1..{TICA_MAX_DIM}")
        self.lagtime, self.dim, self.epsilon = int(lagtime), int(dim), float(epsilon)
        self.device = torch.device(device)
        binding.load_library()
        self._workspace = None
        self.reset()

    def reset(self):
        self.n_beads = None
        self._shift = self._acc = self._model = None
        self.n_pairs = 0
        return self

    def _accumulate(self, xyz, lengths):
        x = _frames(xyz, self.device)
        n, N = int(x.shape[0]), int(x.shape[1])
        lengths = [int(v) for v in lengths]
        if sum(lengths) != n or min(lengths, default=0) < 0:
            raise ValueError(f"TICA: trajectory lengths {lengths} do not add up to the {n} frames given")
        if n == 0:
            return self
        if self.n_beads is None:
            F = binding.struct_tic_num_features(N)
            if F == 0:
                raise ValueError("TICA: structures need at least 4 beads")
            self.n_beads = N
            self._shift = binding.struct_tic_features(x[:1])[0].double()
            self._acc = [torch.zeros(shape, dtype=torch.float64, device=self.device) for shape in ((F,), (F,), (F, F), (F, F))]
        elif N != self.n_beads:
            raise ValueError(f"TICA: fitted on {self.n_beads} beads, got {N}")
        need = binding.tica_workspace_bytes(N, n, self.lagtime)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        binding.tica_moments(x, lengths, self.lagtime, self._shift, *self._acc, workspace=self._workspace)
        self.n_pairs += sum(max(L - self.lagtime, 0) for L in lengths)
        self._model = None
        return self

    def partial_fit(self, traj):
        """Add one time-ordered trajectory (n, N, 3) to the running sums."""
        return self._accumulate(traj, [len(traj)])

    def fit(self, data, traj_lengths=None):
        self.reset()
        if isinstance(data, (list, tuple)):
            if traj_lengths is not None:
                raise ValueError("TICA.fit: traj_lengths applies to a single array, not to a list of trajectories")
            for traj in data:
                self.partial_fit(traj)
        else:
            self._accumulate(data, [len(data)] if traj_lengths is None else traj_lengths)
        self._estimate()
        return self

    def _estimate(self):
        if self._model is None:
            if self._acc is None:
                raise ValueError("TICA: no data fitted")
            sx, sy, m0, mt = (a.cpu().numpy() for a in self._acc)
            mean, c00, c0t = tica_covariances(sx, sy, m0, mt, self.n_pairs, self._shift.cpu().numpy())
            m = tica_from_covariances(c00, c0t, mean, self.dim, self.epsilon)
            m["cov_00"], m["cov_0t"] = c00, c0t
            self._model = m
        return self._model

    mean = property(lambda self: self._estimate()["mean"])
    cov_00 = property(lambda self: self._estimate()["cov_00"])
    cov_0t = property(lambda self: self._estimate()["cov_0t"])
    singular_values = property(lambda self: self._estimate()["singular_values"])
    coeff = property(lambda self: self._estimate()["coeff"])
    rank = property(lambda self: self._estimate()["rank"])

    def timescales(self):
        return tica_timescales(self.singular_values, self.lagtime)

    def transform(self, xyz):
        """(n, dim) float64 TIC projections of the structures xyz (n, N, 3) in Angstrom, on the GPU."""
        return binding.struct_tic(_frames(xyz, self.device), self.mean, self.coeff).cpu().numpy()

    def fit_transform(self, data, traj_lengths=None):
        self.fit(data, traj_lengths)
        x = torch.cat([_frames(d, self.device) for d in data]) if isinstance(data, (list, tuple)) else data
        return self.transform(x)

    def save(self, path, **extra):
        """Write an .npz that load_tica_reference reads (save_tica_model)."""
        save_tica_model(path, self._estimate(), self.lagtime, **extra)


def save_tica_model(path, model, lagtime, **extra):
    """Write a fitted model (tica_from_covariances' dict, + cov_00 / cov_0t when present) to `path` as an .npz of mean,
    coeff, singular_values, [cov_00, cov_0t,] lagtime and the `extra` arrays: what load_tica_reference reads."""
    arrays = {k: model[k] for k in ("mean", "coeff", "singular_values", "cov_00", "cov_0t") if k in model}
    with open(path, "wb") as f:
        np.savez(f, lagtime=np.int64(lagtime), **arrays, **extra)


# ---- host reductions, as the reference writes them ----
def get_prob(tors_data, n_bins=61):
    """evaluators_CGflowmatching.py:39-49: phi / psi histogram on linspace(-pi, pi, n_bins), normalised to sum 1."""
    bin_edges = np.linspace(-np.pi, np.pi, n_bins)
    hist, _, _ = np.histogram2d(tors_data[:, 0], tors_data[:, 1], bins=bin_edges, density=True)
    return hist / hist.sum()


def mse_free_energy(density1, density2):
    """evaluators_CGflowmatching.py:19-28 (mse)."""
    with np.errstate(divide="ignore"):
        U1 = K_BT_IN_KCAL_PER_MOL * np.log(density1)
        U2 = K_BT_IN_KCAL_PER_MOL * np.log(density2)
    U1 = np.where(np.isinf(U1), np.nan, U1)
    U2 = np.where(np.isinf(U2), np.nan, U2)
    count = np.sum(np.isfinite(U1 - U2))
    return np.nansum(np.square(U1 - U2)) / count


def kl_div(density1, density2):
    """evaluators_CGflowmatching.py:52-60."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = density2 / density1
    ratio[density1 == 0] = 1
    ratio[density2 == 0] = 1
    return -np.nansum(density1 * np.log(ratio))


def dihedral_scores(probs, gt_probs):
    """(mse, js, kl_1, kl_2) of DihedralEnergiesEvaluator.eval (evaluators.py:153-157)."""
    return (mse_free_energy(probs, gt_probs), js_divergence(probs, gt_probs), kl_div(probs, gt_probs),
            kl_div(gt_probs, probs))


def tic_js(proj, gt_prob, bin_edges_x, bin_edges_y):
    """TicEvaluator.eval's reduction (evaluators.py:463-470) of the (n, 2) projections: (js, prob_samp)."""
    prob_samp, _, _ = np.histogram2d(proj[:, 0], proj[:, 1], bins=[bin_edges_x, bin_edges_y], density=True)
    return js_divergence(gt_prob.flatten(), prob_samp.flatten()), prob_samp


def rmsd_curve(rmsd, nbins, cutoff=None):
    """RmsdEvaluator.eval's free-energy curve (evaluators.py:664-676) of per-frame RMSDs (NaN = invalid frame)."""
    rmsd = np.asarray(rmsd, np.float64)
    if cutoff is None:
        cutoff = rmsd[~np.isnan(rmsd)].max()
    h, bin_edges = np.histogram(rmsd, bins=nbins, range=[0, cutoff], density=True)
    out = {"bin_mids": (bin_edges[:-1] + bin_edges[1:]) / 2.0}
    with np.errstate(divide="ignore"):
        out["energies"] = -np.log(h)
    return out


def contact_bce_from_mismatch(mismatch, n_pairs):
    """Per-frame binary cross-entropy of _eval_bce_dynamics (evaluators.py:836-845) from mismatch counts, and its
    mean: contacts are 0 / 1 and torch clamps log at -100, so a mismatch costs exactly 100 and the float32 mean over
    the pairs is float32(100 m) / float32(n_pairs)."""
    m = torch.as_tensor(np.asarray(mismatch)).to(torch.float32)
    bce = (m * 100.0) / float(n_pairs)
    return bce.numpy(), bce.mean()


# ---- folded structures ----
_SOLVENT = {"HOH", "WAT", "SOL", "TIP", "TIP3", "NA", "CL", "K", "CA", "MG", "ZN", "SO4", "NA+", "CL-"}


def folded_ca(pdb_path, mol_name):
    """C-alpha coordinates (Angstrom, float64 (N, 3)) of a folded PDB by process_pdb's rule (evaluators.py:862-872):
    atoms named CA of the first model, solvent and ions removed; protein G keeps C-alphas [5:61]."""
    xyz = []
    with open(pdb_path) as f:
        for line in f:
            if line.startswith("ENDMDL"):
                break
            if not line.startswith(("ATOM  ", "HETATM")):
                continue
            if line[12:16].strip() != "CA" or line[17:21].strip() in _SOLVENT or line[16] not in " A":
                continue
            xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
    xyz = np.asarray(xyz, np.float64)
    if mol_name.upper() == "PROTEIN_G":
        xyz = xyz[5:61]
    return xyz


def _folded_coords(folded, mol_name):
    if isinstance(folded, (str, os.PathLike)):
        return folded_ca(folded, mol_name)
    return np.asarray(torch.as_tensor(folded).cpu(), np.float64).reshape(-1, 3)


def _frames(x, device):
    x = torch.as_tensor(x)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError("structures must be (n, n_beads, 3)")
    return x.to(device=device, dtype=torch.float32).contiguous()


def _reference_frames(ref_data):
    """The frames of an evaluator's ref_data: a tensor or an array as it is, else a dataset whose [:][0] they are."""
    if ref_data is None or isinstance(ref_data, (torch.Tensor, np.ndarray)):
        return ref_data
    return ref_data[:][0]


def _log10_ratio(a, b):
    """log10(a / b), NaN unless both are finite and positive; two lists of equal length go element by element."""
    if isinstance(a, list) or isinstance(b, list):
        if not (isinstance(a, list) and isinstance(b, list) and len(a) == len(b)):
            raise ValueError("_log10_ratio: two numbers, or two lists of equal length")
        return [_log10_ratio(u, v) for u, v in zip(a, b)]
    ok = np.isfinite(a) and np.isfinite(b) and a > 0 and b > 0
    return float(np.log10(a / b)) if ok else float("nan")


class DihedralEnergiesEvaluator:
    """Drop-in for evaluate.evaluators.DihedralEnergiesEvaluator (alanine dipeptide phi / psi free energy).
    `topology` is unused: the quadruples are the reference's [[0, 1, 2, 3], [1, 2, 3, 4]]."""

    def __init__(self, val_data, topology=None, plots_folder=None, n_bins=61,
                 saved_ref="./saved_references/saved_dih_probs_ala2_testset.pickle", *, device="cuda:0"):
        self.topology = topology
        self.plots_folder = plots_folder
        self.n_bins = n_bins
        self.device = torch.device(device)
        binding.load_library()
        if os.path.exists(saved_ref):
            self.gt_probs = np.asarray(restricted_load(saved_ref))
        else:
            self.gt_probs = get_prob(self.torsions(val_data), n_bins=self.n_bins)
            d = os.path.dirname(saved_ref)
            if d == "" or os.path.isdir(d):
                with open(saved_ref, "wb") as f:
                    pickle.dump(self.gt_probs, f)

    def torsions(self, xyz):
        """(n, 2) phi / psi in radians (get_torsions, evaluators_CGflowmatching.py:30-36), on the GPU."""
        return binding.struct_dihedrals(_frames(xyz, self.device))[:, :2].cpu().numpy()

    def eval(self, all_mol, plot_freeE=False, milestone=0, plot_title="Ramachandran plot", save_plot=True):
        if plot_freeE:
            raise NotImplementedError("plotting (evaluators.py:159-175) is outside the hot path")
        probs = get_prob(self.torsions(all_mol), n_bins=self.n_bins)
        return dihedral_scores(probs, self.gt_probs)

    def unit_histograms(self, samples, unit_lengths):
        """(hist int32 CUDA (U, 1, (n_bins - 1)^2), nbins (1,), ref (1, (n_bins - 1)^2), units): the phi / psi histogram of
        every unit on get_prob's grid, binned on the device; a frame without finite torsions is counted nowhere."""
        tors = binding.struct_dihedrals(_frames(samples, self.device))[:, :2]
        edges = np.linspace(-np.pi, np.pi, self.n_bins)
        nb = np.array([(self.n_bins - 1) ** 2], np.int32)
        units = np.asarray(unit_lengths, np.int64).reshape(-1)
        return unit_histograms(bin_indices_2d(tors, edges, edges), nb, units), nb, np.asarray(self.gt_probs, np.float64).reshape(1, -1), units

    def eval_bootstrap(self, samples, traj_lengths=None, block_frames=None, n_blocks=256, n_resamples=200, seed=0, *,
                       weights=None, unit_lengths=None):
        """Block bootstrap of eval()'s JS (the second of its four scores) on get_prob's grid -> JsBootstrap."""
        units = _js_units(len(samples), traj_lengths, block_frames, n_blocks, unit_lengths)
        hist, nb, ref, units = self.unit_histograms(samples, units)
        return bootstrap_js(hist, nb, ref, n_resamples=n_resamples, seed=seed, weights=weights, unit_lengths=units,
                            device=self.device)


class TicEvaluator:
    """Drop-in for evaluate.evaluators.TicEvaluator with a saved reference (the reference's own
    saved_TICA_*.pickle, read without deeptime, or an .npz of its arrays).  eval() returns (tic_js, None).

    Without a saved reference, `fit_data` (keyword-only: one time-ordered trajectory (n, N, 3) in Angstrom, or a list
    of them) fits TICA(lagtime, dim=2) on the GPU as evaluators.py:384-420 does on the sorted dataset, projects
    val_data, takes gt_prob = histogram2d(..., bins, density=True) and writes <saved_ref stem>.npz.  A later construction
    loads that .npz when it is named as saved_ref, or when it is given fit_data again (it does not refit then).  Without
    fit_data and without the saved_ref file, NotImplementedError as before."""

    def __init__(self, val_data, mol_name, eval_folder=None, data_folder=None, folded_pdb_folder="./datasets/folded_pdbs",
                 bins=101, saved_ref="none", evalset="testset", *, fit_data=None, lagtime=100, device="cuda:0"):
        self.mol_name = mol_name
        self.plots_folder = eval_folder
        self.bins = bins
        self.device = torch.device(device)
        binding.load_library()
        if saved_ref == "none":
            saved_ref = f"./saved_references/saved_TICA_{mol_name.upper()}_{evalset}.pickle"
        ref = None
        if not os.path.exists(saved_ref) and fit_data is not None:
            fitted_ref = os.path.splitext(saved_ref)[0] + ".npz"
            if os.path.exists(fitted_ref):           # fitted by an earlier construction: load it, do not refit
                saved_ref = fitted_ref
            else:
                ref = self._fit(val_data, fit_data, lagtime, fitted_ref)
        elif not os.path.exists(saved_ref):
            raise NotImplementedError(
                f"no saved TICA reference at {saved_ref}: fitting a new TICA model (evaluators.py:384-410) needs the "
                f"training dataset and deeptime and is not supported; pass the reference's saved_TICA_*.pickle or an "
                f".npz with mean, coeff, gt_prob, bin_edges_x, bin_edges_y")
        if ref is None:
            ref = load_tica_reference(saved_ref)
        self.mean, self.coeff = ref["mean"], ref["coeff"]
        self.gt_prob, self.bin_edges_x, self.bin_edges_y = ref["gt_prob"], ref["bin_edges_x"], ref["bin_edges_y"]
        self.bin_mids_x = (self.bin_edges_x[1:] + self.bin_edges_x[:-1]) / 2
        self.bin_mids_y = (self.bin_edges_y[1:] + self.bin_edges_y[:-1]) / 2
        self.bin_x_folded = self.bin_y_folded = None
        protid = PROTEIN_IDS.get(mol_name.lower())
        folded_pdb = f"{folded_pdb_folder}/{protid}.pdb"
        if protid is not None and os.path.exists(folded_pdb):      # the folded structure's bins (plots only)
            ft = self.transform(folded_ca(folded_pdb, mol_name)[None])[0]
            self.bin_x_folded = np.argmin(abs(self.bin_mids_x - ft[0]))
            self.bin_y_folded = np.argmin(abs(self.bin_mids_y - ft[1]))

    def _fit(self, val_data, fit_data, lagtime, path):
        """evaluators.py:384-420 on the GPU: fit, project val_data, histogram; write `path` (.npz) when its folder
        exists, and return the reference as load_tica_reference would read it back."""
        if val_data is None:
            raise ValueError("TicEvaluator: fitting a TICA model needs val_data for the reference histogram")
        trajs = list(fit_data) if isinstance(fit_data, (list, tuple)) else [fit_data]
        tica = TICA(lagtime, dim=2, device=self.device).fit(trajs)
        proj = tica.transform(val_data)
        gt_prob, edges_x, edges_y = np.histogram2d(proj[:, 0], proj[:, 1], bins=self.bins, density=True)
        d = os.path.dirname(path)
        if d == "" or os.path.isdir(d):
            tica.save(path, gt_prob=gt_prob, bin_edges_x=edges_x, bin_edges_y=edges_y)
        return {"mean": tica.mean, "coeff": tica.coeff, "gt_prob": gt_prob, "bin_edges_x": edges_x,
                "bin_edges_y": edges_y}

    def transform(self, xyz):
        """(n, dim) float64 TIC projections of the structures xyz (n, N, 3) in Angstrom, on the GPU."""
        return binding.struct_tic(_frames(xyz, self.device), self.mean, self.coeff).cpu().numpy()

    def eval(self, xyz_samples, title="", plot_tic=False, save_object=False, path=None, cmap="OrRd", gradient=True,
             steps=3, linewidth=2):
        if plot_tic:
            raise NotImplementedError("plotting (evaluators.py:472-500) is outside the hot path")
        js, prob_samp = tic_js(self.transform(xyz_samples), self.gt_prob, self.bin_edges_x, self.bin_edges_y)
        if save_object:
            for name, arr in (("prob_samp.npy", prob_samp), ("bin_mids_x.npy", self.bin_mids_x),
                              ("bin_mids_y.npy", self.bin_mids_y)):
                with open(name, "wb") as f:
                    np.save(f, arr)
        return js, None

    def unit_histograms(self, samples, unit_lengths):
        """(hist int32 CUDA (U, 1, nx ny), nbins (1,), ref (1, nx ny), units): the histogram of every unit's TIC projections on
        the reference's grid, projected and binned on the device (flattened as ix ny + iy, like gt_prob.flatten())."""
        proj = binding.struct_tic(_frames(samples, self.device), self.mean, self.coeff)
        nb = np.array([(len(self.bin_edges_x) - 1) * (len(self.bin_edges_y) - 1)], np.int32)
        units = np.asarray(unit_lengths, np.int64).reshape(-1)
        bins = bin_indices_2d(proj[:, :2], self.bin_edges_x, self.bin_edges_y)
        return unit_histograms(bins, nb, units), nb, np.asarray(self.gt_prob, np.float64).reshape(1, -1), units

    def eval_bootstrap(self, samples, traj_lengths=None, block_frames=None, n_blocks=256, n_resamples=200, seed=0, *,
                       weights=None, unit_lengths=None):
        """Block bootstrap of eval()'s JS: one channel of (len(edges_x) - 1) (len(edges_y) - 1) bins -> JsBootstrap."""
        units = _js_units(len(samples), traj_lengths, block_frames, n_blocks, unit_lengths)
        hist, nb, ref, units = self.unit_histograms(samples, units)
        return bootstrap_js(hist, nb, ref, n_resamples=n_resamples, seed=seed, weights=weights, unit_lengths=units,
                            device=self.device)


class RmsdEvaluator:
    """Drop-in for evaluate.evaluators.RmsdEvaluator.  `folded_pdb` is a PDB path (C-alphas by process_pdb's rule)
    or the folded C-alpha coordinates (N, 3) in Angstrom."""

    def __init__(self, mol_name, folded_pdb, eval_folder=None, *, saved_ref_dir="./saved_references", device="cuda:0"):
        self.plots_folder = eval_folder
        self.folded = _folded_coords(folded_pdb, mol_name)
        self.plot_dict = {}
        self.mol_name = mol_name
        self.device = torch.device(device)
        binding.load_library()
        self.saved_ref = os.path.join(saved_ref_dir, f"saved_rmsd_{mol_name.upper()}_reference_total.pickle")
        self.cutoff_dict_ref = dict(RMSD_CUTOFF_REF)
        self.cutoff_ref = self.cutoff_dict_ref[mol_name.lower()]
        self.nbins_ref = RMSD_NBINS_REF

    def rmsd(self, xyz):
        """(n,) float64 C-alpha RMSD (Angstrom) to the folded structure, NaN for frames with non-finite coordinates."""
        x = _frames(xyz, self.device)
        return binding.struct_rmsd(x, torch.from_numpy(self.folded).float()).cpu().numpy().astype(np.float64)

    def eval(self, method, xyz, nbins, cutoff=None, save_dynamics=False):
        if method == "Reference" and os.path.exists(self.saved_ref):
            assert nbins == self.nbins_ref and cutoff == self.cutoff_ref, \
                f"Reference data only exists for nbins={self.nbins_ref} and cutoff={self.cutoff_ref}"
            self.plot_dict[method] = dict(restricted_load(self.saved_ref))
            return
        rmsd = self.rmsd(xyz)
        self.plot_dict[method] = {}
        if save_dynamics:
            self.plot_dict[method]["rmsd"] = rmsd
        self.plot_dict[method].update(rmsd_curve(rmsd, nbins, cutoff))
        if method == "Reference" and os.path.isdir(os.path.dirname(self.saved_ref) or "."):
            with open(self.saved_ref, "wb") as f:
                pickle.dump(self.plot_dict[method], f)

    def _plot_rmsd(self, *args, **kwargs):
        raise NotImplementedError("plotting (evaluators.py:681-708) is outside the hot path")


class ContactEvaluator:
    """Drop-in for evaluate.evaluators.ContactEvaluator's numbers: the normalised contact count (:794-806) and the
    contact BCE to the folded structure (:829-859), without the plots."""

    def __init__(self, mol_name, folded_pdb, eval_folder=None, contact_cutoff=10, *, device="cuda:0"):
        self.mol_name = mol_name
        self.contact_cutoff = contact_cutoff
        self.plots_folder = eval_folder
        self.device = torch.device(device)
        binding.load_library()
        self.folded = torch.from_numpy(_folded_coords(folded_pdb, mol_name)).float()
        self.pwd_folded = torch.norm(self.folded[:, None, :] - self.folded[None, :, :], dim=-1)
        self.contacts_folded = self.pwd_folded < self.contact_cutoff

    def contact_counts(self, xyz, offset=3):
        """(counts (N, N) int64 over frames, mismatch (n,) int64 over pairs j >= i + offset), on the GPU."""
        counts, mism = binding.struct_contacts(_frames(xyz, self.device), self.contact_cutoff,
                                               self.contacts_folded.to(torch.uint8), offset)
        return counts.cpu(), mism.cpu()

    def normalized_contact_count(self, xyz):
        """norm_sum = contacts_samp.sum(dim=0) / len(contacts_samp), float32 (N, N)."""
        x = _frames(xyz, self.device)
        counts, _ = binding.struct_contacts(x, self.contact_cutoff)
        return counts.cpu() / len(x)

    def contact_bce(self, xyz):
        """(per-frame BCE float32 (n,), its mean) of _eval_bce_dynamics (offset 3)."""
        N = self.contacts_folded.shape[-1]
        _, mism = self.contact_counts(xyz, 3)
        return contact_bce_from_mismatch(mism.numpy(), binding.pwd_num_pairs(N, 3))


class Evaluator:
    """Drop-in for evaluate.evaluators.Evaluator: Dihedral JS (alanine), TIC JS (every protein but protein G) and
    PWD JS (all but protein G), composed as the reference composes them.  ref_data may be None when the saved
    references exist (found under `saved_ref_dir`).  The reference hands `evalsetname` to its TIC and PWD
    evaluators, which name it `evalset`; here it is passed on as evalset, "" meaning their default "testset".
    `tica_fit_data` (keyword-only) is TicEvaluator's fit_data: the trajectories a TICA model is fitted on when no saved
    TICA reference exists, at lag time `tica_lagtime` frames."""

    def __init__(self, ref_data, topology=None, mol_name="alanine", eval_folder=None,
                 folded_pdb_folder="./datasets/folded_pdbs", data_folder="./data", evalsetname="", *,
                 saved_ref_dir="./saved_references", tica_fit_data=None, tica_lagtime=100, device="cuda:0"):
        self.ref_data = ref_data = _reference_frames(ref_data)
        self.topology = topology
        self.eval_folder = eval_folder
        self.folded_pdb_folder = folded_pdb_folder
        self.mol_name = mol_name
        evalset = evalsetname or "testset"
        if "alanine" in mol_name:
            self.dihedral_evaluator = DihedralEnergiesEvaluator(
                ref_data, topology, eval_folder,
                saved_ref=os.path.join(saved_ref_dir, "saved_dih_probs_ala2_testset.pickle"), device=device)
        elif "protein_g" != mol_name.lower():
            tic_ref = os.path.join(saved_ref_dir, f"saved_TICA_{mol_name.upper()}_{evalset}")
            tic_ref = tic_ref + ".npz" if os.path.exists(tic_ref + ".npz") else tic_ref + ".pickle"
            self.tic = TicEvaluator(ref_data, mol_name, eval_folder=eval_folder, data_folder=data_folder,
                                    folded_pdb_folder=folded_pdb_folder, saved_ref=tic_ref, evalset=evalset,
                                    fit_data=tica_fit_data, lagtime=tica_lagtime, device=device)
        if "protein_g" != mol_name.lower():
            pwd_ref = os.path.join(saved_ref_dir, f"saved_pwd_{mol_name.upper()}_{evalset}_offset_0.pickle")
            if ref_data is None and not os.path.exists(pwd_ref):
                raise ValueError(f"PWD evaluation needs ref_data or a saved reference at {pwd_ref}")
            self.pwd_evaluator = PwdEvaluator(ref_data, eval_folder, mol_name, saved_ref=pwd_ref, evalset=evalset,
                                              device=device)

    def eval(self, sampled_mol, milestone=0, save_plots=False):
        dict_results = {}
        if "alanine" in self.mol_name:
            _, dihedral_js, _, _ = self.dihedral_evaluator.eval(sampled_mol, save_plots, milestone)
            dict_results["Dihedral JS"] = float(dihedral_js)
        elif "protein_g" != self.mol_name.lower():
            dict_results["TIC JS"] = float(self.tic.eval(sampled_mol, title=f"tic_{milestone}", plot_tic=save_plots)[0])
        if "protein_g" != self.mol_name.lower():
            dict_results["PWD JS"] = float(self.pwd_evaluator.eval(sampled_mol))
        if self.eval_folder is not None:
            with open(os.path.join(self.eval_folder, f"results-{milestone}.json"), "w") as f:
                json.dump(dict_results, f)
        return dict_results

    def eval_bootstrap(self, samples, traj_lengths=None, block_frames=None, n_blocks=256, n_resamples=200, seed=0,
                       confidence=0.95):
        """eval()'s keys with block-bootstrap error bars: "<key>" (the point estimate in fp64 on the bootstrap's bins: eval()'s
        number up to its float32 rounding), "<key>_lo" / "_hi" (the percentile interval at `confidence`), "_std", "_bias"
        (mean over the resamples - point), and "n_units", "n_resamples".  One weight matrix serves all metrics: they are
        resampled jointly.  Nothing is written to eval_folder."""
        units = sample_units(len(samples), traj_lengths, block_frames, n_blocks)
        weights = bootstrap_weights(len(units), n_resamples, seed)
        res = {}
        kw = dict(unit_lengths=units, weights=weights)
        if "alanine" in self.mol_name:
            res.update(js_error_bars("Dihedral JS", self.dihedral_evaluator.eval_bootstrap(samples, **kw), confidence))
        elif "protein_g" != self.mol_name.lower():
            res.update(js_error_bars("TIC JS", self.tic.eval_bootstrap(samples, **kw), confidence))
        if "protein_g" != self.mol_name.lower():
            res.update(js_error_bars("PWD JS", self.pwd_evaluator.eval_bootstrap(samples, **kw), confidence))
        res["n_units"], res["n_resamples"] = int(len(units)), int(weights.shape[0])
        return res


# =====================================================================================================
# Dynamics: states in TIC space and the transitions between them (evaluate_fastfolders.ipynb, cells 20-24)
# deeptime 0.4.4 and its MiniBatchKMeans / TransitionCountEstimator are not installed where this was written, so they
# could not be run side by side; what follows restates their documented semantics: fit_transform with max_iter=0 and
# initial_centers assigns every point to its nearest centre (Euclidean, lowest index on a tie), and count("sliding",
# dtrajs, lagtime) counts every pair (t, t + lagtime) inside each discrete trajectory.
def transition_matrix(counts):
    """Row-normalise count matrices (..., K, K) to transition probabilities, as sklearn.preprocessing.normalize(counts,
    axis=1, norm="l1") does: every row is divided by the sum of its absolute values, an all-zero row stays zero."""
    c = np.asarray(counts, np.float64)
    norm = np.abs(c).sum(axis=-1, keepdims=True)
    norm[norm == 0.0] = 1.0
    return c / norm


def msm_timescales(T, lagtime):
    """Implied timescales -lagtime / ln|lambda_i|, i >= 2, of the eigenvalues of the transition matrix T (K, K) sorted
    by magnitude, largest first (in frames; the stationary eigenvalue lambda_1 is left out)."""
    lam = np.abs(np.linalg.eigvals(np.asarray(T, np.float64)))
    lam = np.sort(lam)[::-1][1:]
    with np.errstate(divide="ignore"):
        return -float(lagtime) / np.log(lam)


def _points(points, device):
    p = torch.as_tensor(points)
    if p.dim() != 2:
        raise ValueError("points must be (n, d)")
    return p.to(device=device, dtype=torch.float64).contiguous()


class KMeans:
    """Lloyd's k-means on the GPU (dff_kmeans_step per iteration; centres and the stopping rule on the host in float64).

    A centre is the mean of its members; a cluster that lost all members keeps its centre.  Iteration i assigns to the
    current centres (inertia_i = the sum of the squared distances to them), then moves them; it stops after the
    iteration with |inertia_{i-1} - inertia_i| <= tolerance * inertia_{i-1}, or after max_iter iterations.  `inertia` is
    that of the final centres.  init="kmeans++": the first centre is drawn uniformly, every further one with probability
    proportional to the squared distance to the nearest centre drawn so far (torch on the device, generator seeded by
    `seed`); initial_centers (K, d) overrides it.  max_iter=0 with initial_centers only assigns: the reference's
    MiniBatchKMeans(max_iter=0, initial_centers=...).fit_transform call.  Points with a non-finite coordinate get label
    -1 and take part in nothing."""

    # what a subclass for another pair of library calls overrides: the limit and the two calls (looked up in the binding
    # at every call)
    MAX_CLUSTERS = 64

    def _step(self, *args, **kw):
        return binding.kmeans_step(*args, **kw)

    def _workspace_bytes(self, n, d):
        return binding.kmeans_workspace_bytes(n, d, self.n_clusters)

    def __init__(self, n_clusters, max_iter=100, tolerance=1e-5, init="kmeans++", initial_centers=None, seed=0, *,
                 device="cuda:0"):
        self.n_clusters, self.max_iter, self.tolerance = int(n_clusters), int(max_iter), float(tolerance)
        if not 1 <= self.n_clusters <= self.MAX_CLUSTERS:
            raise ValueError(f"{type(self).__name__}: n_clusters must be 1..{self.MAX_CLUSTERS}")
        if self.max_iter < 0:
            raise ValueError(f"{type(self).__name__}: max_iter must be >= 0")
        if initial_centers is None and init != "kmeans++":
            raise ValueError(f"{type(self).__name__}: init must be 'kmeans++' (or give initial_centers), not {init!r}")
        self.init, self.seed = init, int(seed)
        self.initial_centers = None
        if initial_centers is not None:
            c = np.array(initial_centers, np.float64)
            if c.ndim != 2 or c.shape[0] != self.n_clusters or not np.all(np.isfinite(c)):
                raise ValueError(f"{type(self).__name__}: initial_centers must be finite and ({self.n_clusters}, d)")
            self.initial_centers = c
        self.device = torch.device(device)
        binding.load_library()
        self.cluster_centers = self.inertia = None
        self.n_iter = 0

    def _seed_centers(self, pts):
        n, K = int(pts.shape[0]), self.n_clusters
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.seed)
        finite = torch.isfinite(pts).all(dim=1)
        idx = torch.nonzero(finite).reshape(-1)
        if idx.numel() < K:
            raise ValueError(f"{type(self).__name__}: {int(idx.numel())} finite points for {K} clusters")
        first = idx[torch.randint(int(idx.numel()), (1,), generator=gen, device=self.device)]
        centers = pts[first].clone()
        for _ in range(1, K):
            d2 = torch.nan_to_num(self._step(pts, centers, accumulate=False)["dist2"], nan=0.0)
            cum = torch.cumsum(d2, 0)
            u = torch.rand(1, dtype=torch.float64, generator=gen, device=self.device) * cum[-1]
            nxt = torch.searchsorted(cum, u, right=True).clamp_(max=n - 1)
            if not bool(d2[nxt] > 0):                 # every point sits on a centre already: any finite point will do
                nxt = first
            centers = torch.cat([centers, pts[nxt]])
        return centers.cpu().numpy()

    def fit(self, points):
        pts = _points(points, self.device)
        n, d = int(pts.shape[0]), int(pts.shape[1])
        if self.initial_centers is not None:
            if self.initial_centers.shape[1] != d:
                raise ValueError(f"{type(self).__name__}: initial_centers are {self.initial_centers.shape}, points have d = {d}")
            centers = self.initial_centers.copy()
        else:
            centers = self._seed_centers(pts)
        ws = torch.empty(max(self._workspace_bytes(n, d), 8), dtype=torch.uint8, device=self.device)
        prev, self.n_iter = None, 0
        for _ in range(self.max_iter):
            r = self._step(pts, centers, workspace=ws)
            sums, counts, inertia = r["sums"].cpu().numpy(), r["counts"].cpu().numpy(), float(r["inertia"][0])
            has = counts > 0
            centers = centers.copy()
            centers[has] = sums[has] / counts[has, None]
            self.n_iter += 1
            if prev is not None and abs(prev - inertia) <= self.tolerance * prev:
                break
            prev = inertia
        self.cluster_centers = centers
        self.inertia = float(self._step(pts, centers, workspace=ws)["inertia"][0])
        return self

    def _assign(self, pts):
        if self.cluster_centers is None:
            raise ValueError(f"{type(self).__name__}: not fitted")
        return self._step(pts, self.cluster_centers, accumulate=False)["labels"]

    def transform(self, points):
        """(n,) int32 labels of the nearest centre."""
        return self._assign(_points(points, self.device)).cpu().numpy()

    def fit_transform(self, points):
        pts = _points(points, self.device)
        return self.fit(pts)._assign(pts).cpu().numpy()


def kmeans_inertias(points, ks, *, max_iter=100, tolerance=1e-5, seed=0, device="cuda:0"):
    """The inertia of KMeans(k).fit(points) for every k of `ks` (float64 array): the curve of the elbow method."""
    pts = _points(points, torch.device(device))
    return np.array([KMeans(k, max_iter, tolerance, seed=seed, device=device).fit(pts).inertia for k in ks])


def _tica_arrays(tica, dim=2):
    if isinstance(tica, (str, os.PathLike)):
        ref = load_tica_reference(tica, dim)
        return ref["mean"], ref["coeff"]
    if isinstance(tica, (tuple, list)) and len(tica) == 2:
        return np.asarray(tica[0], np.float64), np.asarray(tica[1], np.float64)
    if hasattr(tica, "mean") and hasattr(tica, "coeff"):             # TicEvaluator, TICA
        return np.asarray(tica.mean, np.float64), np.asarray(tica.coeff, np.float64)
    raise ValueError("tica must be a TicEvaluator, a TICA, a saved-reference path or a (mean, coeff) pair")


def _tica_model(tica, what, max_dim=None):
    """(mean (F,), coeff (F, k)) of _tica_arrays(tica), shapes checked; max_dim bounds k for the callers that project
    through dff_struct_tic (TICA_MAX_DIM)."""
    mean, coeff = _tica_arrays(tica)
    if coeff.ndim != 2 or mean.shape != (coeff.shape[0],) or not (max_dim is None or 1 <= coeff.shape[1] <= max_dim):
        raise ValueError(f"{what}: mean must be (F,) and coeff (F, k)" + ("" if max_dim is None else f", k <= {max_dim}"))
    return mean, coeff


def _check_lengths(traj_lengths, n):
    lengths = [int(n)] if traj_lengths is None else [int(v) for v in traj_lengths]
    if sum(lengths) != n or min(lengths, default=0) < 0:
        raise ValueError(f"trajectory lengths add up to {sum(lengths)}, not to the {n} frames given")
    return lengths


class StateTransitionEvaluator:
    """The reference's dynamics analysis (evaluate_fastfolders.ipynb, cells 20-24) on the GPU: frames -> TIC projection
    -> nearest state centre (one fused kernel) -> sliding-window transition counts -> transition probabilities.

    `tica` is a TicEvaluator, an evaluate.TICA, the path of a saved reference, or a (mean, coeff) pair.  `centers`
    (K, k) are the states; None takes the reference's preset for `mol_name` (STATE_CENTERS: only meaningful with the
    reference's own saved TICA model) or, with `fit_data` (structures (n, N, 3) in Angstrom), fits
    KMeans(n_clusters) on the projections of fit_data (n_clusters defaults to STATE_COUNTS[mol_name]).
    eval(xyz, traj_lengths=None, ...) treats the frames as ONE trajectory, which reproduces the notebook exactly -- it
    also counts the jump from the last frame of one simulation to the first of the next; traj_lengths =
    [n_timesteps // save_interval] * parallel_sim gives the correct counts for LangevinDiffusion.sample()'s
    simulation-major output.  A traj_lengths given at construction is eval's default."""

    def __init__(self, mol_name, tica, centers=None, *, n_clusters=None, fit_data=None, traj_lengths=None,
                 seed=0, device="cuda:0"):
        self.mol_name = mol_name
        self.device = torch.device(device)
        self.traj_lengths = traj_lengths
        mol = str(mol_name).lower()
        if centers is None and fit_data is None:
            if n_clusters is not None:
                raise ValueError("StateTransitionEvaluator: n_clusters needs fit_data to fit the centres on")
            if mol not in STATE_CENTERS:
                raise ValueError(f"StateTransitionEvaluator: no preset state centres for {mol_name!r}; pass centers, or "
                                 f"fit_data and n_clusters")
            centers = STATE_CENTERS[mol]
        self.mean, self.coeff = _tica_model(tica, "StateTransitionEvaluator")
        binding.load_library()
        self.kmeans = None
        if centers is None:
            k = n_clusters if n_clusters is not None else STATE_COUNTS.get(mol)
            if k is None:
                raise ValueError(f"StateTransitionEvaluator: n_clusters is needed to fit centres for {mol_name!r}")
            proj = binding.struct_tic(_frames(fit_data, self.device), self.mean, self.coeff)
            self.kmeans = KMeans(k, seed=seed, device=self.device).fit(proj)
            centers = self.kmeans.cluster_centers
        self.centers = np.array(centers, np.float64)
        if self.centers.ndim != 2 or self.centers.shape[1] != self.coeff.shape[1] or not np.all(np.isfinite(self.centers)):
            raise ValueError(f"StateTransitionEvaluator: centers must be finite and (K, {self.coeff.shape[1]})")
        if n_clusters is not None and int(n_clusters) != len(self.centers):
            raise ValueError(f"StateTransitionEvaluator: {len(self.centers)} centers given, n_clusters = {n_clusters}")
        self.n_states = len(self.centers)

    def _assign(self, xyz):
        return binding.struct_tic_assign(_frames(xyz, self.device), self.mean, self.coeff, self.centers)

    def assign(self, xyz):
        """(n,) int32 state labels of the structures xyz (n, N, 3) in Angstrom; -1 for a frame with a non-finite
        projection."""
        return self._assign(xyz).cpu().numpy()

    def eval(self, xyz, traj_lengths=None, lagtimes=(1,), plot_assignments=False, plot_transitions=False):
        if plot_assignments or plot_transitions:
            raise NotImplementedError("plotting (evaluate_fastfolders.ipynb, cells 23-24) is outside the hot path")
        n = len(xyz)
        lengths = _check_lengths(self.traj_lengths if traj_lengths is None else traj_lengths, n)
        lagtimes = [int(v) for v in lagtimes]
        labels = self._assign(xyz)
        counts = binding.transition_counts(labels, lengths, lagtimes, self.n_states).cpu().numpy()
        lab = labels.cpu().numpy()
        pop = np.bincount(lab[lab >= 0], minlength=self.n_states).astype(np.float64)
        T = transition_matrix(counts)
        return {"assignments": lab, "populations": pop / max(pop.sum(), 1.0), "count_matrices": counts,
                "transition_matrices": T, "lagtimes": lagtimes,
                "timescales": [msm_timescales(T[i], lag) for i, lag in enumerate(lagtimes)]}


# =====================================================================================================
# Novelty, coverage and diversity: nearest-structure RMSD between two ensembles (dff_rmsd_nearest / dff_rmsd_matrix,
# csrc/dff_ensemble.hip).  The reference has no counterpart: its only RMSD is md.rmsd to ONE folded structure
# (evaluators.py:656-662); this applies the same distance between every sample and every reference frame.
# =====================================================================================================
NEAREST_CHUNK = 1 << 18        # queries per dff_rmsd_nearest call of nearest_rmsd (12 N bytes of fp32 frames each)


def nearest_rmsd(xyz, refs, *, exclude_self=False, chunk=None, device="cuda:0"):
    """For every structure of xyz (n, N, 3) the RMSD (Angstrom, optimal proper rotation) to its nearest structure of refs
    (m, N, 3), and that structure's index -> (rmsd float32 (n,), index int64 (n,)), torch tensors on `device`.  NaN / -1
    for a structure with a non-finite coordinate or without a usable candidate; non-finite candidates are never nearest;
    the lowest index wins among equal RMSDs.  The queries go to the device `chunk` at a time (default NEAREST_CHUNK), refs
    once; the result does not depend on `chunk`.  exclude_self=True (xyz is refs, or the same shape: the same ensemble)
    leaves out the pair of a structure with itself: the nearest OTHER structure."""
    dev = torch.device(device)
    same = xyz is refs
    y = _frames(refs, dev)
    xs = y
    if not same:
        xs = torch.as_tensor(xyz)
        if xs.dim() != 3 or xs.shape[-1] != 3:
            raise ValueError("structures must be (n, n_beads, 3)")
        if int(xs.shape[1]) != int(y.shape[1]):
            raise ValueError(f"xyz has {int(xs.shape[1])} beads, refs {int(y.shape[1])}")
        if exclude_self and tuple(xs.shape) != tuple(y.shape):
            raise ValueError("exclude_self needs xyz and refs to be the same ensemble (xyz is refs, or equal shapes)")
    chunk = NEAREST_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    n = len(xs)
    rmsd = torch.empty(n, dtype=torch.float32, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    ws = None
    for o in range(0, n, chunk):
        xc = _frames(xs[o:o + chunk], dev)
        if ws is None:
            ws = torch.empty(max(binding.rmsd_nearest_workspace_bytes(len(xc), len(y), int(y.shape[1])), 1),
                             dtype=torch.uint8, device=dev)
        r, i = binding.rmsd_nearest(xc, y, self_first=o if exclude_self else -1, workspace=ws)
        rmsd[o:o + len(xc)] = r
        index[o:o + len(xc)] = i
    return rmsd, index


def rmsd_matrix(a, b, *, device="cuda:0"):
    """RMSD (Angstrom, optimal proper rotation) between every structure of a (n, N, 3) and every structure of b (m, N, 3)
    -> float32 tensor (n, m) on `device`; for small sets (n * m <= 2^28).  nearest_rmsd is its row minimum, bit for bit."""
    dev = torch.device(device)
    return binding.rmsd_matrix(_frames(a, dev), _frames(b, dev))


def nearest_summary(d, prefix, stats=("mean", "median")):
    """{prefix_rmsd_<stat>: float} over the entries of the nearest-RMSD tensor d (n,) that are not NaN (NaN = a frame left
    out); NaN when none is left.  stats out of mean, median (the mean of the two middle values for an even count, as
    numpy), min, max.  Reduced where d lives: only scalars are read."""
    v = d[~torch.isnan(d)].double()
    k = int(v.numel())
    out = {}
    for s in stats:
        if k == 0:
            val = float("nan")
        elif s == "median":
            sv = torch.sort(v).values
            val = float((sv[(k - 1) // 2] + sv[k // 2]) / 2)
        else:
            val = float(getattr(v, s)())
        out[f"{prefix}_rmsd_{s}"] = val
    return out


def share_within(d, delta, inclusive=True):
    """Share of the non-NaN entries of d at most (inclusive) or strictly less than (not inclusive) delta; NaN when every
    entry is NaN."""
    ok = ~torch.isnan(d)
    k = int(ok.sum())
    if k == 0:
        return float("nan")
    hit = (d <= delta) if inclusive else (d < delta)          # NaN compares false
    return float(hit.sum()) / k


def _count_nonfinite(x):
    return int((~torch.isfinite(x).all(dim=2).all(dim=1)).sum())


class EnsembleCoverageEvaluator:
    """How a sampled ensemble sits against a reference ensemble, by nearest-structure RMSD on the GPU.

    ref_data (m, N, 3) in Angstrom: the training structures (for novelty) or a held-out set (for coverage); it is
    uploaded once.  eval(samples) returns a plain dict of floats, d in Angstrom and delta running over `thresholds`:
      novelty_rmsd_{mean,median,min}    samples -> their nearest reference structure
      precision@delta                   share of samples with a reference structure within delta (d <= delta)
      coverage_rmsd_{mean,median,max}   reference structures -> their nearest sample
      recall@delta                      share of reference structures with a sample within delta (d <= delta)
      diversity_rmsd_{mean,median}      samples -> their nearest OTHER sample
      duplicates@delta_min              share of samples with another sample closer than the smallest threshold (d < delta_min)
      samples_nonfinite, refs_nonfinite frames with a non-finite coordinate: left out of every statistic on their side
                                        and never anybody's nearest structure
    Shares and means are over the frames that are left.  Without the HIP library: DffLibraryError."""

    def __init__(self, ref_data, mol_name="", thresholds=(1.0, 2.0, 4.0), *, chunk=None, device="cuda:0"):
        self.mol_name = mol_name
        self.thresholds = tuple(float(t) for t in thresholds)
        if not self.thresholds or min(self.thresholds) <= 0:
            raise ValueError("EnsembleCoverageEvaluator: thresholds must be positive")
        self.chunk = chunk
        self.device = torch.device(device)
        binding.load_library()
        self.refs = _frames(_reference_frames(ref_data), self.device)
        self.refs_nonfinite = _count_nonfinite(self.refs)

    def nearest(self, samples):
        """The three nearest-RMSD tensors on the device: {"novelty" (n,), "coverage" (m,), "diversity" (n,)}."""
        x = _frames(samples, self.device)
        if x.shape[1] != self.refs.shape[1]:
            raise ValueError(f"samples have {int(x.shape[1])} beads, the reference ensemble {int(self.refs.shape[1])}")
        kw = dict(chunk=self.chunk, device=self.device)
        return x, {"novelty": nearest_rmsd(x, self.refs, **kw)[0], "coverage": nearest_rmsd(self.refs, x, **kw)[0],
                   "diversity": nearest_rmsd(x, x, exclude_self=True, **kw)[0]}

    def summarize(self, novelty, coverage, diversity, samples_nonfinite=0, refs_nonfinite=0):
        """eval()'s dict from the three nearest-RMSD tensors (NaN = a frame left out)."""
        out = nearest_summary(novelty, "novelty", ("mean", "median", "min"))
        for t in self.thresholds:
            out[f"precision@{t:g}"] = share_within(novelty, t)
        out.update(nearest_summary(coverage, "coverage", ("mean", "median", "max")))
        for t in self.thresholds:
            out[f"recall@{t:g}"] = share_within(coverage, t)
        out.update(nearest_summary(diversity, "diversity", ("mean", "median")))
        tmin = min(self.thresholds)
        out[f"duplicates@{tmin:g}"] = share_within(diversity, tmin, inclusive=False)
        out["samples_nonfinite"] = float(samples_nonfinite)
        out["refs_nonfinite"] = float(refs_nonfinite)
        return out

    def eval(self, samples):
        x, d = self.nearest(samples)
        return self.summarize(d["novelty"], d["coverage"], d["diversity"], _count_nonfinite(x), self.refs_nonfinite)


# =====================================================================================================
# Superposition on a reference: aligned frames, mean structure, per-bead fluctuation (dff_superpose, csrc/dff_superpose.hip).
# The reference's data pipeline puts a trajectory into a common frame with traj.superpose(traj, 0)
# (datasets/dataset_utils_empty.py:319-321); its evaluators have no per-bead flexibility metric.
# =====================================================================================================
SUPERPOSE_CHUNK = 1 << 20      # frames per dff_superpose call of superpose / superpose_stats


def _superpose_chunks(xyz, ref, chunk, device):
    """(device, reference (N, 3) float32 on it, the frames as given, chunk size) after the argument checks"""
    dev = torch.device(device)
    xs = torch.as_tensor(xyz)
    if xs.dim() != 3 or xs.shape[-1] != 3:
        raise ValueError("structures must be (n, n_beads, 3)")
    r = torch.as_tensor(ref)
    if tuple(r.shape) != (int(xs.shape[1]), 3):
        raise ValueError(f"xyz has {int(xs.shape[1])} beads, the reference structure has shape {tuple(r.shape)}")
    chunk = SUPERPOSE_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    return dev, r.to(device=dev, dtype=torch.float32).contiguous(), xs, chunk


def superpose(xyz, ref, *, return_rotations=False, chunk=None, device="cuda:0"):
    """Every structure of xyz (n, N, 3) rotated (optimal proper rotation) and moved onto ref (N, 3): float32 tensor
    (n, N, 3) on `device`, the frames on ref's centroid as mdtraj's superpose leaves them; with return_rotations also the
    rotations, float64 (n, 3, 3).  NaN rows for a structure with a non-finite coordinate.  The frames go to the device
    `chunk` at a time (default SUPERPOSE_CHUNK); the result does not depend on `chunk`."""
    dev, r, xs, chunk = _superpose_chunks(xyz, ref, chunk, device)
    n, N = int(xs.shape[0]), int(xs.shape[1])
    aligned = torch.empty((n, N, 3), dtype=torch.float32, device=dev)
    rot = torch.empty((n, 3, 3), dtype=torch.float64, device=dev) if return_rotations else None
    for o in range(0, n, chunk):
        xc = _frames(xs[o:o + chunk], dev)
        res = binding.superpose(xc, r, rot=return_rotations, out=aligned[o:o + len(xc)])
        if return_rotations:
            rot[o:o + len(xc)] = res["rot"]
    return (aligned, rot) if return_rotations else aligned


def superpose_stats(xyz, ref, *, chunk=None, device="cuda:0"):
    """The sums a mean structure and an RMSF are made of, over the finite structures of xyz (n, N, 3) superposed on ref
    (N, 3, used as float32): (dsum float64 (N, 3), dsq float64 (N,), count int) with d = aligned - ref in float64 on the
    device.  One dff_superpose call per chunk with no aligned output; the chunks' sums are added here in float64."""
    dev, r, xs, chunk = _superpose_chunks(xyz, ref, chunk, device)
    N = int(xs.shape[1])
    dsum, dsq, count = np.zeros((N, 3)), np.zeros(N), 0
    ws = None
    for o in range(0, len(xs), chunk):
        xc = _frames(xs[o:o + chunk], dev)
        if ws is None:
            ws = torch.empty(max(binding.superpose_workspace_bytes(len(xc), N), 8), dtype=torch.uint8, device=dev)
        res = binding.superpose(xc, r, aligned=False, stats=True, workspace=ws)
        dsum += res["dsum"].cpu().numpy()
        dsq += res["dsq"].cpu().numpy()
        count += int(res["count"])
    return dsum, dsq, count


def _first_finite_frame(xyz):
    xs = torch.as_tensor(xyz)
    ok = torch.isfinite(xs).reshape(len(xs), -1).all(dim=1)
    if not bool(ok.any()):
        raise ValueError("no structure with finite coordinates")
    return xs[int(torch.nonzero(ok)[0])]


def _as_ref32(ref):
    """the reference as the kernel sees it (float32), in float64"""
    return np.asarray(torch.as_tensor(ref).detach().cpu().to(torch.float32), np.float64).reshape(-1, 3)


def mean_structure(xyz, ref=None, max_iter=10, tol=1e-4, *, chunk=None, device="cuda:0", aligner=None):
    """Mean structure of the ensemble xyz (n, N, 3) by generalised Procrustes -> (mean float64 (N, 3), n_iter).
    All finite structures are superposed on the current reference (ref, or the first finite structure when None), the mean
    of the superposed structures -- reference + dsum / count -- becomes the next reference, until the RMSD between
    successive means (they share a frame: no further rotation) falls below tol Angstrom; n_iter counts the passes over
    the ensemble, each one dff_superpose call per chunk with no aligned output.  Without convergence in max_iter passes
    the last mean is returned with a RuntimeWarning.  aligner(xyz, ref) -> (dsum, dsq, count) replaces superpose_stats
    (for tests of this loop without a GPU)."""
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    if aligner is None:
        def aligner(x, r):
            return superpose_stats(x, r, chunk=chunk, device=device)
    cur = _as_ref32(_first_finite_frame(xyz) if ref is None else ref)
    for it in range(1, max_iter + 1):
        dsum, _, count = aligner(xyz, cur)
        if count == 0:
            raise ValueError("no structure with finite coordinates (or a non-finite reference)")
        step = np.asarray(dsum, np.float64) / count
        cur = _as_ref32(cur) + step
        if np.sqrt((step * step).sum() / len(cur)) < tol:
            return cur, it
    import warnings
    warnings.warn(f"mean_structure: successive means still {np.sqrt((step * step).sum() / len(cur)):.3g} A apart after "
                  f"{max_iter} passes (tol {tol:g})", RuntimeWarning)
    return cur, max_iter


def rmsf_from_sums(dsum, dsq, count):
    """Per-bead fluctuation sqrt(<|d|^2> - |<d>|^2) (Angstrom, float64 (N,)) from the sums of superpose_stats."""
    if count == 0:
        return np.full(len(dsq), np.nan)
    m = np.asarray(dsum, np.float64) / count
    return np.sqrt(np.maximum(np.asarray(dsq, np.float64) / count - (m * m).sum(1), 0.0))


def rmsf(xyz, ref="mean", *, max_iter=10, tol=1e-4, chunk=None, device="cuda:0", aligner=None):
    """Root-mean-square fluctuation of every bead (Angstrom, float64 (N,)) of the ensemble xyz (n, N, 3) about its own
    mean position, after superposing every finite structure on ref: a structure (N, 3), or "mean" for the converged
    mean_structure of xyz."""
    if aligner is None:
        def aligner(x, r):
            return superpose_stats(x, r, chunk=chunk, device=device)
    if isinstance(ref, str):
        if ref != "mean":
            raise ValueError('ref must be a structure (N, 3) or "mean"')
        ref, _ = mean_structure(xyz, None, max_iter, tol, aligner=aligner)
    return rmsf_from_sums(*aligner(xyz, _as_ref32(ref)))


def kabsch_rmsd64(a, b):
    """RMSD (optimal proper rotation, float64, numpy) between two structures (N, 3): for the two mean structures of
    FlexibilityEvaluator.summarize, not for ensembles."""
    a = np.asarray(a, np.float64) - np.mean(a, 0)
    b = np.asarray(b, np.float64) - np.mean(b, 0)
    U, S, Vt = np.linalg.svd(a.T @ b)
    S[-1] *= np.sign(np.linalg.det(U @ Vt))
    return float(np.sqrt(max(((a * a).sum() + (b * b).sum() - 2.0 * S.sum()) / len(a), 0.0)))


class FlexibilityEvaluator:
    """Per-bead flexibility of a sampled ensemble against a reference ensemble (MD data), on the GPU.

    ref_data (m, N, 3) in Angstrom.  Both ensembles are superposed on `folded` (a structure (N, 3) or a folded PDB) when
    given, otherwise on the reference ensemble's mean structure (mean_structure).  eval(samples) returns a plain dict of
    floats:
      rmsf_mae, rmsf_max_abs      mean and largest |RMSF_samples - RMSF_refs| over the beads (Angstrom)
      rmsf_pearson                correlation of the two RMSF profiles (NaN when one of them is constant)
      mean_structure_rmsd         RMSD (optimal proper rotation) between the two ensembles' mean structures
      samples_nonfinite, refs_nonfinite   frames with a non-finite coordinate: left out on their side
    and keeps the two profiles on .profiles: {"samples" / "refs": {"rmsf" (N,), "mean" (N, 3), "count"}}.
    Without the HIP library: DffLibraryError."""

    def __init__(self, ref_data, mol_name="", folded=None, *, max_iter=10, tol=1e-4, chunk=None, device="cuda:0"):
        self.mol_name = mol_name
        self.chunk = chunk
        self.device = torch.device(device)
        binding.load_library()
        self.refs = _frames(_reference_frames(ref_data), self.device)
        self.refs_nonfinite = _count_nonfinite(self.refs)
        if folded is not None:
            self.align_on = _as_ref32(_folded_coords(folded, mol_name))
        else:
            self.align_on, _ = mean_structure(self.refs, None, max_iter, tol, chunk=chunk, device=self.device)
        if len(self.align_on) != int(self.refs.shape[1]):
            raise ValueError(f"the structure to align on has {len(self.align_on)} beads, the reference ensemble "
                             f"{int(self.refs.shape[1])}")
        self.profiles = {"refs": self.profile(self.refs)}

    def profile(self, x):
        """{"rmsf" (N,), "mean" (N, 3), "count"} of the frames x superposed on the evaluator's structure"""
        dsum, dsq, count = superpose_stats(x, self.align_on, chunk=self.chunk, device=self.device)
        mean = _as_ref32(self.align_on) + dsum / count if count else np.full_like(dsum, np.nan)
        return {"rmsf": rmsf_from_sums(dsum, dsq, count), "mean": mean, "count": count}

    @staticmethod
    def summarize(rmsf_samples, rmsf_refs, mean_samples, mean_refs, samples_nonfinite=0, refs_nonfinite=0):
        """eval()'s dict from the two RMSF profiles (N,) and the two mean structures (N, 3): numpy only."""
        a, b = np.asarray(rmsf_samples, np.float64), np.asarray(rmsf_refs, np.float64)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("the two RMSF profiles must be (N,) both")
        diff = np.abs(a - b)
        pearson = float("nan")
        if len(a) > 1 and a.std() > 0 and b.std() > 0:
            pearson = float(np.corrcoef(a, b)[0, 1])
        return {"rmsf_mae": float(diff.mean()), "rmsf_max_abs": float(diff.max()), "rmsf_pearson": pearson,
                "mean_structure_rmsd": kabsch_rmsd64(mean_samples, mean_refs),
                "samples_nonfinite": float(samples_nonfinite), "refs_nonfinite": float(refs_nonfinite)}

    def eval(self, samples):
        x = _frames(samples, self.device)
        if x.shape[1] != self.refs.shape[1]:
            raise ValueError(f"samples have {int(x.shape[1])} beads, the reference ensemble {int(self.refs.shape[1])}")
        s, r = self.profile(x), self.profiles["refs"]
        self.profiles["samples"] = s
        return self.summarize(s["rmsf"], r["rmsf"], s["mean"], r["mean"], _count_nonfinite(x), self.refs_nonfinite)


# =====================================================================================================
# Clustering an ensemble under the RMSD with a cutoff: the method of Daura et al. (1999), `gmx cluster -method gromos`
# (dff_rmsd_neighbors, dff_gromos_steps; csrc/dff_cluster.hip).  The reference's evaluators have no model-free answer to
# "which conformations are in this ensemble, and how populated is each": its states live in TIC space.
# =====================================================================================================
class RmsdClusters:
    """Result of cluster_rmsd: labels (n,) int64 numpy (-1: a frame with a non-finite coordinate, or one beyond
    max_clusters), centers (K,) frame indices, sizes (K,) in order of creation (non-increasing), and the cutoff.  With a
    stride the indices count the STRIDED frames xyz[::stride]; `stride` is kept."""

    def __init__(self, labels, centers, sizes, cutoff, stride=1):
        self.labels, self.centers, self.sizes = labels, centers, sizes
        self.cutoff, self.stride = float(cutoff), int(stride)

    @property
    def n_clusters(self):
        return len(self.centers)

    def __repr__(self):
        return f"RmsdClusters({self.n_clusters} clusters of {len(self.labels)} frames at {self.cutoff:g} A, sizes {self.sizes[:8].tolist()})"


def cluster_rmsd(xyz, cutoff, *, max_clusters=None, stride=1, steps_per_sync=64, device="cuda:0"):
    """Cluster the structures xyz (n, N, 3) (Angstrom) under the minimum RMSD over proper rotations with `cutoff`: count every
    frame's neighbours within the cutoff; the frame with the most (the lowest index among ties) becomes a centre and takes
    its neighbours with it; repeat on what is left.  -> RmsdClusters.  The neighbour matrix is one bit per pair on the
    device (n^2 / 8 bytes, n <= 2^18); `stride` > 1 clusters xyz[::stride] (for ensembles beyond that) and the labels,
    centres and sizes are those of the STRIDED frames.  The loop runs on the device steps_per_sync iterations at a time;
    between rounds two integers (clusters, frames left) are read."""
    dev = torch.device(device)
    stride, steps = int(stride), int(steps_per_sync)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    if steps < 1:
        raise ValueError("steps_per_sync must be >= 1")
    if max_clusters is not None and int(max_clusters) < 1:
        raise ValueError("max_clusters must be >= 1")
    xs = torch.as_tensor(xyz)
    if xs.dim() != 3 or xs.shape[-1] != 3:
        raise ValueError("structures must be (n, n_beads, 3)")
    x = _frames(xs[::stride] if stride > 1 else xs, dev)
    n = len(x)
    if n > binding.CLUSTER_MAX_FRAMES:
        raise ValueError(f"{n} frames exceed the {binding.CLUSTER_MAX_FRAMES} of the neighbour matrix: pass a stride")
    kmax = n if max_clusters is None else int(max_clusters)
    if n == 0:
        e = np.empty(0, np.int64)
        return RmsdClusters(e, e.copy(), e.copy(), cutoff, stride)
    adj, _ = binding.rmsd_neighbors(x, cutoff, degree=False)
    state = binding.gromos_state(adj, kmax)
    while True:
        binding.gromos_steps(adj, state, steps)
        k, left = (int(v) for v in state["progress"].cpu())
        if left <= 0 or k >= kmax:
            break
    return RmsdClusters(state["labels"].cpu().numpy().astype(np.int64), state["centers"][:k].cpu().numpy().astype(np.int64),
                        state["sizes"][:k].cpu().numpy().astype(np.int64), cutoff, stride)


class RmsdClusterEvaluator:
    """Populations of the conformations of a reference ensemble (MD data) in a sampled ensemble, by RMSD clustering.

    ref_data (m, N, 3) in Angstrom is clustered once (cluster_rmsd with `cutoff`, `max_clusters`, `stride`); the centres
    are the structures ref[::stride][centers].  eval(samples) assigns every sample to its nearest centre (nearest_rmsd);
    it belongs to that cluster when the RMSD is <= cutoff and is unassigned otherwise.  A plain dict:
      n_clusters                      clusters of the reference ensemble with at least min_size frames
      populations_ref, populations_samples   lists over those clusters (order of creation), shares of the finite frames
                                      of each side; the reference's are its own cluster sizes
      population_js                   js_divergence of the two count vectors, unassigned as one extra bin (for the
                                      reference: the frames of clusters below min_size, or beyond max_clusters)
      unassigned_share                share of the finite samples that belong to no cluster of size >= min_size
      largest_cluster_share_ref, largest_cluster_share_samples
      samples_nonfinite, refs_nonfinite   frames with a non-finite coordinate: left out on their side
    Without the HIP library: DffLibraryError."""

    def __init__(self, ref_data, mol_name="", cutoff=2.0, max_clusters=None, min_size=1, stride=1, *, chunk=None,
                 device="cuda:0"):
        self.mol_name = mol_name
        self.cutoff = float(cutoff)
        self.min_size = int(min_size)
        if not np.isfinite(self.cutoff) or self.cutoff < 0:
            raise ValueError("RmsdClusterEvaluator: cutoff must be finite and >= 0")
        if self.min_size < 1:
            raise ValueError("RmsdClusterEvaluator: min_size must be >= 1")
        self.chunk = chunk
        self.device = torch.device(device)
        binding.load_library()
        refs = _frames(_reference_frames(ref_data), self.device)
        self.refs = refs[::int(stride)].contiguous() if int(stride) > 1 else refs
        self.refs_nonfinite = _count_nonfinite(self.refs)
        self.clusters = cluster_rmsd(self.refs, self.cutoff, max_clusters=max_clusters, device=self.device)
        self.centers = self.refs[torch.as_tensor(self.clusters.centers, device=self.device)]

    @staticmethod
    def summarize(sizes_ref, n_ref_finite, labels_samples, min_size=1, samples_nonfinite=0, refs_nonfinite=0):
        """eval()'s dict from the reference's cluster sizes (K,), the number of its finite frames, and the samples' labels
        (n,): the cluster of each FINITE sample, -1 for one that is unassigned (non-finite samples are not in it): numpy only."""
        sizes = np.asarray(sizes_ref, np.int64).reshape(-1)
        lab = np.asarray(labels_samples, np.int64).reshape(-1)
        keep = sizes >= int(min_size)
        ref_counts = sizes[keep]
        smp_all = np.bincount(lab[lab >= 0], minlength=len(sizes))[:len(sizes)] if len(sizes) else np.zeros(0, np.int64)
        smp_counts = smp_all[keep]
        n_ref, n_smp = int(n_ref_finite), int(len(lab))
        ref_un, smp_un = n_ref - int(ref_counts.sum()), n_smp - int(smp_counts.sum())
        nan = float("nan")
        pr = ref_counts / n_ref if n_ref else np.full(len(ref_counts), nan)
        ps = smp_counts / n_smp if n_smp else np.full(len(smp_counts), nan)
        js = nan
        if n_ref and n_smp:
            js = float(js_divergence(np.append(ref_counts, ref_un).astype(np.float64),
                                     np.append(smp_counts, smp_un).astype(np.float64)))
        return {"n_clusters": float(keep.sum()), "populations_ref": pr.tolist(), "populations_samples": ps.tolist(),
                "population_js": js, "unassigned_share": smp_un / n_smp if n_smp else nan,
                "largest_cluster_share_ref": float(pr.max()) if len(pr) else nan,
                "largest_cluster_share_samples": float(ps.max()) if len(ps) else nan,
                "samples_nonfinite": float(samples_nonfinite), "refs_nonfinite": float(refs_nonfinite)}

    def assign(self, samples):
        """(frames on the device, labels int64 numpy (n,): the cluster of the nearest centre when it is within the cutoff,
        -1 otherwise, -2 for a sample with a non-finite coordinate)"""
        x = _frames(samples, self.device)
        if x.shape[1] != self.refs.shape[1]:
            raise ValueError(f"samples have {int(x.shape[1])} beads, the reference ensemble {int(self.refs.shape[1])}")
        if len(self.centers) == 0 or len(x) == 0:
            d = torch.full((len(x),), float("nan"), device=self.device)
            idx = torch.full((len(x),), -1, dtype=torch.int64, device=self.device)
        else:
            d, idx = nearest_rmsd(x, self.centers, chunk=self.chunk, device=self.device)
        lab = torch.where(d <= self.cutoff, idx, torch.full_like(idx, -1))           # NaN compares false
        fin = torch.isfinite(x).all(dim=2).all(dim=1)
        lab = torch.where(fin, lab, torch.full_like(lab, -2))
        return x, lab.cpu().numpy()

    def eval(self, samples):
        x, lab = self.assign(samples)
        n_ref = len(self.refs) - self.refs_nonfinite
        return self.summarize(self.clusters.sizes, n_ref, lab[lab >= -1], self.min_size, int((lab == -2).sum()),
                              self.refs_nonfinite)


# =====================================================================================================
# Folding kinetics from an order parameter: the fraction of native contacts Q (or the RMSD to the folded structure) per
# frame, dual-cutoff core states along each trajectory, dwell runs and censoring-aware rates (dff_struct_native_q,
# dff_core_states, dff_label_runs; csrc/dff_kinetics.hip).  The reference looks at per-trajectory RMSD and contact dynamics
# (RmsdEvaluator.eval(save_dynamics=True), _plot_rmsd_dynamics, _eval_bce_dynamics) and stops at plots.
# =====================================================================================================
def native_pairs(folded, cutoff=10.0, offset=3):
    """The native contacts of the folded structure (N, 3) in Angstrom: the pairs j >= i + offset whose folded distance
    (float32, as ContactEvaluator computes it) is < cutoff -- the defaults are ContactEvaluator's (contact_cutoff 10,
    offset 3) -> (pairs int32 (P, 2) in triu order, r0 float32 (P,)).  Validated on the host."""
    f = np.asarray(torch.as_tensor(folded).cpu(), np.float64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("native_pairs: the folded structure must be (n_beads, 3)")
    N = len(f)
    if not 4 <= N <= binding.DFF_MAX_BEADS:
        raise ValueError(f"native_pairs: n_beads must be 4..{binding.DFF_MAX_BEADS}")
    if not np.all(np.isfinite(f)):
        raise ValueError("native_pairs: the folded structure has a non-finite coordinate")
    if not (np.isfinite(cutoff) and cutoff > 0):
        raise ValueError("native_pairs: cutoff must be finite and > 0")
    if int(offset) != offset or not 1 <= offset < N:
        raise ValueError(f"native_pairs: offset must be an integer in 1..{N - 1}")
    f32 = torch.from_numpy(f).float()
    d = torch.norm(f32[:, None, :] - f32[None, :, :], dim=-1).numpy()
    i, j = np.triu_indices(N, int(offset))
    keep = d[i, j] < cutoff
    if not keep.any():
        raise ValueError(f"native_pairs: no pair at offset {offset} is closer than {cutoff} A in the folded structure")
    return np.stack([i[keep], j[keep]], 1).astype(np.int32), d[i, j][keep].astype(np.float32)


def native_contacts_q(xyz, folded, *, cutoff=10.0, offset=3, beta=5.0, lam=1.2, device="cuda:0"):
    """Soft fraction of native contacts of every structure of xyz (n, N, 3) in Angstrom, Q = mean over the native pairs
    (native_pairs(folded, cutoff, offset)) of 1 / (1 + exp(beta (r - lam r0))): the form of Best, Hummer & Eaton (2013),
    float64 arithmetic, -> float32 tensor (n,) on `device`; NaN for a frame with a non-finite coordinate.
    beta = 5 / A and lam = 1.2 are THIS PROJECT'S choice for C-alpha beads (Best et al. use 5 / A and 1.8 for all heavy
    atoms at a 4.5 A cutoff); the reference has no soft Q, only the hard contact map of ContactEvaluator."""
    pairs, r0 = native_pairs(folded, cutoff, offset)
    x = _frames(xyz, torch.device(device))
    _check_beads(x, folded)
    return binding.struct_native_q(x, pairs, r0, beta, lam)


def _check_beads(x, folded):
    if x.shape[1] != len(folded):
        raise ValueError(f"structures have {int(x.shape[1])} beads, the folded structure {len(folded)}")


def _check_cores(lo, hi, what):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"{what}: lo and hi must be finite with lo < hi")
    return lo, hi


def _series(t, dtype, device):
    t = torch.as_tensor(t)
    if t.dim() != 1:
        raise ValueError("a series must be (n,)")
    dev = t.device if t.is_cuda and device is None else torch.device(device or "cuda:0")
    return t.to(device=dev, dtype=dtype).contiguous()


def core_states(cv, lo, hi, traj_lengths=None, *, device=None):
    """Dual-cutoff (core-set, "transition-based") states of the series cv (n,): per trajectory, a frame is in state 0 from
    a frame with cv <= lo on and in state 1 from one with cv >= hi on, and keeps the last state in between; -1 before a
    trajectory's first core visit and at a non-finite frame, which resets the history -> int32 tensor (n,) on the device
    (cv's, when it is a CUDA tensor).  traj_lengths=None: one trajectory."""
    lo, hi = _check_cores(lo, hi, "core_states")
    c = _series(cv, torch.float32, device)
    return binding.core_states(c, _check_lengths(traj_lengths, len(c)), lo, hi)


def label_runs(labels, traj_lengths=None, *, device=None):
    """The runs of equal labels inside the trajectories of labels (n,) -> a dict of numpy arrays over the runs in time
    order: start int64, length int64, label int32, flags uint8 (bit 0: the run begins at its trajectory's first frame,
    bit 1: it ends at its trajectory's last frame).  traj_lengths=None: one trajectory."""
    lab = _series(labels, torch.int32, device)
    res = binding.label_runs(lab, _check_lengths(traj_lengths, len(lab)))
    k = int(res["n_runs"].cpu())
    return {key: res[key][:k].cpu().numpy() for key in ("start", "length", "label", "flags")}


def dwell_summary(runs, frame_time=1.0):
    """Dwell statistics from the runs of label_runs: numpy only.  For the labels a >= 0 (a negative label is "undetermined"):
      frames[a]          frames spent in a (every run of a, censored ones included)
      events[(a, b)]     runs of a followed, in the same trajectory, by a run of b >= 0 (b != a); a run of a negative label
                         in between breaks the event
      rates[(a, b)]      events / (frames[a] * frame_time): the maximum-likelihood rate under censoring -- a trajectory's
                         first and last dwells add time but no event; NaN when the time is 0
      mean_dwell[a], median_dwell[a], n_completed[a]   over the COMPLETED dwells of a, those that start with an entry event
                         and end with an exit event, in units of frame_time; NaN without one
    and total_frames, undetermined_frames.  `labels` lists the a >= 0 that occur, ascending."""
    lab = np.asarray(runs["label"], np.int64).reshape(-1)
    length = np.asarray(runs["length"], np.int64).reshape(-1)
    flags = np.asarray(runs["flags"], np.int64).reshape(-1)
    if not (len(lab) == len(length) == len(flags)):
        raise ValueError("dwell_summary: label, length and flags must have one entry per run")
    if not (np.isfinite(frame_time) and frame_time > 0):
        raise ValueError("dwell_summary: frame_time must be finite and > 0")
    states = sorted(int(a) for a in np.unique(lab[lab >= 0]))
    # run k and run k + 1 lie in one trajectory when run k does not end its trajectory; an event needs both labels >= 0
    joined = np.zeros(len(lab), bool)
    if len(lab) > 1:
        joined[:-1] = ((flags[:-1] & 2) == 0) & (lab[:-1] >= 0) & (lab[1:] >= 0)
    exits = joined                                           # run k ends with an exit event
    enters = np.concatenate([[False], joined[:-1]])         # run k starts with an entry event
    frames = {a: int(length[lab == a].sum()) for a in states}
    events = {(a, b): int((exits[:-1] & (lab[:-1] == a) & (lab[1:] == b)).sum()) if len(lab) > 1 else 0
              for a in states for b in states if a != b}
    nan = float("nan")
    rates = {ab: (n / (frames[ab[0]] * frame_time) if frames[ab[0]] > 0 else nan) for ab, n in events.items()}
    mean, median, n_completed = {}, {}, {}
    for a in states:
        done = length[(lab == a) & exits & enters]
        n_completed[a] = int(len(done))
        mean[a] = float(done.mean() * frame_time) if len(done) else nan
        median[a] = float(np.median(done) * frame_time) if len(done) else nan
    return {"labels": states, "frames": frames, "events": events, "rates": rates, "mean_dwell": mean, "median_dwell": median,
            "n_completed": n_completed, "total_frames": int(length.sum()), "undetermined_frames": int(length[lab < 0].sum())}


class _Observable:
    """Frames -> one series, the step the trajectory evaluators share.  cv="q": the soft fraction of native contacts of
    native_contacts_q (native_pairs(folded, cutoff, offset), beta, lam); cv="rmsd": the RMSD to the folded structure
    (dff_struct_rmsd); cv="tic": the k components of the TIC projection of `tica` (dff_struct_tic).  `allowed` lists the cv
    the caller takes, `what` is the caller's name in the error texts.  folded, pairs, r0 (q, rmsd) and mean, coeff (tic) are
    None where the cv has no use for them."""

    def __init__(self, what, cv, allowed, folded=None, mol_name=None, tica=None, cutoff=10.0, offset=3, beta=5.0, lam=1.2):
        if cv not in allowed:
            raise ValueError(f"{what}: cv must be " + " or ".join([", ".join(repr(c) for c in allowed[:-1]), repr(allowed[-1])]))
        self.cv = cv
        self.folded = self.pairs = self.r0 = self.mean = self.coeff = None
        self.beta, self.lam = float(beta), float(lam)
        if cv == "tic":
            if tica is None:
                raise ValueError(f"{what}: cv='tic' needs tica")
            self.mean, self.coeff = _tica_model(tica, what, TICA_MAX_DIM)
            return
        if folded is None:
            raise ValueError(f"{what}: cv={cv!r} needs the folded structure")
        self.folded = _folded_coords(folded, mol_name)
        if cv == "q":
            if not (np.isfinite(self.beta) and self.beta > 0 and np.isfinite(self.lam) and self.lam > 0):
                raise ValueError(f"{what}: beta and lam must be finite and > 0")
            self.pairs, self.r0 = native_pairs(self.folded, cutoff, offset)

    def __call__(self, x):
        """the series of the frames x (n, N, 3) already on the device: (n,) float32 for q and rmsd, (n, k) float64 for tic"""
        if self.cv == "tic":
            return binding.struct_tic(x, self.mean, self.coeff)
        _check_beads(x, self.folded)
        if self.cv == "q":
            return binding.struct_native_q(x, self.pairs, self.r0, self.beta, self.lam)
        return binding.struct_rmsd(x, torch.from_numpy(self.folded).float())


class _TrajectoryEvaluator:
    """What FoldingKineticsEvaluator, RelaxationEvaluator, MsmEvaluator and MsmPassageEvaluator share.  A subclass checks its
    own arguments between super().__init__ and self._start(ref_data, ref_traj_lengths), and writes
      _analyse(x, lengths, name)   the result dict of one ensemble, name "samples" or "refs": frames x (n, N, 3) float32 on the
                                   device in trajectories of `lengths`; what it keeps for the caller (series, models, ...) goes
                                   on dicts under that name
      _compare(res, ref)           adds the keys that compare the samples' result with the reference's to res.
    eval() is the samples' dict, then with ref_data the reference's keys with the suffix _ref, then _compare's keys."""

    def __init__(self, what, mol_name, frame_time, device):
        self.frame_time = float(frame_time)
        if not (np.isfinite(self.frame_time) and self.frame_time > 0):
            raise ValueError(f"{what}: frame_time must be finite and > 0")
        self.mol_name = mol_name
        self.device = torch.device(device)
        self.ref_result = None

    def _start(self, ref_data, ref_traj_lengths):
        """the end of a constructor: the library, and the reference's result when there is ref_data"""
        binding.load_library()
        if ref_data is not None:
            self.ref_result = self._ensemble(_reference_frames(ref_data), ref_traj_lengths, "refs")

    def _ensemble(self, xyz, traj_lengths, name):
        x = _frames(xyz, self.device)
        return self._analyse(x, _check_lengths(traj_lengths, len(x)), name)

    def eval(self, xyz, traj_lengths=None):
        res = self._ensemble(xyz, traj_lengths, "samples")
        if self.ref_result is not None:
            res.update({k + "_ref": v for k, v in self.ref_result.items()})
            self._compare(res, self.ref_result)
        return res


class FoldingKineticsEvaluator(_TrajectoryEvaluator):
    """How often does a trajectory fold and unfold, and how long does it stay: the order-parameter route of the fast-folder
    literature on the GPU.  Frames -> order parameter (cv="q": the soft fraction of native contacts of native_contacts_q;
    cv="rmsd": the RMSD to the folded structure, dff_struct_rmsd) -> dual-cutoff core states with the cores cv <= lo and
    cv >= hi (core_states) -> runs (label_runs) -> dwell_summary.  Folded is label 1 for Q (Q >= hi) and label 0 for the RMSD
    (rmsd <= lo).  `folded` is a PDB path or the folded C-alpha coordinates (N, 3) in Angstrom; frame_time is the time
    between two frames, in the unit the rates and dwell times are wanted in.

    eval(xyz, traj_lengths=None) -- None: the frames are ONE trajectory, as for StateTransitionEvaluator -- returns a plain
    dict of floats:
      folded_share, unfolded_share, undetermined_share   shares of ALL frames (undetermined: label -1)
      n_folding, n_unfolding                              events unfolded -> folded and folded -> unfolded
      rate_folding, rate_unfolding                        events / time spent in the state left (dwell_summary's rates)
      mean_dwell_folded, mean_dwell_unfolded, median_dwell_folded, median_dwell_unfolded   over completed dwells
      free_energy_folding_kT                              -ln(folded_share / unfolded_share); NaN when a share is 0
      samples_nonfinite                                   frames with a non-finite coordinate (label -1, history reset)
    With ref_data (MD frames (m, N, 3), trajectories of ref_traj_lengths) the same keys with the suffix _ref, and
    log10_rate_ratio_folding, log10_rate_ratio_unfolding (samples over reference; NaN unless both rates are positive) and
    folded_share_diff.  The series stay on .series: {"samples" / "refs": {"cv", "labels", "runs", "summary"}}.
    Without the HIP library: DffLibraryError."""

    KEYS = ("folded_share", "unfolded_share", "undetermined_share", "n_folding", "n_unfolding", "rate_folding",
            "rate_unfolding", "mean_dwell_folded", "mean_dwell_unfolded", "median_dwell_folded", "median_dwell_unfolded",
            "free_energy_folding_kT", "samples_nonfinite")

    def __init__(self, mol_name, folded, *, cv="q", lo, hi, frame_time=1.0, ref_data=None, ref_traj_lengths=None,
                 cutoff=10.0, offset=3, beta=5.0, lam=1.2, device="cuda:0"):
        super().__init__("FoldingKineticsEvaluator", mol_name, frame_time, device)
        self.lo, self.hi = _check_cores(lo, hi, "FoldingKineticsEvaluator")
        self._cv = _Observable("FoldingKineticsEvaluator", cv, ("q", "rmsd"), folded, mol_name, None, cutoff, offset, beta, lam)
        self.cv, self.folded, self.pairs, self.r0 = cv, self._cv.folded, self._cv.pairs, self._cv.r0
        self.folded_label, self.unfolded_label = (1, 0) if cv == "q" else (0, 1)
        self.series = {}
        self._start(ref_data, ref_traj_lengths)

    def order_parameter(self, x):
        """float32 tensor (n,) on the device: Q or the RMSD of the frames x (n, N, 3) already there"""
        return self._cv(x)

    @staticmethod
    def summarize(summary, folded_label, unfolded_label, samples_nonfinite=0):
        """eval()'s dict from a dwell_summary: numpy only."""
        nan = float("nan")
        F, U = folded_label, unfolded_label
        n = summary["total_frames"]
        nf, nu = summary["frames"].get(F, 0), summary["frames"].get(U, 0)
        share = lambda k: k / n if n else nan     # noqa: E731
        res = {"folded_share": share(nf), "unfolded_share": share(nu), "undetermined_share": share(n - nf - nu),
               "n_folding": float(summary["events"].get((U, F), 0)), "n_unfolding": float(summary["events"].get((F, U), 0)),
               "rate_folding": summary["rates"].get((U, F), nan), "rate_unfolding": summary["rates"].get((F, U), nan)}
        for name, a in (("folded", F), ("unfolded", U)):
            res[f"mean_dwell_{name}"] = summary["mean_dwell"].get(a, nan)
            res[f"median_dwell_{name}"] = summary["median_dwell"].get(a, nan)
        res["free_energy_folding_kT"] = float(-np.log(nf / nu)) if nf > 0 and nu > 0 else nan
        res["samples_nonfinite"] = float(samples_nonfinite)
        return res

    def _analyse(self, x, lengths, name):
        cv = self.order_parameter(x)
        labels = binding.core_states(cv, lengths, self.lo, self.hi)
        runs = label_runs(labels, lengths)
        summary = dwell_summary(runs, self.frame_time)
        self.series[name] = {"cv": cv.cpu().numpy(), "labels": labels.cpu().numpy(), "runs": runs, "summary": summary}
        return self.summarize(summary, self.folded_label, self.unfolded_label, _count_nonfinite(x))

    def eval(self, xyz, traj_lengths=None, plot_dynamics=False):
        if plot_dynamics:
            raise NotImplementedError("plotting (evaluators.py: _plot_rmsd_dynamics) is outside the hot path")
        return super().eval(xyz, traj_lengths)

    def _compare(self, res, ref):
        for which in ("folding", "unfolding"):
            res[f"log10_rate_ratio_{which}"] = _log10_ratio(res[f"rate_{which}"], ref[f"rate_{which}"])
        res["folded_share_diff"] = res["folded_share"] - ref["folded_share"]


# =====================================================================================================
# Autocorrelation of trajectory observables: relaxation times without a model, effective sample sizes and standard errors
# (dff_autocorr; csrc/dff_autocorr.hip).  The reference reports point estimates only; these are the uncertainties of the
# means above and the first check on whether sampled dynamics relax as fast as the MD data do.
# =====================================================================================================
class Autocorrelation:
    """What autocorrelation() returns, float64 numpy arrays: acf and cov (max_lag + 1, d), counts int64 (max_lag + 1,) -- the
    usable pairs per lag --, mean and variance (d,) over the usable frames; n_usable = counts[0], estimator, max_lag."""

    def __init__(self, acf, cov, counts, mean, variance, estimator):
        self.acf, self.cov, self.counts, self.mean, self.variance = acf, cov, counts, mean, variance
        self.estimator = estimator
        self.max_lag = len(counts) - 1
        self.n_usable = int(counts[0])


AUTOCORR_ESTIMATORS = ("per_lag", "global")


def autocorr_estimate(sxy, sx, sy, count, estimator="per_lag"):
    """C(l) from the sums of dff_autocorr over the usable pairs of lag l (torch tensors or arrays: sxy, sx, sy (L, d),
    count (L,)) -> float64 tensor (L, d).  "per_lag": sxy / count - (sx / count)(sy / count), the covariance of the two ends
    of the pairs with each end's own mean.  "global": the lag-0 mean m0 = sx[0] / count[0] for both factors,
    sxy / count - m0 (sx + sy) / count + m0^2.  A lag without a pair gives NaN."""
    if estimator not in AUTOCORR_ESTIMATORS:
        raise ValueError(f"estimator must be one of {AUTOCORR_ESTIMATORS}")
    sxy, sx, sy = (torch.as_tensor(v, dtype=torch.float64) for v in (sxy, sx, sy))
    cnt = torch.as_tensor(count).to(device=sxy.device, dtype=torch.float64)[:, None]
    if estimator == "per_lag":
        return sxy / cnt - (sx / cnt) * (sy / cnt)                  # 0 / 0 = NaN where count is 0
    m0 = sx[:1] / cnt[:1]
    return sxy / cnt - m0 * (sx + sy) / cnt + m0 * m0


def autocorrelation(series, max_lag, traj_lengths=None, *, estimator="per_lag", device="cuda:0"):
    """Autocorrelation function of the observable `series` ((n,) or (n, d), d <= 8; float32 or float64, torch or numpy) inside
    the trajectories of traj_lengths (back to back; None: one trajectory) for the lags 0 .. max_lag -> Autocorrelation.
    A frame with a non-finite component is left out together with every pair it is part of; pairs never cross a trajectory
    boundary.  The series is converted once to contiguous float64 on the device, its mean over the usable frames is
    computed there and subtracted inside the kernel (dff_autocorr), C(l) is formed by autocorr_estimate and
    acf = C(l) / C(0); everything comes back in one copy.  Lags without a pair give NaN."""
    if estimator not in AUTOCORR_ESTIMATORS:
        raise ValueError(f"estimator must be one of {AUTOCORR_ESTIMATORS}")
    dev = torch.device(device)
    s = torch.as_tensor(series)
    if s.dim() == 1:
        s = s[:, None]
    if s.dim() != 2 or not s.is_floating_point():
        raise ValueError("autocorrelation: the series must be a floating-point (n,) or (n, d)")
    n, d, L = int(s.shape[0]), int(s.shape[1]), int(max_lag)
    if not 1 <= d <= binding.AUTOCORR_MAX_D:
        raise ValueError(f"autocorrelation: d must be 1..{binding.AUTOCORR_MAX_D}")
    if L != max_lag or not 0 <= L <= binding.AUTOCORR_MAX_LAG:
        raise ValueError(f"autocorrelation: max_lag must be an integer in 0..{binding.AUTOCORR_MAX_LAG}")
    lengths = _check_lengths(traj_lengths, n)
    s = s.to(device=dev, dtype=torch.float64).contiguous()
    usable = torch.isfinite(s).all(1, keepdim=True)
    shift = (torch.where(usable, s, torch.zeros_like(s)).sum(0) / usable.sum().clamp(min=1)).contiguous()
    sums = binding.autocorr(s, lengths, L, shift)
    cov = autocorr_estimate(sums["sxy"], sums["sx"], sums["sy"], sums["count"], estimator)
    cnt = sums["count"].to(torch.float64)
    mean = shift + sums["sx"][0] / cnt[0]
    packed = torch.cat([cov.reshape(-1), (cov / cov[:1]).reshape(-1), cnt, mean, cov[0]]).cpu().numpy()      # the one read-back
    k = (L + 1) * d
    return Autocorrelation(packed[k:2 * k].reshape(L + 1, d), packed[:k].reshape(L + 1, d),
                           packed[2 * k:2 * k + L + 1].astype(np.int64), packed[2 * k + L + 1:2 * k + L + 1 + d],
                           packed[2 * k + L + 1 + d:], estimator)


def _acf_1d(acf):
    rho = np.asarray(acf, np.float64)
    if rho.ndim == 2 and rho.shape[1] == 1:
        rho = rho[:, 0]
    if rho.ndim != 1 or len(rho) < 1:
        raise ValueError("the ACF must be (max_lag + 1,): one component")
    return rho


def integrated_autocorr_time(acf, c=5.0):
    """Integrated autocorrelation time of one component's ACF rho (max_lag + 1,), in frames, with Sokal's automatic window:
    tau(W) = 1/2 + sum_{l=1..W} rho(l), W the smallest window >= 1 with W >= c tau(W) -> (tau, window, converged).
    converged is False when no window up to the last available lag qualifies (available: before the first non-finite
    rho); tau is then the sum over all available lags and window the last of them."""
    rho = _acf_1d(acf)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("integrated_autocorr_time: c must be finite and > 0")
    bad = np.flatnonzero(~np.isfinite(rho[1:]))
    last = int(bad[0]) if len(bad) else len(rho) - 1              # the last available lag
    tau = 0.5 + np.cumsum(rho[1:last + 1])                          # tau[W - 1] = tau(W)
    ok = np.flatnonzero(np.arange(1, last + 1) >= c * tau)
    if len(ok):
        return float(tau[ok[0]]), int(ok[0]) + 1, True
    return (float(tau[-1]) if last else 0.5), last, False


def crossing_time(acf, level=float(np.exp(-1.0))):
    """The first time, in frames, at which one component's ACF rho (max_lag + 1,) falls below `level` (1 / e: the relaxation
    time of a single exponential), linearly interpolated between the two lags around the crossing; NaN when rho never
    falls below it (or meets a non-finite value first)."""
    rho = _acf_1d(acf)
    for l in range(len(rho)):
        if not np.isfinite(rho[l]):
            break
        if rho[l] < level:
            return float(l - 1 + (rho[l - 1] - level) / (rho[l - 1] - rho[l])) if l else 0.0
    return float("nan")


def effective_sample_size(n, tau):
    """n / (2 tau): the number of independent samples n correlated frames are worth (tau in frames)."""
    return n / (2.0 * tau)


def standard_error(variance, n, tau):
    """sqrt(variance * 2 tau / n): the standard error of the mean of n frames with integrated autocorrelation time tau."""
    return np.sqrt(variance * 2.0 * tau / n)


class RelaxationEvaluator(_TrajectoryEvaluator):
    """How fast does an observable decorrelate along the trajectories, and how many independent samples do they hold.
    Frames -> series (cv="q": native_contacts_q's soft fraction of native contacts; cv="rmsd": the RMSD to the folded
    structure, dff_struct_rmsd; cv="tic": the k components of the TIC projection of `tica`, a TicEvaluator, a TICA, a saved
    reference or a (mean, coeff) pair) -> autocorrelation(series, max_lag, traj_lengths).  `folded` (q, rmsd) is a PDB path
    or the folded C-alpha coordinates (N, 3) in Angstrom; frame_time is the time between two frames.

    eval(xyz, traj_lengths=None) -- None: ONE trajectory -- returns a dict, a float per key for q and rmsd and a list over
    the components for tic:
      tau_int, window_converged   integrated autocorrelation time (Sokal's window, c = 5) in units of frame_time, and whether
                                  the window closed inside max_lag (0.0 / 1.0)
      tau_e                       first crossing of 1 / e, in units of frame_time; NaN without one
      ess, ess_share              usable frames / (2 tau_int in frames), and that over the usable frames
      mean, stderr                mean over the usable frames and its standard error sqrt(variance 2 tau / n)
      samples_nonfinite           frames left out (a non-finite coordinate or component)
    With ref_data (MD frames (m, N, 3), trajectories of ref_traj_lengths) the same keys with the suffix _ref, and
    log10_tau_int_ratio (samples over reference; NaN unless both are positive).  The series and the Autocorrelation objects
    stay on .series and .acf under "samples" / "refs".  Without the HIP library: DffLibraryError."""

    KEYS = ("tau_int", "tau_e", "window_converged", "ess", "ess_share", "mean", "stderr", "samples_nonfinite")

    def __init__(self, mol_name, folded=None, *, cv="q", tica=None, max_lag, frame_time=1.0, ref_data=None,
                 ref_traj_lengths=None, device="cuda:0"):
        super().__init__("RelaxationEvaluator", mol_name, frame_time, device)
        self.max_lag = int(max_lag)
        if self.max_lag != max_lag or not 1 <= self.max_lag <= binding.AUTOCORR_MAX_LAG:
            raise ValueError(f"RelaxationEvaluator: max_lag must be an integer in 1..{binding.AUTOCORR_MAX_LAG}")
        self._cv = _Observable("RelaxationEvaluator", cv, ("q", "rmsd", "tic"), folded, mol_name, tica)
        self.cv, self.folded, self.pairs, self.r0 = cv, self._cv.folded, self._cv.pairs, self._cv.r0
        self.mean, self.coeff = self._cv.mean, self._cv.coeff
        self.series, self.acf = {}, {}
        self._start(ref_data, ref_traj_lengths)

    def observable(self, x):
        """the series of the frames x (n, N, 3) already on the device: (n,) float32 for q and rmsd, (n, k) float64 for tic"""
        return self._cv(x)

    @staticmethod
    def summarize(ac, frame_time=1.0, as_list=False):
        """eval()'s dict from an Autocorrelation (or anything with its acf, counts, mean and variance) of n frames, counts[0]
        of them usable: numpy only."""
        acf = np.asarray(ac.acf, np.float64)
        n_usable = int(ac.counts[0])
        res = {k: [] for k in RelaxationEvaluator.KEYS[:-1]}
        for c in range(acf.shape[1]):
            tau, _, converged = integrated_autocorr_time(acf[:, c])
            ok = n_usable > 0 and np.isfinite(tau) and tau > 0
            ess = effective_sample_size(n_usable, tau) if ok else float("nan")
            res["tau_int"].append(tau * frame_time)
            res["tau_e"].append(crossing_time(acf[:, c]) * frame_time)
            res["window_converged"].append(float(converged))
            res["ess"].append(float(ess))
            res["ess_share"].append(float(ess / n_usable) if ok else float("nan"))
            res["mean"].append(float(ac.mean[c]))
            res["stderr"].append(float(standard_error(ac.variance[c], n_usable, tau)) if ok else float("nan"))
        if not as_list:
            res = {k: v[0] for k, v in res.items()}
        return res

    def _analyse(self, x, lengths, name):
        series = self.observable(x)
        ac = autocorrelation(series, min(self.max_lag, max(len(x) - 1, 0)), lengths, device=self.device)
        self.series[name], self.acf[name] = series.cpu().numpy(), ac
        res = self.summarize(ac, self.frame_time, as_list=self.cv == "tic")
        res["samples_nonfinite"] = float(len(x) - ac.n_usable)
        return res

    def _compare(self, res, ref):
        res["log10_tau_int_ratio"] = _log10_ratio(res["tau_int"], ref["tau_int"])


# =====================================================================================================
# Markov state models at microstate resolution (dff_micro_kmeans_step, dff_micro_transition_counts,
# dff_msm_reversible_steps; csrc/dff_msm.hip).  The reference builds a four-state model with deeptime
# (evaluate_fastfolders.ipynb, cells 20-24); deeptime is not installed where this was written, so the semantics are
# restated from the literature -- k-means microstates, sliding-window counts, the largest strongly connected set, the
# reversible maximum-likelihood estimator of Bowman et al. 2009 / Prinz et al. 2011 (algorithm 1, plain form) -- and tested
# against a from-scratch fp64 oracle (oracle/msm.py).
# Out of scope: optimised PCCA+ and coarse-grained models (metastable_sets and chapman_kolmogorov are at the end of this file), Bayesian
# posteriors (error bars: bootstrap_msm below), sparse count matrices.
# =====================================================================================================
MSM_MAX_STATES = binding.MSM_MAX_STATES


class MicrostateKMeans(KMeans):
    """KMeans with up to 1024 centres (dff_micro_kmeans_step): the same contract, stopping rule and attributes.  The
    k-means++ seeding follows KMeans' generator protocol draw by draw but keeps the squared distance to the nearest centre
    drawn so far and folds in each new centre with ONE single-centre assignment call (torch.minimum): O(n K) instead of
    O(n K^2), and the same centres as KMeans for the same seed and K <= 64."""

    MAX_CLUSTERS = MSM_MAX_STATES

    def _step(self, *args, **kw):
        return binding.micro_kmeans_step(*args, **kw)

    def _workspace_bytes(self, n, d):
        return binding.micro_kmeans_workspace_bytes(n, d, self.n_clusters)

    def _seed_centers(self, pts):
        n, K = int(pts.shape[0]), self.n_clusters
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.seed)
        finite = torch.isfinite(pts).all(dim=1)
        idx = torch.nonzero(finite).reshape(-1)
        if idx.numel() < K:
            raise ValueError(f"{type(self).__name__}: {int(idx.numel())} finite points for {K} clusters")
        first = idx[torch.randint(int(idx.numel()), (1,), generator=gen, device=self.device)]
        picks = [first]
        d2 = None
        for _ in range(1, K):
            new = torch.nan_to_num(self._step(pts, pts[picks[-1]], accumulate=False)["dist2"], nan=0.0)
            d2 = new if d2 is None else torch.minimum(d2, new)
            cum = torch.cumsum(d2, 0)
            u = torch.rand(1, dtype=torch.float64, generator=gen, device=self.device) * cum[-1]
            nxt = torch.searchsorted(cum, u, right=True).clamp_(max=n - 1)
            if not bool(d2[nxt] > 0):                 # every point sits on a centre already: any finite point will do
                nxt = first
            picks.append(nxt)
        return pts[torch.cat(picks)].cpu().numpy()


REACH_PIVOTS, REACH_STEPS = 8, 64


def _reach(A, p, within):
    """mask of the states of `within` that p reaches inside `within` (p included) by breadth-first array steps; None when the
    search is deeper than REACH_STEPS"""
    seen = np.zeros(len(A), bool)
    seen[p] = True
    front = np.array([p])
    for _ in range(REACH_STEPS):
        nxt = A[front].any(axis=0) & within & ~seen
        if not nxt.any():
            return seen
        seen |= nxt
        front = np.flatnonzero(nxt)
    return None


def _largest_by_reachability(A):
    """largest_connected_set's answer for the boolean adjacency A where a few array searches settle it, else None.  The
    component of the lowest state left is what it reaches and is reached from among the states left (a component never
    straddles one already taken out); it goes on until the best component is at least as large as what is left, which also
    settles ties for the lowest index.  Count matrices of metastable dynamics are one giant component plus a few lost states:
    two or three searches of a handful of steps, where Tarjan's walk in Python visits every edge."""
    K = len(A)
    if K == 0:
        return None
    left, best, At = np.ones(K, bool), None, A.T
    for _ in range(REACH_PIVOTS):
        p = int(np.argmax(left))
        fwd = _reach(A, p, left)
        bwd = _reach(At, p, left) if fwd is not None else None
        if bwd is None:
            return None
        comp = fwd & bwd
        if best is None or comp.sum() > best.sum():
            best = comp
        left &= ~comp
        if best.sum() >= left.sum():
            return np.flatnonzero(best).astype(np.int64)
    return None


def largest_connected_set(counts):
    """Sorted indices (int64 array) of the largest strongly connected component of the directed graph with an edge i -> j
    wherever counts[i, j] > 0.  Largest by the number of states; among equals the component that holds the lowest index.
    (Tarjan's algorithm with an explicit stack; a state without transitions is a component of its own.)"""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError("largest_connected_set: counts must be a square matrix")
    K = c.shape[0]
    fast = _largest_by_reachability(c > 0)
    if fast is not None:
        return fast
    adj = [np.nonzero(row > 0)[0] for row in c]
    index = np.full(K, -1, np.int64)
    low = np.zeros(K, np.int64)
    on_stack = np.zeros(K, bool)
    stack, best, counter = [], None, 0
    for root in range(K):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on_stack[root] = True
        while work:
            v, pos = work.pop()
            nb = adj[v]
            while pos < len(nb):
                w = int(nb[pos])
                pos += 1
                if index[w] < 0:
                    work.append((v, pos))
                    index[w] = low[w] = counter
                    counter += 1
                    stack.append(w)
                    on_stack[w] = True
                    work.append((w, 0))
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            else:
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop()
                        on_stack[w] = False
                        comp.append(w)
                        if w == v:
                            break
                    if best is None or (len(comp), -min(comp)) > (len(best), -min(best)):
                        best = comp
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
    return np.sort(np.asarray(best if best is not None else [], np.int64))


class _DeviceSweeps:
    """S and c on the device once; sweep(x, n) runs n sweeps from the host vector x -> (x after them, err (n,))."""

    def __init__(self, S, c, device):
        self.S = torch.from_numpy(np.ascontiguousarray(S, np.float64)).to(device)
        self.c = torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(device)
        self.ws = torch.empty(max(binding.msm_workspace_bytes(len(c)), 8), dtype=torch.uint8, device=device)

    def __call__(self, x, n):
        xd = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(self.S.device)
        err = binding.msm_reversible_steps(self.S, self.c, xd, n, workspace=self.ws)
        return xd.cpu().numpy(), err.cpu().numpy()


def reversible_sweeper(S, c, device):
    """sweep(x, n) -> (x', err) for the reversible estimator on S = C + C^T (K, K) and c (K,): n sweeps of
    x_i' = sum_j S_ij / (c_i / x_i + c_j / x_j) on the GPU (dff_msm_reversible_steps), err_s = max_i |x_i' - x_i| / x_i."""
    return _DeviceSweeps(S, c, device)


def _reversible_flow(S, c, x):
    """The symmetric flow S_ij / (c_i / x_i + c_j / x_j) of the estimator at x (its row sums are x at the fixed point)."""
    S, c, x = np.asarray(S, np.float64), np.asarray(c, np.float64), np.asarray(x, np.float64)
    q = c / x
    den = q[:, None] + q[None, :]
    return np.divide(S, den, out=np.zeros_like(S), where=S != 0), x


def reversible_transition_matrix(S, c, x):
    """T_ij = S_ij / (c_i / x_i + c_j / x_j) / x_i and pi = x / sum x from a (converged) x: numpy, one K^2 expression."""
    flow, x = _reversible_flow(S, c, x)
    return flow / x[:, None], x / x.sum()


def reversible_model(S, c, x):
    """(T, pi, X) from one evaluation of the flow: reversible_transition_matrix's T and pi, and the flow scaled to sum 1,
    X_ij = pi_i T_ij of the converged estimator, symmetric by construction (MarkovStateModel.flux_matrix; what mfpt, committor
    and reactive_flux solve on)."""
    flow, x = _reversible_flow(S, c, x)
    return flow / x[:, None], x / x.sum(), flow / flow.sum()


def _reversible_problem(Ca):
    """(S, c) of the reversible estimator from the counts within the active set: S = C + C^T, c its row sums."""
    return Ca + Ca.T, Ca.sum(axis=1)


def _sweeps_outcome(err, tol):
    """The stopping rule on one problem's err of a batch of sweeps -> (converged, sweeps to count, stop): converged at the
    first sweep below tol, which is the last one counted; stop when converged or when an err is not finite."""
    hit = np.nonzero(err < tol)[0]
    converged = hit.size > 0
    return converged, int(hit[0]) + 1 if converged else len(err), converged or not np.all(np.isfinite(err))


class MarkovStateModel:
    """A Markov state model at one lag time: counts -> largest strongly connected ("active") set -> transition matrix.

    reversible=True: the maximum-likelihood transition matrix under detailed balance, by the fixed-point iteration
    x_i' = sum_j (C_ij + C_ji) / (c_i / x_i + c_j / x_j) from x_i = sum_j (C_ij + C_ji) / 2, swept on the GPU in batches
    of `steps_per_sync` until a sweep changes no x_i by more than `tol` relative (converged) or max_iter sweeps are spent.
    reversible=False: transition_matrix(counts) on the active set (row normalisation), its stationary distribution from
    the leading left eigenvector.

    fit(labels, traj_lengths=None, n_states=None) counts sliding-window transitions at `lagtime` on the GPU (labels < 0
    are skipped; n_states defaults to max(label) + 1); fit_counts(counts) starts from a (K, K) count matrix.  Afterwards:
    count_matrix (K, K, all states), active_set (sorted indices), active_count_share (the counts that stay inside the
    active set over all counts), transition_matrix and stationary_distribution (on the active set), n_iter, converged, and
    flux_matrix: the symmetric flow S_ij / (c_i / x_i + c_j / x_j) of the converged estimator scaled to sum 1 (pi_i T_ij on the
    active set; None with reversible=False)."""

    def __init__(self, lagtime, reversible=True, tol=1e-12, max_iter=1_000_000, steps_per_sync=256, *, device="cuda:0"):
        self.lagtime = int(lagtime)
        if self.lagtime != lagtime or self.lagtime < 1:
            raise ValueError("MarkovStateModel: lagtime must be an integer >= 1")
        self.reversible = bool(reversible)
        self.tol, self.max_iter, self.steps_per_sync = float(tol), int(max_iter), int(steps_per_sync)
        if not self.tol > 0 or self.max_iter < 0 or self.steps_per_sync < 1:
            raise ValueError("MarkovStateModel: tol must be > 0, max_iter >= 0 and steps_per_sync >= 1")
        self.device = torch.device(device)
        self.transition_matrix = self.stationary_distribution = self.active_set = self.count_matrix = None
        self.flux_matrix = None
        self.active_count_share, self.n_iter, self.converged = float("nan"), 0, False

    def fit(self, labels, traj_lengths=None, n_states=None):
        lab = torch.as_tensor(labels).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        n = int(lab.numel())
        lengths = _check_lengths(traj_lengths, n)
        if n_states is None:
            n_states = int(lab.max()) + 1 if n else 0
        if not 1 <= int(n_states) <= MSM_MAX_STATES:
            raise ValueError(f"MarkovStateModel: n_states must be 1..{MSM_MAX_STATES}, not {n_states}")
        counts = binding.micro_transition_counts(lab, lengths, [self.lagtime], int(n_states))
        return self.fit_counts(counts[0].cpu().numpy())

    def _active_counts(self, counts):
        """The first half of fit_counts: count_matrix, active_set and active_count_share from `counts`, n_iter = 0 and
        converged = True.  Returns the counts within the active set, from which the estimators start -- or None when the
        active set is one state, whose model (T = [[1]]) is set here."""
        C = np.array(counts, np.float64)
        if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1 or not np.all(np.isfinite(C)) or (C < 0).any():
            raise ValueError("MarkovStateModel: counts must be a finite, non-negative (K, K) matrix")
        self.count_matrix = C
        act = largest_connected_set(C)
        self.active_set = act
        Ca = C[np.ix_(act, act)]
        total = C.sum()
        self.active_count_share = float(Ca.sum() / total) if total > 0 else 0.0
        self.n_iter, self.converged = 0, True
        self.flux_matrix = None
        if len(act) == 1:
            self.transition_matrix, self.stationary_distribution = np.ones((1, 1)), np.ones(1)
            self.flux_matrix = np.ones((1, 1)) if self.reversible else None
            return None
        return Ca

    def fit_counts(self, counts):
        Ca = self._active_counts(counts)
        if Ca is None:
            pass
        elif self.reversible:
            self._fit_reversible(*_reversible_problem(Ca))
        else:
            T = transition_matrix(Ca)
            w, v = np.linalg.eig(T.T)
            pi = np.abs(np.real(v[:, np.argmax(np.real(w))]))
            self.transition_matrix, self.stationary_distribution = T, pi / pi.sum()
        return self

    def _fit_reversible(self, S, c):
        x = 0.5 * S.sum(axis=1)
        sweep = reversible_sweeper(S, c, self.device)
        self.converged = stop = False
        while self.n_iter < self.max_iter and not stop:
            n = min(self.steps_per_sync, self.max_iter - self.n_iter)
            x, err = sweep(x, n)
            self.converged, more, stop = _sweeps_outcome(err, self.tol)
            self.n_iter += more
        self.transition_matrix, self.stationary_distribution, self.flux_matrix = reversible_model(S, c, x)

    def _need_fit(self):
        if self.transition_matrix is None:
            raise ValueError("MarkovStateModel: not fitted")

    def eigenvalues(self):
        """Eigenvalues of the transition matrix, largest first: real, from the symmetric pi^(1/2) T pi^(-1/2) (eigvalsh), when
        reversible; else by magnitude."""
        self._need_fit()
        T = self.transition_matrix
        if self.reversible:
            r = np.sqrt(self.stationary_distribution)
            M = r[:, None] * T / r[None, :]
            return np.linalg.eigvalsh(0.5 * (M + M.T))[::-1]
        return np.sort(np.abs(np.linalg.eigvals(T)))[::-1]

    def timescales(self, k=3):
        """The k slowest implied timescales -lagtime / ln(lambda_i), i = 2 .. k + 1, in frames (float64 (k,)); NaN for an
        eigenvalue <= 0 and where the active set has fewer than k + 1 states."""
        return _timescales_of(self.eigenvalues()[1:int(k) + 1], int(k), self.lagtime)

    def symmetrized(self):
        """M_ij = X_ij / sqrt(pi_i pi_j) from flux_matrix: pi^(1/2) T pi^(-1/2) of a reversible model, EXACTLY symmetric (X is,
        and the denominator commutes), with T's eigenvalues; its eigenvectors v give T's right ones as v / sqrt(pi) and its
        left ones as sqrt(pi) v.  ValueError when the model is not reversible or not fitted."""
        if not self.reversible:
            raise ValueError("MarkovStateModel: symmetrized needs a reversible model")
        self._need_fit()
        r = np.sqrt(self.stationary_distribution)
        return self.flux_matrix / (r[:, None] * r[None, :])

    def eigenvectors(self, k=3, side="right"):
        """The eigenvectors of the k + 1 largest eigenvalues of the transition matrix, stationary one first -> float64
        (k + 1, n_active), on the GPU (msm_spectrum; reversible models only).  side="right": psi with T psi = lambda psi,
        sum_i pi_i psi_i^2 = 1 and the component of largest magnitude positive, so psi_1 = 1 everywhere; "left": phi =
        pi psi, so phi_1 = pi.  Rows from n_active on are NaN."""
        if side not in ("right", "left"):
            raise ValueError("MarkovStateModel: side must be 'right' or 'left'")
        sp = msm_spectrum(self, k=k, vectors=True, device=self.device)
        if sp.status[0] != 0:
            raise ValueError(f"MarkovStateModel: the eigenvectors did not converge (status {int(sp.status[0])})")
        return (sp.right if side == "right" else sp.left)[0][:, self.active_set]

    def log_likelihood(self):
        """sum_ij C_ij ln T_ij over the active set (pairs without counts contribute 0)."""
        self._need_fit()
        Ca = self.count_matrix[np.ix_(self.active_set, self.active_set)]
        m = Ca > 0
        with np.errstate(divide="ignore"):
            return float(np.sum(Ca[m] * np.log(self.transition_matrix[m])))


def _timescales_of(lam, k, lagtime):
    """-lagtime / ln(lambda) of the eigenvalues lam (2nd, 3rd, ...) -> (k,); NaN for lambda <= 0, NaN or missing"""
    out = np.full(k, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:lam.size] = np.where(lam > 0, -float(lagtime) / np.log(np.where(lam > 0, lam, 1.0)), np.nan)
    return out


EIGENSOLVERS = ("host", "device")


def _check_eigensolver(eigensolver, what):
    if eigensolver not in EIGENSOLVERS:
        raise ValueError(f"{what}: eigensolver must be 'host' or 'device', not {eigensolver!r}")
    return eigensolver == "device"


def implied_timescales(labels, lagtimes, traj_lengths=None, n_states=None, k=3, reversible=True, *, tol=1e-12,
                       max_iter=1_000_000, steps_per_sync=256, eigensolver="host", device="cuda:0"):
    """The k slowest implied timescales (frames) of a MarkovStateModel at every lag time of `lagtimes` -> float64
    (n_lags, k).  The count matrices of up to 8 lag times come from one pass over the labels.  eigensolver="device": the
    spectra of each group of lag times from one msm_spectrum call (reversible models only) instead of np.linalg.eigvalsh."""
    on_device = _check_eigensolver(eigensolver, "implied_timescales")
    dev = torch.device(device)
    lab = torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    lengths = _check_lengths(traj_lengths, int(lab.numel()))
    lagtimes = [int(v) for v in lagtimes]
    if n_states is None:
        n_states = int(lab.max()) + 1 if lab.numel() else 0
    if not 1 <= int(n_states) <= MSM_MAX_STATES:
        raise ValueError(f"implied_timescales: n_states must be 1..{MSM_MAX_STATES}, not {n_states}")
    out = np.full((len(lagtimes), int(k)), np.nan)
    for l0 in range(0, len(lagtimes), binding.MSM_MAX_LAGS):
        group = lagtimes[l0:l0 + binding.MSM_MAX_LAGS]
        counts = binding.micro_transition_counts(lab, lengths, group, int(n_states)).cpu().numpy()
        models = [MarkovStateModel(lag, reversible, tol, max_iter, steps_per_sync, device=dev).fit_counts(counts[i])
                  for i, lag in enumerate(group)]
        out[l0:l0 + len(group)] = (msm_spectrum(models, k=k, device=dev).timescales if on_device
                                   else [m.timescales(k) for m in models])
    return out


# ---- bootstrap error bars: counts resampled over trajectories or blocks of them, the model re-estimated per resample ----
# What the bootstrap does NOT cover: the discretisation is fixed (the centres are not refitted per resample), and blocks
# shorter than the slowest relaxation are not independent, which understates the error (integrated_autocorr_time of a slow
# observable is the guide for block_frames).
MSM_MAX_BATCH = binding.MSM_MAX_BATCH


def resampling_units(traj_lengths, block_frames=None):
    """The lengths (int64 array) of the units a bootstrap resamples, back to back over the frames.  block_frames=None: the
    trajectories themselves.  Otherwise every trajectory is cut into blocks of block_frames frames, a shorter last block
    being a unit of its own; an empty trajectory gives no block."""
    ln = np.asarray(traj_lengths, np.int64).reshape(-1)
    if (ln < 0).any():
        raise ValueError("resampling_units: negative trajectory length")
    if block_frames is None:
        return ln.copy()
    bf = int(block_frames)
    if bf != block_frames or bf < 1:
        raise ValueError("resampling_units: block_frames must be an integer >= 1")
    out = []
    for n in ln.tolist():
        out += [bf] * (n // bf) + ([n % bf] if n % bf else [])
    return np.asarray(out, np.int64)


def bootstrap_weights(n_units, n_resamples, seed):
    """uint32 (n_resamples, n_units): how often unit u is drawn in resample b when n_units units are drawn with replacement.
    Pinned: np.random.default_rng(seed).multinomial(n_units, np.full(n_units, 1 / n_units), size=n_resamples)."""
    n_units, B = int(n_units), int(n_resamples)
    if n_units < 1 or B < 1:
        raise ValueError("bootstrap_weights: n_units and n_resamples must be >= 1")
    return np.random.default_rng(seed).multinomial(n_units, np.full(n_units, 1 / n_units), size=B).astype(np.uint32)


class _DeviceResampledCounts:
    """labels on the device once; count(weights (b, n_units)) -> the b weighted count matrices, uint64 (b, K, K) on the host."""

    def __init__(self, labels, lengths, unit_lengths, lag, K, device):
        self.labels = torch.as_tensor(labels).reshape(-1).to(device=device, dtype=torch.int32).contiguous()
        self.lengths, self.units, self.lag, self.K = lengths, unit_lengths, int(lag), int(K)
        self.ws = torch.empty(max(binding.micro_resampled_counts_workspace_bytes(len(lengths), len(unit_lengths)), 8),
                              dtype=torch.uint8, device=device)

    def __call__(self, weights):
        w = torch.from_numpy(np.ascontiguousarray(weights, np.uint32)).to(self.labels.device)
        out = binding.micro_resampled_counts(self.labels, self.lengths, self.units, self.lag, self.K, w, workspace=self.ws)
        return out.cpu().numpy()


def resampled_counter(labels, lengths, unit_lengths, lag, K, device):
    """count(weights) -> (b, K, K) for weights (b, n_units): the weighted sliding-window counts of b resamples on the GPU
    (dff_micro_resampled_counts)."""
    return _DeviceResampledCounts(labels, lengths, unit_lengths, lag, K, device)


class _DeviceBatchedSweeps:
    """The problems' S and c on the device once; sweep(x, n, skip) runs n sweeps of every problem not skipped from the host
    array x (B, Kmax) -> (x after them, err (n, B))."""

    def __init__(self, S, c, ks, device):
        self.S = torch.from_numpy(np.ascontiguousarray(S, np.float64)).to(device)
        self.c = torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(device)
        self.ks = np.asarray(ks, np.int32)
        self.ws = torch.empty(max(binding.msm_batched_workspace_bytes(len(self.ks), self.c.shape[1]), 8), dtype=torch.uint8,
                              device=device)

    def __call__(self, x, n, skip=None):
        xd = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(self.S.device)
        err = binding.msm_reversible_steps_batched(self.S, self.c, self.ks, xd, n, skip=skip, workspace=self.ws)
        return xd.cpu().numpy(), err.cpu().numpy()


def batched_reversible_sweeper(S, c, ks, device):
    """sweep(x, n, skip) -> (x', err (n, B)) for B problems: S (B, Kmax, Kmax) with problem b's COMPACT (ks[b], ks[b]) matrix
    at the start of its slot (flat), c and x (B, Kmax) with its first ks[b] entries (dff_msm_reversible_steps_batched)."""
    return _DeviceBatchedSweeps(S, c, ks, device)


class MsmBootstrap:
    """What bootstrap_msm returns.  timescales (B, k) in frames, NaN where undefined; stationary (B, K) on the full state
    index, zero outside a resample's active set; n_active, active_count_share, converged, n_iter (B,); weights (B, n_units)
    and unit_lengths as resampled; point: the MarkovStateModel of the unresampled counts."""

    def __init__(self, timescales, stationary, n_active, active_count_share, converged, n_iter, weights, unit_lengths, point):
        self.timescales, self.stationary, self.n_active = timescales, stationary, n_active
        self.active_count_share, self.converged, self.n_iter = active_count_share, converged, n_iter
        self.weights, self.unit_lengths, self.point = weights, unit_lengths, point

    @property
    def n_failed(self):
        """Resamples that did not converge or have no k-th timescale."""
        return int(np.sum(~self.converged | np.isnan(self.timescales[:, -1])))

    def std(self):
        """Standard deviation (ddof = 1) of each timescale over the resamples where it is finite -> (k,); NaN below two."""
        return percentile_std(self.timescales)

    def interval(self, confidence=0.95):
        """The percentile interval of each timescale over the resamples where it is finite -> (lo, hi), each (k,)."""
        return percentile_interval(self.timescales, confidence)


def percentile_std(values):
    out = np.full(values.shape[1], np.nan)
    for j, col in enumerate(values.T):
        col = col[np.isfinite(col)]
        if col.size >= 2:
            out[j] = col.std(ddof=1)
    return out


def percentile_interval(values, confidence=0.95):
    """(lo, hi), each (k,): the (1 -+ confidence) / 2 percentiles of every column of values (B, k) over its finite entries."""
    if not 0 < float(confidence) < 1:
        raise ValueError("confidence must lie in (0, 1)")
    lo, hi = np.full(values.shape[1], np.nan), np.full(values.shape[1], np.nan)
    for j, col in enumerate(values.T):
        col = col[np.isfinite(col)]
        if col.size:
            lo[j], hi[j] = np.percentile(col, [50 * (1 - confidence), 50 * (1 + confidence)])
    return lo, hi


def bootstrap_msm(labels, lagtime, traj_lengths=None, n_states=None, *, n_resamples=100, block_frames=None, seed=0,
                  weights=None, k=3, tol=1e-12, max_iter=1_000_000, steps_per_sync=256, resample_batch=None,
                  eigensolver="host", device="cuda:0"):
    """Bootstrap of a reversible MarkovStateModel at `lagtime`: the units of resampling_units(traj_lengths, block_frames) are
    drawn with replacement n_resamples times (bootstrap_weights(n_units, n_resamples, seed), or `weights` (B, n_units)), the
    weighted counts of all resamples come from one pass over the labels and their estimators advance together, a problem
    leaving the batch at its first sweep below tol.  Resample b equals
    MarkovStateModel(lagtime, tol=tol, max_iter=max_iter, steps_per_sync=steps_per_sync).fit_counts(counts_b) bit for bit.
    resample_batch bounds the resamples in flight (default: B K^2 counts and matrices under 1 GiB each) -> MsmBootstrap.
    eigensolver="host": the timescales of each resample from np.linalg.eigvalsh; "device": those of each batch from one
    msm_spectrum call (dff_sym_eig_topk), equal up to the two solvers' rounding; every other field is the same."""
    k = int(k)
    if k < 1:
        raise ValueError("bootstrap_msm: k must be >= 1")
    on_device = _check_eigensolver(eigensolver, "bootstrap_msm")
    plan = _BootstrapPlan("bootstrap_msm", labels, lagtime, traj_lengths, n_states, n_resamples, block_frames, seed, weights, tol,
                          max_iter, steps_per_sync, resample_batch, device)
    B, K = plan.B, plan.K
    point = plan.point()
    ts = np.full((B, k), np.nan)
    stationary = np.zeros((B, K))
    n_active, share = np.zeros(B, np.int64), np.zeros(B)
    converged, n_iter = np.zeros(B, bool), np.zeros(B, np.int64)
    for b0, models in plan.batches():
        if on_device:
            ts[b0:b0 + len(models)] = msm_spectrum(models, k=k, device=plan.device).timescales
        for i, m in enumerate(models):
            b = b0 + i
            if not on_device:
                ts[b] = m.timescales(k)
            stationary[b, m.active_set] = m.stationary_distribution
            n_active[b], share[b], converged[b], n_iter[b] = len(m.active_set), m.active_count_share, m.converged, m.n_iter
    return MsmBootstrap(ts, stationary, n_active, share, converged, n_iter, plan.weights, plan.units, point)


class _BootstrapPlan:
    """What bootstrap_msm and bootstrap_passage share: the checked arguments, the units and their multiplicities, the counter,
    and batches(): the fitted reversible models of the resamples, resample_batch at a time, as (first resample, models)."""

    def __init__(self, what, labels, lagtime, traj_lengths, n_states, n_resamples, block_frames, seed, weights, tol, max_iter,
                 steps_per_sync, resample_batch, device):
        self.device = dev = torch.device(device)
        lab = torch.as_tensor(labels).reshape(-1)
        n = int(lab.numel())
        lengths = _check_lengths(traj_lengths, n)
        if n_states is None:
            n_states = int(lab.max()) + 1 if n else 0
        self.K = K = int(n_states)
        if not 1 <= K <= MSM_MAX_STATES:
            raise ValueError(f"{what}: n_states must be 1..{MSM_MAX_STATES}, not {n_states}")
        proto = MarkovStateModel(lagtime, True, tol, max_iter, steps_per_sync, device=dev)          # checks the settings
        self.lagtime, self.settings = proto.lagtime, (tol, max_iter, steps_per_sync)
        self.units = units = resampling_units(lengths, block_frames)
        if units.size < 1:
            raise ValueError(f"{what}: no resampling units (no frames)")
        if weights is None:
            w = bootstrap_weights(units.size, n_resamples, seed)
        else:
            w = np.asarray(weights)
            if w.ndim != 2 or w.shape[1] != units.size or w.shape[0] < 1 or (w < 0).any() or (w > 2 ** 32 - 1).any():
                raise ValueError(f"{what}: weights must be (B, {units.size}) multiplicities in 0 .. 2^32 - 1")
            w = w.astype(np.uint32)
        self.weights, self.B = w, int(w.shape[0])
        if resample_batch is None:
            resample_batch = max(1, min(self.B, MSM_MAX_BATCH, (1 << 30) // (8 * K * K)))
        self.rb = int(resample_batch)
        if not 1 <= self.rb <= MSM_MAX_BATCH:
            raise ValueError(f"{what}: resample_batch must be 1..{MSM_MAX_BATCH}")
        self.count = resampled_counter(lab, lengths, units, proto.lagtime, K, dev)

    def model(self):
        tol, max_iter, steps_per_sync = self.settings
        return MarkovStateModel(self.lagtime, True, tol, max_iter, steps_per_sync, device=self.device)

    def point(self):
        """the model of the unresampled counts"""
        return self.model().fit_counts(self.count(np.ones((1, self.units.size), np.uint32))[0])

    def batches(self):
        tol, max_iter, steps_per_sync = self.settings
        for b0 in range(0, self.B, self.rb):
            counts = self.count(self.weights[b0:b0 + self.rb])
            models, prob = [], []                                    # prob: (model, S, c) of the resamples that iterate
            for Cb in counts:
                m = self.model()
                Ca = m._active_counts(Cb)
                if Ca is not None:
                    prob.append((m, *_reversible_problem(Ca)))
                models.append(m)
            if prob:
                _sweep_batch(prob, batched_reversible_sweeper, self.device, tol, max_iter, steps_per_sync)
            yield b0, models


def _sweep_batch(prob, sweeper, device, tol, max_iter, steps_per_sync):
    """MarkovStateModel._fit_reversible on every (model, S, c) of prob at once: the same start, the same batches of sweeps,
    the same stopping rule per problem; a problem is skipped from the batch after the one it stops in."""
    P = len(prob)
    ks = np.array([len(c) for _, _, c in prob], np.int32)
    Kmax = int(ks.max())
    S_all, c_all, x = np.zeros((P, Kmax * Kmax)), np.zeros((P, Kmax)), np.zeros((P, Kmax))
    for p, (m, S, c) in enumerate(prob):
        S_all[p, :ks[p] * ks[p]] = S.reshape(-1)
        c_all[p, :ks[p]] = c
        x[p, :ks[p]] = 0.5 * S.sum(axis=1)
        m.converged = False
    sweep = sweeper(S_all.reshape(P, Kmax, Kmax), c_all, ks, device)
    live = np.ones(P, bool)
    done = 0                                                         # sweeps every live problem has behind it
    while done < max_iter and live.any():
        n = min(steps_per_sync, max_iter - done)
        x, err = sweep(x, n, ~live)
        done += n
        for p in np.nonzero(live)[0]:
            m = prob[p][0]
            m.converged, more, stop = _sweeps_outcome(err[:, p], tol)
            m.n_iter += more
            live[p] = not stop
    for p, (m, S, c) in enumerate(prob):
        m.transition_matrix, m.stationary_distribution, m.flux_matrix = reversible_model(S, c, x[p, :ks[p]])


def implied_timescales_bootstrap(labels, lagtimes, traj_lengths=None, n_states=None, k=3, *, n_resamples=100,
                                 block_frames=None, seed=0, confidence=0.95, tol=1e-12, max_iter=1_000_000,
                                 steps_per_sync=256, resample_batch=None, eigensolver="host", device="cuda:0"):
    """implied_timescales with error bars: (point, lo, hi), each float64 (n_lags, k) in frames -- the timescales of the
    unresampled model at every lag time and the percentile interval of bootstrap_msm over the same draws at each
    (eigensolver: as bootstrap_msm)."""
    on_device = _check_eigensolver(eigensolver, "implied_timescales_bootstrap")
    lagtimes = [int(v) for v in lagtimes]
    point, lo, hi = (np.full((len(lagtimes), int(k)), np.nan) for _ in range(3))
    for i, lag in enumerate(lagtimes):
        bs = bootstrap_msm(labels, lag, traj_lengths, n_states, n_resamples=n_resamples, block_frames=block_frames, seed=seed,
                           k=k, tol=tol, max_iter=max_iter, steps_per_sync=steps_per_sync, resample_batch=resample_batch,
                           eigensolver=eigensolver, device=device)
        point[i] = msm_spectrum(bs.point, k=k, device=device).timescales[0] if on_device else bs.point.timescales(k)
        lo[i], hi[i] = bs.interval(confidence)
    return point, lo, hi


class _Microstates:
    """TIC projections (n, k) -> microstate labels, for MsmEvaluator and MsmPassageEvaluator.  The microstates are `centers`
    (n_microstates, k) when given, else MicrostateKMeans(n_microstates, seed=seed) fitted on the first projections labels()
    sees and kept on .kmeans; every call discretises on the same .centers.  `what` is the caller's name in the error texts."""

    def __init__(self, what, n_microstates, k, centers, seed, device):
        self.n_microstates = int(n_microstates)
        if not 1 <= self.n_microstates <= MSM_MAX_STATES:
            raise ValueError(f"{what}: n_microstates must be 1..{MSM_MAX_STATES}")
        self.seed, self.device = int(seed), device
        self.kmeans = self.centers = None
        if centers is not None:
            c = np.array(centers, np.float64)
            if c.ndim != 2 or c.shape != (self.n_microstates, k) or not np.all(np.isfinite(c)):
                raise ValueError(f"{what}: centers must be finite and ({self.n_microstates}, {k})")
            self.centers = c

    def labels(self, proj):
        """int32 tensor (n,) on proj's device; -1 for a non-finite projection"""
        if self.centers is None:
            self.kmeans = MicrostateKMeans(self.n_microstates, seed=self.seed, device=self.device).fit(proj)
            self.centers = self.kmeans.cluster_centers
        return binding.micro_kmeans_step(proj, self.centers, accumulate=False)["labels"]


class _PointModel:
    """The model MsmEvaluator and MsmPassageEvaluator estimate from labels: the checked lag time and bootstrap settings, and
    fit().  `what` is the caller's name in the error texts."""

    def __init__(self, what, lagtime, n_bootstrap, block_frames, confidence, bootstrap_seed, device):
        if lagtime is None or int(lagtime) != lagtime or int(lagtime) < 1:
            raise ValueError(f"{what}: lagtime must be an integer >= 1 (frames)")
        self.n_bootstrap, self.block_frames = int(n_bootstrap), block_frames
        self.confidence, self.bootstrap_seed = float(confidence), int(bootstrap_seed)
        if self.n_bootstrap < 0 or not 0 < self.confidence < 1:
            raise ValueError(f"{what}: n_bootstrap must be >= 0 and confidence in (0, 1)")
        if block_frames is not None and (int(block_frames) != block_frames or int(block_frames) < 1):
            raise ValueError(f"{what}: block_frames must be an integer >= 1")
        self.lagtime, self.device = int(lagtime), device

    def fit(self, labels, lengths, n_states, name, bootstrap=None, **kw):
        """(the reversible MarkovStateModel of the labels of `name`, "samples" or "refs", its bootstrap or None).  With
        n_bootstrap > 0 and `bootstrap` (bootstrap_msm or bootstrap_passage; kw: its own arguments) the model is the
        bootstrap's point model; refs and samples draw independently: the reference's seed is one higher."""
        if bootstrap is None or self.n_bootstrap == 0:
            return MarkovStateModel(self.lagtime, device=self.device).fit(labels, lengths, n_states), None
        bs = bootstrap(labels, self.lagtime, traj_lengths=lengths, n_states=n_states, n_resamples=self.n_bootstrap,
                       block_frames=self.block_frames, seed=self.bootstrap_seed + (name == "refs"), device=self.device, **kw)
        return (bs.point["model"] if isinstance(bs.point, dict) else bs.point), bs


class MsmEvaluator(_TrajectoryEvaluator):
    """Do the sampled trajectories relax like the reference's?  Frames -> TIC projection (`tica`: a TicEvaluator, a TICA, a
    saved reference or a (mean, coeff) pair, at most 8 components) -> n_microstates k-means microstates -> a reversible
    MarkovStateModel at `lagtime` (frames).  The microstates are `centers` (K, k) when given, else fitted on the
    reference's projection (ref_data: MD frames (m, N, 3) in Angstrom, trajectories of ref_traj_lengths), else on the first
    samples eval() sees; both ensembles are discretised on the same centres.

    eval(xyz, traj_lengths=None) -- None: ONE trajectory -- returns a dict:
      timescales           list of the n_timescales slowest implied timescales, in units of frame_time (NaN where undefined)
      n_active             states in the largest strongly connected set
      active_count_share   share of the transition counts that stay inside it
      converged            1.0 when the estimator met its tolerance, else 0.0
      samples_nonfinite    frames left out (a non-finite projection)
    and with ref_data the same keys with the suffix _ref, log10_timescale_ratio (list: samples over reference, NaN unless
    both are positive and finite) and stationary_js, js_divergence of the two stationary distributions over the union of
    the two active sets (zero outside one's own).  The models stay on .models under "samples" / "refs".  Without the HIP
    library: DffLibraryError.

    n_bootstrap > 0 adds error bars from bootstrap_msm (units: the trajectories, or blocks of block_frames frames):
    timescales_lo / timescales_hi (the percentile interval at `confidence`), timescales_std and bootstrap_failed, with
    ref_data also their _ref counterparts and log10_timescale_ratio_lo / _hi, percentiles of the ratio of resample b of
    the samples to resample b of the reference (seeds bootstrap_seed and bootstrap_seed + 1: independent draws).  The
    discretisation is fixed: the centres are not refitted per resample.  The bootstraps stay on .bootstraps.
    eigensolver="device" takes every spectrum from msm_spectrum (dff_sym_eig_topk) instead of np.linalg.eigvalsh."""

    KEYS = ("timescales", "n_active", "active_count_share", "converged", "samples_nonfinite")

    def __init__(self, mol_name, tica, n_microstates=200, lagtime=None, n_timescales=3, frame_time=1.0, ref_data=None,
                 ref_traj_lengths=None, centers=None, seed=0, *, n_bootstrap=0, block_frames=None, confidence=0.95,
                 bootstrap_seed=0, eigensolver="host", device="cuda:0"):
        super().__init__("MsmEvaluator", mol_name, frame_time, device)
        self.eigensolver = eigensolver
        self._spectrum_on_device = _check_eigensolver(eigensolver, "MsmEvaluator")
        self._point = _PointModel("MsmEvaluator", lagtime, n_bootstrap, block_frames, confidence, bootstrap_seed, self.device)
        self.lagtime = self._point.lagtime
        self.n_timescales = int(n_timescales)
        if self.n_timescales < 1:
            raise ValueError("MsmEvaluator: n_timescales must be >= 1")
        self.mean, self.coeff = _tica_model(tica, "MsmEvaluator", TICA_MAX_DIM)
        self._micro = _Microstates("MsmEvaluator", n_microstates, self.coeff.shape[1], centers, seed, self.device)
        self.n_microstates = self._micro.n_microstates
        self.models, self.labels, self.bootstraps = {}, {}, {}
        self._start(ref_data, ref_traj_lengths)

    centers = property(lambda self: self._micro.centers, doc="the microstate centres (K, k); None until they are fitted")
    kmeans = property(lambda self: self._micro.kmeans, doc="the fitted MicrostateKMeans; None when the centres were given")

    def project(self, x):
        return binding.struct_tic(x, self.mean, self.coeff)

    def _analyse(self, x, lengths, name):
        labels = self._micro.labels(self.project(x))
        model, bs = self._point.fit(labels, lengths, self.n_microstates, name, bootstrap_msm, k=self.n_timescales,
                                    eigensolver=self.eigensolver)
        self.models[name], self.labels[name] = model, labels.cpu().numpy()
        ts = msm_spectrum(model, k=self.n_timescales, device=self.device).timescales[0] if self._spectrum_on_device else None
        res = self.summarize(model, self.n_timescales, self.frame_time, int((labels < 0).sum()), timescales=ts)
        if bs is not None:
            self.bootstraps[name] = bs
            lo, hi = bs.interval(self._point.confidence)
            res.update({"timescales_lo": [float(v) * self.frame_time for v in lo],
                        "timescales_hi": [float(v) * self.frame_time for v in hi],
                        "timescales_std": [float(v) * self.frame_time for v in bs.std()],
                        "bootstrap_failed": float(bs.n_failed)})
        return res

    @staticmethod
    def summarize(model, n_timescales=3, frame_time=1.0, samples_nonfinite=0, timescales=None):
        """eval()'s dict from a fitted MarkovStateModel: numpy only.  timescales: the model's, in frames, when they were
        computed elsewhere (eigensolver="device"); None: model.timescales(n_timescales)."""
        ts = model.timescales(n_timescales) if timescales is None else timescales
        return {"timescales": [float(v) * frame_time for v in ts],
                "n_active": float(len(model.active_set)), "active_count_share": float(model.active_count_share),
                "converged": float(bool(model.converged)), "samples_nonfinite": float(samples_nonfinite)}

    @staticmethod
    def stationary_js(model_a, model_b):
        """js_divergence of two stationary distributions over the union of the two active sets, zero outside one's own."""
        union = np.union1d(model_a.active_set, model_b.active_set)
        p = np.zeros((2, len(union)))
        for row, m in zip(p, (model_a, model_b)):
            row[np.searchsorted(union, m.active_set)] = m.stationary_distribution
        return float(js_divergence(p[0], p[1]))

    def _compare(self, res, ref):
        res["log10_timescale_ratio"] = _log10_ratio(res["timescales"], ref["timescales"])
        res["stationary_js"] = self.stationary_js(self.models["samples"], self.models["refs"])
        if self._point.n_bootstrap > 0:                              # resample b of the samples over resample b of the reference
            a, b = self.bootstraps["samples"].timescales, self.bootstraps["refs"].timescales
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where((a > 0) & (b > 0), np.log10(a / b), np.nan)
            lo, hi = percentile_interval(r, self._point.confidence)
            res["log10_timescale_ratio_lo"], res["log10_timescale_ratio_hi"] = [float(v) for v in lo], [float(v) for v in hi]


# ---- spectra of reversible models on the device: the largest eigenpairs of pi^(1/2) T pi^(-1/2), many models per call ----
SPECTRUM_MAX_BATCH = binding.SYM_EIG_MAX_BATCH
SPECTRUM_MAX_K = binding.SYM_EIG_MAX_K
SPECTRUM_BYTES = 1 << 30         # matrices, vectors and workspace of one dff_sym_eig_topk call of spectral_solver


def _device_chunks(device, P, per, cap, max_batch, outputs, call, mats=None, mat_of=None, most=None):
    """The loop behind spectral_solver, dirichlet_solver and propagator: problems 0 .. P - 1 go to the GPU in chunks of at most
    max_batch (and `most`) problems of `per` bytes each that stay under `cap` bytes, one library call per chunk.  call(sl, up,
    mats_dev, local) -> device tensors, one per host array of `outputs` (NaN- or zero-filled; None: not wanted), whose rows sl
    receive them; up(a) puts a host array on the device.  With mats and mat_of (P,) a chunk uploads only the matrices it uses,
    and local (int32) indexes them."""
    chunk = max(1, min(max_batch, cap // per, *(() if most is None else (most,))))

    def up(a):
        return torch.from_numpy(a).to(device)

    for p0 in range(0, P, chunk):
        sl = slice(p0, min(P, p0 + chunk))
        if mat_of is None:
            res = call(sl, up, None, None)
        else:
            used, local = np.unique(mat_of[sl], return_inverse=True)
            res = call(sl, up, up(mats[used]), local.astype(np.int32))
        for host, dev in zip(outputs, res):
            if host is not None:
                host[sl] = dev.cpu().numpy()
    return outputs


class _DeviceSpectral:
    """solve(a (P, Kmax, Kmax), ks (P,), k, vectors) -> (w (P, k), v (P, k, Kmax) | None, status (P,)), host arrays in and out:
    the problems go to the GPU in chunks that stay under SPECTRUM_BYTES, each chunk one dff_sym_eig_topk call."""

    def __init__(self, device):
        self.device = torch.device(device)

    def __call__(self, a, ks, k, vectors):
        a = np.ascontiguousarray(a, np.float64)
        P, Kmax = a.shape[0], a.shape[1]
        ks = np.asarray(ks, np.int32).reshape(-1)
        per = 8 * (2 * Kmax * Kmax + 5 + k * (1 + Kmax))             # a matrix, a slice of the workspace, the outputs
        outputs = (np.full((P, k), np.nan), np.full((P, k, Kmax), np.nan) if vectors else None, np.zeros(P, np.int32))

        def call(sl, up, _mats, _local):
            return binding.sym_eig_topk(up(a[sl]), ks[sl], k, vectors=vectors)

        return _device_chunks(self.device, P, per, SPECTRUM_BYTES, SPECTRUM_MAX_BATCH, outputs, call)


def spectral_solver(device):
    """solve(a (P, Kmax, Kmax), ks (P,), k, vectors) -> (w, v | None, status) on the GPU (dff_sym_eig_topk): the k largest
    eigenvalues, descending and NaN-padded, of P symmetric matrices, matrix p a compact (ks[p], ks[p]) matrix at the start of
    its slot; unit eigenvectors in rows, the component of largest magnitude positive."""
    return _DeviceSpectral(device)


class MsmSpectrum:
    """What msm_spectrum returns for P models: eigenvalues (P, k + 1), largest first (the first is 1), NaN-padded where an
    active set has fewer states; timescales (P, k) in frames by the rule of MarkovStateModel.timescales; right and left
    (P, k + 1, K) on the FULL state index, zero outside a model's active set (None when no vectors were asked for); status
    (P,): dff_sym_eig_topk's (0 solved, 2: the vectors did not converge and are NaN)."""

    def __init__(self, eigenvalues, timescales, right, left, status):
        self.eigenvalues, self.timescales, self.right, self.left, self.status = eigenvalues, timescales, right, left, status


def msm_spectrum(models, k=3, vectors=False, *, device=None):
    """The k + 1 largest eigenvalues, the k slowest timescales and optionally the eigenvectors of one fitted reversible
    MarkovStateModel or of a list of them, in ONE dff_sym_eig_topk call on their symmetrized() matrices (active sets of
    differing size share it) -> MsmSpectrum.  Right eigenvectors psi = v / sqrt(pi): sum_i pi_i psi_i^2 = 1, the component of
    largest magnitude positive (psi_1 = 1); left ones phi = pi psi (phi_1 = pi).  A model whose active set is one state is
    not sent: lambda = 1, psi = phi = 1.  device: default the first model's.  ValueError for a model that is not reversible or
    not fitted."""
    ms = [models] if isinstance(models, MarkovStateModel) else list(models)
    k = int(k)
    if not 1 <= k < SPECTRUM_MAX_K:
        raise ValueError(f"msm_spectrum: k must be 1..{SPECTRUM_MAX_K - 1}")
    if not ms:
        raise ValueError("msm_spectrum: no model")
    mats = [m.symmetrized() for m in ms]
    P, K = len(ms), max(len(m.count_matrix) for m in ms)
    lam, status = np.full((P, k + 1), np.nan), np.zeros(P, np.int32)
    right, left = (np.zeros((P, k + 1, K)), np.zeros((P, k + 1, K))) if vectors else (None, None)
    send = [p for p, M in enumerate(mats) if len(M) > 1]
    for p, M in enumerate(mats):
        if len(M) == 1:
            lam[p, 0] = 1.0
            if vectors:
                right[p, 0, ms[p].active_set] = left[p, 0, ms[p].active_set] = 1.0
                right[p, 1:, ms[p].active_set] = left[p, 1:, ms[p].active_set] = np.nan
    if send:
        ks = np.array([len(mats[p]) for p in send], np.int32)
        Kmax = int(ks.max())
        a = np.zeros((len(send), Kmax * Kmax))
        for i, p in enumerate(send):
            a[i, :mats[p].size] = mats[p].reshape(-1)
        w, v, st = spectral_solver(device if device is not None else ms[0].device)(a.reshape(len(send), Kmax, Kmax), ks, k + 1,
                                                                                 bool(vectors))
        for i, p in enumerate(send):
            lam[p], status[p] = w[i], st[i]
            if vectors:
                act, r = ms[p].active_set, np.sqrt(ms[p].stationary_distribution)
                psi = v[i][:, :len(act)] / r
                top = np.argmax(np.abs(np.nan_to_num(psi)), axis=1)
                sign = np.where(psi[np.arange(k + 1), top] < 0, -1.0, 1.0)[:, None]
                right[p][:, act] = psi * sign
                left[p][:, act] = v[i][:, :len(act)] * r * sign
    ts = np.stack([_timescales_of(lam[p, 1:], k, m.lagtime) for p, m in enumerate(ms)])
    return MsmSpectrum(lam, ts, right, left, status)


# ---- mean first-passage times, committors and reactive flux of a Markov state model ----
# Each quantity is one Dirichlet problem on the model's flux matrix X_ij = pi_i T_ij (dff_msm_dirichlet_solve): the states of
# the target sets are the boundary, the rest of the active set the interior.  Sets are given on the FULL state index of the
# count matrix; states outside the active set are dropped.
DIRICHLET_MAX_BATCH = binding.MSM_DIRICHLET_MAX_BATCH
DIRICHLET_BYTES = 1 << 30        # flux matrices plus workspace of one dff_msm_dirichlet_solve call of dirichlet_solver


class _DeviceDirichlet:
    """solve(flux, flux_of, ks, role, g, s) -> (u (P, Kmax), status (P,)), host arrays in and out: the problems go to the GPU
    in chunks whose flux matrices and workspace stay under DIRICHLET_BYTES, each chunk one dff_msm_dirichlet_solve call."""

    def __init__(self, device):
        self.device = torch.device(device)

    def __call__(self, flux, flux_of, ks, role, g, s):
        role = np.ascontiguousarray(role, np.int32)
        P, Kmax = role.shape
        flux = np.ascontiguousarray(flux, np.float64).reshape(-1, Kmax, Kmax)
        flux_of, ks = np.asarray(flux_of, np.int64).reshape(-1), np.asarray(ks, np.int32).reshape(-1)
        g, s = np.ascontiguousarray(g, np.float64), np.ascontiguousarray(s, np.float64)
        per = 8 * (2 * Kmax * Kmax + 33 * Kmax + 1)                  # a matrix of its own and a slice of the workspace

        def call(sl, up, flux_dev, local):
            return binding.msm_dirichlet_solve(flux_dev, ks[sl], up(role[sl]), up(g[sl]), up(s[sl]), flux_of=local)

        outputs = (np.full((P, Kmax), np.nan), np.zeros(P, np.int32))
        return _device_chunks(self.device, P, per, DIRICHLET_BYTES, DIRICHLET_MAX_BATCH, outputs, call, mats=flux, mat_of=flux_of)


def dirichlet_solver(device):
    """solve(flux (M, Kmax, Kmax), flux_of (P,), ks (P,), role, g, s (P, Kmax)) -> (u (P, Kmax), status (P,)) on the GPU
    (dff_msm_dirichlet_solve); matrix m is a compact (K, K) matrix at the start of its slot."""
    return _DeviceDirichlet(device)


def _active_states(model, states, what, name):
    """indices within the active set of the states of `states` (full index) that are active; ValueError when none is"""
    model._need_fit()
    st = np.unique(np.asarray(states, np.int64).reshape(-1))
    if st.size and (st[0] < 0 or st[-1] >= len(model.count_matrix)):
        raise ValueError(f"{what}: {name} holds a state outside 0 .. {len(model.count_matrix) - 1}")
    idx = np.flatnonzero(np.isin(model.active_set, st))
    if idx.size == 0:
        raise ValueError(f"{what}: {name} has no state in the active set")
    return idx


def _passage_problems(model, A, B, what):
    """The three problems of a pair of disjoint sets on one model, as rows (role, g, s): MFPT to B, MFPT to A, committor A -> B."""
    a, b = _active_states(model, A, what, "A"), _active_states(model, B, what, "B")
    if np.intersect1d(a, b).size:
        raise ValueError(f"{what}: A and B overlap")
    K = len(model.active_set)
    role, g, s = np.zeros((3, K), np.int32), np.zeros((3, K)), np.zeros((3, K))
    role[0, b] = role[1, a] = role[2, a] = role[2, b] = 1
    s[:2] = float(model.lagtime)
    g[2, b] = 1.0
    return a, b, role, g, s


def _host_dirichlet(T, role, g, s):
    """The fallback for a model without detailed balance: np.linalg.solve on (I - T_II) u_I = s_I + T_IB g_B."""
    I, Bd = np.flatnonzero(role == 0), np.flatnonzero(role == 1)
    u = np.where(role == 1, g, 0.0)
    if I.size:
        u[I] = np.linalg.solve(np.eye(I.size) - T[np.ix_(I, I)], s[I] + T[np.ix_(I, Bd)] @ g[Bd])
    return u


def _solve_on_model(model, role, g, s, what):
    """u (P, K) of P problems on one fitted model: the GPU call on its flux matrix, or the host fallback (reversible=False)"""
    if model.flux_matrix is None:
        return np.stack([_host_dirichlet(model.transition_matrix, r, gg, ss) for r, gg, ss in zip(role, g, s)])
    P, K = role.shape
    u, status = dirichlet_solver(model.device)(model.flux_matrix.reshape(1, K, K), np.zeros(P, np.int64), np.full(P, K, np.int32),
                                               role, g, s)
    if (status != 0).any():
        raise ValueError(f"{what}: the linear system of problem {int(np.flatnonzero(status)[0])} failed (status "
                         f"{int(status[status != 0][0])}): the flux matrix is not that of a connected reversible model")
    return u


def mfpt(model, target, source=None):
    """Mean first-passage times to the set `target` of a fitted MarkovStateModel, in frames: float64 (n_active,), zero on the
    target -- or, with `source`, their stationary-weighted mean over that set (a float).  Sets are state indices of the count
    matrix; states outside the active set are dropped.  ValueError when a set has no active state or the two overlap.
    reversible=True: one dff_msm_dirichlet_solve problem on model.flux_matrix; reversible=False: np.linalg.solve on I - T_II on
    the host (the device call needs the symmetry of detailed balance)."""
    t = _active_states(model, target, "mfpt", "target")
    src = None
    if source is not None:
        src = _active_states(model, source, "mfpt", "source")
        if np.intersect1d(src, t).size:
            raise ValueError("mfpt: source and target overlap")
    K = len(model.active_set)
    role = np.zeros((1, K), np.int32)
    role[0, t] = 1
    m = _solve_on_model(model, role, np.zeros((1, K)), np.full((1, K), float(model.lagtime)), "mfpt")[0]
    if src is None:
        return m
    pi = model.stationary_distribution[src]
    return float(np.dot(pi, m[src]) / pi.sum())


def committor(model, A, B):
    """The forward committor from A to B of a fitted MarkovStateModel: q (n_active,), the probability of reaching B before A,
    0 on A and 1 on B.  The backward committor of a reversible model is 1 - q.  Sets and paths as mfpt."""
    _, _, role, g, s = _passage_problems(model, A, B, "committor")
    return _solve_on_model(model, role[2:], g[2:], s[2:], "committor")[0]


class ReactiveFlux:
    """What reactive_flux returns: committor q (n_active,), net_flux (n_active, n_active) f+_ij = max(0, X_ij (q_j - q_i)),
    total_flux F = sum_{i in A, j not in A} X_ij q_j, rate k_AB = F / (lagtime sum_i pi_i (1 - q_i)) per frame."""

    def __init__(self, committor, net_flux, total_flux, rate):
        self.committor, self.net_flux, self.total_flux, self.rate = committor, net_flux, float(total_flux), float(rate)


def _reactive_flux(X, pi, q, a, lagtime):
    """transition-path theory of a reversible model from its flux matrix, stationary distribution and forward committor"""
    net = np.maximum(0.0, X * (q[None, :] - q[:, None]))
    out = np.ones(len(q), bool)
    out[a] = False
    F = float((X[np.ix_(a, np.flatnonzero(out))] @ q[out]).sum())
    return ReactiveFlux(q, net, F, F / (float(lagtime) * float(np.dot(pi, 1.0 - q))))


def reactive_flux(model, A, B):
    """Transition-path theory from A to B on a fitted reversible MarkovStateModel -> ReactiveFlux."""
    if model.flux_matrix is None:
        model._need_fit()
        raise ValueError("reactive_flux: needs a reversible model (its flux matrix)")
    a, _, role, g, s = _passage_problems(model, A, B, "reactive_flux")
    q = _solve_on_model(model, role[2:], g[2:], s[2:], "reactive_flux")[0]
    return _reactive_flux(model.flux_matrix, model.stationary_distribution, q, a, model.lagtime)


class PassageBootstrap:
    """What bootstrap_passage returns.  mfpt_ab, mfpt_ba (frames), rate_ab, rate_ba (per frame): (B,), NaN where a resample has
    no answer (a set without an active state, a failed system); committor (B, K) on the full state index, NaN outside a
    resample's active set; converged (B,); weights, unit_lengths as resampled; point: a dict of the same quantities of the
    unresampled model ("model": the MarkovStateModel)."""

    FIELDS = ("mfpt_ab", "mfpt_ba", "rate_ab", "rate_ba")

    def __init__(self, mfpt_ab, mfpt_ba, rate_ab, rate_ba, committor, converged, weights, unit_lengths, point):
        self.mfpt_ab, self.mfpt_ba, self.rate_ab, self.rate_ba = mfpt_ab, mfpt_ba, rate_ab, rate_ba
        self.committor, self.converged, self.weights, self.unit_lengths, self.point = committor, converged, weights, unit_lengths, point

    def _table(self):
        return np.stack([getattr(self, f) for f in self.FIELDS], axis=1)

    @property
    def n_failed(self):
        """Resamples whose estimator did not converge or that lack one of the four numbers."""
        return int(np.sum(~self.converged | ~np.isfinite(self._table()).all(axis=1)))

    def std(self):
        """{field: standard deviation (ddof = 1) over the resamples where it is finite}; NaN below two."""
        return dict(zip(self.FIELDS, (float(v) for v in percentile_std(self._table()))))

    def interval(self, confidence=0.95):
        """{field: (lo, hi)}: the percentile interval over the resamples where the field is finite."""
        lo, hi = percentile_interval(self._table(), confidence)
        return {f: (float(a), float(b)) for f, a, b in zip(self.FIELDS, lo, hi)}


def _passage_batch(models, A, B, K_full, device):
    """mfpt A -> B, mfpt B -> A, rates and the committor of every model of `models`: ONE dirichlet_solver call with three
    problems per model that has both sets, each model's flux matrix shared by its three -> rows (len(models), 4), committor
    (len(models), K_full)."""
    out, comm = np.full((len(models), 4), np.nan), np.full((len(models), K_full), np.nan)
    todo = []
    for i, m in enumerate(models):
        try:
            todo.append((i, m) + _passage_problems(m, A, B, "bootstrap_passage"))
        except ValueError:
            continue                                                 # a set lost all its states in this resample
    if not todo:
        return out, comm
    Kmax = max(len(m.active_set) for _, m, *_ in todo)
    P = 3 * len(todo)
    flux = np.zeros((len(todo), Kmax * Kmax))
    role, g, s = np.ones((P, Kmax), np.int32), np.zeros((P, Kmax)), np.zeros((P, Kmax))
    ks = np.zeros(P, np.int32)
    for n, (i, m, a, b, r3, g3, s3) in enumerate(todo):
        K = len(m.active_set)
        flux[n, :K * K] = m.flux_matrix.reshape(-1)
        role[3 * n:3 * n + 3, :K], g[3 * n:3 * n + 3, :K], s[3 * n:3 * n + 3, :K], ks[3 * n:3 * n + 3] = r3, g3, s3, K
    u, status = dirichlet_solver(device)(flux.reshape(len(todo), Kmax, Kmax), np.repeat(np.arange(len(todo)), 3), ks, role, g, s)
    for n, (i, m, a, b, *_ ) in enumerate(todo):
        K = len(m.active_set)
        if (status[3 * n:3 * n + 3] != 0).any():
            continue
        pi = m.stationary_distribution
        m_ab, m_ba, q = u[3 * n, :K], u[3 * n + 1, :K], u[3 * n + 2, :K]
        out[i, 0] = np.dot(pi[a], m_ab[a]) / pi[a].sum()
        out[i, 1] = np.dot(pi[b], m_ba[b]) / pi[b].sum()
        out[i, 2] = _reactive_flux(m.flux_matrix, pi, q, a, m.lagtime).rate
        out[i, 3] = _reactive_flux(m.flux_matrix, pi, 1.0 - q, b, m.lagtime).rate
        comm[i, m.active_set] = q
    return out, comm


def bootstrap_passage(labels, lagtime, A, B, traj_lengths=None, n_states=None, *, n_resamples=100, block_frames=None, seed=0,
                      weights=None, tol=1e-12, max_iter=1_000_000, steps_per_sync=256, resample_batch=None, device="cuda:0"):
    """Bootstrap of the passage between the state sets A and B of a reversible MarkovStateModel at `lagtime`: the resamples of
    bootstrap_msm (the same units, draws and estimator, batch by batch), and per resample the stationary-weighted MFPT from A
    to B and from B to A, the transition-path rates both ways and the committor -- all 3 x (resamples of a batch) linear
    systems in one dff_msm_dirichlet_solve call, each resample's flux matrix shared by its three.  Resample b equals mfpt /
    committor on MarkovStateModel(...).fit_counts(counts_b) bit for bit -> PassageBootstrap."""
    plan = _BootstrapPlan("bootstrap_passage", labels, lagtime, traj_lengths, n_states, n_resamples, block_frames, seed, weights, tol,
                          max_iter, steps_per_sync, resample_batch, device)
    A, B_ = np.unique(np.asarray(A, np.int64).reshape(-1)), np.unique(np.asarray(B, np.int64).reshape(-1))
    for name, st in (("A", A), ("B", B_)):
        if st.size == 0 or st[0] < 0 or st[-1] >= plan.K:
            raise ValueError(f"bootstrap_passage: {name} must hold states in 0 .. {plan.K - 1}")
    if np.intersect1d(A, B_).size:
        raise ValueError("bootstrap_passage: A and B overlap")
    pm = plan.point()
    prow, pcomm = _passage_batch([pm], A, B_, plan.K, plan.device)
    point = dict(zip(PassageBootstrap.FIELDS, (float(v) for v in prow[0])), committor=pcomm[0], model=pm)
    rows, comm = np.full((plan.B, 4), np.nan), np.full((plan.B, plan.K), np.nan)
    converged = np.zeros(plan.B, bool)
    for b0, models in plan.batches():
        rows[b0:b0 + len(models)], comm[b0:b0 + len(models)] = _passage_batch(models, A, B_, plan.K, plan.device)
        converged[b0:b0 + len(models)] = [m.converged for m in models]
    return PassageBootstrap(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], comm, converged, plan.weights, plan.units, point)


def states_by_cv(labels, cv, lo, hi, n_states):
    """(A, B): the microstates whose mean collective variable over their member frames is <= lo, or >= hi (int64 arrays).
    labels (n,) integers (< 0: left out), cv (n,); the means are taken with torch on the device the cv lives on (frames with a
    non-finite cv are left out); a state without frames is in neither set."""
    lo, hi = _check_cores(lo, hi, "states_by_cv")
    n_states = int(n_states)
    if not 1 <= n_states <= MSM_MAX_STATES:
        raise ValueError(f"states_by_cv: n_states must be 1..{MSM_MAX_STATES}")
    cv = torch.as_tensor(cv).reshape(-1).to(torch.float64)
    lab = torch.as_tensor(labels).reshape(-1).to(device=cv.device, dtype=torch.int64)
    if lab.numel() != cv.numel():
        raise ValueError(f"states_by_cv: {lab.numel()} labels for {cv.numel()} values")
    ok = (lab >= 0) & (lab < n_states) & torch.isfinite(cv)
    sums = torch.zeros(n_states, dtype=torch.float64, device=cv.device).index_add_(0, lab[ok], cv[ok])
    cnt = torch.zeros(n_states, dtype=torch.float64, device=cv.device).index_add_(0, lab[ok], torch.ones_like(cv[ok]))
    mean = (sums / cnt).cpu().numpy()                                 # NaN for a state without frames: in neither set
    return np.flatnonzero(mean <= lo).astype(np.int64), np.flatnonzero(mean >= hi).astype(np.int64)


class MsmPassageEvaluator(_TrajectoryEvaluator):
    """How long does folding take in the sampled dynamics, and through which states does it go?  Frames -> TIC projection and
    k-means microstates (`tica`, n_microstates, centers, seed: as for MsmEvaluator) and an order parameter (`folded` and
    cv="q" or "rmsd": as for FoldingKineticsEvaluator) -> the folded and the unfolded SETS of microstates, those whose mean
    order parameter lies in the folded or the unfolded core (states_by_cv with lo, hi; taken from the reference when there is
    ref_data, else from the first samples, and kept) -> a reversible MarkovStateModel at `lagtime` -> mfpt, committor and
    reactive_flux between the two sets.

    eval(xyz, traj_lengths=None) -- None: ONE trajectory -- returns a dict of floats, times in units of frame_time:
      mfpt_folding, mfpt_unfolding      stationary-weighted mean first-passage time unfolded -> folded set and back
      rate_folding, rate_unfolding      transition-path-theory rates k_AB (per frame_time)
      n_folded_states, n_unfolded_states   states of each set inside the model's active set
      committor_mid_share               stationary mass of the states with 0.4 < q < 0.6
      samples_nonfinite                 frames left out (a non-finite projection)
    NaN where a set has no active state.  With ref_data the same keys with the suffix _ref and log10_mfpt_ratio_folding /
    log10_mfpt_ratio_unfolding (samples over reference).  n_bootstrap > 0 adds, from bootstrap_passage over the trajectories or
    blocks of block_frames frames, <key>_lo / _hi (the percentile interval at `confidence`) and <key>_std for the two times and
    the two rates, and bootstrap_failed.  The models stay on .models, the committors on .committors, the bootstraps on
    .bootstraps, under "samples" / "refs".  Without the HIP library: DffLibraryError."""

    KEYS = ("mfpt_folding", "mfpt_unfolding", "rate_folding", "rate_unfolding", "n_folded_states", "n_unfolded_states",
            "committor_mid_share", "samples_nonfinite")
    BARS = (("mfpt_folding", "mfpt_ab"), ("mfpt_unfolding", "mfpt_ba"), ("rate_folding", "rate_ab"), ("rate_unfolding", "rate_ba"))

    def __init__(self, mol_name, tica, folded, n_microstates=200, lagtime=None, cv="q", lo=0.2, hi=0.9, frame_time=1.0,
                 ref_data=None, ref_traj_lengths=None, centers=None, seed=0, *, n_bootstrap=0, block_frames=None,
                 confidence=0.95, bootstrap_seed=0, device="cuda:0"):
        # the error texts name the evaluator whose argument it is, MsmEvaluator or FoldingKineticsEvaluator, as they always have
        super().__init__("MsmEvaluator", mol_name, frame_time, device)
        self._point = _PointModel("MsmEvaluator", lagtime, n_bootstrap, block_frames, confidence, bootstrap_seed, self.device)
        self.lagtime = self._point.lagtime
        self.mean, self.coeff = _tica_model(tica, "MsmEvaluator", TICA_MAX_DIM)
        self._micro = _Microstates("MsmEvaluator", n_microstates, self.coeff.shape[1], centers, seed, self.device)
        self.n_microstates = self._micro.n_microstates
        self.lo, self.hi = _check_cores(lo, hi, "FoldingKineticsEvaluator")
        self._cv = _Observable("FoldingKineticsEvaluator", cv, ("q", "rmsd"), folded, mol_name)
        self.cv, self.folded, self.pairs, self.r0 = cv, self._cv.folded, self._cv.pairs, self._cv.r0
        self.folded_states = self.unfolded_states = None
        self.models, self.labels, self.committors, self.bootstraps = {}, {}, {}, {}
        self._start(ref_data, ref_traj_lengths)

    centers = property(lambda self: self._micro.centers, doc="the microstate centres (K, k); None until they are fitted")
    kmeans = property(lambda self: self._micro.kmeans, doc="the fitted MicrostateKMeans; None when the centres were given")

    def project(self, x):
        return binding.struct_tic(x, self.mean, self.coeff)

    def discretise(self, x):
        """(labels int32 (n,), order parameter (n,)) of frames already on the device; the first call fits the centres"""
        return self._micro.labels(self.project(x)), self._cv(x)

    @staticmethod
    def summarize(model, row, committor, folded_states, unfolded_states, frame_time=1.0, samples_nonfinite=0):
        """eval()'s dict from a fitted model, its (mfpt_ab, mfpt_ba, rate_ab, rate_ba) in frames with A the unfolded set, and its
        committor on the full index: numpy only."""
        q = committor[model.active_set]
        mid = (q > 0.4) & (q < 0.6)
        return {"mfpt_folding": float(row[0]) * frame_time, "mfpt_unfolding": float(row[1]) * frame_time,
                "rate_folding": float(row[2]) / frame_time, "rate_unfolding": float(row[3]) / frame_time,
                "n_folded_states": float(np.isin(model.active_set, folded_states).sum()),
                "n_unfolded_states": float(np.isin(model.active_set, unfolded_states).sum()),
                "committor_mid_share": float(model.stationary_distribution[mid].sum()) if np.isfinite(q).all() else float("nan"),
                "samples_nonfinite": float(samples_nonfinite)}

    def _analyse(self, x, lengths, name):
        labels, cv = self.discretise(x)
        if self.folded_states is None:
            low, high = states_by_cv(labels, cv, self.lo, self.hi, self.n_microstates)
            self.unfolded_states, self.folded_states = (low, high) if self.cv == "q" else (high, low)
        U, F = self.unfolded_states, self.folded_states
        solvable = U.size > 0 and F.size > 0                         # else no state reaches a core: nothing to solve or resample
        model, bs = self._point.fit(labels, lengths, self.n_microstates, name, bootstrap_passage if solvable else None, A=U, B=F)
        if not solvable:
            row, comm = np.full(4, np.nan), np.full(self.n_microstates, np.nan)
        elif bs is not None:
            self.bootstraps[name] = bs
            comm = bs.point["committor"]
            row = np.array([bs.point[f] for f in PassageBootstrap.FIELDS])
        else:
            rows, comms = _passage_batch([model], U, F, self.n_microstates, self.device)
            row, comm = rows[0], comms[0]
        self.models[name], self.labels[name], self.committors[name] = model, labels.cpu().numpy(), comm
        res = self.summarize(model, row, comm, F, U, self.frame_time, int((labels < 0).sum()))
        if bs is not None:
            iv, sd = bs.interval(self._point.confidence), bs.std()
            for key, field in self.BARS:
                scale = self.frame_time if key.startswith("mfpt") else 1.0 / self.frame_time
                res[key + "_lo"], res[key + "_hi"], res[key + "_std"] = iv[field][0] * scale, iv[field][1] * scale, sd[field] * scale
            res["bootstrap_failed"] = float(bs.n_failed)
        return res

    def _compare(self, res, ref):
        for which in ("folding", "unfolding"):
            res[f"log10_mfpt_ratio_{which}"] = _log10_ratio(res[f"mfpt_{which}"], ref[f"mfpt_{which}"])


# ---- propagation: row vectors through a model's transition matrix, step after step (dff_msm_propagate) ----
# What needs it: the Chapman-Kolmogorov test (does T(tau)^k predict what the model estimated at lag k tau shows?), the relaxation
# of an observable from a start distribution, and the model's autocorrelation function, which reads against autocorrelation()
# on the trajectories.  Vectors and observables are given on the FULL state index; states outside the active set are dropped.
PROPAGATE_MAX_BATCH = binding.MSM_PROPAGATE_MAX_BATCH
PROPAGATE_MAX_ROWS = binding.MSM_PROPAGATE_MAX_ROWS
PROPAGATE_MAX_STEPS = binding.MSM_PROPAGATE_MAX_STEPS
PROPAGATE_BYTES = 1 << 30        # matrices, vectors and outputs of one dff_msm_propagate call of propagator


class _DevicePropagator:
    """propagate(t (n_mat, Kmax, Kmax), mat_of (P,), ks (P,), w0 (P, M, Kmax), obs (P, R, Kmax), n_steps, want_last) -> (out
    (P, n_steps + 1, M, R), w_last (P, M, Kmax) | None, status (P,)), host arrays in and out: the problems go to the GPU in chunks
    that stay under PROPAGATE_BYTES, each chunk one dff_msm_propagate call on the matrices it uses."""

    def __init__(self, device):
        self.device = torch.device(device)

    def __call__(self, t, mat_of, ks, w0, obs, n_steps, want_last=False):
        w0, obs = np.ascontiguousarray(w0, np.float64), np.ascontiguousarray(obs, np.float64)
        P, M, Kmax = w0.shape
        R, S = obs.shape[1], int(n_steps)
        t = np.ascontiguousarray(t, np.float64).reshape(-1, Kmax, Kmax)
        mat_of, ks = np.asarray(mat_of, np.int64).reshape(-1), np.asarray(ks, np.int32).reshape(-1)
        per = 8 * (Kmax * Kmax + (2 * M + R) * Kmax + (S + 1) * M * R + 2)
        outputs = (np.full((P, S + 1, M, R), np.nan), np.full((P, M, Kmax), np.nan) if want_last else None, np.zeros(P, np.int32))

        def call(sl, up, t_dev, local):
            return binding.msm_propagate(t_dev, local, ks[sl], up(w0[sl]), up(obs[sl]), S, want_last=want_last)

        return _device_chunks(self.device, P, per, PROPAGATE_BYTES, PROPAGATE_MAX_BATCH, outputs, call, mats=t, mat_of=mat_of,
                              most=(1 << 28) // ((S + 1) * M * R))          # the call's cap on its output values


def propagator(device):
    """propagate(t (n_mat, Kmax, Kmax), mat_of (P,), ks (P,), w0 (P, M, Kmax), obs (P, R, Kmax), n_steps, want_last=False) ->
    (out (P, n_steps + 1, M, R), w_last | None, status (P,)) on the GPU (dff_msm_propagate): w_{s+1} = w_s T, out[p, s, m, r] =
    sum_j w_s[m][j] obs[r][j]; matrix m is a compact (K, K) matrix at the start of its slot."""
    return _DevicePropagator(device)


def _check_steps(n_steps, what):
    S = int(n_steps)
    if S != n_steps or not 0 <= S <= PROPAGATE_MAX_STEPS:
        raise ValueError(f"{what}: n_steps must be an integer in 0..{PROPAGATE_MAX_STEPS}")
    return S


def _state_rows(x, n_states, what, name):
    """x as finite float64 (rows, n_states), rows 1..PROPAGATE_MAX_ROWS"""
    a = np.array(x, np.float64, ndmin=2)
    if a.ndim != 2 or a.shape[1] != n_states or not 1 <= a.shape[0] <= PROPAGATE_MAX_ROWS:
        raise ValueError(f"{what}: {name} must be (1..{PROPAGATE_MAX_ROWS}, {n_states}) on the full state index")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: {name} must be finite")
    return a


def _propagate_on_models(models, mat_of, starts, observables, n_steps, device, what):
    """One propagator call: problem p runs on models[mat_of[p]] with the start rows starts[p] (M, n_active) and the observables
    observables[p] (R, n_active), both on the model's ACTIVE index -> out (P, n_steps + 1, M, R)."""
    P = len(mat_of)
    ks_m = [len(m.active_set) for m in models]
    Kmax = max(ks_m)
    t = np.zeros((len(models), Kmax * Kmax))
    for i, m in enumerate(models):
        m._need_fit()
        t[i, :ks_m[i] * ks_m[i]] = np.asarray(m.transition_matrix, np.float64).reshape(-1)
    M, R = starts[0].shape[0], observables[0].shape[0]
    w0, obs, ks = np.zeros((P, M, Kmax)), np.zeros((P, R, Kmax)), np.zeros(P, np.int32)
    for p in range(P):
        K = ks_m[mat_of[p]]
        w0[p, :, :K], obs[p, :, :K], ks[p] = starts[p], observables[p], K
    out, _, status = propagator(device if device is not None else models[0].device)(
        t.reshape(len(models), Kmax, Kmax), np.asarray(mat_of, np.int64), ks, w0, obs, n_steps)
    if (status != 0).any():
        bad = int(np.flatnonzero(status)[0])
        raise ValueError(f"{what}: problem {bad} failed (status {int(status[bad])}): a non-finite entry in its transition matrix, "
                         "or an overflow on the way")
    return out


def msm_propagate(models, start, observables, n_steps, *, device=None):
    """Distributions through the transition matrices of one fitted MarkovStateModel or a list of them, in ONE
    dff_msm_propagate call (active sets of differing size share it; reversible or not): `start` (M, n_states) row vectors and
    `observables` (R, n_states), both on the full state index, M, R <= 16; a model's inactive states are dropped from both
    -> float64 (P, n_steps + 1, M, R), out[p, s, m, r] = sum_j (start_m T_p^s)_j observable_r,j over model p's active set."""
    ms = [models] if isinstance(models, MarkovStateModel) else list(models)
    if not ms:
        raise ValueError("msm_propagate: no model")
    S = _check_steps(n_steps, "msm_propagate")
    for m in ms:
        m._need_fit()
    n = len(ms[0].count_matrix)
    if any(len(m.count_matrix) != n for m in ms):
        raise ValueError("msm_propagate: the models must share one state index")
    w, o = _state_rows(start, n, "msm_propagate", "start"), _state_rows(observables, n, "msm_propagate", "observables")
    return _propagate_on_models(ms, list(range(len(ms))), [w[:, m.active_set] for m in ms], [o[:, m.active_set] for m in ms], S,
                                device, "msm_propagate")


def msm_relaxation(model, p0, a, n_steps, *, device=None):
    """E[a] after s = 0 .. n_steps lag times when the model starts from the distribution p0 (n_states,): sum_j (p0 T^s)_j a_j ->
    float64 (n_steps + 1,), or (n_steps + 1, d) for a of shape (d, n_states), d <= 16.  p0 is used as given (restricted to the
    active set, not renormalised)."""
    a = np.asarray(a, np.float64)
    out = msm_propagate(model, np.asarray(p0, np.float64).reshape(1, -1), a, n_steps, device=device)[0, :, 0, :]
    return out[:, 0] if a.ndim == 1 else out


class MsmAutocorrelation:
    """What msm_autocorrelation returns: lags (n_steps + 1,) in frames (s lagtime), cov and acf (n_steps + 1,) -- or
    (n_steps + 1, d) for d observables --, mean (the stationary mean of each observable)."""

    def __init__(self, lags, cov, acf, mean):
        self.lags, self.cov, self.acf, self.mean = lags, cov, acf, mean


def msm_autocorrelation(model, a, n_steps, *, device=None):
    """The autocorrelation function the model predicts for the state function a (n_states,) or (d, n_states), d <= 16, at the
    lags s lagtime, s = 0 .. n_steps: C(s) = sum_i pi_i a~_i (T^s a~)_i with a~ = a - sum_i pi_i a_i, acf = C(s) / C(0) ->
    MsmAutocorrelation.  The start rows are pi a~, the observables a~ (one dff_msm_propagate call).  acf[s] reads against
    autocorrelation(series, ...).acf[s * lagtime] of the series a[labels]."""
    model._need_fit()
    S = _check_steps(n_steps, "msm_autocorrelation")
    a = np.asarray(a, np.float64)
    rows = _state_rows(a, len(model.count_matrix), "msm_autocorrelation", "a")[:, model.active_set]
    pi = model.stationary_distribution
    mean = rows @ pi
    at = rows - mean[:, None]
    out = _propagate_on_models([model], [0], [at * pi], [at], S, device, "msm_autocorrelation")[0]
    cov = np.stack([out[:, i, i] for i in range(len(rows))], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        acf = cov / cov[:1]
    lags = np.arange(S + 1, dtype=np.int64) * model.lagtime
    if a.ndim == 1:
        return MsmAutocorrelation(lags, cov[:, 0], acf[:, 0], float(mean[0]))
    return MsmAutocorrelation(lags, cov, acf, mean)


# ---- metastable sets: the inner-simplex step of PCCA+ (Weber & Galliat) on the model's right eigenvectors ----
def inner_simplex(psi):
    """The rows of psi (n, m) that span the largest simplex, greedily: the row of largest norm; the rows shifted by it; m - 1
    times the row of largest norm, projected out of all rows -> (m,) row indices.  The lowest index wins a tie."""
    v = np.array(psi, np.float64)
    n, m = v.shape
    idx = np.zeros(m, np.int64)
    idx[0] = int(np.argmax((v * v).sum(axis=1)))
    v = v - v[idx[0]]
    for j in range(1, m):
        nrm = np.sqrt((v * v).sum(axis=1))
        idx[j] = int(np.argmax(nrm))
        if not nrm[idx[j]] > 0:
            raise ValueError("inner_simplex: the rows span fewer than m - 1 dimensions")
        u = v[idx[j]] / nrm[idx[j]]
        v = v - np.outer(v @ u, u)
    return idx


def pcca_memberships(model, m):
    """chi (n_active, m): the memberships of the active states in m metastable sets from the inner-simplex start of PCCA+, chi =
    psi psi[vertices]^-1 on the m leading right eigenvectors psi (model.eigenvectors(m - 1): the GPU call of msm_spectrum;
    reversible models).  Rows sum to 1; a vertex state has membership 1 in its own set.  The optimisation of the transformation
    matrix that PCCA+ runs after this start is not done: entries may lie slightly outside [0, 1]."""
    model._need_fit()
    m = int(m)
    n = len(model.active_set)
    if not 1 <= m <= min(n, PROPAGATE_MAX_ROWS):
        raise ValueError(f"pcca_memberships: m must be 1..min(n_active, {PROPAGATE_MAX_ROWS}) = {min(n, PROPAGATE_MAX_ROWS)}, not {m}")
    if m == 1:
        return np.ones((n, 1))
    psi = np.asarray(model.eigenvectors(m - 1)).T
    return psi @ np.linalg.inv(psi[inner_simplex(psi)])


def metastable_sets(model, m):
    """m metastable sets of a fitted reversible MarkovStateModel: every active state goes to the set of its largest
    pcca_memberships entry (the lowest index wins a tie) -> a list of m int64 arrays of state indices on the FULL index, ordered
    by their smallest state.  ValueError when a set stays empty."""
    chi = pcca_memberships(model, m)
    of = np.argmax(chi, axis=1)
    sets = [np.asarray(model.active_set, np.int64)[of == c] for c in range(chi.shape[1])]
    if any(s.size == 0 for s in sets):
        raise ValueError(f"metastable_sets: only {sum(s.size > 0 for s in sets)} of {chi.shape[1]} sets have a state")
    return sorted(sets, key=lambda s: int(s[0]))


# ---- the Chapman-Kolmogorov test ----
class ChapmanKolmogorov:
    """What chapman_kolmogorov returns.  lagtimes (n_k,) = lagtime * multiples, in frames; predicted and estimated (n_k, m, m):
    the probability of being in set b after k lag times when started from the stationary distribution restricted to set a, by
    T(tau)^k and by one step of the model at lag k tau (NaN rows where a set has no active state); max_abs_diff and rms_diff
    over the finite entries; models: {multiple: MarkovStateModel} (1: the base model); sets.  With n_resamples > 0 also
    predicted_lo / _hi, estimated_lo / _hi (the percentile interval at `confidence` over the resamples), share_inside (the share
    of finite entries whose point prediction lies inside the estimate's interval) and predicted_resamples /
    estimated_resamples (B, n_k, m, m); else those are None."""

    def __init__(self, lagtimes, multiples, sets, predicted, estimated, models):
        self.lagtimes, self.multiples, self.sets, self.predicted, self.estimated, self.models = (lagtimes, multiples, sets, predicted,
                                                                                                 estimated, models)
        d = (predicted - estimated)[np.isfinite(predicted) & np.isfinite(estimated)]
        self.max_abs_diff = float(np.abs(d).max()) if d.size else float("nan")
        self.rms_diff = float(np.sqrt(np.mean(d * d))) if d.size else float("nan")
        self.predicted_lo = self.predicted_hi = self.estimated_lo = self.estimated_hi = None
        self.predicted_resamples = self.estimated_resamples = None
        self.share_inside = float("nan")


def _check_sets(sets, n_states, what):
    """m <= 16 disjoint, non-empty lists of states of the full index -> a list of sorted int64 arrays"""
    out = [np.unique(np.asarray(s, np.int64).reshape(-1)) for s in sets]
    if not 1 <= len(out) <= PROPAGATE_MAX_ROWS:
        raise ValueError(f"{what}: 1..{PROPAGATE_MAX_ROWS} sets, not {len(out)}")
    for a, s in enumerate(out):
        if s.size == 0:
            raise ValueError(f"{what}: set {a} is empty")
        if s[0] < 0 or s[-1] >= n_states:
            raise ValueError(f"{what}: set {a} holds a state outside 0 .. {n_states - 1}")
    allst = np.concatenate(out)
    if np.unique(allst).size != allst.size:
        raise ValueError(f"{what}: the sets overlap")
    return out


def _ck_rows(model, sets):
    """(start rows (m, n_active): pi restricted to each set and divided by its sum, zero where the set has no active state;
    indicators (m, n_active) of the sets; empty (m,) bool)"""
    act, pi = np.asarray(model.active_set), model.stationary_distribution
    ind = np.stack([np.isin(act, s).astype(np.float64) for s in sets])
    w = ind * pi
    tot = w.sum(axis=1)
    empty = ind.sum(axis=1) == 0
    w[~empty] /= tot[~empty][:, None]
    return w, ind, empty


def chapman_kolmogorov_of_models(groups, multiples, sets, *, device=None):
    """The tables of the test for fitted models: groups is a list of (base model at lag tau, {k: model at lag k tau}) -- one
    entry per data set or resample --, every one evaluated by the definitions of ChapmanKolmogorov in ONE propagator call: the
    base model runs max(multiples) steps, each other model one -> (predicted, estimated), each (len(groups), n_k, m, m).  The
    model of multiple 1 is the base model itself: both rows are then the same problem on the same matrix."""
    multiples = [int(k) for k in multiples]
    S, m = max(multiples), len(sets)
    models, mat_of, starts, obs, where = [], [], [], [], []
    for base, tests in groups:
        for mdl in [base] + [tests[k] for k in multiples]:
            at = next((i for i, x in enumerate(models) if x is mdl), None)
            if at is None:
                at = len(models)
                models.append(mdl)
            w, ind, empty = _ck_rows(mdl, sets)
            mat_of.append(at)
            starts.append(w)
            obs.append(ind)
            where.append(empty)
    out = _propagate_on_models(models, mat_of, starts, obs, S, device, "chapman_kolmogorov")
    n_k = len(multiples)
    pred, est = np.full((len(groups), n_k, m, m), np.nan), np.full((len(groups), n_k, m, m), np.nan)
    for g in range(len(groups)):
        p0 = g * (n_k + 1)
        for i, k in enumerate(multiples):
            pred[g, i], est[g, i] = out[p0, k], out[p0 + 1 + i, 1]
            pred[g, i][where[p0]] = np.nan
            est[g, i][where[p0 + 1 + i]] = np.nan
    return pred, est


def chapman_kolmogorov(labels, lagtime, sets, multiples=(1, 2, 3, 4, 5), traj_lengths=None, n_states=None, *, reversible=True,
                       n_resamples=0, block_frames=None, seed=0, confidence=0.95, tol=1e-12, max_iter=1_000_000,
                       steps_per_sync=256, resample_batch=None, device="cuda:0"):
    """The Chapman-Kolmogorov test of a MarkovStateModel at `lagtime` on the sets `sets` (m <= 16 disjoint, non-empty lists of
    states on the full index): for every multiple k, predicted[k][a][b] = sum over set b of (pi restricted to set a, normalised)
    T(tau)^k, and estimated[k][a][b] the same with ONE step of the model estimated at lag k tau, with that model's own pi and
    active set -> ChapmanKolmogorov.  The count matrices of up to 8 lag times come from one pass over the labels; every
    propagation of the test is in one dff_msm_propagate call.  n_resamples > 0 (reversible models): the bootstrap of
    bootstrap_msm at every lag with the same seed, so that resample b draws the same units at every lag; all resamples of a
    batch in one call; resample b equals chapman_kolmogorov_of_models on the models of fit_counts(counts_b) bit for bit."""
    dev = torch.device(device)
    lab = torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    lengths = _check_lengths(traj_lengths, int(lab.numel()))
    if n_states is None:
        n_states = int(lab.max()) + 1 if lab.numel() else 0
    if not 1 <= int(n_states) <= MSM_MAX_STATES:
        raise ValueError(f"chapman_kolmogorov: n_states must be 1..{MSM_MAX_STATES}, not {n_states}")
    sets = _check_sets(sets, int(n_states), "chapman_kolmogorov")
    mult = [int(k) for k in multiples]
    if not mult or any(k != kk or k < 1 or k > PROPAGATE_MAX_STEPS for k, kk in zip(mult, multiples)) or len(set(mult)) != len(mult):
        raise ValueError("chapman_kolmogorov: multiples must be distinct integers >= 1")
    n_resamples = int(n_resamples)
    if n_resamples < 0:
        raise ValueError("chapman_kolmogorov: n_resamples must be >= 0")
    if n_resamples and not reversible:
        raise ValueError("chapman_kolmogorov: the bootstrap needs reversible models")
    proto = MarkovStateModel(lagtime, reversible, tol, max_iter, steps_per_sync, device=dev)          # checks the settings
    ks_all = sorted(set(mult) | {1})
    models = {}
    for l0 in range(0, len(ks_all), binding.MSM_MAX_LAGS):
        group = ks_all[l0:l0 + binding.MSM_MAX_LAGS]
        counts = binding.micro_transition_counts(lab, lengths, [proto.lagtime * k for k in group], int(n_states)).cpu().numpy()
        for i, k in enumerate(group):
            models[k] = MarkovStateModel(proto.lagtime * k, reversible, tol, max_iter, steps_per_sync, device=dev).fit_counts(counts[i])
    pred, est = chapman_kolmogorov_of_models([(models[1], models)], mult, sets, device=dev)
    ck = ChapmanKolmogorov(np.array([proto.lagtime * k for k in mult], np.int64), mult, sets, pred[0], est[0], models)
    if n_resamples:
        plans = {k: _BootstrapPlan("chapman_kolmogorov", lab, proto.lagtime * k, lengths, n_states, n_resamples, block_frames, seed,
                                   None, tol, max_iter, steps_per_sync, resample_batch, dev) for k in ks_all}
        B = plans[1].B
        shape = (B,) + pred[0].shape
        pr, es = np.full(shape, np.nan), np.full(shape, np.nan)
        for batch in zip(*(plans[k].batches() for k in ks_all)):
            b0, n = batch[0][0], len(batch[0][1])
            groups = [(batch[0][1][i], {k: batch[j][1][i] for j, k in enumerate(ks_all)}) for i in range(n)]
            pr[b0:b0 + n], es[b0:b0 + n] = chapman_kolmogorov_of_models(groups, mult, sets, device=dev)
        ck.predicted_resamples, ck.estimated_resamples = pr, es
        flat = lambda v: v.reshape(B, -1)     # noqa: E731
        ck.predicted_lo, ck.predicted_hi = (v.reshape(pred[0].shape) for v in percentile_interval(flat(pr), confidence))
        ck.estimated_lo, ck.estimated_hi = (v.reshape(pred[0].shape) for v in percentile_interval(flat(es), confidence))
        ck.share_inside = share_inside(ck.predicted, ck.estimated_lo, ck.estimated_hi)
    return ck


def share_inside(point, lo, hi):
    """the share of the entries where point, lo and hi are all finite with lo <= point <= hi (NaN when there is none)"""
    ok = np.isfinite(point) & np.isfinite(lo) & np.isfinite(hi)
    return float(np.mean((point[ok] >= lo[ok]) & (point[ok] <= hi[ok]))) if ok.any() else float("nan")


def state_means(labels, values, n_states):
    """The mean of `values` (n,) over the frames of every state of `labels` (n,; < 0: left out) -> float64 (n_states,), 0 for a
    state without frames; taken with torch on the device the values live on (non-finite values are left out)."""
    v = torch.as_tensor(values).reshape(-1).to(torch.float64)
    lab = torch.as_tensor(labels).reshape(-1).to(device=v.device, dtype=torch.int64)
    ok = (lab >= 0) & (lab < n_states) & torch.isfinite(v)
    sums = torch.zeros(n_states, dtype=torch.float64, device=v.device).index_add_(0, lab[ok], v[ok])
    cnt = torch.zeros(n_states, dtype=torch.float64, device=v.device).index_add_(0, lab[ok], torch.ones_like(v[ok]))
    return (sums / cnt.clamp(min=1)).cpu().numpy()


class ChapmanKolmogorovEvaluator(_TrajectoryEvaluator):
    """Is the Markov state model of the sampled dynamics VALID at its lag time?  Frames -> TIC projection and k-means
    microstates (`tica`, n_microstates, centers, seed: as for MsmEvaluator) -> a reversible MarkovStateModel at `lagtime` -> n_sets
    metastable sets (metastable_sets of the first ensemble analysed: the reference when there is ref_data; kept and reused for
    the samples) -> chapman_kolmogorov at `multiples`, and the model's autocorrelation of the first TIC (msm_autocorrelation of
    its state means) against the one measured on the trajectories (autocorrelation).

    eval(xyz, traj_lengths=None) -- None: ONE trajectory -- returns a dict:
      ck_max_abs_diff, ck_rms_diff                    predicted against estimated over all multiples and pairs of sets
      ck_diagonal_predicted, ck_diagonal_estimated    lists over the multiples of lists over the sets: the staying probabilities
      acf_rms_diff                                    model against measured ACF of the first TIC at the lags s lagtime, s = 0 .. max(multiples)
      n_sets, samples_nonfinite
    and with n_bootstrap > 0 ck_share_inside (the share of point predictions inside the estimates' percentile interval).  With
    ref_data the same keys with the suffix _ref and ck_max_abs_diff_minus_ref.  The results stay on .results, the models on
    .models, under "samples" / "refs".  Without the HIP library: DffLibraryError."""

    KEYS = ("ck_max_abs_diff", "ck_rms_diff", "ck_diagonal_predicted", "ck_diagonal_estimated", "acf_rms_diff", "n_sets",
            "samples_nonfinite")

    def __init__(self, mol_name, tica, n_microstates=200, lagtime=None, n_sets=3, multiples=(1, 2, 3, 4, 5), frame_time=1.0,
                 ref_data=None, ref_traj_lengths=None, centers=None, seed=0, *, n_bootstrap=0, block_frames=None, confidence=0.95,
                 bootstrap_seed=0, device="cuda:0"):
        what = "ChapmanKolmogorovEvaluator"
        super().__init__(what, mol_name, frame_time, device)
        self._point = _PointModel(what, lagtime, n_bootstrap, block_frames, confidence, bootstrap_seed, self.device)
        self.lagtime = self._point.lagtime
        self.n_sets = int(n_sets)
        if not 1 <= self.n_sets <= PROPAGATE_MAX_ROWS:
            raise ValueError(f"{what}: n_sets must be 1..{PROPAGATE_MAX_ROWS}")
        self.multiples = [int(k) for k in multiples]
        if not self.multiples or any(k < 1 for k in self.multiples) or len(set(self.multiples)) != len(self.multiples):
            raise ValueError(f"{what}: multiples must be distinct integers >= 1")
        self.mean, self.coeff = _tica_model(tica, what, TICA_MAX_DIM)
        self._micro = _Microstates(what, n_microstates, self.coeff.shape[1], centers, seed, self.device)
        self.n_microstates = self._micro.n_microstates
        self.sets = None
        self.models, self.labels, self.results = {}, {}, {}
        self._start(ref_data, ref_traj_lengths)

    centers = property(lambda self: self._micro.centers, doc="the microstate centres (K, k); None until they are fitted")

    def project(self, x):
        return binding.struct_tic(x, self.mean, self.coeff)

    @staticmethod
    def summarize(ck, acf_model, acf_measured, samples_nonfinite=0):
        """eval()'s dict from a ChapmanKolmogorov and the two ACFs at the same lags: numpy only."""
        d = np.asarray(acf_model, np.float64) - np.asarray(acf_measured, np.float64)
        d = d[np.isfinite(d)]
        res = {"ck_max_abs_diff": ck.max_abs_diff, "ck_rms_diff": ck.rms_diff,
               "ck_diagonal_predicted": [[float(v) for v in np.diag(t)] for t in ck.predicted],
               "ck_diagonal_estimated": [[float(v) for v in np.diag(t)] for t in ck.estimated],
               "acf_rms_diff": float(np.sqrt(np.mean(d * d))) if d.size else float("nan"),
               "n_sets": float(len(ck.sets)), "samples_nonfinite": float(samples_nonfinite)}
        if ck.estimated_lo is not None:
            res["ck_share_inside"] = ck.share_inside
        return res

    def _analyse(self, x, lengths, name):
        proj = self.project(x)
        labels = self._micro.labels(proj)
        if self.sets is None:
            first, _ = self._point.fit(labels, lengths, self.n_microstates, name)
            self.sets = metastable_sets(first, self.n_sets)
        seed = self._point.bootstrap_seed + (name == "refs")
        ck = chapman_kolmogorov(labels, self.lagtime, self.sets, self.multiples, lengths, self.n_microstates,
                                n_resamples=self._point.n_bootstrap, block_frames=self._point.block_frames, seed=seed,
                                confidence=self._point.confidence, device=self.device)
        model, S = ck.models[1], max(self.multiples)
        tic1 = proj[:, 0]
        predicted = msm_autocorrelation(model, state_means(labels, tic1, self.n_microstates), S, device=self.device).acf
        measured = autocorrelation(tic1, S * self.lagtime, lengths, device=self.device).acf[::self.lagtime, 0]
        self.models[name], self.labels[name], self.results[name] = model, labels.cpu().numpy(), ck
        return self.summarize(ck, predicted, measured, int((labels < 0).sum()))

    def _compare(self, res, ref):
        res["ck_max_abs_diff_minus_ref"] = res["ck_max_abs_diff"] - ref["ck_max_abs_diff"]


# ---- hidden Markov models on the microstate trajectory: Baum-Welch with the E-step on the GPU (dff_hmm_estep) ----
HMM_MAX_HIDDEN = binding.HMM_MAX_HIDDEN


class _DeviceHmm:
    """What the three device solvers share: the device, a workspace that is kept between calls and only grows, and the upload
    of a model's three host arrays as float64 tensors."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._ws = None

    def _workspace(self, need):
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        return self._ws

    def _upload(self, *arrays):
        return [torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(self.device) for x in arrays]


class _DeviceHmmEstep(_DeviceHmm):
    """estep(labels (n,) int32 tensor on the device, lengths, lag, A (m, m), B (m, K), p0 (m,), want_post=False) -> (stats
    float64 host array, packed as dff_hmm_estep packs it, chain_loglik host array | None, post (n, m) float64 DEVICE tensor |
    None, status int): one dff_hmm_estep call and one read-back of the packed statistics (the status is read only when they are
    NaN).  The workspace is kept between calls."""

    def __call__(self, labels, lengths, lag, A, B, p0, want_post=False):
        par = self._upload(A, B, p0)
        ws = self._workspace(binding.hmm_workspace_bytes(int(labels.numel()), lengths, lag, par[1].shape[0], par[1].shape[1]))
        res = binding.hmm_estep(labels, lengths, lag, *par, chain_loglik=want_post, post=want_post, workspace=ws)
        stats = res["stats"].cpu().numpy()
        status = int(res["status"].cpu()) if np.isnan(stats[0]) else 0
        return stats, (res["chain_loglik"].cpu().numpy() if want_post else None), res["post"], status


def hmm_estep_solver(device):
    """estep(labels, lengths, lag, A, B, p0, want_post=False) -> (stats, chain_loglik | None, post | None, status) on the GPU
    (dff_hmm_estep): stats = loglik | xi (m, m) | gamma0 (m) | gamma_sym (m, K) as one host array, post the (n, m) posteriors
    as a tensor on the device."""
    return _DeviceHmmEstep(device)


class _DeviceHmmViterbi(_DeviceHmm):
    """viterbi(labels (n,) int32 tensor on the device, lengths, lag, la (m, m), lb (m, K), lp (m,), chain_order=False) -> (path
    int32 (n,) DEVICE tensor, chain_logprob host array (n_traj lag,), status int): one dff_hmm_viterbi call on LOG-parameters and
    one read-back of the log-probabilities and the status.  The workspace is kept between calls."""

    def __call__(self, labels, lengths, lag, la, lb, lp, chain_order=False):
        par = self._upload(la, lb, lp)
        ws = self._workspace(binding.hmm_viterbi_workspace_bytes(int(labels.numel()), lengths, lag, par[1].shape[0], par[1].shape[1]))
        res = binding.hmm_viterbi(labels, lengths, lag, *par, chain_order=chain_order, chain_logprob=True, workspace=ws)
        return res["path"], res["chain_logprob"].cpu().numpy(), int(res["status"].cpu())


def hmm_viterbi_solver(device):
    """viterbi(labels, lengths, lag, la, lb, lp, chain_order=False) -> (path, chain_logprob, status) on the GPU (dff_hmm_viterbi):
    la, lb, lp the LOGARITHMS of A, B, p0; path int32 (n,) as a tensor on the device, in frame order or (chain_order=True) with
    the chains back to back; chain_logprob a host array.  The seam for host tests, like hmm_estep_solver."""
    return _DeviceHmmViterbi(device)


class _DeviceHmmFit(_DeviceHmm):
    """steps(...) of hmm_fit_solver on the GPU.  One float64 buffer holds A | B | p0 | pi | the state's 32 bytes | the
    log-likelihoods, so a call reads back once; it, the workspace and with them the parameters and the state of the fit stay
    on the device between the calls of one fit."""

    def __init__(self, device):
        super().__init__(device)
        self._buf = self._shape = None

    def _views(self, m, K, n_steps):
        o = [int(v) for v in np.cumsum([0, m * m, m * K, m, m, 4])]
        if self._shape != (m, K) or self._buf is None or self._buf.numel() < o[-1] + n_steps:
            old = self._buf if self._shape == (m, K) else None
            self._buf = torch.full((int(o[-1]) + max(n_steps, 32),), float("nan"), dtype=torch.float64, device=self.device)
            if old is not None:
                self._buf[:o[-1]] = old[:o[-1]]
            self._shape = (m, K)
        b = self._buf
        return (b[o[0]:o[1]].view(m, m), b[o[1]:o[2]].view(m, K), b[o[2]:o[3]], b[o[3]:o[4]], b[o[4]:o[5]].view(torch.int32),
                b[o[5]:o[5] + n_steps], o)

    def steps(self, labels, lengths, lag, A, B, p0, reversible, n_steps, accuracy, state=None, *, rev_tol=1e-12,
              rev_max_sweeps=1_000_000):
        m, K = np.shape(B)
        n_steps = int(n_steps)
        if state is not None and self._shape != (m, K):
            raise ValueError("hmm_fit_solver: a state to continue from, but this solver holds no fit of that shape")
        tA, tB, tp, tpi, tst, tll, o = self._views(m, K, n_steps)
        if state is None:                                            # a new fit: the parameters go up, the state is zeroed
            host = np.concatenate([np.ravel(np.asarray(x, np.float64)) for x in (A, B, p0)] + [np.full(m, np.nan), np.zeros(4)])
            self._buf[:o[5]] = torch.from_numpy(host).to(self.device)
        ws = self._workspace(binding.hmm_fit_workspace_bytes(int(labels.numel()), lengths, lag, m, K))
        binding.hmm_fit_steps(labels, lengths, lag, tA, tB, tp, reversible, n_steps, accuracy, rev_tol, rev_max_sweeps, state=tst,
                              loglik=tll, stationary=tpi, workspace=ws)
        h = self._buf[:o[5] + n_steps].cpu().numpy()                 # the one read-back
        pi = h[o[3]:o[4]].copy()
        return (h[o[0]:o[1]].reshape(m, m).copy(), h[o[1]:o[2]].reshape(m, K).copy(), h[o[2]:o[3]].copy(), h[o[5]:].copy(),
                None if np.isnan(pi).any() else pi, binding.hmm_fit_state_dict(h[o[4]:o[5]].view(np.int32)))


def hmm_fit_solver(device):
    """An object whose steps(labels, lengths, lag, A, B, p0, reversible, n_steps, accuracy, state=None, *, rev_tol=1e-12,
    rev_max_sweeps=1_000_000) runs n_steps iterations of Baum-Welch on the GPU (dff_hmm_fit_steps) and reads back once ->
    (A, B, p0 host arrays, loglik (n_steps,) with NaN for the steps of a stopped fit, pi (m,) of the last reversible M-step |
    None before one, the state as a dict of dff_hmm_fit_state's fields).  state=None starts a fit from A, B, p0; the state
    the last call returned continues it FROM THE PARAMETERS ON THE DEVICE (those that call returned; A, B, p0 are then not
    read).  The seam for host tests, like hmm_estep_solver."""
    return _DeviceHmmFit(device)


def hmm_chain_lengths(traj_lengths, lag):
    """The lengths of the chains of trajectories of `traj_lengths` at `lag`, in chain order (r-major, f-minor; empty chains
    included): chain (r, f) holds the frames f, f + lag, ... of trajectory r.  They are the trajectory lengths that label_runs
    takes with a path in chain order."""
    lag = int(lag)
    if lag < 1:
        raise ValueError("hmm_chain_lengths: lag must be an integer >= 1")
    out = []
    for n in traj_lengths:
        q, rem = divmod(int(n), lag)
        out.extend([q + 1] * rem + [q] * (lag - rem))
    return np.array(out, np.int64)


def _row_normalised(x):
    s = x.sum(axis=1)[:, None]
    return x / np.where(s > 0, s, 1.0)


def _hmm_labels(labels, traj_lengths, n_states, device, what):
    lab = torch.as_tensor(labels).reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    lengths = _check_lengths(traj_lengths, int(lab.numel()))
    if n_states is None:
        n_states = int(lab.max()) + 1 if lab.numel() else 0
    if not 1 <= int(n_states) <= MSM_MAX_STATES:
        raise ValueError(f"{what}: n_states must be 1..{MSM_MAX_STATES}, not {n_states}")
    return lab, lengths, int(n_states)


def initial_hmm(labels, lagtime, n_hidden, traj_lengths=None, n_states=None, *, device="cuda:0"):
    """The start of Baum-Welch from a Markov state model -> (A (m, m), B (m, K), p0 (m,)), m = n_hidden, K = n_states.  A
    reversible MarkovStateModel is fitted at `lagtime`; M = pcca_memberships(model, m), clipped at 0 and row-normalised;
    A = row-normalised M^T Pi T M (non-negative, with a symmetric flux), p0 ~ M^T pi, B[i, s] ~ f_s M~[s, i], row-normalised, with
    f_s the empirical frequency of symbol s and M~ the membership for symbols of the active set and 1 / m for observed symbols
    outside it: no observed symbol is impossible.  ValueError when the active set has fewer than m states."""
    m = int(n_hidden)
    if m != n_hidden or not 1 <= m <= HMM_MAX_HIDDEN:
        raise ValueError(f"initial_hmm: n_hidden must be an integer in 1..{HMM_MAX_HIDDEN}")
    lab, lengths, K = _hmm_labels(labels, traj_lengths, n_states, torch.device(device), "initial_hmm")
    model = MarkovStateModel(lagtime, device=device).fit(lab, lengths, K)
    act = np.asarray(model.active_set, np.int64)
    if len(act) < m:
        raise ValueError(f"initial_hmm: the active set has {len(act)} states, fewer than n_hidden = {m}")
    M = _row_normalised(np.clip(pcca_memberships(model, m), 0.0, None))
    pi, T = model.stationary_distribution, model.transition_matrix
    A = _row_normalised(M.T @ (pi[:, None] * T) @ M)
    p0 = M.T @ pi
    ok = lab[(lab >= 0) & (lab < K)].to(torch.int64)
    f = torch.bincount(ok, minlength=K).cpu().numpy().astype(np.float64)
    Mt = np.full((K, m), 1.0 / m)
    Mt[act] = M
    B = _row_normalised((f[:, None] * Mt).T)
    return A, B, p0 / p0.sum()


class HiddenMarkovModel:
    """A discrete hidden Markov model over a microstate trajectory at one lag time, by Baum-Welch: the E-step is one
    dff_hmm_estep call and one packed read-back per iteration (hmm_estep_solver), the M-step runs on the host.  The defaults
    (reversible=True, accuracy=1e-3, max_iter=1000) are those of deeptime's MaximumLikelihoodHMM as remembered; nothing here
    is held to deeptime.

    fit(labels, traj_lengths=None, n_states=None, initial=None): labels (n,), negative = a missing observation; at lag tau the
    tau strided sub-sequences of every trajectory are the chains.  initial: (A, B, p0), default initial_hmm(...).  M-step:
    B = row-normalised Gamma, p0 = gamma0 / sum, A = row-normalised Xi, or with reversible=True the transition matrix of
    MarkovStateModel(lagtime).fit_counts(Xi); when its active set is not all hidden states the fit stops with converged =
    False and a .message.  A hidden state with zero expected occupancy keeps its previous row and sets degenerate = True.  The
    loop stops when the log-likelihood changes by less than `accuracy` (converged = True; the parameters are those the last
    log-likelihood was computed with) or after max_iter E-steps.  Afterwards the hidden states are renumbered by decreasing
    stationary probability, the lower index winning a tie (fit(..., renumber=False) keeps them in the order of `initial`).

    m_step="host" is the above.  m_step="device": the whole loop runs on the GPU (dff_hmm_fit_steps through hmm_fit_solver), in
    calls of min(steps_per_sync, max_iter - n_iter) iterations with ONE read-back each; the M-step is the call's fixed-order
    statement, its reversible estimator swept to rev_tol or rev_max_sweeps sweeps.  The same attributes and messages, equal to
    the host path's up to the rounding of the two M-steps; log_likelihoods are the finite entries the calls returned, and
    rev_sweeps (the estimator's sweeps, all M-steps together) and rev_unconverged (an M-step spent rev_max_sweeps) are set.

    transition_matrix (m, m), observation_probabilities (m, K), initial_distribution (m,), stationary_distribution (m,),
    log_likelihoods (one per E-step), n_iter, converged, degenerate, message."""

    M_STEPS = ("host", "device")
    MESSAGES = {1: "a parameter became non-finite or negative", 2: "a chain has likelihood zero under the model", 3: "a label >= n_states"}
    LOST = "the reversible estimator's active set lost a hidden state"

    def __init__(self, n_hidden, lagtime, reversible=True, accuracy=1e-3, max_iter=1000, *, device="cuda:0", m_step="host",
                 steps_per_sync=32, rev_tol=1e-12, rev_max_sweeps=1_000_000):
        self.n_hidden, self.lagtime = int(n_hidden), int(lagtime)
        if self.n_hidden != n_hidden or not 1 <= self.n_hidden <= HMM_MAX_HIDDEN:
            raise ValueError(f"HiddenMarkovModel: n_hidden must be an integer in 1..{HMM_MAX_HIDDEN}")
        if self.lagtime != lagtime or self.lagtime < 1:
            raise ValueError("HiddenMarkovModel: lagtime must be an integer >= 1")
        self.reversible, self.accuracy, self.max_iter = bool(reversible), float(accuracy), int(max_iter)
        if not self.accuracy > 0 or self.max_iter < 1:
            raise ValueError("HiddenMarkovModel: accuracy must be > 0 and max_iter >= 1")
        if m_step not in self.M_STEPS:
            raise ValueError('HiddenMarkovModel: m_step must be "host" or "device"')
        self.m_step, self.steps_per_sync = m_step, int(steps_per_sync)
        self.rev_tol, self.rev_max_sweeps = float(rev_tol), int(rev_max_sweeps)
        if self.steps_per_sync != steps_per_sync or self.steps_per_sync < 1 or not self.rev_tol > 0 or self.rev_max_sweeps < 1:
            raise ValueError("HiddenMarkovModel: steps_per_sync and rev_max_sweeps must be integers >= 1 and rev_tol > 0")
        self.device = torch.device(device)
        self.transition_matrix = self.observation_probabilities = self.initial_distribution = None
        self.stationary_distribution = None
        self.log_likelihoods, self.n_iter, self.converged, self.degenerate, self.message = [], 0, False, False, ""
        self.rev_sweeps, self.rev_unconverged = 0, False
        self._estep = None

    def _check_parameters(self, A, B, p0, K):
        A, B, p0 = (np.array(x, np.float64) for x in (A, B, p0))
        m = self.n_hidden
        if A.shape != (m, m) or B.shape != (m, K) or p0.shape != (m,):
            raise ValueError(f"HiddenMarkovModel: initial must be (A ({m}, {m}), B ({m}, {K}), p0 ({m},))")
        if not all(np.isfinite(x).all() and (x >= 0).all() for x in (A, B, p0)):
            raise ValueError("HiddenMarkovModel: initial parameters must be finite and non-negative")
        return A, B, p0

    def _m_step(self, A, B, p0, stats):
        """the next (A, B, p0, pi | None) from the packed statistics, or None when the reversible estimator lost a state"""
        m, K = B.shape
        xi = stats[1:1 + m * m].reshape(m, m)
        g0 = stats[1 + m * m:1 + m * m + m]
        gs = stats[1 + m * m + m:].reshape(m, K)
        occ = gs.sum(axis=1)
        if (occ <= 0).any():
            self.degenerate = True
        Bn = np.where(occ[:, None] > 0, gs / np.where(occ > 0, occ, 1.0)[:, None], B)
        pn = g0 / g0.sum() if g0.sum() > 0 else p0
        if self.reversible:
            msm = MarkovStateModel(self.lagtime, device=self.device).fit_counts(xi)
            if len(msm.active_set) != m:
                return None
            return msm.transition_matrix, Bn, pn, msm.stationary_distribution
        rows = xi.sum(axis=1)
        if (rows <= 0).any():
            self.degenerate = True
        An = np.where(rows[:, None] > 0, xi / np.where(rows > 0, rows, 1.0)[:, None], A)
        return An, Bn, pn, None

    def _fit_device(self, lab, lengths, A, B, p0):
        """the loop of fit() through hmm_fit_solver -> (A, B, p0, pi | None)"""
        solver = hmm_fit_solver(self.device)
        state = pi = None
        while self.n_iter < self.max_iter:
            n = min(self.steps_per_sync, self.max_iter - self.n_iter)
            A, B, p0, ll, got, state = solver.steps(lab, lengths, self.lagtime, A, B, p0, self.reversible, n, self.accuracy, state,
                                                    rev_tol=self.rev_tol, rev_max_sweeps=self.rev_max_sweeps)
            pi = got if got is not None else pi
            self.log_likelihoods.extend(float(v) for v in ll if np.isfinite(v))
            self.n_iter = int(state["n_estep"])
            if state["stop"]:
                break
        if state is not None:
            self.converged = state["stop"] == 1
            self.degenerate, self.rev_unconverged = bool(state["flags"] & 1), bool(state["flags"] & 2)
            self.rev_sweeps = int(state["rev_sweeps"])
            if state["stop"] == 2:
                self.message = self.MESSAGES.get(state["estep_status"], f"status {state['estep_status']}")
            elif state["stop"] == 3:
                self.message = self.LOST
        return A, B, p0, pi

    def fit(self, labels, traj_lengths=None, n_states=None, initial=None, renumber=True):
        lab, lengths, K = _hmm_labels(labels, traj_lengths, n_states, self.device, "HiddenMarkovModel")
        if initial is None:
            initial = initial_hmm(lab, self.lagtime, self.n_hidden, lengths, K, device=self.device)
        A, B, p0 = self._check_parameters(*initial, K)
        self.log_likelihoods, self.n_iter, self.converged, self.degenerate, self.message = [], 0, False, False, ""
        self.rev_sweeps, self.rev_unconverged = 0, False
        pi = None
        if self.m_step == "device":
            self._estep = None
            A, B, p0, pi = self._fit_device(lab, lengths, A, B, p0)
            return self._finish(A, B, p0, pi, renumber)
        self._estep = estep = hmm_estep_solver(self.device)
        while self.n_iter < self.max_iter:
            stats, _, _, status = estep(lab, lengths, self.lagtime, A, B, p0)
            self.n_iter += 1
            if status:
                self.message = self.MESSAGES.get(status, f"status {status}")
                break
            self.log_likelihoods.append(float(stats[0]))
            if len(self.log_likelihoods) > 1 and abs(self.log_likelihoods[-1] - self.log_likelihoods[-2]) < self.accuracy:
                self.converged = True
                break
            nxt = self._m_step(A, B, p0, stats)
            if nxt is None:
                self.message = self.LOST
                break
            A, B, p0, pi = nxt
        return self._finish(A, B, p0, pi, renumber)

    def _finish(self, A, B, p0, pi, renumber):
        if pi is None or not self.reversible:
            w, v = np.linalg.eig(A.T)
            pi = np.abs(np.real(v[:, np.argmax(np.real(w))]))
            pi = pi / pi.sum()
        order = np.argsort(-pi, kind="stable") if renumber else np.arange(len(pi))
        self.transition_matrix = A[np.ix_(order, order)]
        self.observation_probabilities, self.initial_distribution = B[order], p0[order]
        self.stationary_distribution = pi[order]
        return self

    def _need_fit(self):
        if self.transition_matrix is None:
            raise ValueError("HiddenMarkovModel: not fitted")

    def timescales(self, k=None):
        """The k slowest implied timescales -lagtime / ln(lambda_i), i = 2 .. k + 1, in frames (k defaults to n_hidden - 1); NaN
        for an eigenvalue <= 0 and beyond the model's size."""
        self._need_fit()
        k = self.n_hidden - 1 if k is None else int(k)
        lam = np.linalg.eigvals(self.transition_matrix)
        lam = np.sort(np.real(lam))[::-1] if self.reversible else np.sort(np.abs(lam))[::-1]
        return _timescales_of(lam[1:k + 1], k, self.lagtime)

    def lifetimes(self):
        """-lagtime / ln(A_ii) per hidden state, in frames (inf for A_ii = 1, NaN for A_ii = 0)"""
        self._need_fit()
        d = np.diag(self.transition_matrix)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(d > 0, -self.lagtime / np.log(d), np.nan)

    def metastable_memberships(self):
        """(K, m): P(hidden state | symbol) = pi_i B[i, s] / sum_i pi_i B[i, s]; NaN rows for symbols the model never emits"""
        self._need_fit()
        w = (self.stationary_distribution[:, None] * self.observation_probabilities).T
        s = w.sum(axis=1)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s > 0, w / s, np.nan)

    def _posterior(self, labels, traj_lengths):
        self._need_fit()
        K = self.observation_probabilities.shape[1]
        lab, lengths, _ = _hmm_labels(labels, traj_lengths, K, self.device, "HiddenMarkovModel")
        estep = self._estep or hmm_estep_solver(self.device)
        stats, _, post, status = estep(lab, lengths, self.lagtime, self.transition_matrix, self.observation_probabilities,
                                       self.initial_distribution, want_post=True)
        if status:
            raise ValueError(f"HiddenMarkovModel: the E-step failed on these labels (status {status})")
        return stats, post

    def hidden_probabilities(self, labels, traj_lengths=None):
        """the posteriors P(hidden state | all observations of the frame's chain): float64 (n, m) on the device"""
        return self._posterior(labels, traj_lengths)[1]

    def hidden_states(self, labels, traj_lengths=None):
        """the most probable hidden state of every frame (argmax of hidden_probabilities): int32 (n,) on the device"""
        return torch.argmax(self.hidden_probabilities(labels, traj_lengths), dim=1).to(torch.int32)

    def log_likelihood(self, labels, traj_lengths=None):
        return float(self._posterior(labels, traj_lengths)[0][0])

    def viterbi(self, labels, traj_lengths=None, order="frame", return_log_probabilities=False):
        """The most probable hidden path of every chain (dff_hmm_viterbi through hmm_viterbi_solver): int32 (n,) on the device.
        Unlike hidden_states -- the individually most probable state of every frame -- it is ONE path the model gives a
        positive probability, and the most probable one; ties go to the lowest state.  order="frame": the state of every frame
        in frame order; order="chain": the chains back to back (r-major, f-minor; their lengths: hmm_chain_lengths), the form
        label_runs takes.  A missing observation gets a state too.  The logarithms of A, B and p0 are taken here, on the host; a
        zero becomes -inf, an impossible step.  return_log_probabilities: also the joint log-probability of every chain's path and
        labels, a host array (n_traj lagtime,) in chain order (0 for an empty chain).  ValueError when the call fails, e. g. on a
        chain the model cannot emit (status 2)."""
        self._need_fit()
        if order not in ("frame", "chain"):
            raise ValueError('HiddenMarkovModel: order must be "frame" or "chain"')
        K = self.observation_probabilities.shape[1]
        lab, lengths, _ = _hmm_labels(labels, traj_lengths, K, self.device, "HiddenMarkovModel")
        with np.errstate(divide="ignore"):
            par = [np.log(x) for x in (self.transition_matrix, self.observation_probabilities, self.initial_distribution)]
        path, logprob, status = hmm_viterbi_solver(self.device)(lab, lengths, self.lagtime, *par, chain_order=order == "chain")
        if status:
            raise ValueError(f"HiddenMarkovModel: the Viterbi pass failed on these labels (status {status})")
        return (path, logprob) if return_log_probabilities else path


# ---- bootstrap error bars of a hidden Markov model: the labels resampled over trajectories or blocks, a device fit per resample ----
# What resampling_units' comment says holds here too: the discretisation is fixed, and blocks shorter than the slowest
# relaxation understate the error.  A block is a trajectory of its own, so it must hold chains of two frames at least.
def resampled_labels(labels, unit_lengths, weights_row):
    """The labels of one resample -> (labels' on the device of `labels`, lengths' int64): unit u (unit_lengths[u] frames, the
    units back to back over `labels`) appears weights_row[u] times, unit-major in unit order, a unit's copies adjacent, every
    copy a trajectory of its own (an empty unit gives empty trajectories).  The index is built on the host; the labels move by
    ONE gather on their device."""
    lab = torch.as_tensor(labels).reshape(-1)
    ul = np.asarray(unit_lengths, np.int64).reshape(-1)
    w = np.asarray(weights_row).reshape(-1)
    if w.shape != ul.shape or (ul < 0).any() or (w < 0).any() or int(ul.sum()) != int(lab.numel()):
        raise ValueError("resampled_labels: one non-negative weight per unit, the units' lengths summing to the number of labels")
    w = w.astype(np.int64)
    starts = np.cumsum(ul) - ul
    lengths = np.repeat(ul, w)
    first = np.repeat(starts, w)
    index = np.repeat(first - (np.cumsum(lengths) - lengths), lengths) + np.arange(int(lengths.sum()), dtype=np.int64)
    return lab.index_select(0, torch.from_numpy(index).to(lab.device)), lengths


class HmmBootstrap:
    """What bootstrap_hmm returns, B resamples of a model of m hidden states, the states in the point model's order:
    timescales (B, m - 1) and lifetimes (B, m) in frames, stationary (B, m), transition_matrices (B, m, m), log_likelihood (the
    last one), n_iter and converged (B,); the rows of a resample whose fit failed (the E-step failed, or the reversible
    estimator lost a hidden state) are NaN and `failed` (B,) is True there.  weights (B, n_units) and unit_lengths as
    resampled; point: the HiddenMarkovModel of the unresampled labels."""

    NAMES = ("timescales", "lifetimes", "stationary")

    def __init__(self, timescales, lifetimes, stationary, transition_matrices, log_likelihood, n_iter, converged, failed, weights,
                 unit_lengths, point):
        self.timescales, self.lifetimes, self.stationary = timescales, lifetimes, stationary
        self.transition_matrices, self.log_likelihood, self.n_iter = transition_matrices, log_likelihood, n_iter
        self.converged, self.failed, self.weights, self.unit_lengths, self.point = converged, failed, weights, unit_lengths, point

    @property
    def n_failed(self):
        """Resamples whose fit failed (NaN rows)."""
        return int(np.sum(self.failed))

    def _values(self, name):
        if name not in self.NAMES:
            raise ValueError(f"HmmBootstrap: name must be one of {self.NAMES}")
        return getattr(self, name)

    def std(self, name="timescales"):
        """Standard deviation (ddof = 1) of every column of `name` over the resamples where it is finite; NaN below two."""
        return percentile_std(self._values(name))

    def interval(self, name="timescales", confidence=0.95):
        """The percentile interval (lo, hi) of every column of `name` over the resamples where it is finite."""
        return percentile_interval(self._values(name), confidence)


def bootstrap_hmm(labels, lagtime, n_hidden, traj_lengths=None, n_states=None, *, n_resamples=100, block_frames=None, seed=0,
                  weights=None, reversible=True, accuracy=1e-3, max_iter=1000, steps_per_sync=32, point=None, device="cuda:0"):
    """Bootstrap of a HiddenMarkovModel at `lagtime`: the units of resampling_units(traj_lengths, block_frames) are drawn with
    replacement n_resamples times (bootstrap_weights(n_units, n_resamples, seed), or `weights` (B, n_units)); every resample
    is HiddenMarkovModel(m_step="device").fit(*resampled_labels(...), initial=the point model's parameters, renumber=False):
    warm-started, so its hidden states keep the point model's identity.  The resamples run one after the other.  point: a
    fitted HiddenMarkovModel of these labels, default HiddenMarkovModel(m_step="device").fit(labels, ...).  block_frames below
    2 lagtime is refused: such a block has no chain of two frames -> HmmBootstrap."""
    dev = torch.device(device)
    settings = dict(reversible=reversible, accuracy=accuracy, max_iter=max_iter, device=dev, m_step="device", steps_per_sync=steps_per_sync)
    proto = HiddenMarkovModel(n_hidden, lagtime, **settings)                                       # checks the settings
    if block_frames is not None and int(block_frames) < 2 * proto.lagtime:
        raise ValueError("bootstrap_hmm: block_frames must be at least 2 lagtime")
    lab, lengths, K = _hmm_labels(labels, traj_lengths, n_states, dev, "bootstrap_hmm")
    units = resampling_units(lengths, block_frames)
    if units.size < 1:
        raise ValueError("bootstrap_hmm: no resampling units (no frames)")
    if weights is None:
        w = bootstrap_weights(units.size, n_resamples, seed)
    else:
        w = np.asarray(weights)
        if w.ndim != 2 or w.shape[1] != units.size or w.shape[0] < 1 or (w < 0).any() or (w > 2 ** 32 - 1).any():
            raise ValueError(f"bootstrap_hmm: weights must be (B, {units.size}) multiplicities in 0 .. 2^32 - 1")
        w = w.astype(np.uint32)
    if point is None:
        point = proto.fit(lab, lengths, K)
    elif point.transition_matrix is None or point.n_hidden != proto.n_hidden or point.observation_probabilities.shape[1] != K:
        raise ValueError("bootstrap_hmm: point must be a fitted HiddenMarkovModel of n_hidden states on n_states symbols")
    start = (point.transition_matrix, point.observation_probabilities, point.initial_distribution)
    B, m = int(w.shape[0]), proto.n_hidden
    nan = np.nan
    ts, life, stat, T = np.full((B, m - 1), nan), np.full((B, m), nan), np.full((B, m), nan), np.full((B, m, m), nan)
    ll, n_iter, converged, failed = np.full(B, nan), np.zeros(B, np.int64), np.zeros(B, bool), np.zeros(B, bool)
    for b in range(B):
        model = HiddenMarkovModel(n_hidden, lagtime, **settings).fit(*resampled_labels(lab, units, w[b]), K, initial=start, renumber=False)
        n_iter[b], converged[b], failed[b] = model.n_iter, model.converged, bool(model.message)
        if not failed[b]:
            ts[b], life[b], stat[b], T[b] = model.timescales(), model.lifetimes(), model.stationary_distribution, model.transition_matrix
            ll[b] = model.log_likelihoods[-1] if model.log_likelihoods else nan
    return HmmBootstrap(ts, life, stat, T, ll, n_iter, converged, failed, w, units, point)


class HmmEvaluator(_TrajectoryEvaluator):
    """The metastable states of the sampled dynamics and their kinetics.  Frames -> TIC projection and k-means microstates
    (`tica`, n_microstates, centers, seed: as for MsmEvaluator) -> a HiddenMarkovModel of n_hidden states at `lagtime` (frames)
    on the microstate trajectory; a non-finite frame is a missing observation.

    eval(xyz, traj_lengths=None) -- None: ONE trajectory -- returns a dict:
      timescales           list of the n_hidden - 1 implied timescales of the hidden transition matrix, in units of frame_time
      hidden_populations   list: the stationary distribution of the hidden states, largest first
      lifetimes            list: -lagtime / ln A_ii in units of frame_time, in the same order
      n_iter, converged    E-steps spent; 1.0 when the log-likelihood met `accuracy`
      loglik_per_frame     the last log-likelihood over the number of frames
      samples_nonfinite    frames with a non-finite projection
    and with ref_data the same keys with the suffix _ref, log10_timescale_ratio, log10_lifetime_ratio and population_js
    (js_divergence of the populations): two separately fitted models share no labelling, so these compare the hidden states in
    the order of their populations.  The models stay on .models, the argmax hidden states on .hidden and their dwell
    statistics (label_runs -> dwell_summary) on .dwell, under "samples" / "refs".  Without the HIP library: DffLibraryError.

    path="posterior" (the default) is the above: .hidden is hidden_states(), the individually most probable state of every
    frame, and .dwell is taken on that frame-ordered series in units of frame_time -- at lagtime > 1 it interleaves lagtime
    separately decoded chains.  path="viterbi": .hidden holds the Viterbi path (HiddenMarkovModel.viterbi) in frame order, and
    .dwell = dwell_summary(label_runs(the path in chain order, hmm_chain_lengths(traj_lengths, lagtime)), frame_time *
    lagtime): dwells and events are taken INSIDE the chains, not across the interleave, one step of a chain being lagtime
    frames.  eval()'s dict is the same either way.

    n_bootstrap > 0 adds error bars from bootstrap_hmm(n_resamples=n_bootstrap, block_frames, seed=bootstrap_seed, point=the
    fitted model) to every ensemble's dict, in units of frame_time and in the order of the model's hidden states:
      timescales_std, lifetimes_std, hidden_populations_std   standard deviations over the resamples
      timescales_lo, timescales_hi                             the 95 % percentile interval
      bootstrap_failed                                         resamples whose fit failed
    The HmmBootstrap stays on .bootstrap under "samples" / "refs".  With n_bootstrap = 0 the dict is unchanged."""

    KEYS = ("timescales", "hidden_populations", "lifetimes", "n_iter", "converged", "loglik_per_frame", "samples_nonfinite")
    BOOTSTRAP_KEYS = ("timescales_std", "lifetimes_std", "hidden_populations_std", "timescales_lo", "timescales_hi", "bootstrap_failed")

    def __init__(self, mol_name, tica, n_microstates=200, n_hidden=2, lagtime=None, frame_time=1.0, ref_data=None,
                 ref_traj_lengths=None, centers=None, seed=0, *, reversible=True, accuracy=1e-3, max_iter=1000, path="posterior",
                 n_bootstrap=0, block_frames=None, bootstrap_seed=0, device="cuda:0"):
        what = "HmmEvaluator"
        super().__init__(what, mol_name, frame_time, device)
        if path not in ("posterior", "viterbi"):
            raise ValueError(f'{what}: path must be "posterior" or "viterbi"')
        self.path = path
        if lagtime is None or int(lagtime) != lagtime or int(lagtime) < 1:
            raise ValueError(f"{what}: lagtime must be an integer >= 1 (frames)")
        self.lagtime, self.n_hidden = int(lagtime), int(n_hidden)
        if self.n_hidden != n_hidden or not 1 <= self.n_hidden <= HMM_MAX_HIDDEN:
            raise ValueError(f"{what}: n_hidden must be an integer in 1..{HMM_MAX_HIDDEN}")
        self._hmm = dict(reversible=reversible, accuracy=accuracy, max_iter=max_iter)
        HiddenMarkovModel(self.n_hidden, self.lagtime, device="cpu", **self._hmm)       # its argument checks, now
        self.n_bootstrap, self.block_frames, self.bootstrap_seed = int(n_bootstrap), block_frames, bootstrap_seed
        if self.n_bootstrap != n_bootstrap or self.n_bootstrap < 0:
            raise ValueError(f"{what}: n_bootstrap must be an integer >= 0")
        if block_frames is not None and (int(block_frames) != block_frames or int(block_frames) < 2 * self.lagtime):
            raise ValueError(f"{what}: block_frames must be an integer >= 2 lagtime")
        self.bootstrap = {}
        self.mean, self.coeff = _tica_model(tica, what, TICA_MAX_DIM)
        self._micro = _Microstates(what, n_microstates, self.coeff.shape[1], centers, seed, self.device)
        self.n_microstates = self._micro.n_microstates
        self.models, self.labels, self.hidden, self.dwell = {}, {}, {}, {}
        self._start(ref_data, ref_traj_lengths)

    centers = property(lambda self: self._micro.centers, doc="the microstate centres (K, k); None until they are fitted")

    def project(self, x):
        return binding.struct_tic(x, self.mean, self.coeff)

    @staticmethod
    def summarize(model, n_frames, frame_time=1.0, samples_nonfinite=0):
        """eval()'s dict from a fitted HiddenMarkovModel: numpy only."""
        ll = model.log_likelihoods[-1] if model.log_likelihoods else float("nan")
        return {"timescales": [float(v) * frame_time for v in model.timescales()],
                "hidden_populations": [float(v) for v in model.stationary_distribution],
                "lifetimes": [float(v) * frame_time for v in model.lifetimes()],
                "n_iter": float(model.n_iter), "converged": float(bool(model.converged)),
                "loglik_per_frame": float(ll / n_frames) if n_frames else float("nan"),
                "samples_nonfinite": float(samples_nonfinite)}

    def _analyse(self, x, lengths, name):
        labels = self._micro.labels(self.project(x))
        model = HiddenMarkovModel(self.n_hidden, self.lagtime, device=self.device, **self._hmm)
        model.fit(labels, lengths, self.n_microstates)
        if self.path == "viterbi":
            hidden = model.viterbi(labels, lengths)
            runs = label_runs(model.viterbi(labels, lengths, order="chain"), hmm_chain_lengths(lengths, self.lagtime), device=self.device)
            step = self.frame_time * self.lagtime
        else:
            hidden = model.hidden_states(labels, lengths)
            runs, step = label_runs(hidden, lengths, device=self.device), self.frame_time
        self.models[name], self.labels[name], self.hidden[name] = model, labels.cpu().numpy(), hidden.cpu().numpy()
        self.dwell[name] = dwell_summary(runs, step)
        res = self.summarize(model, int(labels.numel()), self.frame_time, int((labels < 0).sum()))
        if self.n_bootstrap:
            bs = bootstrap_hmm(labels, self.lagtime, self.n_hidden, lengths, self.n_microstates, n_resamples=self.n_bootstrap,
                               block_frames=self.block_frames, seed=self.bootstrap_seed, point=model, device=self.device, **self._hmm)
            self.bootstrap[name] = bs
            res.update(self.error_bars(bs, self.frame_time))
        return res

    @staticmethod
    def error_bars(bs, frame_time=1.0):
        """the keys n_bootstrap adds, from an HmmBootstrap: numpy only"""
        lo, hi = bs.interval("timescales", 0.95)
        scaled = lambda v: [float(x) * frame_time for x in v]     # noqa: E731
        return {"timescales_std": scaled(bs.std("timescales")), "lifetimes_std": scaled(bs.std("lifetimes")),
                "hidden_populations_std": [float(x) for x in bs.std("stationary")], "timescales_lo": scaled(lo),
                "timescales_hi": scaled(hi), "bootstrap_failed": float(bs.n_failed)}

    def _compare(self, res, ref):
        res["log10_timescale_ratio"] = _log10_ratio(res["timescales"], ref["timescales"])
        res["log10_lifetime_ratio"] = _log10_ratio(res["lifetimes"], ref["lifetimes"])
        res["population_js"] = float(js_divergence(np.array(res["hidden_populations"]), np.array(ref["hidden_populations"])))


# =====================================================================================================
# Bootstrap error bars for the Jensen-Shannon metrics (PWD JS, TIC JS, Dihedral JS): a histogram is additive over frames, so
# the histogram of a resample is the weighted sum of the resampling units' histograms and no frame is looked at again.
# dff_unit_hist (or dff_pwd_hist per unit, whose bins are the reference's) gives the units' histograms once;
# dff_resampled_js forms every resample's histogram on chip and reduces it to its JS against the reference histogram.
# The bins are those of the point estimate, fixed for every resample.  The reference would give a resample whose largest
# distance is smaller fewer PWD bins; here those bins stay, empty, and each adds a term of order 1e-10 to that pair's JS.
# =====================================================================================================
def _bin_axis(v, edges):
    """searchsorted(edges, v, side="right") - 1 with numpy's histogramdd rule for explicit edges: a value equal to the last edge
    goes into the last bin; outside, and NaN, give -1.  int64, on v's device."""
    v = v.to(torch.float64)
    e = torch.as_tensor(np.asarray(edges, np.float64) if not isinstance(edges, torch.Tensor) else edges).to(
        device=v.device, dtype=torch.float64).contiguous()
    if e.dim() != 1 or e.numel() < 2:
        raise ValueError("bin edges must be a 1-D array of at least two values")
    idx = torch.searchsorted(e, v.contiguous(), right=True) - 1
    idx = torch.where(v == e[-1], torch.full_like(idx, e.numel() - 2), idx)
    return torch.where((v >= e[0]) & (v <= e[-1]), idx, torch.full_like(idx, -1))


def bin_indices_1d(values, edges):
    """int32 (n,): the bin of every value in np.histogram(values, bins=edges), -1 where numpy counts nothing (outside the
    edges, NaN).  torch, on the device `values` is on."""
    v = torch.as_tensor(values)
    return _bin_axis(v.reshape(-1), edges).to(torch.int32)


def bin_indices_2d(xy, edges_x, edges_y):
    """int32 (n,): ix * ny + iy, the flattened bin of every point (n, 2) in np.histogram2d(x, y, bins=[edges_x, edges_y]), -1
    where numpy counts nothing.  torch, on the device `xy` is on."""
    xy = torch.as_tensor(xy)
    if xy.dim() != 2 or xy.shape[1] != 2:
        raise ValueError("bin_indices_2d: points must be (n, 2)")
    ix, iy = _bin_axis(xy[:, 0], edges_x), _bin_axis(xy[:, 1], edges_y)
    ny = len(edges_y) - 1
    return torch.where((ix >= 0) & (iy >= 0), ix * ny + iy, torch.full_like(ix, -1)).to(torch.int32)


def sample_units(n, traj_lengths=None, block_frames=None, n_blocks=256):
    """The lengths (int64 array, summing to n) of the units a bootstrap of n frames resamples.  With traj_lengths: the
    trajectories or their blocks, resampling_units(traj_lengths, block_frames).  Without, for independent samples:
    min(n_blocks, n) consecutive near-equal blocks, the first n mod n_blocks one frame longer (any partition of
    exchangeable samples is a valid unit set)."""
    n = int(n)
    if traj_lengths is not None:
        units = resampling_units(_check_lengths(traj_lengths, n), block_frames)
        if units.size == 0:
            raise ValueError("sample_units: no frames")
        return units
    k = min(int(n_blocks), n)
    if k < 1:
        raise ValueError("sample_units: need n >= 1 frames and n_blocks >= 1")
    units = np.full(k, n // k, np.int64)
    units[: n % k] += 1
    return units


def unit_histograms(bins, nbins, unit_lengths):
    """int32 CUDA (U, C, max(nbins)): the histogram of every unit and channel (dff_unit_hist).  bins int32 CUDA (n, C) or
    (n,) for one channel, as bin_indices_1d / bin_indices_2d give them."""
    bins = torch.as_tensor(bins)
    if bins.dim() == 1:
        bins = bins[:, None]
    return binding.unit_hist(bins.to(torch.int32).contiguous(), unit_lengths, nbins)


class _DeviceJsResampler:
    """resample(unit_hist (U, C, ld), nbins (C,), ref (C, ld), weights (b, U)) -> (js float64 (b, C), total uint64 (b, C)) on
    the host; the histograms and the reference go to the GPU once per distinct array."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._key, self._hist, self._ref, self._ws = None, None, None, None

    def __call__(self, unit_hist, nbins, ref, weights):
        if self._key is None or self._key[0] is not unit_hist or self._key[1] is not ref:
            h = torch.as_tensor(unit_hist)
            if h.dtype not in (torch.int32, torch.uint32):
                h = h.to(torch.int32)
            self._hist = h.to(self.device).contiguous()
            self._ref = torch.as_tensor(np.asarray(ref, np.float64) if not isinstance(ref, torch.Tensor) else ref).to(
                device=self.device, dtype=torch.float64).contiguous()
            U, C = int(self._hist.shape[0]), int(self._hist.shape[1])
            self._ws = torch.empty(max(binding.resampled_js_workspace_bytes(U, C), 8), dtype=torch.uint8, device=self.device)
            self._key = (unit_hist, ref)
        w = torch.from_numpy(np.ascontiguousarray(weights, np.uint32)).to(self.device)
        js, tot = binding.resampled_js(self._hist, nbins, w, self._ref, workspace=self._ws)
        return js.cpu().numpy(), tot.cpu().numpy()


def js_resampler(device):
    """resample(unit_hist, nbins, ref, weights) -> (js (b, C), total (b, C)) on the GPU (dff_resampled_js)."""
    return _DeviceJsResampler(device)


class JsBootstrap:
    """What bootstrap_js returns.  per_channel (B, C): the JS of every resample and channel; values (B,): its mean over the
    channels (as the reference averages the PWD pairs); point_per_channel (C,) and point: the same for the unresampled data
    (all weights 1, through the same kernel); weights (B, U) and unit_lengths (U,) as resampled."""

    def __init__(self, per_channel, point_per_channel, weights, unit_lengths):
        self.per_channel, self.point_per_channel = per_channel, point_per_channel
        self.values = per_channel.mean(axis=1)
        self.point = float(point_per_channel.mean())
        self.weights, self.unit_lengths = weights, unit_lengths

    @property
    def n_failed(self):
        """Resamples whose value is not finite (a channel without a count)."""
        return int(np.sum(~np.isfinite(self.values)))

    def std(self):
        """Standard deviation (ddof = 1) of the value over the resamples where it is finite; NaN below two."""
        return float(percentile_std(self.values[:, None])[0])

    def interval(self, confidence=0.95):
        """The percentile interval (lo, hi) of the value over the resamples where it is finite."""
        lo, hi = percentile_interval(self.values[:, None], confidence)
        return float(lo[0]), float(hi[0])

    def bias(self):
        """mean(values) - point over the finite resamples: what finite histograms add to a JS, to first order."""
        v = self.values[np.isfinite(self.values)]
        return float(v.mean() - self.point) if v.size else float("nan")


JS_RESAMPLE_BYTES = 1 << 28       # weights in flight per call of the resampler


def bootstrap_js(unit_hist, nbins, ref_hist, *, n_resamples=200, seed=0, weights=None, resample_batch=None, unit_lengths=None,
                 device=None):
    """Bootstrap of a JS metric from the units' histograms: unit_hist (U, C, ld) integer counts (a CUDA tensor as
    unit_histograms gives it, or an array), nbins (C,), ref_hist (C, ld) the reference histogram of every channel (counts or
    densities).  The units are drawn with replacement n_resamples times (bootstrap_weights(U, n_resamples, seed), or
    `weights` (B, U)); resample_batch bounds the resamples per call.  The split changes no bit -> JsBootstrap."""
    U = int(unit_hist.shape[0])
    nb = np.asarray(nbins, np.int32).reshape(-1)
    if weights is None:
        weights = bootstrap_weights(U, n_resamples, seed)
    weights = np.ascontiguousarray(weights, np.uint32)
    if weights.ndim != 2 or weights.shape[1] != U or weights.shape[0] < 1:
        raise ValueError(f"bootstrap_js: weights must be (B, {U})")
    B = weights.shape[0]
    if device is None:
        device = unit_hist.device if isinstance(unit_hist, torch.Tensor) and unit_hist.is_cuda else "cuda:0"
    resample = js_resampler(device)
    batch = int(resample_batch) if resample_batch else max(1, min(binding.JS_MAX_RESAMPLES, JS_RESAMPLE_BYTES // (4 * U)))
    if batch < 1:
        raise ValueError("bootstrap_js: resample_batch must be >= 1")
    per = np.empty((B, nb.size))
    for b0 in range(0, B, batch):
        per[b0:b0 + batch] = resample(unit_hist, nb, ref_hist, weights[b0:b0 + batch])[0]
    point = resample(unit_hist, nb, ref_hist, np.ones((1, U), np.uint32))[0][0]
    units = None if unit_lengths is None else np.asarray(unit_lengths, np.int64)
    return JsBootstrap(per, point, weights, units)


def _js_units(n, traj_lengths, block_frames, n_blocks, unit_lengths):
    if unit_lengths is not None:
        units = np.asarray(unit_lengths, np.int64).reshape(-1)
        if units.sum() != n or (units < 0).any() or units.size < 1:
            raise ValueError(f"unit lengths must be non-negative and add up to the {n} frames given")
        return units
    return sample_units(n, traj_lengths, block_frames, n_blocks)


def js_error_bars(key, boot, confidence=0.95):
    """The keys Evaluator.eval_bootstrap adds for one metric, from its JsBootstrap: numpy only."""
    lo, hi = boot.interval(confidence)
    return {key: boot.point, key + "_lo": lo, key + "_hi": hi, key + "_std": boot.std(), key + "_bias": boot.bias()}


# =====================================================================================================
# Transition paths, read directly from the trajectories (dff_path_states; csrc/dff_paths.hip): the path times single-molecule
# experiments measure for fast folders (Chung & Eaton), p(TP | q), the Best-Hummer test of a reaction coordinate, and the
# empirical committor, the model-free counterpart of committor(model, A, B).  One device call gives, per frame, the core
# visited last AND the core visited next; everything after it composes bin_indices_1d, unit_histograms, resampling_units and
# bootstrap_weights.  The weighted sums of the bootstrap run on the host: at most 65 536 units x (bins x 8) counts.
# =====================================================================================================
class PathStates:
    """What path_states returns, tensors (n,) on the device: prev, next int8 -- the core (0: cv <= lo, 1: cv >= hi) visited
    last / next inside the trajectory, -1 when there is none or a non-finite frame lies in between; t_prev, t_next int64 -- the
    frames of those visits, -1 likewise; cls int8 -- 0 / 1 in a core, 2 / 3 on a path 0 -> 1 / 1 -> 0, 4 / 5 on a loop out of
    core 0 / 1 and back, -1 undetermined."""

    def __init__(self, prev, next, t_prev, t_next, cls):
        self.prev, self.next, self.t_prev, self.t_next, self.cls = prev, next, t_prev, t_next, cls

    def numpy(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("prev", "next", "t_prev", "t_next", "cls")}


def path_states(cv, lo, hi, traj_lengths=None, *, device=None):
    """The previous and the next core of every frame of the series cv (n,), cores cv <= lo (0) and cv >= hi (1) as in
    core_states, per trajectory -> PathStates on the device (cv's, when it is a CUDA tensor).  prev is what core_states
    returns.  traj_lengths=None: one trajectory."""
    lo, hi = _check_cores(lo, hi, "path_states")
    c = _series(cv, torch.float32, device)
    res = binding.path_states(c, _check_lengths(traj_lengths, len(c)), lo, hi, paths=False)
    return PathStates(res["prev"], res["next"], res["t_prev"], res["t_next"], res["cls"])


def _path_table(res):
    k = int(res["n_paths"].cpu())
    out = {"exit": res["exit"][:k].cpu().numpy(), "entry": res["entry"][:k].cpu().numpy(),
           "direction": res["direction"][:k].cpu().numpy()}
    out["duration"] = out["entry"] - out["exit"]
    return out


def transition_paths(cv, lo, hi, traj_lengths=None, *, device=None):
    """The transition paths of the series cv (n,) between the cores cv <= lo (0) and cv >= hi (1) -> a dict of numpy arrays
    over the paths in ascending entry: exit int64, the last frame in the core left; entry int64, the first frame in the core
    reached; direction int8, that core (1: 0 -> 1); duration int64 = entry - exit >= 1 frames (1: a direct jump).  A path lies
    inside one trajectory and holds no non-finite frame.  traj_lengths=None: one trajectory."""
    lo, hi = _check_cores(lo, hi, "transition_paths")
    c = _series(cv, torch.float32, device)
    return _path_table(binding.path_states(c, _check_lengths(traj_lengths, len(c)), lo, hi, frames=False, times=False))


def path_time_summary(paths, frame_time=1.0):
    """Transition-path times from the table of transition_paths: numpy only.  {direction: {"n", "mean", "median", "p10",
    "p90"}} for direction 1 (0 -> 1) and 0 (1 -> 0): the number of paths and the mean, the median and the 10th and 90th
    percentiles of their durations in units of frame_time; NaN without a path."""
    if not (np.isfinite(frame_time) and frame_time > 0):
        raise ValueError("path_time_summary: frame_time must be finite and > 0")
    direction = np.asarray(paths["direction"], np.int64).reshape(-1)
    duration = np.asarray(paths["duration"], np.float64).reshape(-1)
    if len(direction) != len(duration):
        raise ValueError("path_time_summary: direction and duration must have one entry per path")
    out = {}
    for d in (1, 0):
        t = duration[direction == d] * float(frame_time)
        nan = float("nan")
        p10, p90 = (float(v) for v in np.percentile(t, [10, 90])) if len(t) else (nan, nan)
        out[d] = {"n": int(len(t)), "mean": float(t.mean()) if len(t) else nan, "median": float(np.median(t)) if len(t) else nan,
                  "p10": p10, "p90": p90}
    return out


PATH_CLASSES = 6


def path_histograms(coordinate, edges, states, unit_lengths=None, *, n_states=None):
    """Per resampling unit and per bin of `coordinate` -- cv itself or any other series of the same frames -- the frames of
    every class and of every committor outcome: a dict of numpy arrays classes int64 (U, bins, 6), the frames of class 0 .. 5
    of `states` (a PathStates); next int64 (U, bins, 2), the frames whose next core is 0 / 1; edges; unit_lengths.  Frames of
    class -1 (next -1), and frames outside the edges or with a non-finite coordinate, are counted nowhere.  An integer
    coordinate with edges=None and n_states=K bins by microstate label 0 .. K - 1 instead.  unit_lengths=None: one unit of all
    frames; else consecutive units summing to n, as resampling_units gives them.  bin_indices_1d, a combined index (bin * 6 +
    class, bin * 2 + next) and unit_histograms with two channels: no other kernel."""
    cls, nxt = states.cls.reshape(-1), states.next.reshape(-1)
    dev = cls.device
    c = torch.as_tensor(coordinate).reshape(-1).to(dev)
    if len(c) != len(cls):
        raise ValueError(f"path_histograms: {len(c)} coordinate values for {len(cls)} frames")
    if edges is None:
        if n_states is None or int(n_states) < 1 or c.dtype.is_floating_point:
            raise ValueError("path_histograms: edges=None needs an integer coordinate and n_states >= 1")
        nb = int(n_states)
        b = torch.where((c >= 0) & (c < nb), c, torch.full_like(c, -1)).to(torch.int64)
    else:
        edges = np.asarray(edges, np.float64)
        b = bin_indices_1d(c, edges).to(torch.int64)
        nb = len(edges) - 1
    cls, nxt = cls.to(torch.int64), nxt.to(torch.int64)
    minus = torch.full_like(b, -1)
    idx = torch.stack([torch.where((b >= 0) & (cls >= 0), b * PATH_CLASSES + cls, minus),
                       torch.where((b >= 0) & (nxt >= 0), b * 2 + nxt, minus)], dim=1).to(torch.int32).contiguous()
    units = np.asarray([len(c)] if unit_lengths is None else unit_lengths, np.int64).reshape(-1)
    h = unit_histograms(idx, [nb * PATH_CLASSES, nb * 2], units).cpu().numpy().astype(np.int64)
    return {"classes": h[:, 0, :].reshape(len(units), nb, PATH_CLASSES), "next": h[:, 1, :nb * 2].reshape(len(units), nb, 2),
            "edges": edges, "unit_lengths": units}


def _conditional(counts, picks, min_count, weights, confidence):
    """counts int64 (U, bins, k) -> for every name in picks the share of the columns picks[name] among all k columns, per
    bin: {name: (bins,), "count": (bins,)} from the counts summed over the units, NaN in a bin with fewer than min_count
    counted frames; with weights (B, U) also name_resamples (B, bins), the same from every resample's weighted counts, and
    name_lo / name_hi, their percentile interval (a resample's bin under min_count is left out of that bin's interval)."""
    counts = np.asarray(counts, np.int64)
    if counts.ndim != 3:
        raise ValueError("conditional histograms must be (units, bins, columns)")
    if int(min_count) < 1:
        raise ValueError("min_count must be >= 1")

    def shares(c):                                                  # c (..., bins, k)
        det = c.sum(axis=-1)
        ok = det >= int(min_count)
        safe = np.where(ok, det, 1).astype(np.float64)
        return {name: np.where(ok, c[..., cols].sum(axis=-1) / safe, np.nan) for name, cols in picks.items()}, det

    out, det = shares(counts.sum(axis=0))
    out["count"] = det
    if weights is not None:
        w = np.asarray(weights, np.int64)
        if w.ndim != 2 or w.shape[1] != counts.shape[0]:
            raise ValueError(f"weights must be (resamples, {counts.shape[0]} units)")
        res, _ = shares(np.einsum("bu,unk->bnk", w, counts))
        for name in picks:
            out[name + "_resamples"] = res[name]
            out[name + "_lo"], out[name + "_hi"] = percentile_interval(res[name], confidence)
    return out


def tp_probability(hist, min_count=1, *, weights=None, confidence=0.95):
    """p(TP | bin) of Best & Hummer from path_histograms: the share of the frames on a transition path among the determined
    frames of a bin, p_tp = (class 2 + class 3) / (classes 0 .. 5), with p_tp_ab (class 2: paths 0 -> 1) and p_tp_ba (class
    3) separately, and count, the determined frames per bin.  A bin with fewer than min_count determined frames is NaN: a
    condition on the data, not a tolerance; the default 1 leaves out only empty bins.  For a perfect coordinate and diffusive
    dynamics the maximum is 1 / 2, at the transition state.  weights uint32 (B, U) as bootstrap_weights(U, B, seed) gives them,
    over the units of path_histograms: also p_tp_resamples (B, bins) and p_tp_lo / p_tp_hi (and _ab, _ba), the `confidence` percentile interval
    over the resamples of the units.  numpy only."""
    return _conditional(hist["classes"], {"p_tp": [2, 3], "p_tp_ab": [2], "p_tp_ba": [3]}, min_count, weights, confidence)


def empirical_committor(hist, min_count=1, *, weights=None, confidence=0.95):
    """The empirical committor from path_histograms: p_b(bin) = frames whose next core is 1 / frames whose next core is
    known, and count, the latter per bin -- which core does the trajectory reach next, read off the trajectories, the
    model-free counterpart of committor(model, A, B).  Frames inside core 1 count as 1, inside core 0 as 0.  A bin with fewer
    than min_count such frames is NaN (a condition, not a tolerance; default 1).  weights: as for tp_probability, giving
    p_b_resamples and p_b_lo / p_b_hi.  numpy only."""
    return _conditional(hist["next"], {"p_b": [1]}, min_count, weights, confidence)


def _half_crossing(x, p):
    """the coordinate where p (NaN: no estimate) first crosses 1 / 2 between two neighbouring estimated bins at x, linearly
    interpolated; NaN when it never does"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    ok = np.isfinite(p)
    x, p = x[ok], p[ok]
    for i in range(len(p) - 1):
        a, b = p[i] - 0.5, p[i + 1] - 0.5
        if a == 0.0:
            return float(x[i])
        if a * b < 0.0:
            return float(x[i] + (x[i + 1] - x[i]) * a / (a - b))
    return float(x[-1]) if len(p) and p[-1] == 0.5 else float("nan")


class TransitionPathEvaluator(_TrajectoryEvaluator):
    """The transitions themselves: how long a barrier crossing takes, whether the order parameter is a good reaction coordinate,
    and where the trajectories commit.  Frames -> order parameter (cv="q" or "rmsd", as for FoldingKineticsEvaluator) ->
    binding.path_states with the cores cv <= lo and cv >= hi -> path table, class and committor histograms over nbins equal
    bins of cv_range (default 0 .. 1 for Q, 0 .. 1.5 hi for the RMSD; frames outside are counted in no bin).  Folded is label 1
    for Q and label 0 for the RMSD; a folding path is one that ENTERS the folded core.

    eval(xyz, traj_lengths=None) returns a plain dict of floats:
      n_paths_folding, n_paths_unfolding
      mean_path_time_folding / _unfolding, median_path_time_folding / _unfolding   in units of frame_time; NaN without a path
      path_frames_share, loop_frames_share, undetermined_share   shares of ALL frames: class 2 + 3, class 4 + 5, class -1
      ptp_max, ptp_max_at          the largest p(TP | bin) over the bins with >= min_count determined frames, and that bin's centre
      committor_half               the coordinate where the empirical committor p_b first crosses 1 / 2 (interpolated)
      samples_nonfinite            frames with a non-finite coordinate
    With n_resamples > 0 also ptp_max_lo / _hi (the interval of p(TP) in that bin) and committor_half_lo / _hi, over resamples
    of the trajectories (or of their blocks of block_frames frames).  With ref_data the same keys with the suffix _ref, and
    log10_path_time_ratio_folding / _unfolding (mean path times, samples over reference), ptp_max_diff and committor_rmsd, the
    root mean square difference of p_b over the bins estimated in both.  Series and histograms stay on .series: {"samples" /
    "refs": {"cv", "states", "paths", "summary", "hist", "p_tp", "p_b"}}.  Without the HIP library: DffLibraryError."""

    KEYS = ("n_paths_folding", "n_paths_unfolding", "mean_path_time_folding", "mean_path_time_unfolding",
            "median_path_time_folding", "median_path_time_unfolding", "path_frames_share", "loop_frames_share",
            "undetermined_share", "ptp_max", "ptp_max_at", "committor_half", "samples_nonfinite")

    def __init__(self, mol_name, folded, *, cv="q", lo, hi, frame_time=1.0, nbins=50, cv_range=None, min_count=1, ref_data=None,
                 ref_traj_lengths=None, n_resamples=0, block_frames=None, seed=0, confidence=0.95, cutoff=10.0, offset=3, beta=5.0,
                 lam=1.2, device="cuda:0"):
        what = "TransitionPathEvaluator"
        super().__init__(what, mol_name, frame_time, device)
        self.lo, self.hi = _check_cores(lo, hi, what)
        self._cv = _Observable(what, cv, ("q", "rmsd"), folded, mol_name, None, cutoff, offset, beta, lam)
        self.cv, self.folded = cv, self._cv.folded
        self.folded_label, self.unfolded_label = (1, 0) if cv == "q" else (0, 1)
        if int(nbins) != nbins or not 1 <= int(nbins) <= 1 << 16:
            raise ValueError(f"{what}: nbins must be an integer in 1 .. 65536")
        a, b = (float(v) for v in (cv_range if cv_range is not None else ((0.0, 1.0) if cv == "q" else (0.0, 1.5 * self.hi))))
        if not (np.isfinite(a) and np.isfinite(b) and a < b):
            raise ValueError(f"{what}: cv_range must be finite and ascending")
        self.edges = np.linspace(a, b, int(nbins) + 1)
        self.centres = 0.5 * (self.edges[:-1] + self.edges[1:])
        if int(min_count) < 1 or int(n_resamples) < 0:
            raise ValueError(f"{what}: min_count must be >= 1 and n_resamples >= 0")
        self.min_count, self.n_resamples, self.block_frames, self.seed = int(min_count), int(n_resamples), block_frames, seed
        self.confidence = float(confidence)
        self.series = {}
        self._start(ref_data, ref_traj_lengths)

    def order_parameter(self, x):
        """float32 tensor (n,) on the device: Q or the RMSD of the frames x (n, N, 3) already there"""
        return self._cv(x)

    @staticmethod
    def summarize(summary, cls_counts, p_tp, p_b, centres, folded_label, samples_nonfinite=0):
        """eval()'s dict from a path_time_summary, the frames of every class -1, 0 .. 5 (7 counts), p_tp and p_b per bin and
        the bins' centres: numpy only."""
        nan = float("nan")
        cls_counts = np.asarray(cls_counts, np.int64)
        n = int(cls_counts.sum())
        F = folded_label
        res = {}
        for name, d in (("folding", F), ("unfolding", 1 - F)):
            res[f"n_paths_{name}"] = float(summary[d]["n"])
            res[f"mean_path_time_{name}"] = summary[d]["mean"]
            res[f"median_path_time_{name}"] = summary[d]["median"]
        share = lambda k: float(k) / n if n else nan     # noqa: E731
        res["path_frames_share"] = share(cls_counts[3] + cls_counts[4])
        res["loop_frames_share"] = share(cls_counts[5] + cls_counts[6])
        res["undetermined_share"] = share(cls_counts[0])
        p_tp = np.asarray(p_tp, np.float64)
        if np.isfinite(p_tp).any():
            k = int(np.nanargmax(p_tp))
            res["ptp_max"], res["ptp_max_at"] = float(p_tp[k]), float(centres[k])
        else:
            res["ptp_max"] = res["ptp_max_at"] = nan
        res["committor_half"] = _half_crossing(centres, p_b)
        res["samples_nonfinite"] = float(samples_nonfinite)
        return {k: res[k] for k in TransitionPathEvaluator.KEYS}

    def _analyse(self, x, lengths, name):
        cv = self.order_parameter(x)
        out = binding.path_states(cv, lengths, self.lo, self.hi)
        states = PathStates(out["prev"], out["next"], out["t_prev"], out["t_next"], out["cls"])
        paths = _path_table(out)
        summary = path_time_summary(paths, self.frame_time)
        units = resampling_units(lengths, self.block_frames)
        units = units[units > 0]
        weights = bootstrap_weights(len(units), self.n_resamples, self.seed) if self.n_resamples and len(units) else None
        hist = path_histograms(cv, self.edges, states, units if len(units) else None)
        p_tp = tp_probability(hist, self.min_count, weights=weights, confidence=self.confidence)
        p_b = empirical_committor(hist, self.min_count, weights=weights, confidence=self.confidence)
        cls_counts = np.bincount(states.cls.cpu().numpy().astype(np.int64) + 1, minlength=PATH_CLASSES + 1)
        self.series[name] = {"cv": cv.cpu().numpy(), "states": states.numpy(), "paths": paths, "summary": summary, "hist": hist,
                             "p_tp": p_tp, "p_b": p_b}
        res = self.summarize(summary, cls_counts, p_tp["p_tp"], p_b["p_b"], self.centres, self.folded_label, _count_nonfinite(x))
        if weights is not None:
            k = int(np.nanargmax(p_tp["p_tp"])) if np.isfinite(p_tp["p_tp"]).any() else None
            res["ptp_max_lo"] = float(p_tp["p_tp_lo"][k]) if k is not None else float("nan")
            res["ptp_max_hi"] = float(p_tp["p_tp_hi"][k]) if k is not None else float("nan")
            half = np.array([[_half_crossing(self.centres, row)] for row in p_b["p_b_resamples"]])
            lo, hi = percentile_interval(half, self.confidence)
            res["committor_half_lo"], res["committor_half_hi"] = float(lo[0]), float(hi[0])
        return res

    def _compare(self, res, ref):
        for which in ("folding", "unfolding"):
            res[f"log10_path_time_ratio_{which}"] = _log10_ratio(res[f"mean_path_time_{which}"], ref[f"mean_path_time_{which}"])
        res["ptp_max_diff"] = res["ptp_max"] - ref["ptp_max"]
        a, b = self.series["samples"]["p_b"]["p_b"], self.series["refs"]["p_b"]["p_b"]
        both = np.isfinite(a) & np.isfinite(b)
        res["committor_rmsd"] = float(np.sqrt(np.mean((a[both] - b[both]) ** 2))) if both.any() else float("nan")
