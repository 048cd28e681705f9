"""ctypes binding of libdff_amd.so (C ABI: include/dff.h).

The HIP library is the product path: there is NO CPU / PyTorch fallback.  If the shared
library is missing or fails to load, importing a sampler raises ``DffLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFF_LIB_PATH") or os.path.join(_HERE, "libdff_amd.so")   # DFF_LIB_PATH: development builds
DFF_MAX_BEADS = 64
FORWARD_STEP = 0xFFFFFFFE00000000    # Philox step of the forward-process draws is FORWARD_STEP | draw (include/dff.h)
LOSS_TYPES = {"l1": 1, "l2": 2}

SCHEDULE_NAMES = (
    "betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
    "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
    "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
    "posterior_mean_coef1", "posterior_mean_coef2",
)


class DffLibraryError(RuntimeError):
    pass


class DffConfig(C.Structure):
    _fields_ = [("n_beads", C.c_int32), ("hidden", C.c_int32), ("n_layers", C.c_int32),
                ("timesteps", C.c_int32), ("use_intrinsic_coords", C.c_int32),
                ("use_distances", C.c_int32), ("use_abs_coords", C.c_int32),
                ("conservative", C.c_int32)]


class DffLangevinParams(C.Structure):
    _fields_ = [("t_norm", C.c_float), ("force_scale", C.c_float), ("dt", C.c_float),
                ("vscale", C.c_float), ("noisescale", C.c_float), ("beta", C.c_float),
                ("dtau", C.c_float), ("overdamped", C.c_int32),
                ("masses", C.c_float * DFF_MAX_BEADS)]


class DffDispatch(C.Structure):
    """dff_dispatch: what kernel selection reads of a model besides its config (Model.dispatch, plan_launch)."""
    _fields_ = [(n, C.c_int32) for n in ("split", "small_split", "fold_kv", "n_cus", "group_override", "small_waves",
                                         "max_wgs", "force_generic", "l0_off", "pair_off", "sticky", "small_pair",
                                         "small_h96")]


class DffLaunchPlan(C.Structure):
    _fields_ = [("kernel", C.c_char_p)] + [(n, C.c_int32) for n in ("G", "workgroups", "launches", "last_grid", "lds_bytes",
                                                                     "threads", "pair", "table")] + [("table_kernel", C.c_char_p)]


class DffMsmBatchLaunch(C.Structure):
    """dff_msm_batch_launch: one of the two launches of a batched solver (msm_batch_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("launched", "path", "lo", "hi", "sized_for", "lds_bytes")]


class DffMsmBatchPlan(C.Structure):
    _fields_ = [("launch", DffMsmBatchLaunch * 2)]


class DffPwdPlan(C.Structure):
    """dff_pwd_plan: the launch layout of dff_pwd_hist (pwd_hist_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("n_pairs", "tile_n", "pc_log2", "npc", "ldl", "lds_bytes")] + \
               [(n, C.c_longlong) for n in ("chunk", "chunks", "chunks_rounded", "grid")]


# every symbol include/dff.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "dff_weight_count": (C.c_size_t, [C.POINTER(DffConfig)]),
    "dff_model_create": (C.c_int, [C.POINTER(DffConfig), _P, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "dff_model_destroy": (None, [_P]),
    "dff_schedule": (C.c_int, [_P, C.c_int, _P]),
    "dff_score": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P]),
    "dff_langevin_run": (C.c_int, [_P, C.POINTER(DffLangevinParams), C.c_int, _P, _P, _P, C.c_uint64,
                                   C.c_uint64, C.c_uint64, C.c_int, C.c_int, _P, _P, _P]),
    "dff_ddpm_run": (C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int,
                               _P, _P]),
    "dff_q_sample": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "dff_denoise_workspace_bytes": (C.c_longlong, [_P, C.c_int]),
    "dff_denoise_loss": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, _P, _P, _P, _P,
                                   _P, C.c_size_t, _P]),
    "dff_set_group": (C.c_int, [_P, C.c_int]),
    "dff_debug_force_generic": (C.c_int, [_P, C.c_int]),
    "dff_debug_small_waves": (C.c_int, [_P, C.c_int]),
    "dff_debug_l0_table": (C.c_int, [_P, C.c_int]),
    "dff_debug_max_workgroups": (C.c_int, [_P, C.c_int]),
    "dff_last_launch": (C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dff_debug_dispatch": (C.c_int, [_P, C.POINTER(DffDispatch)]),
    "dff_debug_plan_launch": (C.c_int, [C.POINTER(DffConfig), C.POINTER(DffDispatch), C.c_int, C.c_int,
                                        C.POINTER(DffLaunchPlan)]),
    "dff_debug_gemm": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "dff_debug_stash": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t]),
    "dff_debug_profile": (C.c_int, [_P, C.c_int]),
    "dff_debug_profile_read": (C.c_int, [_P, _P]),
    "dff_pwd_num_pairs": (C.c_int, [C.c_int, C.c_int]),
    "dff_pwd_max": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, C.c_int, _P, _P]),
    "dff_pwd_hist": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P]),
    "dff_pwd_hist_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(DffPwdPlan)]),
    "dff_struct_rmsd": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P, _P]),
    "dff_struct_dihedrals": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P]),
    "dff_struct_tic_num_features": (C.c_int, [C.c_int]),
    "dff_struct_tic": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P, C.c_int, _P, _P]),
    "dff_struct_contacts": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, C.c_float, _P, C.c_int, _P, _P, _P]),
    "dff_struct_tic_features": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P]),
    "dff_tica_workspace_bytes": (C.c_longlong, [C.c_int, C.c_longlong, C.c_int]),
    "dff_tica_moments": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_size_t,
                                   _P, _P, _P, _P, _P]),
    "dff_tica_debug_plan": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_longlong, _P, C.c_int]),
    "dff_struct_tic_assign": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "dff_kmeans_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_int, C.c_int]),
    "dff_kmeans_step": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t,
                                  _P]),
    "dff_transition_counts": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "dff_rmsd_nearest_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int]),
    "dff_rmsd_nearest": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_longlong, C.c_int, C.c_longlong, _P, _P, _P,
                                   C.c_size_t, _P]),
    "dff_rmsd_matrix": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_longlong, C.c_int, _P, _P]),
    "dff_superpose_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_int]),
    "dff_superpose": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_rmsd_neighbors": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, C.c_float, _P, _P, _P]),
    "dff_gromos_workspace_bytes": (C.c_longlong, [C.c_longlong]),
    "dff_gromos_steps": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_struct_native_q": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, _P, C.c_int, C.c_double, C.c_double, _P, _P]),
    "dff_kinetics_workspace_bytes": (C.c_longlong, [C.c_longlong]),
    "dff_core_states": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, C.c_size_t, _P]),
    "dff_label_runs": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_longlong, _P, _P, _P, _P, _P, _P, C.c_size_t,
                                 _P]),
    "dff_path_states_workspace_bytes": (C.c_longlong, [C.c_longlong]),
    "dff_path_states": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_longlong,
                                  _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_autocorr_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_int, C.c_int]),
    "dff_autocorr": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t,
                               _P]),
    "dff_micro_chunk": (C.c_int, []),
    "dff_micro_kmeans_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_int, C.c_int]),
    "dff_micro_kmeans_step": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t,
                                        _P]),
    "dff_micro_transition_counts": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "dff_msm_workspace_bytes": (C.c_longlong, [C.c_int]),
    "dff_msm_reversible_steps": (C.c_int, [C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "dff_debug_msm_driver": (C.c_int, [C.c_int]),
    "dff_msm_driver_for": (C.c_int, [C.c_int]),
    "dff_micro_resampled_counts_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_micro_resampled_counts": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int,
                                             _P, _P, C.c_size_t, _P]),
    "dff_msm_batched_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_msm_reversible_steps_batched": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_size_t,
                                                   _P]),
    "dff_msm_batched_driver_for": (C.c_int, [C.c_int, C.c_int]),
    "dff_msm_dirichlet_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_msm_dirichlet_lds_limit": (C.c_int, []),
    "dff_msm_dirichlet_solve": (C.c_int, [C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t,
                                          _P]),
    "dff_debug_msm_dirichlet_path": (C.c_int, [C.c_int]),
    "dff_sym_eig_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_sym_eig_lds_limit": (C.c_int, []),
    "dff_sym_eig_topk": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_debug_sym_eig_path": (C.c_int, [C.c_int]),
    "dff_msm_propagate_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dff_msm_propagate_lds_limit": (C.c_int, []),
    "dff_msm_propagate": (C.c_int, [C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P,
                                    _P, C.c_size_t, _P]),
    "dff_debug_msm_propagate_path": (C.c_int, [C.c_int]),
    "dff_debug_msm_batch_plan": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(DffMsmBatchPlan)]),
    "dff_hmm_chunk": (C.c_int, []),
    "dff_hmm_plan": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dff_hmm_workspace_bytes": (C.c_longlong, [C.c_longlong, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dff_hmm_estep": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                C.c_size_t, _P]),
    "dff_debug_hmm_stages": (C.c_int, [C.c_int]),
    "dff_hmm_fit_workspace_bytes": (C.c_longlong, [C.c_longlong, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dff_hmm_fit_steps": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_double, C.c_double, C.c_longlong, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_hmm_viterbi_workspace_bytes": (C.c_longlong, [C.c_longlong, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dff_hmm_viterbi": (C.c_int, [C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P,
                                  _P, C.c_size_t, _P]),
    "dff_debug_hmm_viterbi_stages": (C.c_int, [C.c_int]),
    "dff_unit_hist_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_unit_hist": (C.c_int, [C.c_int, _P, C.c_longlong, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "dff_resampled_js_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "dff_resampled_js": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "dff_resampled_js_path_for": (C.c_int, [C.c_int, C.c_int]),
    "dff_debug_resampled_js_path": (C.c_int, [C.c_int]),
    "dff_last_error": (C.c_char_p, []),
    "dff_debug_pair": (C.c_int, [_P, C.c_int]),
    "dff_debug_pair_status": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "dff_model_status": (C.c_int, [_P, C.POINTER(C.c_uint)]),
    "dff_model_status_clear": (C.c_int, [_P]),
    "dff_debug_poke_status": (C.c_int, [_P, C.c_uint]),
    "dff_version": (C.c_char_p, []),
}

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libdff_amd.so and type every exported entry point; loud failure if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise DffLibraryError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            f"or ./build.sh).  There is no CPU fallback.")
    try:
        lib = C.CDLL(p)
    except OSError as e:  # e.g. libamdhip64 missing
        raise DffLibraryError(f"cannot load {p}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise DffLibraryError(f"{p} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.dff_last_error().decode(errors="replace")
        if rc == 1:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Model:
    """Owner of one ``dff_model`` handle (packed weights + scratch on one GPU)."""

    def __init__(self, n_beads: int, hidden: int, n_layers: int, flat_weights: np.ndarray,
                 timesteps: int = 1000, device: int = 0, use_intrinsic_coords=True,
                 use_distances=False, use_abs_coords=False, conservative=True):
        self.lib = load_library()
        self.cfg = DffConfig(n_beads, hidden, n_layers, timesteps, int(bool(use_intrinsic_coords)),
                             int(bool(use_distances)), int(bool(use_abs_coords)), int(bool(conservative)))
        w = np.ascontiguousarray(flat_weights, dtype=np.float32)
        self.handle = C.c_void_p()
        rc = self.lib.dff_model_create(C.byref(self.cfg), w.ctypes.data_as(C.c_void_p), w.size, device,
                                       C.byref(self.handle))
        _check(self.lib, rc, "dff_model_create")
        self.device = device
        self.n_beads, self.hidden, self.n_layers, self.timesteps = n_beads, hidden, n_layers, timesteps

    def close(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            self.lib.dff_model_destroy(h)
            h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: ctypes may already be torn down
            pass

    # ---- helpers
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev_tensor(self, t, shape=None, name="tensor"):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor")
        if t.device.index != self.device:
            raise ValueError(f"{name} is on {t.device}, model is on cuda:{self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def schedule(self, name: str) -> np.ndarray:
        out = np.empty(self.timesteps, np.float32)
        _check(self.lib, self.lib.dff_schedule(self.handle, SCHEDULE_NAMES.index(name), out.ctypes.data_as(C.c_void_p)),
               "dff_schedule")
        return out

    def set_group(self, g: int):
        _check(self.lib, self.lib.dff_set_group(self.handle, int(g)), "dff_set_group")

    def force_generic(self, on: bool = True):
        _check(self.lib, self.lib.dff_debug_force_generic(self.handle, int(on)), "dff_debug_force_generic")

    def small_waves(self, waves: int = 0):
        _check(self.lib, self.lib.dff_debug_small_waves(self.handle, int(waves)), "dff_debug_small_waves")

    def max_workgroups(self, n: int = 2048):
        _check(self.lib, self.lib.dff_debug_max_workgroups(self.handle, int(n)), "dff_debug_max_workgroups")

    def pair(self, on=True):
        """True / False: allow / never use the two-workgroups-per-protein variants; 2: allow, and force their cross-XCD exchange protocol;
        3: allow, with the two workgroups of a protein on adjacent blocks (different XCDs: the protocol is chosen by the kernel's own check)."""
        _check(self.lib, self.lib.dff_debug_pair(self.handle, int(on)), "dff_debug_pair")

    def pair_status(self) -> int:
        st = C.c_int(0)
        _check(self.lib, self.lib.dff_debug_pair_status(self.handle, C.byref(st)), "dff_debug_pair_status")
        return st.value

    def status(self) -> int:
        """Sticky status word of every launch so far (dff_model_status; synchronises the device)."""
        st = C.c_uint(0)
        _check(self.lib, self.lib.dff_model_status(self.handle, C.byref(st)), "dff_model_status")
        return st.value

    def check(self):
        """Raise if any launch so far reported a failure the kernels cannot return synchronously (bit 0: a
        two-workgroups-per-protein launch lost its partner workgroup).  Called at the samplers' host sync points."""
        w = self.status()
        if w:
            # reported once: the word is cleared, so the model is usable again (a transient co-tenant must not poison every
            # later run); the launches since the failure produced nothing -- the kernels leave at entry while the word is set
            self.status_clear()
            raise RuntimeError(f"libdff_amd: device-side failure word {w:#x}: a two-workgroups-per-protein kernel launch timed "
                               f"out waiting for its partner workgroup (GPU shared or partitioned?); the results since then "
                               f"are invalid.  The word has been cleared; Model.pair(False) selects the one-workgroup kernels.")

    def poke_status(self, word: int):
        _check(self.lib, self.lib.dff_debug_poke_status(self.handle, int(word)), "dff_debug_poke_status")

    def status_clear(self):
        _check(self.lib, self.lib.dff_model_status_clear(self.handle), "dff_model_status_clear")

    def l0_table(self, on: bool = True):
        _check(self.lib, self.lib.dff_debug_l0_table(self.handle, int(on)), "dff_debug_l0_table")

    def last_launch(self):
        name, grid, lds = C.c_char_p(), C.c_int(), C.c_int()
        _check(self.lib, self.lib.dff_last_launch(self.handle, C.byref(name), C.byref(grid), C.byref(lds)), "dff_last_launch")
        return (name.value or b"").decode(), grid.value, lds.value

    def dispatch(self) -> dict:
        """What kernel selection reads of this model, as the next launch would see it (dff_debug_dispatch; host only)."""
        d = DffDispatch()
        _check(self.lib, self.lib.dff_debug_dispatch(self.handle, C.byref(d)), "dff_debug_dispatch")
        return {n: getattr(d, n) for n, _ in DffDispatch._fields_}

    # ---- the three entry points
    def score(self, x, tnorm, return_energy=False):
        import torch
        B = x.shape[0]
        self._dev_tensor(x, (B, self.n_beads, 3), "x")
        self._dev_tensor(tnorm, (B,), "t")
        force = torch.empty_like(x)
        energy = torch.empty(B, self.n_beads, device=x.device, dtype=torch.float32) if return_energy else None
        rc = self.lib.dff_score(self.handle, _ptr(x), _ptr(tnorm), B, _ptr(force), _ptr(energy), self._stream())
        _check(self.lib, rc, "dff_score")
        return (force, energy) if return_energy else force

    def langevin_run(self, params: DffLangevinParams, x, v, n_steps: int, save_interval: int,
                     noise=None, seed: int = 0, traj_offset: int = 0, step_offset: int = 0,
                     frames=None, ke=None):
        P = x.shape[0]
        self._dev_tensor(x, (P, self.n_beads, 3), "x")
        if v is not None:
            self._dev_tensor(v, (P, self.n_beads, 3), "v")
        if noise is not None:
            self._dev_tensor(noise, (n_steps, P, self.n_beads, 3), "noise")
        nf = n_steps // save_interval if save_interval > 0 else 0
        if frames is not None:
            self._dev_tensor(frames, (nf, P, self.n_beads, 3), "frames")
        if ke is not None:
            self._dev_tensor(ke, (nf, P), "ke")
        rc = self.lib.dff_langevin_run(self.handle, C.byref(params), P, _ptr(x), _ptr(v), _ptr(noise),
                                       seed & (2 ** 64 - 1), traj_offset, step_offset, n_steps, save_interval,
                                       _ptr(frames), _ptr(ke), self._stream())
        _check(self.lib, rc, "dff_langevin_run")

    def ddpm_run(self, x, t_start: int, t_end: int = 0, noise=None, seed: int = 0, sample_offset: int = 0,
                 init_prior: bool = False, clamp_flag=None):
        B = x.shape[0]
        self._dev_tensor(x, (B, self.n_beads, 3), "x")
        if noise is not None:
            self._dev_tensor(noise, (t_start - t_end + 1, B, self.n_beads, 3), "noise")
        rc = self.lib.dff_ddpm_run(self.handle, B, _ptr(x), _ptr(noise), seed & (2 ** 64 - 1), sample_offset,
                                   t_start, t_end, int(init_prior), _ptr(clamp_flag), self._stream())
        _check(self.lib, rc, "dff_ddpm_run")

    # ---- the forward process and its loss
    def _levels(self, t, B):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and tuple(t.shape) == (B,)
                and not t.is_floating_point()):
            raise ValueError(f"t must be an integer CUDA tensor of shape ({B},) on cuda:{self.device}")
        return t.to(torch.int32).contiguous()

    def q_sample(self, x0, t, noise=None, seed: int = 0, sample_offset: int = 0, draw: int = 0, return_tnorm=False):
        """x_t = center_zero(sqrt_ac[t] x0 + sqrt_1mac[t] center_zero(z)) (dff_q_sample): z = `noise`, or in-kernel Philox
        draws keyed by (seed; sample_offset + b, FORWARD_STEP | draw).  t: integer levels (B,); NaN rows for a level
        outside 0 .. T - 1."""
        import torch
        B = x0.shape[0]
        self._dev_tensor(x0, (B, self.n_beads, 3), "x0")
        t32 = self._levels(t, B)
        if noise is not None:
            self._dev_tensor(noise, (B, self.n_beads, 3), "noise")
        xt = torch.empty_like(x0)
        tn = torch.empty(B, dtype=torch.float32, device=x0.device) if return_tnorm else None
        rc = self.lib.dff_q_sample(self.handle, _ptr(x0), _ptr(t32), B, _ptr(noise), seed & (2 ** 64 - 1), sample_offset,
                                   draw, _ptr(xt), _ptr(tn), self._stream())
        _check(self.lib, rc, "dff_q_sample")
        return (xt, tn) if return_tnorm else xt

    def denoise_workspace_bytes(self, batch: int) -> int:
        b = int(self.lib.dff_denoise_workspace_bytes(self.handle, int(batch)))
        if b < 0:
            _check(self.lib, 1, "dff_denoise_workspace_bytes")
        return b

    def denoise_loss(self, x0, t, noise=None, seed: int = 0, sample_offset: int = 0, draw: int = 0, loss_type="l2",
                     total=None, return_xt=False, return_model_out=False):
        """Per-sample denoising loss (dff_denoise_loss) -> float32 CUDA tensor (B,), or a tuple (loss[, x_t][, model_out]).
        `total`, a float64 CUDA tensor (2,), is added to on the device: (sum of the losses, B).  The workspace is
        allocated once and kept (it is bounded: one pass of the library's chunk size)."""
        import torch
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"invalid loss type {loss_type}")
        B = x0.shape[0]
        self._dev_tensor(x0, (B, self.n_beads, 3), "x0")
        t32 = self._levels(t, B)
        if noise is not None:
            self._dev_tensor(noise, (B, self.n_beads, 3), "noise")
        if total is not None and not (isinstance(total, torch.Tensor) and total.is_cuda and total.dtype == torch.float64
                                      and total.device.index == self.device and total.is_contiguous() and total.numel() == 2):
            raise ValueError("total must be a contiguous float64 CUDA tensor of 2 elements on the model's device")
        need = self.denoise_workspace_bytes(B)
        ws = getattr(self, "_loss_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._loss_ws = torch.empty(need, dtype=torch.uint8, device=x0.device)
        loss = torch.empty(B, dtype=torch.float32, device=x0.device)
        xt = torch.empty_like(x0) if return_xt else None
        out = torch.empty_like(x0) if return_model_out else None
        rc = self.lib.dff_denoise_loss(self.handle, _ptr(x0), _ptr(t32), B, _ptr(noise), seed & (2 ** 64 - 1), sample_offset,
                                       draw, LOSS_TYPES[loss_type], _ptr(loss), _ptr(total), _ptr(xt), _ptr(out), _ptr(ws),
                                       ws.numel(), self._stream())
        _check(self.lib, rc, "dff_denoise_loss")
        res = (loss,) + ((xt,) if return_xt else ()) + ((out,) if return_model_out else ())
        return res if len(res) > 1 else loss

    # ---- debugging
    PROFILE_STAGES = ("centre", "embed+ln1", "gemm_u", "gemm_qkv", "softmax", "pv+xrel", "gemm_wo", "gate1+ln2",
                      "gemm_w1+gelu", "gemm_w2", "gate2", "b_gate2", "b_gemm_w2T", "b_gemm_w1T", "b_ln2+gate1",
                      "b_gemm_woc+u", "b_reload+gemm_woT", "b_ds", "b_dx+dqkv", "b_gemm_qkvT", "b_ln1", "update",
                      "x22", "x23")

    def profile(self, enable: bool = True):
        _check(self.lib, self.lib.dff_debug_profile(self.handle, int(enable)), "dff_debug_profile")

    def profile_read(self) -> dict:
        out = np.zeros(24, np.uint64)
        _check(self.lib, self.lib.dff_debug_profile_read(self.handle, out.ctypes.data_as(C.c_void_p)), "dff_debug_profile_read")
        return {n: int(v) for n, v in zip(self.PROFILE_STAGES, out) if n != "-"}

    def debug_stash(self, b: int, layer: int, what: str) -> np.ndarray:
        N, H = self.n_beads, self.hidden
        items = dict(nodes_in=(0, (N, H)), attn_out=(1, (N, H)), ff=(2, (N, H)), h_pre=(3, (N, 4 * H)),
                     q=(4, (N, 512)), k=(5, (N, 512)), v=(6, (N, 512)), P=(7, (8, N, N)), u=(8, (N, 32)))
        code, shape = items[what]
        out = np.empty(shape, np.float32)
        rc = self.lib.dff_debug_stash(self.handle, b, layer, code, out.ctypes.data_as(C.c_void_p), out.size)
        _check(self.lib, rc, "dff_debug_stash")
        return out


def plan_launch(cfg: DffConfig, dispatch: dict, mode: int, batch: int) -> dict:
    """The launch plan of a call of `mode` (0 score, 1 Langevin, 2 DDPM) over `batch` proteins for a model of config `cfg`
    and dispatch `dispatch` (the fields of DffDispatch; missing ones are 0): dff_debug_plan_launch, host only, no GPU."""
    lib = load_library()
    plan = DffLaunchPlan()
    _check(lib, lib.dff_debug_plan_launch(C.byref(cfg), C.byref(DffDispatch(**dispatch)), int(mode), int(batch), C.byref(plan)),
           "dff_debug_plan_launch")
    return {n: v.decode() if isinstance(v, bytes) else v for n, v in ((n, getattr(plan, n)) for n, _ in DffLaunchPlan._fields_)}


def debug_gemm(A: np.ndarray, W: np.ndarray, device: int = 0) -> np.ndarray:
    lib = load_library()
    A = np.ascontiguousarray(A, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    M, K = A.shape
    K2, Nout = W.shape
    assert K == K2
    out = np.empty((M, Nout), np.float32)
    rc = lib.dff_debug_gemm(device, A.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p), M, K, Nout,
                            out.ctypes.data_as(C.c_void_p))
    _check(lib, rc, "dff_debug_gemm")
    return out


# ---- PWD histograms (dff_pwd_*): stateless entry points, no model handle ----
def _coords(x):
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and x.dim() == 3 and x.shape[-1] == 3):
        raise ValueError("structures must be a contiguous float32 CUDA tensor of shape (n, n_beads, 3)")
    return x, int(x.shape[0]), int(x.shape[1])


def _stream(x):
    import torch
    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _lengths(lengths):
    return np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))


def _workspace_bytes(name, *args):
    lib = load_library()
    b = int(getattr(lib, name)(*args))
    if b < 0:
        _check(lib, 1, name)
    return b


def _workspace(workspace, device, symbol, *args, always=True):
    """The workspace of a call: the caller's, or a new uint8 tensor of the bytes that the library's `symbol`(*args) asks for.
    always: the symbol is asked for a caller's workspace too (its refusal is then the call's first); else only to size a new one."""
    import torch
    if workspace is not None and not always:
        return workspace
    need = _workspace_bytes(symbol, *args)
    return workspace if workspace is not None else torch.empty(max(need, 8), dtype=torch.uint8, device=device)


def _nbytes(t) -> int:
    return int(t.numel() * t.element_size())


def _host_i32(values, count, name, what, per="problem", of="P"):
    """`values` as a contiguous host int32 array of exactly `count` entries: "`name` must hold one `what` per `per`" otherwise."""
    h = np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))
    if h.size != count:
        raise ValueError(f"{name} must hold one {what} per {per}: {h.size} for {of} = {count}")
    return h


def pwd_num_pairs(n_beads: int, offset: int) -> int:
    return int(load_library().dff_pwd_num_pairs(int(n_beads), int(offset)))


def pwd_max(x, offset: int):
    """Per-pair maximum distance over the structures x (n, N, 3) -> float32 CUDA tensor (n_pairs,)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    out = torch.empty(pwd_num_pairs(N, offset), dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_pwd_max(x.device.index, _ptr(x), n, N, int(offset), _ptr(out), _stream(x)), "dff_pwd_max")
    return out


def pwd_hist(x, offset: int, nbins, hmax, out=None):
    """Per-pair histograms (torch.histc semantics, min=0, max=hmax[p], bins=nbins[p]) of the
    pairwise distances of x (n, N, 3) -> int32 CUDA tensor (n_pairs, max(nbins)) of counts.  `out`: a contiguous int32 CUDA
    tensor (n_pairs, ld >= max(nbins)) on x's device, a slice of a larger one for instance, to write into instead (it is
    returned; columns from max(nbins) on are zeroed)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    npairs = pwd_num_pairs(N, offset)
    nb = torch.as_tensor(nbins, dtype=torch.int32).reshape(-1)
    hm = torch.as_tensor(hmax, dtype=torch.float32).reshape(-1)
    if nb.numel() != npairs or hm.numel() != npairs:
        raise ValueError(f"nbins / hmax must have {npairs} entries")
    if int(nb.min()) < 1:
        raise ValueError("nbins must be >= 1")
    if not bool((torch.isfinite(hm) & (hm > 0)).all()):
        raise ValueError("hmax must be finite and > 0")
    max_bins = int(nb.max())
    nb_d, hm_d = nb.to(x.device), hm.to(x.device)
    if out is None:
        out = torch.empty((npairs, max_bins), dtype=torch.int32, device=x.device)
    elif not (_is_tensor(out, torch.int32, dim=2) and out.shape[0] == npairs and out.shape[1] >= max_bins
              and out.device == x.device):
        raise ValueError(f"out must be a contiguous int32 CUDA tensor ({npairs}, >= {max_bins}) on the structures' device")
    _check(lib, lib.dff_pwd_hist(x.device.index, _ptr(x), n, N, int(offset), _ptr(nb_d), _ptr(hm_d), max_bins,
                                 int(out.shape[1]), _ptr(out), _stream(x)), "dff_pwd_hist")
    return out


PWD_MAX_BINS = 30719        # the largest max_bins dff_pwd_hist accepts (include/dff.h)


def pwd_hist_plan(n_beads: int, offset: int, max_bins: int, n: int) -> dict:
    """The launch layout dff_pwd_hist takes for n structures of n_beads beads and histograms of up to max_bins bins
    (the fields of dff_pwd_plan): dff_pwd_hist_plan, host only, no GPU.  ValueError where dff_pwd_hist refuses."""
    lib = load_library()
    plan = DffPwdPlan()
    _check(lib, lib.dff_pwd_hist_plan(int(n_beads), int(offset), int(max_bins), int(n), C.byref(plan)), "dff_pwd_hist_plan")
    return {f: int(getattr(plan, f)) for f, _ in DffPwdPlan._fields_}


# ---- structure metrics (dff_struct_*): stateless entry points, no model handle ----
def struct_rmsd(x, ref):
    """Optimal-rotation RMSD (Angstrom) of every frame of x (n, N, 3) to ref (N, 3) -> float32 CUDA tensor (n,);
    NaN for frames with a non-finite coordinate."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    r = torch.as_tensor(ref, dtype=torch.float32).reshape(N, 3).to(x.device).contiguous()
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_struct_rmsd(x.device.index, _ptr(x), n, N, _ptr(r), _ptr(out), _stream(x)), "dff_struct_rmsd")
    return out


def struct_dihedrals(x):
    """Dihedrals (radians) of the consecutive bead quadruples of x (n, N, 3) -> float32 CUDA tensor (n, N - 3)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    out = torch.empty((n, max(N - 3, 0)), dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_struct_dihedrals(x.device.index, _ptr(x), n, N, _ptr(out), _stream(x)), "dff_struct_dihedrals")
    return out


def struct_tic_num_features(n_beads: int) -> int:
    return int(load_library().dff_struct_tic_num_features(int(n_beads)))


def _tic_model(x, N, mean, coeff):
    """mean (F,) and coeff (F, k) of a TIC model for N-bead frames x, as contiguous float64 tensors on x's device, and k."""
    import torch
    F = struct_tic_num_features(N)
    m = torch.as_tensor(mean, dtype=torch.float64).to(x.device).contiguous()
    A = torch.as_tensor(coeff, dtype=torch.float64).to(x.device).contiguous()
    if m.shape != (F,) or A.dim() != 2 or A.shape[0] != F:
        raise ValueError(f"mean must be ({F},) and coeff ({F}, k) for {N} beads")
    return m, A, int(A.shape[1])


def struct_tic(x, mean, coeff):
    """TIC projection (feat - mean) @ coeff of the N - 3 dihedrals + N (N - 1) / 2 pair distances of every frame of
    x (n, N, 3); mean (F,), coeff (F, k) -> float64 CUDA tensor (n, k)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    m, A, k = _tic_model(x, N, mean, coeff)
    out = torch.empty((n, k), dtype=torch.float64, device=x.device)
    _check(lib, lib.dff_struct_tic(x.device.index, _ptr(x), n, N, _ptr(m), _ptr(A), k, _ptr(out), _stream(x)),
           "dff_struct_tic")
    return out


def struct_contacts(x, cutoff: float, folded=None, offset: int = 3):
    """Contacts d_ij < cutoff of the frames x (n, N, 3): (counts, mismatch) with counts an int64 CUDA tensor (N, N)
    summed over frames and mismatch, when the folded contact map (N, N) is given, an int64 CUDA tensor (n,) of pairs
    j >= i + offset whose contact differs from it (None otherwise)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    f = None
    if folded is not None:
        f = torch.as_tensor(folded).reshape(N, N).to(device=x.device, dtype=torch.uint8).contiguous()
    counts = torch.empty((N, N), dtype=torch.int32, device=x.device)
    mism = torch.empty(n, dtype=torch.int32, device=x.device) if f is not None else None
    _check(lib, lib.dff_struct_contacts(x.device.index, _ptr(x), n, N, float(cutoff), _ptr(f), int(offset),
                                        _ptr(counts), _ptr(mism), _stream(x)), "dff_struct_contacts")
    return counts.to(torch.int64), (mism.to(torch.int64) if mism is not None else None)


def struct_tic_features(x):
    """TIC features (N - 3 dihedrals, then the pair distances in triu_indices order) of every frame of x (n, N, 3)
    -> float32 CUDA tensor (n, F): get_tic_features, the values struct_tic projects."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    out = torch.empty((n, struct_tic_num_features(N)), dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_struct_tic_features(x.device.index, _ptr(x), n, N, _ptr(out), _stream(x)),
           "dff_struct_tic_features")
    return out


# ---- TICA moments (dff_tica_*) ----
def tica_workspace_bytes(n_beads: int, n_frames_max: int, lagtime: int) -> int:
    return _workspace_bytes("dff_tica_workspace_bytes", int(n_beads), int(n_frames_max), int(lagtime))


def tica_moments(x, lengths, lagtime: int, shift, sx, sy, m0, mt, workspace=None):
    """Add the lag-`lagtime` moments of the trajectories x (n, N, 3) (back to back, `lengths` frames each) to the
    float64 CUDA accumulators sx, sy (F,) and m0, mt (F, F) (upper triangles): dff_tica_moments.  g = features - shift
    (float64 (F,) CUDA).  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    F = struct_tic_num_features(N)
    for name, t, shape in (("shift", shift, (F,)), ("sx", sx, (F,)), ("sy", sy, (F,)), ("m0", m0, (F, F)),
                           ("mt", mt, (F, F))):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == x.device
                and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{name} must be a contiguous float64 tensor {shape} on {x.device}")
    ln = _lengths(lengths)
    workspace = _workspace(workspace, x.device, "dff_tica_workspace_bytes", N, n, int(lagtime), always=False)
    _check(lib, lib.dff_tica_moments(x.device.index, _ptr(x), n, N, ln.ctypes.data_as(C.c_void_p), int(ln.size),
                                     int(lagtime), _ptr(shift), _ptr(workspace),
                                     _nbytes(workspace), _ptr(sx),
                                     _ptr(sy), _ptr(m0), _ptr(mt), _stream(x)), "dff_tica_moments")
    return workspace


def tica_debug_plan(n_beads: int, lengths, lagtime: int, chunk_pairs: int = 0) -> np.ndarray:
    """The chunk plan of dff_tica_moments (host only): int64 (runs, 6) of (chunk, f0, rows, chunk pairs, run start - f0,
    run pairs)."""
    lib = load_library()
    ln = _lengths(lengths)
    cap = 1024
    while True:
        out = np.zeros((cap, 6), np.int64)
        k = lib.dff_tica_debug_plan(int(n_beads), ln.ctypes.data_as(C.c_void_p), int(ln.size), int(lagtime),
                                    int(chunk_pairs), out.ctypes.data_as(C.c_void_p), cap)
        if k < 0:
            _check(lib, 1, "dff_tica_debug_plan")
        if k <= cap:
            return out[:k]
        cap = k


# ---- states in TIC space and their transitions (dff_struct_tic_assign, dff_kmeans_*, dff_transition_counts) ----
def _centers(centers, d, device):
    import torch
    c = torch.as_tensor(centers, dtype=torch.float64).to(device).contiguous()
    if c.dim() != 2 or c.shape[1] != d:
        raise ValueError(f"centers must be (K, {d})")
    return c


def struct_tic_assign(x, mean, coeff, centers, return_proj=False, return_dist2=False):
    """State label of every frame of x (n, N, 3): the TIC projection of struct_tic (mean (F,), coeff (F, k)), then the
    nearest of centers (K, k) -> int32 CUDA tensor (n,), -1 for a frame with a non-finite projection.  With return_proj /
    return_dist2 a tuple (labels[, proj float64 (n, k)][, dist2 float64 (n,)])."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    m, A, k = _tic_model(x, N, mean, coeff)
    c = _centers(centers, k, x.device)
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    proj = torch.empty((n, k), dtype=torch.float64, device=x.device) if return_proj else None
    dist2 = torch.empty(n, dtype=torch.float64, device=x.device) if return_dist2 else None
    _check(lib, lib.dff_struct_tic_assign(x.device.index, _ptr(x), n, N, _ptr(m), _ptr(A), k, _ptr(c), int(c.shape[0]),
                                          _ptr(labels), _ptr(proj), _ptr(dist2), _stream(x)), "dff_struct_tic_assign")
    out = (labels,) + ((proj,) if return_proj else ()) + ((dist2,) if return_dist2 else ())
    return out if len(out) > 1 else labels


def kmeans_workspace_bytes(n: int, d: int, K: int) -> int:
    return _workspace_bytes("dff_kmeans_workspace_bytes", int(n), int(d), int(K))


def _is_tensor(t, dtype, shape=None, dim=None):
    """t is a contiguous CUDA tensor of `dtype`, of exactly `shape` or of `dim` dimensions."""
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and (shape is None or tuple(t.shape) == shape) and (dim is None or t.dim() == dim))


def _kmeans_step(symbol, bytes_symbol, points, centers, accumulate, workspace):
    import torch
    lib = load_library()
    if not _is_tensor(points, torch.float64, dim=2):
        raise ValueError("points must be a contiguous float64 CUDA tensor of shape (n, d)")
    n, d = int(points.shape[0]), int(points.shape[1])
    c = _centers(centers, d, points.device)
    K = int(c.shape[0])
    out = {"labels": torch.empty(n, dtype=torch.int32, device=points.device),
           "dist2": torch.empty(n, dtype=torch.float64, device=points.device)}
    ws_bytes = 0
    if accumulate:
        workspace = _workspace(workspace, points.device, bytes_symbol, n, d, K)   # refuses a bad d or K before anything is allocated
        out["sums"] = torch.empty((K, d), dtype=torch.float64, device=points.device)
        out["counts"] = torch.empty(K, dtype=torch.int64, device=points.device)
        out["inertia"] = torch.empty(1, dtype=torch.float64, device=points.device)
        ws_bytes = _nbytes(workspace)
    else:
        workspace = None
    _check(lib, getattr(lib, symbol)(points.device.index, _ptr(points), n, d, _ptr(c), K, _ptr(out["labels"]),
                                     _ptr(out["dist2"]), _ptr(out.get("sums")), _ptr(out.get("counts")),
                                     _ptr(out.get("inertia")), _ptr(workspace), ws_bytes, _stream(points)), symbol)
    return out


def kmeans_step(points, centers, accumulate=True, workspace=None):
    """One Lloyd step over points (n, d) (contiguous float64 CUDA) with centers (K, d): a dict of labels int32 (n,),
    dist2 float64 (n,) and, with `accumulate`, sums float64 (K, d), counts int64 (K,), inertia float64 (1,) over the
    finite points (dff_kmeans_step: deterministic).  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    return _kmeans_step("dff_kmeans_step", "dff_kmeans_workspace_bytes", points, centers, accumulate, workspace)


def _transition_counts(symbol, labels, lengths, lagtimes, n_states):
    import torch
    lib = load_library()
    if not _is_tensor(labels, torch.int32, dim=1):
        raise ValueError("labels must be a contiguous int32 CUDA tensor of shape (n,)")
    ln = _lengths(lengths)
    lg = np.ascontiguousarray(np.asarray(lagtimes, dtype=np.int32).reshape(-1))
    K = int(n_states)
    Ka = min(max(K, 1), MSM_MAX_STATES)                          # what is allocated when K itself will be refused
    out = torch.empty((min(max(int(lg.size), 1), MSM_MAX_LAGS), Ka, Ka), dtype=torch.int64, device=labels.device)
    _check(lib, getattr(lib, symbol)(labels.device.index, _ptr(labels), int(labels.numel()), ln.ctypes.data_as(C.c_void_p),
                                     int(ln.size), lg.ctypes.data_as(C.c_void_p), int(lg.size), K, _ptr(out),
                                     _stream(labels)), symbol)
    return out


def transition_counts(labels, lengths, lagtimes, n_states: int):
    """Sliding-window transition counts of the int32 CUDA labels (n,) -- trajectories back to back, `lengths` frames
    each -- at every lag time of `lagtimes` -> int64 CUDA tensor (n_lags, K, K); pairs with a label outside 0 .. K - 1
    are skipped (dff_transition_counts)."""
    return _transition_counts("dff_transition_counts", labels, lengths, lagtimes, n_states)


# ---- RMSD between two ensembles (dff_rmsd_nearest, dff_rmsd_matrix) ----
def _two_ensembles(x, y):
    x, n, N = _coords(x)
    y, m, Ny = _coords(y)
    if y.device != x.device:
        raise ValueError(f"queries are on {x.device}, candidates on {y.device}")
    if Ny != N:
        raise ValueError(f"queries have {N} beads, candidates {Ny}")
    return x, n, y, m, N


def rmsd_nearest_workspace_bytes(n: int, m: int, n_beads: int) -> int:
    return _workspace_bytes("dff_rmsd_nearest_workspace_bytes", int(n), int(m), int(n_beads))


def rmsd_nearest(x, y, self_first: int = -1, workspace=None):
    """For every frame of x (n, N, 3) the RMSD (Angstrom, optimal proper rotation) to its nearest frame of y (m, N, 3)
    and that frame's index -> (float32 CUDA tensor (n,), int64 CUDA tensor (n,)); NaN / -1 for a query with a non-finite
    coordinate or without a usable candidate; the lowest index among equal RMSDs.  self_first >= 0: query s is candidate
    self_first + s, and that pair is skipped.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    x, n, y, m, N = _two_ensembles(x, y)
    workspace = _workspace(workspace, x.device, "dff_rmsd_nearest_workspace_bytes", n, m, N)
    rmsd = torch.empty(n, dtype=torch.float32, device=x.device)
    index = torch.empty(n, dtype=torch.int64, device=x.device)
    _check(lib, lib.dff_rmsd_nearest(x.device.index, _ptr(x), n, _ptr(y), m, N, int(self_first), _ptr(rmsd), _ptr(index),
                                     _ptr(workspace), _nbytes(workspace), _stream(x)),
           "dff_rmsd_nearest")
    return rmsd, index


def rmsd_matrix(x, y):
    """RMSD (Angstrom, optimal proper rotation) of every frame of x (n, N, 3) to every frame of y (m, N, 3) -> float32
    CUDA tensor (n, m), NaN where either frame has a non-finite coordinate.  n * m <= 2^28."""
    import torch
    lib = load_library()
    x, n, y, m, N = _two_ensembles(x, y)
    out = torch.empty((n, m), dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_rmsd_matrix(x.device.index, _ptr(x), n, _ptr(y), m, N, _ptr(out), _stream(x)), "dff_rmsd_matrix")
    return out


# ---- superposition on a reference (dff_superpose) ----
def superpose_workspace_bytes(n: int, n_beads: int) -> int:
    return _workspace_bytes("dff_superpose_workspace_bytes", int(n), int(n_beads))


def superpose(x, ref, aligned=True, rot=False, rmsd=False, stats=False, out=None, workspace=None):
    """Optimal proper rotation of every frame of x (n, N, 3) onto ref (N, 3) (dff_superpose) -> a dict of CUDA tensors with the
    outputs asked for: "aligned" float32 (n, N, 3), the frames rotated and moved onto ref's centroid (written to `out` when
    given; out = x aligns in place); "rot" float64 (n, 3, 3); "rmsd" float32 (n,); with `stats` "dsum" float64 (N, 3),
    "dsq" float64 (N,) and "count" int64 (1,) over the finite frames, d = aligned - ref in float64.  NaN rows for a frame
    with a non-finite coordinate.  Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    r = torch.as_tensor(ref, dtype=torch.float32).reshape(N, 3).to(x.device).contiguous()
    res = {}
    if out is not None:
        o, no, No = _coords(out)
        if (no, No) != (n, N) or o.device != x.device:
            raise ValueError(f"out must be a ({n}, {N}, 3) tensor on {x.device}")
        res["aligned"] = o
    elif aligned:
        res["aligned"] = torch.empty_like(x)
    if rot:
        res["rot"] = torch.empty((n, 3, 3), dtype=torch.float64, device=x.device)
    if rmsd:
        res["rmsd"] = torch.empty(n, dtype=torch.float32, device=x.device)
    ws_bytes = 0
    if stats:
        res["dsum"] = torch.empty((N, 3), dtype=torch.float64, device=x.device)
        res["dsq"] = torch.empty(N, dtype=torch.float64, device=x.device)
        res["count"] = torch.empty(1, dtype=torch.int64, device=x.device)
        workspace = _workspace(workspace, x.device, "dff_superpose_workspace_bytes", n, N, always=False)
        ws_bytes = _nbytes(workspace)
    else:
        workspace = None
    _check(lib, lib.dff_superpose(x.device.index, _ptr(x), n, N, _ptr(r), _ptr(res.get("aligned")), _ptr(res.get("rot")),
                                  _ptr(res.get("rmsd")), _ptr(res.get("dsum")), _ptr(res.get("dsq")), _ptr(res.get("count")),
                                  _ptr(workspace), ws_bytes, _stream(x)), "dff_superpose")
    return res


# ---- clustering under the RMSD with a cutoff (dff_rmsd_neighbors, dff_gromos_*) ----
CLUSTER_MAX_FRAMES = 1 << 18


def rmsd_neighbors(x, cutoff: float, degree=True):
    """The neighbour bit-matrix of the frames x (n, N, 3) against themselves (dff_rmsd_neighbors) -> (adj, degree): adj an
    int64 CUDA tensor (n, ceil(n / 64)) whose bit r & 63 of word [s, r >> 6] says RMSD(s, r) <= cutoff (the diagonal bit:
    the frame is finite), degree an int32 CUDA tensor (n,) of row popcounts (None with degree=False).  Nothing is read back."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    adj = torch.empty((n, (n + 63) // 64), dtype=torch.int64, device=x.device)
    deg = torch.empty(n, dtype=torch.int32, device=x.device) if degree else None
    _check(lib, lib.dff_rmsd_neighbors(x.device.index, _ptr(x), n, N, float(cutoff), _ptr(adj), _ptr(deg), _stream(x)),
           "dff_rmsd_neighbors")
    return adj, deg


def gromos_workspace_bytes(n: int) -> int:
    return _workspace_bytes("dff_gromos_workspace_bytes", int(n))


def gromos_state(adj, max_clusters: int):
    """Fresh buffers of a greedy loop on the bit-matrix adj (n, ceil(n / 64)) int64 CUDA: a dict of labels (n,), centers
    and sizes (min(max_clusters, n),), progress (2,), all int32, and the workspace; the first gromos_steps call on it restarts."""
    import torch
    n = int(adj.shape[0])
    k = max(min(int(max_clusters), n), 1)
    i32 = dict(dtype=torch.int32, device=adj.device)
    return {"labels": torch.empty(n, **i32), "centers": torch.empty(k, **i32), "sizes": torch.empty(k, **i32),
            "progress": torch.empty(2, **i32), "max_clusters": int(max_clusters), "fresh": True,
            "workspace": torch.empty(gromos_workspace_bytes(n), dtype=torch.uint8, device=adj.device)}


def gromos_steps(adj, state, n_steps: int, restart=None):
    """Enqueue n_steps iterations of the greedy loop (dff_gromos_steps) on `state` (gromos_state); restart=None restarts a
    fresh state only.  Nothing is read back: state["progress"] holds (clusters, frames left) on the device."""
    import torch
    lib = load_library()
    if not (isinstance(adj, torch.Tensor) and adj.is_cuda and adj.dtype == torch.int64 and adj.is_contiguous()
            and adj.dim() == 2 and adj.shape[1] == (adj.shape[0] + 63) // 64):
        raise ValueError("adj must be a contiguous int64 CUDA tensor of shape (n, ceil(n / 64))")
    n = int(adj.shape[0])
    if int(state["labels"].numel()) != n:
        raise ValueError(f"the state is for {int(state['labels'].numel())} frames, adj has {n}")
    restart = state["fresh"] if restart is None else bool(restart)
    ws = state["workspace"]
    _check(lib, lib.dff_gromos_steps(adj.device.index, _ptr(adj), n, int(restart), int(n_steps), int(state["max_clusters"]),
                                     _ptr(state["labels"]), _ptr(state["centers"]), _ptr(state["sizes"]),
                                     _ptr(state["progress"]), _ptr(ws), int(ws.numel()), _stream(adj)), "dff_gromos_steps")
    state["fresh"] = False
    return state


# ---- folding kinetics (dff_struct_native_q, dff_core_states, dff_label_runs) ----
def struct_native_q(x, pairs, r0, beta: float = 5.0, lam: float = 1.2):
    """Soft fraction of native contacts of every frame of x (n, N, 3): the mean over the pairs (i, j) of `pairs` (P, 2) of
    1 / (1 + exp(beta (r_ij - lam r0))) with the native distances r0 (P,), in float64, rounded once -> float32 CUDA tensor
    (n,).  NaN for a frame with a non-finite coordinate -- and for EVERY frame when a pair has an index outside 0 .. N - 1
    or i == j (detected on the device: nothing is read back)."""
    import torch
    lib = load_library()
    x, n, N = _coords(x)
    p = torch.as_tensor(pairs).to(device=x.device, dtype=torch.int32).contiguous()
    r = torch.as_tensor(r0).to(device=x.device, dtype=torch.float32).contiguous()
    if p.dim() != 2 or p.shape[1] != 2 or r.shape != (p.shape[0],):
        raise ValueError("pairs must be (P, 2) and r0 (P,)")
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    _check(lib, lib.dff_struct_native_q(x.device.index, _ptr(x), n, N, _ptr(p), _ptr(r), int(p.shape[0]), float(beta),
                                        float(lam), _ptr(out), _stream(x)), "dff_struct_native_q")
    return out


def kinetics_workspace_bytes(n: int) -> int:
    return _workspace_bytes("dff_kinetics_workspace_bytes", int(n))


def _kinetics_workspace(t, workspace):
    workspace = _workspace(workspace, t.device, "dff_kinetics_workspace_bytes", int(t.numel()), always=False)
    return workspace, _nbytes(workspace)


def core_states(cv, lengths, lo: float, hi: float, return_core=False, workspace=None):
    """Dual-cutoff state of every frame of the float32 CUDA series cv (n,) -- trajectories back to back, `lengths` frames
    each: 0 from a frame with cv <= lo on, 1 from one with cv >= hi on, -1 before the first core visit of a trajectory
    and at a non-finite frame (which resets the history) -> int32 CUDA tensor (n,); with return_core also the int8 tensor
    (n,) that is 0 / 1 inside a core and -1 elsewhere (dff_core_states).  `workspace` is a uint8 CUDA tensor (allocated
    here when None)."""
    import torch
    lib = load_library()
    if not (isinstance(cv, torch.Tensor) and cv.is_cuda and cv.dtype == torch.float32 and cv.is_contiguous()
            and cv.dim() == 1):
        raise ValueError("cv must be a contiguous float32 CUDA tensor of shape (n,)")
    ln = _lengths(lengths)
    n = int(cv.numel())
    labels = torch.empty(n, dtype=torch.int32, device=cv.device)
    core = torch.empty(n, dtype=torch.int8, device=cv.device) if return_core else None
    workspace, ws_bytes = _kinetics_workspace(cv, workspace)
    _check(lib, lib.dff_core_states(cv.device.index, _ptr(cv), n, ln.ctypes.data_as(C.c_void_p), int(ln.size), float(lo),
                                    float(hi), _ptr(labels), _ptr(core), _ptr(workspace), ws_bytes, _stream(cv)),
           "dff_core_states")
    return (labels, core) if return_core else labels


def label_runs(labels, lengths, max_runs=None, workspace=None):
    """Runs of equal labels inside the trajectories of the int32 CUDA labels (n,) (back to back, `lengths` frames each):
    a dict of CUDA tensors start int64, length int64, label int32, flags uint8 (bit 0: the run begins at its trajectory's
    first frame, bit 1: it ends at its last), each (max_runs,) with the first n_runs entries written, and n_runs int64
    (1,), the true number of runs (dff_label_runs).  max_runs defaults to n, which every run fits.  Nothing is read back."""
    import torch
    lib = load_library()
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32
            and labels.is_contiguous() and labels.dim() == 1):
        raise ValueError("labels must be a contiguous int32 CUDA tensor of shape (n,)")
    ln = _lengths(lengths)
    n = int(labels.numel())
    m = n if max_runs is None else int(max_runs)
    dev = labels.device
    out = {"start": torch.empty(max(m, 0), dtype=torch.int64, device=dev),
           "length": torch.empty(max(m, 0), dtype=torch.int64, device=dev),
           "label": torch.empty(max(m, 0), dtype=torch.int32, device=dev),
           "flags": torch.empty(max(m, 0), dtype=torch.uint8, device=dev),
           "n_runs": torch.empty(1, dtype=torch.int64, device=dev)}
    workspace, ws_bytes = _kinetics_workspace(labels, workspace)
    _check(lib, lib.dff_label_runs(dev.index, _ptr(labels), n, ln.ctypes.data_as(C.c_void_p), int(ln.size), m,
                                   _ptr(out["start"]), _ptr(out["length"]), _ptr(out["label"]), _ptr(out["flags"]),
                                   _ptr(out["n_runs"]), _ptr(workspace), ws_bytes, _stream(labels)), "dff_label_runs")
    return out


# ---- transition paths (dff_path_states) ----
def path_states_workspace_bytes(n: int) -> int:
    return _workspace_bytes("dff_path_states_workspace_bytes", int(n))


def path_states(cv, lengths, lo: float, hi: float, frames=True, times=True, paths=True, max_paths=None, workspace=None):
    """The previous and the next core of every frame of the float32 CUDA series cv (n,) -- trajectories back to back,
    `lengths` frames each, cores cv <= lo (0) and cv >= hi (1) as in core_states -- and the transition paths between the cores
    (dff_path_states).  A dict of CUDA tensors:
    frames: prev, next, cls int8 (n,) -- the last / next core visited (-1: none inside the trajectory, or a non-finite frame
            in between) and the class of the frame: 0 / 1 in a core, 2 / 3 on a path 0 -> 1 / 1 -> 0, 4 / 5 on a loop out of
            core 0 / 1 and back, -1 undetermined;
    times:  t_prev, t_next int64 (n,) -- the frames of those visits (-1 with prev / next = -1);
    paths:  exit, entry int64 and direction int8 (1: 0 -> 1), each (max_paths,) with the first n_paths records written in
            ascending entry, and n_paths int64 (1,), the true number of paths.  max_paths defaults to n, which every path fits.
    Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    if not (isinstance(cv, torch.Tensor) and cv.is_cuda and cv.dtype == torch.float32 and cv.is_contiguous()
            and cv.dim() == 1):
        raise ValueError("cv must be a contiguous float32 CUDA tensor of shape (n,)")
    ln = _lengths(lengths)
    n = int(cv.numel())
    m = n if max_paths is None else int(max_paths)
    dev = cv.device
    out = {}
    if frames:
        out.update({k: torch.empty(n, dtype=torch.int8, device=dev) for k in ("prev", "next", "cls")})
    if times:
        out.update({k: torch.empty(n, dtype=torch.int64, device=dev) for k in ("t_prev", "t_next")})
    if paths:
        out.update({"exit": torch.empty(max(m, 0), dtype=torch.int64, device=dev),
                    "entry": torch.empty(max(m, 0), dtype=torch.int64, device=dev),
                    "direction": torch.empty(max(m, 0), dtype=torch.int8, device=dev),
                    "n_paths": torch.empty(1, dtype=torch.int64, device=dev)})
    workspace = _workspace(workspace, dev, "dff_path_states_workspace_bytes", n, always=False)
    _check(lib, lib.dff_path_states(dev.index, _ptr(cv), n, ln.ctypes.data_as(C.c_void_p), int(ln.size), float(lo), float(hi),
                                    _ptr(out.get("prev")), _ptr(out.get("next")), _ptr(out.get("t_prev")),
                                    _ptr(out.get("t_next")), _ptr(out.get("cls")), m, _ptr(out.get("exit")),
                                    _ptr(out.get("entry")), _ptr(out.get("direction")), _ptr(out.get("n_paths")),
                                    _ptr(workspace), _nbytes(workspace), _stream(cv)), "dff_path_states")
    return out


# ---- lagged products inside trajectories (dff_autocorr) ----
AUTOCORR_MAX_D = 8
AUTOCORR_MAX_LAG = 65535


def autocorr_workspace_bytes(n: int, d: int, max_lag: int) -> int:
    return _workspace_bytes("dff_autocorr_workspace_bytes", int(n), int(d), int(max_lag))


def autocorr(series, lengths, max_lag: int, shift=None, sx=True, sy=True, count=True, workspace=None):
    """Lagged sums of the contiguous float64 CUDA series (n, d) -- trajectories back to back, `lengths` frames each -- for
    the lags 0 .. max_lag over the pairs (t, t + l) of one trajectory whose two frames are finite, g = series - shift
    (float64 CUDA (d,), None = 0): a dict of CUDA tensors "sxy" float64 (max_lag + 1, d) = sum g_t g_{t+l} and, as asked
    for, "sx" = sum g_t, "sy" = sum g_{t+l} (same shape) and "count" int64 (max_lag + 1,) (dff_autocorr: deterministic).
    Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    if not (isinstance(series, torch.Tensor) and series.is_cuda and series.dtype == torch.float64
            and series.is_contiguous() and series.dim() == 2):
        raise ValueError("series must be a contiguous float64 CUDA tensor of shape (n, d)")
    n, d, L = int(series.shape[0]), int(series.shape[1]), int(max_lag)
    if shift is not None and not (isinstance(shift, torch.Tensor) and shift.dtype == torch.float64 and shift.device == series.device
                                  and shift.is_contiguous() and tuple(shift.shape) == (d,)):
        raise ValueError(f"shift must be a contiguous float64 tensor ({d},) on {series.device}")
    ln = _lengths(lengths)
    workspace = _workspace(workspace, series.device, "dff_autocorr_workspace_bytes", n, d, L)   # refuses a bad d or max_lag first
    f64 = dict(dtype=torch.float64, device=series.device)
    out = {"sxy": torch.empty((L + 1, d), **f64)}
    if sx:
        out["sx"] = torch.empty((L + 1, d), **f64)
    if sy:
        out["sy"] = torch.empty((L + 1, d), **f64)
    if count:
        out["count"] = torch.empty(L + 1, dtype=torch.int64, device=series.device)
    _check(lib, lib.dff_autocorr(series.device.index, _ptr(series), n, d, ln.ctypes.data_as(C.c_void_p), int(ln.size), L,
                                 _ptr(shift), _ptr(out["sxy"]), _ptr(out.get("sx")), _ptr(out.get("sy")),
                                 _ptr(out.get("count")), _ptr(workspace), _nbytes(workspace),
                                 _stream(series)), "dff_autocorr")
    return out


# ---- Markov state models at microstate resolution (dff_micro_*, dff_msm_*) ----
MSM_MAX_STATES = 1024
MSM_MAX_LAGS = 8


def __getattr__(name):
    if name == "MICRO_CHUNK":               # points per workgroup of dff_micro_kmeans_step, read from the library
        return int(load_library().dff_micro_chunk())
    raise AttributeError(name)


def micro_kmeans_workspace_bytes(n: int, d: int, K: int) -> int:
    return _workspace_bytes("dff_micro_kmeans_workspace_bytes", int(n), int(d), int(K))


def micro_kmeans_step(points, centers, accumulate=True, workspace=None):
    """kmeans_step for up to MSM_MAX_STATES centres (dff_micro_kmeans_step): the same arguments and the same dict --
    labels int32 (n,), dist2 float64 (n,) and, with `accumulate`, sums float64 (K, d), counts int64 (K,), inertia float64
    (1,) over the finite points.  Labels and dist2 are kmeans_step's bits for K <= 64; the sums are taken in another
    (fixed) order.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    return _kmeans_step("dff_micro_kmeans_step", "dff_micro_kmeans_workspace_bytes", points, centers, accumulate, workspace)


def micro_transition_counts(labels, lengths, lagtimes, n_states: int):
    """transition_counts for up to MSM_MAX_STATES states and up to MSM_MAX_LAGS lag times (dff_micro_transition_counts) ->
    int64 CUDA tensor (n_lags, K, K); exact, and equal to transition_counts' result for K <= 64."""
    return _transition_counts("dff_micro_transition_counts", labels, lengths, lagtimes, n_states)


def msm_workspace_bytes(K: int) -> int:
    return _workspace_bytes("dff_msm_workspace_bytes", int(K))


def msm_reversible_steps(sym, rowc, x, n_steps: int, err=True, workspace=None):
    """Enqueue n_steps sweeps x_i' = sum_j S_ij / (c_i / x_i + c_j / x_j) of the reversible maximum-likelihood estimator
    (dff_msm_reversible_steps) on sym (K, K), rowc (K,) and x (K,), contiguous float64 CUDA tensors; x is updated in
    place.  Returns the float64 CUDA tensor (n_steps,) of err_s = max_i |x_i' - x_i| / x_i (None with err=False).  Nothing
    is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    K = int(x.shape[0]) if isinstance(x, torch.Tensor) and x.dim() == 1 else -1
    f64 = torch.float64
    if not (_is_tensor(x, f64, (K,)) and _is_tensor(sym, f64, (K, K)) and _is_tensor(rowc, f64, (K,))
            and sym.device == x.device and rowc.device == x.device):
        raise ValueError("sym (K, K), rowc (K,) and x (K,) must be contiguous float64 CUDA tensors on one device")
    n_steps = int(n_steps)
    workspace = _workspace(workspace, x.device, "dff_msm_workspace_bytes", K)
    e = torch.empty(max(n_steps, 0), dtype=torch.float64, device=x.device) if err else None
    _check(lib, lib.dff_msm_reversible_steps(x.device.index, _ptr(sym), _ptr(rowc), K, _ptr(x), n_steps, _ptr(e),
                                             _ptr(workspace), _nbytes(workspace),
                                             _stream(x)), "dff_msm_reversible_steps")
    return e


def debug_msm_driver(driver: int):
    """Benchmarks only: 0 = the library's choice by K, 1 = one launch per sweep, 2 = one workgroup for all sweeps."""
    lib = load_library()
    _check(lib, lib.dff_debug_msm_driver(int(driver)), "dff_debug_msm_driver")


def msm_driver_for(K: int) -> int:
    """The driver msm_reversible_steps would take for K states now: 1 = one launch per sweep, 2 = one workgroup."""
    lib = load_library()
    r = int(lib.dff_msm_driver_for(int(K)))
    if r < 0:
        _check(lib, 1, "dff_msm_driver_for")
    return r


# ---- bootstrap of a Markov state model (dff_micro_resampled_counts, dff_msm_reversible_steps_batched) ----
MSM_MAX_BATCH = 4096


def micro_resampled_counts_workspace_bytes(n_traj: int, n_units: int) -> int:
    return _workspace_bytes("dff_micro_resampled_counts_workspace_bytes", int(n_traj), int(n_units))


def micro_resampled_counts(labels, lengths, unit_lengths, lag: int, K: int, weights, workspace=None):
    """The count matrices of B weighted resamples in one pass over the labels (dff_micro_resampled_counts): labels int32
    CUDA (n,), lengths the trajectories, unit_lengths the resampling units (both host, each summing to n), weights uint32
    CUDA (B, n_units) -> uint64 CUDA tensor (B, K, K).  Exact.  `workspace` is a uint8 CUDA tensor (allocated here when
    None)."""
    import torch
    lib = load_library()
    if not _is_tensor(labels, torch.int32, dim=1):
        raise ValueError("labels must be a contiguous int32 CUDA tensor of shape (n,)")
    ln, un = _lengths(lengths), _lengths(unit_lengths)
    if not (_is_tensor(weights, torch.uint32, dim=2) and weights.shape[1] == un.size and weights.device == labels.device):
        raise ValueError("weights must be a contiguous uint32 CUDA tensor of shape (B, n_units) on the labels' device")
    K, B = int(K), int(weights.shape[0])
    workspace = _workspace(workspace, labels.device, "dff_micro_resampled_counts_workspace_bytes", int(ln.size), int(un.size))
    Ka = min(max(K, 1), MSM_MAX_STATES)                          # what is allocated when K or B will be refused
    Ba = min(max(B, 1), max((1 << 28) // (Ka * Ka), 1), MSM_MAX_BATCH)
    out = torch.empty((Ba, Ka, Ka), dtype=torch.uint64, device=labels.device)
    _check(lib, lib.dff_micro_resampled_counts(labels.device.index, _ptr(labels), int(labels.numel()),
                                               ln.ctypes.data_as(C.c_void_p), int(ln.size), un.ctypes.data_as(C.c_void_p),
                                               int(un.size), int(lag), K, _ptr(weights), B, _ptr(out), _ptr(workspace),
                                               _nbytes(workspace), _stream(labels)),
           "dff_micro_resampled_counts")
    return out


def msm_batched_workspace_bytes(B: int, Kmax: int) -> int:
    return _workspace_bytes("dff_msm_batched_workspace_bytes", int(B), int(Kmax))


def msm_reversible_steps_batched(S, c, ks, x, n_steps: int, skip=None, workspace=None):
    """msm_reversible_steps on B problems at once (dff_msm_reversible_steps_batched): S (B, Kmax, Kmax), c (B, Kmax) and
    x (B, Kmax) contiguous float64 CUDA tensors, problem b a COMPACT (ks[b], ks[b]) matrix at the start of its slot of S and
    the first ks[b] entries of its slots of c and x; ks (B,) host integers; skip (B,) host booleans or None.  x is updated
    in place; returns the float64 CUDA tensor (n_steps, B) of the sweeps' err (0 for a skipped problem).  Bit for bit the
    single call's x and err, problem by problem.  Nothing is read back."""
    import torch
    lib = load_library()
    B, Kmax = (int(x.shape[0]), int(x.shape[1])) if isinstance(x, torch.Tensor) and x.dim() == 2 else (-1, -1)
    f64 = torch.float64
    if not (_is_tensor(x, f64, (B, Kmax)) and _is_tensor(S, f64, (B, Kmax, Kmax)) and _is_tensor(c, f64, (B, Kmax))
            and S.device == x.device and c.device == x.device):
        raise ValueError("S (B, Kmax, Kmax), c (B, Kmax) and x (B, Kmax) must be contiguous float64 CUDA tensors on one device")
    kh = _host_i32(ks, B, "ks", "state count", of="B")
    sh = None
    if skip is not None:
        sh = np.ascontiguousarray(np.asarray(skip).reshape(-1) != 0).astype(np.uint8)
        if sh.size != B:
            raise ValueError(f"skip must hold one flag per problem: {sh.size} for B = {B}")
    n_steps = int(n_steps)
    workspace = _workspace(workspace, x.device, "dff_msm_batched_workspace_bytes", B, Kmax)
    e = torch.empty((max(n_steps, 0), B), dtype=torch.float64, device=x.device)
    _check(lib, lib.dff_msm_reversible_steps_batched(x.device.index, _ptr(S), _ptr(c), kh.ctypes.data_as(C.c_void_p),
                                                     sh.ctypes.data_as(C.c_void_p) if sh is not None else None, B, Kmax,
                                                     _ptr(x), n_steps, _ptr(e), _ptr(workspace),
                                                     _nbytes(workspace), _stream(x)),
           "dff_msm_reversible_steps_batched")
    return e


def msm_batched_driver_for(B: int, Kmax: int) -> int:
    """The driver msm_reversible_steps_batched would take now for B live problems, the largest of Kmax states: 1 = one launch
    per sweep, 2 = one looping workgroup per problem."""
    lib = load_library()
    r = int(lib.dff_msm_batched_driver_for(int(B), int(Kmax)))
    if r < 0:
        _check(lib, 1, "dff_msm_batched_driver_for")
    return r


# ---- mean first-passage times and committors: the Dirichlet problem on a flux matrix (dff_msm_dirichlet_solve) ----
MSM_DIRICHLET_MAX_BATCH = 16384


def msm_dirichlet_workspace_bytes(P: int, Kmax: int) -> int:
    return _workspace_bytes("dff_msm_dirichlet_workspace_bytes", int(P), int(Kmax))


def msm_dirichlet_lds_limit() -> int:
    """The largest interior count dff_msm_dirichlet_solve factors out of LDS, read from the library."""
    return int(load_library().dff_msm_dirichlet_lds_limit())


def debug_msm_dirichlet_path(path: int):
    """Tests and benchmarks only: 0 = by the interior count, 1 = every problem in LDS, 2 = every problem on the blocked path."""
    lib = load_library()
    _check(lib, lib.dff_debug_msm_dirichlet_path(int(path)), "dff_debug_msm_dirichlet_path")


def msm_dirichlet_solve(flux, ks, role, g, s, flux_of=None, u=None, workspace=None):
    """P Dirichlet problems on flux matrices in one call (dff_msm_dirichlet_solve): flux (M, Kmax, Kmax) contiguous float64
    CUDA, matrix m a COMPACT (K, K) matrix at the start of its slot; ks (P,) host integers; role int32, g and s float64, each
    (P, Kmax) contiguous CUDA with problem p in the first ks[p] entries of its row; flux_of (P,) host integers, the matrix of
    each problem (None: problem p reads matrix p).  Returns (u float64 (P, Kmax), status int32 (P,)), CUDA tensors: u holds
    g on the boundary and the solution on the interior, NaN over a failed problem; beyond ks[p] a row of u is left alone (NaN
    when u is allocated here).  status: 0 solved, -1 no boundary state, -2 a bad role, 1 + i the pivot of state i failed.
    Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    P, Kmax = (int(role.shape[0]), int(role.shape[1])) if isinstance(role, torch.Tensor) and role.dim() == 2 else (-1, -1)
    M = int(flux.shape[0]) if isinstance(flux, torch.Tensor) and flux.dim() == 3 else -1
    f64 = torch.float64
    if not (_is_tensor(role, torch.int32, (P, Kmax)) and _is_tensor(flux, f64, (M, Kmax, Kmax)) and _is_tensor(g, f64, (P, Kmax))
            and _is_tensor(s, f64, (P, Kmax)) and flux.device == role.device and g.device == role.device
            and s.device == role.device):
        raise ValueError("flux (M, Kmax, Kmax), g and s (P, Kmax) must be contiguous float64 and role (P, Kmax) contiguous int32 "
                         "CUDA tensors on one device")
    kh = _host_i32(ks, P, "ks", "state count")
    fh = _host_i32(flux_of, P, "flux_of", "matrix index") if flux_of is not None else None
    if u is None:
        u = torch.full((P, Kmax), float("nan"), dtype=f64, device=role.device)
    elif not (_is_tensor(u, f64, (P, Kmax)) and u.device == role.device):
        raise ValueError("u must be a contiguous float64 CUDA tensor of shape (P, Kmax) on the roles' device")
    status = torch.empty(P, dtype=torch.int32, device=role.device)
    workspace = _workspace(workspace, role.device, "dff_msm_dirichlet_workspace_bytes", P, Kmax, always=False)
    _check(lib, lib.dff_msm_dirichlet_solve(role.device.index, _ptr(flux), M, fh.ctypes.data_as(C.c_void_p) if fh is not None else None,
                                            kh.ctypes.data_as(C.c_void_p), P, Kmax, _ptr(role), _ptr(g), _ptr(s), _ptr(u),
                                            _ptr(status), _ptr(workspace), _nbytes(workspace),
                                            _stream(role)), "dff_msm_dirichlet_solve")
    return u, status


# ---- the k largest eigenpairs of many symmetric matrices (dff_sym_eig_topk) ----
SYM_EIG_MAX_BATCH = 16384
SYM_EIG_MAX_K = 32


def sym_eig_workspace_bytes(P: int, Kmax: int) -> int:
    return _workspace_bytes("dff_sym_eig_workspace_bytes", int(P), int(Kmax))


def sym_eig_lds_limit() -> int:
    """The largest matrix dff_sym_eig_topk reduces out of LDS, read from the library."""
    return int(load_library().dff_sym_eig_lds_limit())


def debug_sym_eig_path(path: int):
    """Tests and benchmarks only: 0 = by the matrix size, 1 = every problem in LDS, 2 = every problem in the workspace."""
    lib = load_library()
    _check(lib, lib.dff_debug_sym_eig_path(int(path)), "dff_debug_sym_eig_path")


def sym_eig_topk(a, ks, k: int, vectors=False, workspace=None):
    """The k algebraically largest eigenvalues of P symmetric matrices in one call (dff_sym_eig_topk): a (P, Kmax, Kmax)
    contiguous float64 CUDA, problem p a COMPACT (ks[p], ks[p]) matrix at the start of its slot, only its lower triangle read;
    ks (P,) host integers.  Returns (w, v, status), CUDA tensors: w float64 (P, k) descending, NaN from index ks[p] on; v
    float64 (P, k, Kmax) with eigenvector j of problem p in v[p, j, :ks[p]] (unit 2-norm, largest component positive; what
    lies beyond ks[p] in a row is NaN, as allocated here), or None without `vectors`; status int32 (P,): 0 solved, 1 a
    non-finite entry (all outputs NaN), 2 a vector did not converge (vectors NaN).  Nothing is read back.  `workspace` is a
    uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    P, Kmax = (int(a.shape[0]), int(a.shape[1])) if isinstance(a, torch.Tensor) and a.dim() == 3 else (-1, -1)
    if not _is_tensor(a, torch.float64, (P, Kmax, Kmax)):
        raise ValueError("a must be a contiguous float64 CUDA tensor of shape (P, Kmax, Kmax)")
    kh = _host_i32(ks, P, "ks", "state count")
    k = int(k)
    if not 1 <= k <= SYM_EIG_MAX_K:
        raise ValueError(f"k must be 1..{SYM_EIG_MAX_K}, not {k}")
    w = torch.empty((P, k), dtype=torch.float64, device=a.device)
    v = torch.full((P, k, Kmax), float("nan"), dtype=torch.float64, device=a.device) if vectors else None
    status = torch.empty(P, dtype=torch.int32, device=a.device)
    workspace = _workspace(workspace, a.device, "dff_sym_eig_workspace_bytes", P, Kmax, always=False)
    _check(lib, lib.dff_sym_eig_topk(a.device.index, _ptr(a), kh.ctypes.data_as(C.c_void_p), P, Kmax, k, _ptr(w), _ptr(v),
                                     _ptr(status), _ptr(workspace), _nbytes(workspace),
                                     _stream(a)), "dff_sym_eig_topk")
    return w, v, status


# ---- row vectors through a transition matrix, step after step (dff_msm_propagate) ----
MSM_PROPAGATE_MAX_BATCH = 16384
MSM_PROPAGATE_MAX_ROWS = 16
MSM_PROPAGATE_MAX_STEPS = 65535


def msm_propagate_workspace_bytes(P: int, Kmax: int, M: int, R: int) -> int:
    return _workspace_bytes("dff_msm_propagate_workspace_bytes", int(P), int(Kmax), int(M), int(R))


def msm_propagate_lds_limit() -> int:
    """The largest matrix dff_msm_propagate propagates out of LDS, read from the library."""
    return int(load_library().dff_msm_propagate_lds_limit())


def debug_msm_propagate_path(path: int):
    """Tests and benchmarks only: 0 = by the matrix size, 1 = every problem in LDS, 2 = every matrix streamed from global memory."""
    lib = load_library()
    _check(lib, lib.dff_debug_msm_propagate_path(int(path)), "dff_debug_msm_propagate_path")


def msm_propagate(t, mat_of, ks, w0, obs, n_steps: int, want_last=False, workspace=None):
    """P propagation problems in one call (dff_msm_propagate): t (n_mat, Kmax, Kmax) contiguous float64 CUDA, matrix m a COMPACT
    (K, K) matrix at the start of its slot; mat_of (P,) host integers, the matrix of each problem (None: problem p reads matrix
    p); ks (P,) host integers; w0 (P, M, Kmax) start row vectors and obs (P, R, Kmax) observables, contiguous float64 CUDA,
    read below ks[p].  Returns (out, w_last, status), CUDA tensors: out float64 (P, n_steps + 1, M, R) with out[p, s, m, r] =
    sum_j (w0[p, m] T^s)[j] obs[p, r, j]; w_last float64 (P, M, Kmax), the vectors after the last step (NaN beyond ks[p], as
    allocated here), or None without `want_last`; status int32 (P,): 0 solved, 1 a non-finite input, 2 an overflow that made a
    NaN (all outputs of the problem NaN in both cases).  Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated
    here when None)."""
    import torch
    lib = load_library()
    f64 = torch.float64
    n_mat, Kmax = (int(t.shape[0]), int(t.shape[1])) if isinstance(t, torch.Tensor) and t.dim() == 3 else (-1, -1)
    P, M = (int(w0.shape[0]), int(w0.shape[1])) if isinstance(w0, torch.Tensor) and w0.dim() == 3 else (-1, -1)
    R = int(obs.shape[1]) if isinstance(obs, torch.Tensor) and obs.dim() == 3 else -1
    if not (_is_tensor(t, f64, (n_mat, Kmax, Kmax)) and _is_tensor(w0, f64, (P, M, Kmax)) and _is_tensor(obs, f64, (P, R, Kmax))
            and w0.device == t.device and obs.device == t.device):
        raise ValueError("t (n_mat, Kmax, Kmax), w0 (P, M, Kmax) and obs (P, R, Kmax) must be contiguous float64 CUDA tensors on "
                         "one device")
    kh = _host_i32(ks, P, "ks", "state count")
    mh = _host_i32(mat_of, P, "mat_of", "matrix index") if mat_of is not None else None
    S = int(n_steps)
    if not 0 <= S <= MSM_PROPAGATE_MAX_STEPS:
        raise ValueError(f"n_steps must be 0..{MSM_PROPAGATE_MAX_STEPS}, not {S}")
    if not (1 <= M <= MSM_PROPAGATE_MAX_ROWS and 1 <= R <= MSM_PROPAGATE_MAX_ROWS):
        raise ValueError(f"the numbers of start vectors and observables must be 1..{MSM_PROPAGATE_MAX_ROWS}, not {M} and {R}")
    if P * (S + 1) * M * R > 1 << 28:
        raise ValueError(f"{P * (S + 1) * M * R} output values, at most 2^28 per call")
    out = torch.empty((P, S + 1, M, R), dtype=f64, device=t.device)
    w_last = torch.full((P, M, Kmax), float("nan"), dtype=f64, device=t.device) if want_last else None
    status = torch.empty(P, dtype=torch.int32, device=t.device)
    workspace = _workspace(workspace, t.device, "dff_msm_propagate_workspace_bytes", P, Kmax, M, R, always=False)
    _check(lib, lib.dff_msm_propagate(t.device.index, _ptr(t), n_mat, mh.ctypes.data_as(C.c_void_p) if mh is not None else None,
                                      kh.ctypes.data_as(C.c_void_p), P, Kmax, _ptr(w0), M, _ptr(obs), R, S, _ptr(out),
                                      _ptr(w_last), _ptr(status), _ptr(workspace),
                                      _nbytes(workspace), _stream(t)), "dff_msm_propagate")
    return out, w_last, status


def msm_batch_plan(call: str, ks, Kmax: int) -> list:
    """What `call` ("dirichlet", "eig" or "propagate") launches for problems of ks states in slots of Kmax under its debug path as it
    stands: the LDS kernel's launch, then the other path's, each a dict of launched, path, lo, hi, sized_for, lds_bytes
    (dff_debug_msm_batch_plan: host only, no GPU).  What the call refuses about ks raises here in the same words."""
    lib = load_library()
    kh = np.ascontiguousarray(np.asarray(ks, dtype=np.int32).reshape(-1))
    plan = DffMsmBatchPlan()
    _check(lib, lib.dff_debug_msm_batch_plan(str(call).encode(), kh.ctypes.data_as(C.c_void_p), int(kh.size), int(Kmax),
                                             C.byref(plan)), "dff_debug_msm_batch_plan")
    return [{n: int(getattr(l, n)) for n, _ in DffMsmBatchLaunch._fields_} for l in plan.launch]


# ---- hidden Markov models: one E-step of Baum-Welch over all chains (dff_hmm_estep) ----
HMM_MAX_HIDDEN = 8
HMM_MAX_CHAINS = 1 << 20


def hmm_chunk() -> int:
    """The chunk length of dff_hmm_estep (frames of a chain per chunk), read from the library."""
    return int(load_library().dff_hmm_chunk())


def debug_hmm_stages(stages: int):
    """Benchmarks only: 0 = the whole call, 1 .. 5 = dff_hmm_estep stops after that many of its launches (outputs unfinished)."""
    lib = load_library()
    _check(lib, lib.dff_debug_hmm_stages(int(stages)), "dff_debug_hmm_stages")


def hmm_plan(lengths, lag: int):
    """(n_chains, n_chunks) of a call on trajectories of `lengths` at `lag` (dff_hmm_plan: host arithmetic)."""
    lib = load_library()
    lh = _lengths(lengths)
    a, b = C.c_longlong(0), C.c_longlong(0)
    _check(lib, lib.dff_hmm_plan(lh.ctypes.data_as(C.c_void_p), int(lh.size), int(lag), C.byref(a), C.byref(b)), "dff_hmm_plan")
    return int(a.value), int(b.value)


def _hmm_workspace_bytes(symbol, n, lengths, lag, m, K):
    """the bytes that `symbol`, one of the three dff_hmm*_workspace_bytes, asks for (its refusal raises)"""
    lh = _lengths(lengths)
    return _workspace_bytes(symbol, int(n), lh.ctypes.data_as(C.c_void_p), int(lh.size), int(lag), int(m), int(K))


def _hmm_workspace(symbol, n, lengths, lag, m, K, workspace, device):
    """the workspace of a call (_workspace): `symbol` is asked either way, it is the call's first refusal"""
    lh = _lengths(lengths)
    return _workspace(workspace, device, symbol, int(n), lh.ctypes.data_as(C.c_void_p), int(lh.size), int(lag), int(m), int(K))


def _hmm_arguments(labels, lengths, lag, trans, emit, init, names):
    """What hmm_estep, hmm_fit_steps and hmm_viterbi check first -> (m, K, n, lengths as a host array, lag, device); `names` are
    the call's names of trans, emit and init."""
    import torch
    f64 = torch.float64
    m, K = (int(emit.shape[0]), int(emit.shape[1])) if isinstance(emit, torch.Tensor) and emit.dim() == 2 else (-1, -1)
    if not (_is_tensor(emit, f64, (m, K)) and _is_tensor(trans, f64, (m, m)) and _is_tensor(init, f64, (m,))
            and trans.device == emit.device and init.device == emit.device):
        raise ValueError("%s (m, m), %s (m, K) and %s (m,) must be contiguous float64 CUDA tensors on one device" % names)
    if not (_is_tensor(labels, torch.int32, dim=1) and labels.device == emit.device):
        raise ValueError("labels must be a contiguous int32 CUDA tensor (n,) on the parameters' device")
    return m, K, int(labels.numel()), _lengths(lengths), int(lag), emit.device


def hmm_workspace_bytes(n: int, lengths, lag: int, m: int, K: int) -> int:
    return _hmm_workspace_bytes("dff_hmm_workspace_bytes", n, lengths, lag, m, K)


def hmm_estep(labels, lengths, lag: int, trans, emit, init, chain_loglik=True, post=True, workspace=None):
    """One E-step of Baum-Welch over all chains (dff_hmm_estep): labels int32 CUDA (n,) in trajectories of `lengths` (host), chain
    (r, f) the frames f, f + lag, ... of trajectory r, a negative label a missing observation; trans (m, m), emit (m, K) and init
    (m,) contiguous float64 CUDA tensors, not normalised by the call.  Returns a dict of CUDA tensors: stats float64
    (1 + m m + m + m K,) = loglik | xi (m, m) | gamma0 (m) | gamma_sym (m, K); chain_loglik float64 (n_traj lag,) and post float64
    (n, m), the posteriors in frame order (None when not asked for; post may also be a (n, m) tensor to fill); status int32 (1,):
    0 success, 1 a non-finite or negative parameter, 2 a chain of likelihood zero, 3 a label >= K -- every output NaN unless 0.
    Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    f64 = torch.float64
    m, K, n, lh, lag, dev = _hmm_arguments(labels, lengths, lag, trans, emit, init, ("trans", "emit", "init"))
    workspace = _hmm_workspace("dff_hmm_workspace_bytes", n, lh, lag, m, K, workspace, dev)
    stats = torch.empty(1 + m * m + m + m * K, dtype=f64, device=dev)
    cl = torch.empty(int(lh.size) * lag, dtype=f64, device=dev) if chain_loglik else None
    if isinstance(post, torch.Tensor):
        if not (_is_tensor(post, f64, (n, m)) and post.device == dev):
            raise ValueError("post must be a contiguous float64 CUDA tensor (n, m) on the parameters' device")
        pt = post
    else:
        pt = torch.empty((n, m), dtype=f64, device=dev) if post else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _check(lib, lib.dff_hmm_estep(dev.index, _ptr(labels), n, lh.ctypes.data_as(C.c_void_p), int(lh.size), lag, _ptr(trans),
                                  _ptr(emit), _ptr(init), m, K, _ptr(stats), _ptr(cl), _ptr(pt), _ptr(status), _ptr(workspace),
                                  _nbytes(workspace), _stream(emit)), "dff_hmm_estep")
    return {"stats": stats, "chain_loglik": cl, "post": pt, "status": status}


# ---- hidden Markov models: Baum-Welch on the device, many iterations per call (dff_hmm_fit_steps) ----
HMM_FIT_STATE = np.dtype([("n_estep", "<i4"), ("stop", "<i4"), ("estep_status", "<i4"), ("flags", "<i4"), ("last_loglik", "<f8"),
                          ("rev_sweeps", "<i8")])           # dff_hmm_fit_state: 32 bytes


def hmm_fit_state_dict(words) -> dict:
    """dff_hmm_fit_state as a dict of Python numbers from its 8 int32 words (a host array or tensor)."""
    rec = np.ascontiguousarray(np.asarray(words, np.int32).reshape(8)).view(HMM_FIT_STATE)[0]
    return {"n_estep": int(rec["n_estep"]), "stop": int(rec["stop"]), "estep_status": int(rec["estep_status"]),
            "flags": int(rec["flags"]), "last_loglik": float(rec["last_loglik"]), "rev_sweeps": int(rec["rev_sweeps"])}


def hmm_fit_workspace_bytes(n: int, lengths, lag: int, m: int, K: int) -> int:
    return _hmm_workspace_bytes("dff_hmm_fit_workspace_bytes", n, lengths, lag, m, K)


def hmm_fit_steps(labels, lengths, lag: int, trans, emit, init, reversible, n_steps: int, accuracy: float, rev_tol: float = 1e-12,
                  rev_max_sweeps: int = 1_000_000, state=None, loglik=None, stationary=True, workspace=None):
    """n_steps iterations of Baum-Welch on the device (dff_hmm_fit_steps): labels, lengths and lag as for hmm_estep; trans (m, m),
    emit (m, K) and init (m,) contiguous float64 CUDA tensors, REWRITTEN in place by every M-step.  state: an int32 CUDA tensor of
    8 words (dff_hmm_fit_state; hmm_fit_state_dict reads it), passed back to continue a fit; None starts one from zeros.
    loglik: a float64 CUDA tensor (n_steps,) to fill, or None; stationary: a float64 CUDA tensor (m,) that reversible M-steps
    write, True for a new one filled with NaN, or None / False for none.  Returns a dict of CUDA tensors: loglik (NaN for the
    steps of a stopped fit), stationary (or None), state.  Nothing is read back and nothing synchronises.  `workspace` is a uint8
    CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    f64 = torch.float64
    m, K, n, lh, lag, dev = _hmm_arguments(labels, lengths, lag, trans, emit, init, ("trans", "emit", "init"))
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    if state is None:
        state = torch.zeros(8, dtype=torch.int32, device=dev)
    elif not (_is_tensor(state, torch.int32, (8,)) and state.device == dev):
        raise ValueError("state must be a contiguous int32 CUDA tensor (8,) on the parameters' device")
    if loglik is None:
        loglik = torch.empty(n_steps, dtype=f64, device=dev)
    elif not (_is_tensor(loglik, f64, (n_steps,)) and loglik.device == dev):
        raise ValueError("loglik must be a contiguous float64 CUDA tensor (n_steps,) on the parameters' device")
    if stationary is True:
        stationary = torch.full((m,), float("nan"), dtype=f64, device=dev)
    elif stationary is None or stationary is False:
        stationary = None
    elif not (_is_tensor(stationary, f64, (m,)) and stationary.device == dev):
        raise ValueError("stationary must be a contiguous float64 CUDA tensor (m,) on the parameters' device")
    workspace = _hmm_workspace("dff_hmm_fit_workspace_bytes", n, lh, lag, m, K, workspace, dev)
    _check(lib, lib.dff_hmm_fit_steps(dev.index, _ptr(labels), n, lh.ctypes.data_as(C.c_void_p), int(lh.size), lag, _ptr(trans),
                                      _ptr(emit), _ptr(init), m, K, int(bool(reversible)), n_steps, float(accuracy), float(rev_tol),
                                      int(rev_max_sweeps), _ptr(loglik), _ptr(stationary), _ptr(state), _ptr(workspace),
                                      _nbytes(workspace), _stream(emit)), "dff_hmm_fit_steps")
    return {"loglik": loglik, "stationary": stationary, "state": state}


# ---- hidden Markov models: the most probable hidden path of every chain (dff_hmm_viterbi) ----
def debug_hmm_viterbi_stages(stages: int):
    """Benchmarks only: 0 = the whole call, 1 .. 6 = dff_hmm_viterbi stops after that many of its launches (outputs unfinished)."""
    lib = load_library()
    _check(lib, lib.dff_debug_hmm_viterbi_stages(int(stages)), "dff_debug_hmm_viterbi_stages")


def hmm_viterbi_workspace_bytes(n: int, lengths, lag: int, m: int, K: int) -> int:
    return _hmm_workspace_bytes("dff_hmm_viterbi_workspace_bytes", n, lengths, lag, m, K)


def hmm_viterbi(labels, lengths, lag: int, logtrans, logemit, loginit, chain_order=False, chain_logprob=True, workspace=None):
    """The most probable hidden path of every chain (dff_hmm_viterbi): labels int32 CUDA (n,) in trajectories of `lengths` (host),
    chain (r, f) the frames f, f + lag, ... of trajectory r, a negative label a missing observation; logtrans (m, m), logemit (m, K)
    and loginit (m,) contiguous float64 CUDA tensors holding LOGARITHMS (-inf: impossible).  Returns a dict of CUDA tensors: path
    int32 (n,), in frame order, or with chain_order=True the chains back to back (r-major, f-minor); chain_logprob float64
    (n_traj lag,), the joint log-probability of every chain's path and labels (None when not asked for); status int32 (1,): 0
    success, 1 a NaN or +inf parameter, 3 a label >= K, 2 a chain the model cannot emit -- then the path is -1 and chain_logprob NaN.
    Ties go to the lowest state.  Nothing is read back.  `workspace` is a uint8 CUDA tensor (allocated here when None)."""
    import torch
    lib = load_library()
    f64 = torch.float64
    m, K, n, lh, lag, dev = _hmm_arguments(labels, lengths, lag, logtrans, logemit, loginit, ("logtrans", "logemit", "loginit"))
    workspace = _hmm_workspace("dff_hmm_viterbi_workspace_bytes", n, lh, lag, m, K, workspace, dev)
    path = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(int(lh.size) * lag, dtype=f64, device=dev) if chain_logprob else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _check(lib, lib.dff_hmm_viterbi(dev.index, _ptr(labels), n, lh.ctypes.data_as(C.c_void_p), int(lh.size), lag, _ptr(logtrans),
                                    _ptr(logemit), _ptr(loginit), m, K, _ptr(path), 1 if chain_order else 0, _ptr(cl), _ptr(status),
                                    _ptr(workspace), _nbytes(workspace), _stream(logemit)),
           "dff_hmm_viterbi")
    return {"path": path, "chain_logprob": cl, "status": status}


# ---- bootstrap of the Jensen-Shannon metrics (dff_unit_hist, dff_resampled_js) ----
JS_MAX_UNITS = 65536
JS_MAX_RESAMPLES = 4096


def unit_hist_workspace_bytes(U: int, C: int) -> int:
    return _workspace_bytes("dff_unit_hist_workspace_bytes", int(U), int(C))


def unit_hist(bins, unit_lengths, nbins, ld=None, workspace=None):
    """The histogram of every resampling unit (dff_unit_hist): bins int32 CUDA (n, C), the bin of frame t in channel c (< 0 or
    >= nbins[c]: not counted); unit_lengths (U,) host, consecutive units summing to n; nbins (C,) host; ld the row stride
    (default max(nbins)) -> int32 CUDA tensor (U, C, ld) of counts.  Exact.  `workspace` is a uint8 CUDA tensor (allocated
    here when None)."""
    import torch
    lib = load_library()
    if not _is_tensor(bins, torch.int32, dim=2):
        raise ValueError("bins must be a contiguous int32 CUDA tensor of shape (n, C)")
    n, Cn = int(bins.shape[0]), int(bins.shape[1])
    un, nb = _lengths(unit_lengths), _host_i32(nbins, Cn, "nbins", "bin count", per="channel", of="C")
    ld = int(ld) if ld is not None else int(nb.max()) if nb.size else 0
    U = int(un.size)
    workspace = _workspace(workspace, bins.device, "dff_unit_hist_workspace_bytes", U, Cn)
    ok = 1 <= ld <= 1 << 20 and U * Cn * ld <= 1 << 32                 # what is allocated when the shape will be refused
    out = torch.empty((U, Cn, ld) if ok else (1, 1, 1), dtype=torch.int32, device=bins.device)
    _check(lib, lib.dff_unit_hist(bins.device.index, _ptr(bins), n, Cn, un.ctypes.data_as(C.c_void_p), U,
                                  nb.ctypes.data_as(C.c_void_p), ld, _ptr(out), _ptr(workspace),
                                  _nbytes(workspace), _stream(bins)), "dff_unit_hist")
    return out


def resampled_js_workspace_bytes(U: int, C: int) -> int:
    return _workspace_bytes("dff_resampled_js_workspace_bytes", int(U), int(C))


def resampled_js(hist, nbins, weights, ref, total=True, workspace=None):
    """The Jensen-Shannon divergence of B weighted resamples x C channels against a reference (dff_resampled_js): hist int32 or
    uint32 CUDA (U, C, ld) as unit_hist gives it, nbins (C,) host, weights uint32 CUDA (B, U), ref float64 CUDA (C, ld) ->
    (js float64 CUDA (B, C), total uint64 CUDA (B, C) or None).  js is NaN where a resample holds no count or the reference
    channel cannot be normalised.  No resampled histogram is written to memory.  `workspace` is a uint8 CUDA tensor (allocated
    here when None)."""
    import torch
    lib = load_library()
    if not (isinstance(hist, torch.Tensor) and hist.is_cuda and hist.dtype in (torch.int32, torch.uint32) and hist.dim() == 3
            and hist.is_contiguous()):
        raise ValueError("hist must be a contiguous int32 or uint32 CUDA tensor of shape (U, C, ld)")
    U, Cn, ld = (int(v) for v in hist.shape)
    nb = _host_i32(nbins, Cn, "nbins", "bin count", per="channel", of="C")
    if not (_is_tensor(weights, torch.uint32, dim=2) and weights.shape[1] == U and weights.device == hist.device):
        raise ValueError("weights must be a contiguous uint32 CUDA tensor of shape (B, U) on the histograms' device")
    if not (_is_tensor(ref, torch.float64, (Cn, ld)) and ref.device == hist.device):
        raise ValueError("ref must be a contiguous float64 CUDA tensor of shape (C, ld) on the histograms' device")
    B = int(weights.shape[0])
    workspace = _workspace(workspace, hist.device, "dff_resampled_js_workspace_bytes", U, Cn)
    js = torch.empty((B, Cn), dtype=torch.float64, device=hist.device)
    tot = torch.empty((B, Cn), dtype=torch.uint64, device=hist.device) if total else None
    _check(lib, lib.dff_resampled_js(hist.device.index, _ptr(hist), U, Cn, ld, nb.ctypes.data_as(C.c_void_p), _ptr(weights), B,
                                     _ptr(ref), _ptr(js), _ptr(tot), _ptr(workspace),
                                     _nbytes(workspace), _stream(hist)), "dff_resampled_js")
    return js, tot


def debug_resampled_js_path(path: int):
    """Tests and benchmarks only: 0 = the library's choice by (B, C); 1, 2, 4, 8 = that many resamples per workgroup."""
    lib = load_library()
    _check(lib, lib.dff_debug_resampled_js_path(int(path)), "dff_debug_resampled_js_path")


def resampled_js_path_for(B: int, C: int) -> int:
    """The resamples per workgroup resampled_js would take now for B resamples and C channels."""
    lib = load_library()
    r = int(lib.dff_resampled_js_path_for(int(B), int(C)))
    if r < 0:
        _check(lib, 1, "dff_resampled_js_path_for")
    return r
