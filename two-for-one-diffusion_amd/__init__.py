"""two-for-one-diffusion_amd -- MI355X-native sampler for the denoising force field of
microsoft/two-for-one-diffusion: the score network (energy forward + hand-written VJP) inside
the DDPM reverse loop and the Langevin integrator, as one persistent HIP kernel behind a C ABI
(include/dff.h, libdff_amd.so).  Host side mirrors the reference's Python interfaces.

The directory name is not a Python identifier; import it as ``import dff_amd`` (alias module at
the repository root) or ``importlib.import_module("two-for-one-diffusion_amd")``.
"""
from . import binding, specs, weights  # noqa: F401
from .binding import DffLibraryError, Model, load_library  # noqa: F401
from .sampling import SamplerWrapper, num_to_groups, sample_from_model  # noqa: F401

# what evaluate.py offers under the package's name, one line per analysis layer: __all__ and the lazy import below both read this
_EVALUATE = (
    "KMeans", "StateTransitionEvaluator", "nearest_rmsd", "rmsd_matrix", "EnsembleCoverageEvaluator",
    "superpose", "mean_structure", "rmsf", "FlexibilityEvaluator",
    "cluster_rmsd", "RmsdClusterEvaluator",
    "native_pairs", "native_contacts_q", "core_states", "label_runs", "dwell_summary", "FoldingKineticsEvaluator",
    "path_states", "PathStates", "transition_paths", "path_time_summary", "path_histograms", "tp_probability", "empirical_committor",
    "TransitionPathEvaluator",
    "autocorrelation", "integrated_autocorr_time", "crossing_time", "effective_sample_size", "standard_error", "RelaxationEvaluator",
    "MicrostateKMeans", "largest_connected_set", "MarkovStateModel", "implied_timescales", "MsmEvaluator",
    "resampling_units", "bootstrap_weights", "bootstrap_msm", "MsmBootstrap", "implied_timescales_bootstrap",
    "mfpt", "committor", "reactive_flux", "ReactiveFlux", "bootstrap_passage", "PassageBootstrap", "states_by_cv", "dirichlet_solver",
    "MsmPassageEvaluator",
    "msm_spectrum", "MsmSpectrum", "spectral_solver",
    "propagator", "msm_propagate", "msm_relaxation", "msm_autocorrelation", "MsmAutocorrelation", "pcca_memberships",
    "metastable_sets", "chapman_kolmogorov", "chapman_kolmogorov_of_models", "ChapmanKolmogorov", "ChapmanKolmogorovEvaluator",
    "hmm_estep_solver", "initial_hmm", "HiddenMarkovModel", "HmmEvaluator", "hmm_viterbi_solver", "hmm_chain_lengths",
    "hmm_fit_solver", "resampled_labels", "bootstrap_hmm", "HmmBootstrap",
    "bin_indices_1d", "bin_indices_2d", "sample_units", "unit_histograms", "js_resampler", "bootstrap_js", "JsBootstrap")

__all__ = ["binding", "specs", "weights", "DffLibraryError", "Model", "load_library", "SamplerWrapper",
           "num_to_groups", "sample_from_model", "GraphTransformer", "GaussianDiffusion",
           "LangevinDiffusion", "ForcesWrapper", "eval_loss", "loss_profile", *_EVALUATE]


def __getattr__(name):  # torch-dependent pieces are imported on first use
    if name == "GraphTransformer":
        from .score import GraphTransformer
        return GraphTransformer
    if name == "GaussianDiffusion":
        from .ddpm import GaussianDiffusion
        return GaussianDiffusion
    if name in ("LangevinDiffusion", "ForcesWrapper"):
        from . import langevin
        return getattr(langevin, name)
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("eval_loss", "loss_profile"):
        from . import losses
        return getattr(losses, name)
    raise AttributeError(name)
