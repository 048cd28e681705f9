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

__all__ = ["binding", "specs", "weights", "DffLibraryError", "Model", "load_library", "SamplerWrapper",
           "num_to_groups", "sample_from_model", "GraphTransformer", "GaussianDiffusion",
           "LangevinDiffusion", "ForcesWrapper", "KMeans", "StateTransitionEvaluator", "eval_loss", "loss_profile",
           "nearest_rmsd", "rmsd_matrix", "EnsembleCoverageEvaluator"]
__all__ += ["superpose", "mean_structure", "rmsf", "FlexibilityEvaluator"]
__all__ += ["cluster_rmsd", "RmsdClusterEvaluator"]
__all__ += ["native_pairs", "native_contacts_q", "core_states", "label_runs", "dwell_summary", "FoldingKineticsEvaluator"]
__all__ += ["autocorrelation", "integrated_autocorr_time", "crossing_time", "effective_sample_size", "standard_error", "RelaxationEvaluator"]
__all__ += ["MicrostateKMeans", "largest_connected_set", "MarkovStateModel", "implied_timescales", "MsmEvaluator"]
__all__ += ["resampling_units", "bootstrap_weights", "bootstrap_msm", "MsmBootstrap", "implied_timescales_bootstrap"]
__all__ += ["mfpt", "committor", "reactive_flux", "ReactiveFlux", "bootstrap_passage", "PassageBootstrap", "states_by_cv", "dirichlet_solver", "MsmPassageEvaluator"]


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
    if name in ("KMeans", "StateTransitionEvaluator", "nearest_rmsd", "rmsd_matrix", "EnsembleCoverageEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("superpose", "mean_structure", "rmsf", "FlexibilityEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("cluster_rmsd", "RmsdClusterEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("native_pairs", "native_contacts_q", "core_states", "label_runs", "dwell_summary", "FoldingKineticsEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("autocorrelation", "integrated_autocorr_time", "crossing_time", "effective_sample_size", "standard_error", "RelaxationEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("MicrostateKMeans", "largest_connected_set", "MarkovStateModel", "implied_timescales", "MsmEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("resampling_units", "bootstrap_weights", "bootstrap_msm", "MsmBootstrap", "implied_timescales_bootstrap"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("mfpt", "committor", "reactive_flux", "ReactiveFlux", "bootstrap_passage", "PassageBootstrap", "states_by_cv", "dirichlet_solver", "MsmPassageEvaluator"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("eval_loss", "loss_profile"):
        from . import losses
        return getattr(losses, name)
    raise AttributeError(name)
