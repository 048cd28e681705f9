#!/usr/bin/env python3
"""Score a sample file the way the reference's Evaluator does (evaluate/evaluators.py:28-111): reads the
sample-{mode}.pt that sample.py writes ((n, N, 3) Angstrom) and a saved-references directory (the reference's
evaluate/saved_references, or .npz TICA models), and prints Evaluator.eval() as one JSON line.  Optional extras:
the RMSD free-energy curve and the contact BCE to the folded structure of a folded PDB.

    python tools_eval_samples.py SAMPLES.pt MOL SAVED_REF_DIR [--ref-data VAL.pt] [--folded-pdb PDB]
                                 [--tica-fit-data TRAJ.pt [--lagtime 100]]
                                 [--transitions [--traj-lengths L | --parallel-sim P] [--lagtimes 1,10,100]
                                  [--n-clusters K --centers-fit-data TRAJ.pt]]
                                 [--coverage REF.pt [--rmsd-thresholds 1,2,4] [--coverage-subsample K]]
                                 [--flexibility HELDOUT.pt] [--write-aligned OUT.pt]
                                 [--clusters HELDOUT.pt [--cluster-cutoff 2.0] [--cluster-stride K]]
                                 [--kinetics [HELDOUT.pt] [--kinetics-cv q|rmsd] [--kinetics-cores LO,HI] [--frame-time T]]
                                 [--paths [HELDOUT.pt] [--paths-bins N]]
                                 [--relaxation [HELDOUT.pt] [--relaxation-cv q|rmsd|tic] --max-lag L [--frame-time T]]
                                 [--passage [HELDOUT.pt] --passage-states K --passage-lag L [--passage-cv q|rmsd]
                                  [--passage-cores LO,HI] [--passage-bootstrap B]]
                                 [--ck [HELDOUT.pt] --ck-states K --ck-lag L [--ck-sets M] [--ck-multiples 1,2,3,4,5]
                                  [--ck-bootstrap B]]
                                 [--hmm [HELDOUT.pt] --hmm-states K --hmm-hidden M --hmm-lag L [--hmm-path posterior|viterbi] [--frame-time T]
                                  [--hmm-bootstrap B [--hmm-block-frames N] [--hmm-bootstrap-seed S]]]
                                 [--msm [HELDOUT.pt] --msm-states K --msm-lag L [--msm-lagtimes a,b,c] [--frame-time T]
                                  [--msm-bootstrap B [--msm-block-frames F] [--msm-confidence C]]
                                  [--msm-eigensolver host|device] [--msm-eigenvectors N]]

Without a saved TICA reference for MOL, --tica-fit-data fits one on the GPU (a (n, N, 3) trajectory in Angstrom, or a
list of them, in time order) and writes it to SAVED_REF_DIR as the .npz that tica_path() below names; --ref-data is then
the validation data it is histogrammed on.

--transitions adds the dynamics analysis of evaluate_fastfolders.ipynb (StateTransitionEvaluator) for time-ordered
Langevin samples: state assignments in the plane of MOL's TICA model, transition counts and probabilities per lag time.
Without --traj-lengths / --parallel-sim the samples count as ONE trajectory, as in the notebook; --parallel-sim P splits
them into P simulations of equal length (sample.py's simulation-major output), --traj-lengths L into runs of L frames.
The states are the notebook's presets for MOL, or are fitted by k-means (--n-clusters K) on --centers-fit-data.

--coverage REF.pt adds, under "coverage", the nearest-structure RMSD statistics of the samples against the ensemble REF.pt
((m, N, 3) Angstrom; EnsembleCoverageEvaluator): novelty / precision (samples -> nearest structure of REF), coverage /
recall (REF -> nearest sample), diversity / duplicates (samples -> nearest other sample), at the thresholds (Angstrom) of
--rmsd-thresholds.  Every pair is superposed: n * m + n * n optimal rotations.  --coverage-subsample K keeps at most K
evenly spaced frames of each ensemble.

--flexibility HELDOUT.pt adds, under "flexibility", the per-bead RMSF comparison of the samples with the ensemble HELDOUT.pt
((m, N, 3) Angstrom; FlexibilityEvaluator): both ensembles superposed on the folded structure of --folded-pdb when given,
otherwise on HELDOUT's mean structure.  --write-aligned OUT.pt saves the samples superposed on the folded structure of
--folded-pdb ((n, N, 3) float32, on the folded structure's centroid; NaN rows for non-finite samples).

--clusters HELDOUT.pt adds, under "clusters", the populations of HELDOUT's conformations in the samples
(RmsdClusterEvaluator): HELDOUT ((m, N, 3) Angstrom) is clustered under the RMSD with --cluster-cutoff (Angstrom; the
method of `gmx cluster -method gromos`), every sample goes to the nearest cluster centre when that is within the cutoff.
--cluster-stride K clusters every K-th frame of HELDOUT (the neighbour matrix holds at most 2^18 frames).

--kinetics adds, under "kinetics", the folding kinetics of time-ordered Langevin samples (FoldingKineticsEvaluator; needs
--folded-pdb): the fraction of native contacts Q (--kinetics-cv q, the default) or the RMSD to the folded structure (rmsd) per
frame, dual-cutoff states with the cores cv <= LO and cv >= HI of --kinetics-cores (0.2,0.9 for Q; the RMSD has no default),
folding and unfolding counts, rates and dwell times in units of --frame-time.  The samples split into trajectories by
--traj-lengths / --parallel-sim as for --transitions.  With HELDOUT.pt (MD frames (m, N, 3) in time order, or a list of such
trajectories) the same numbers for it with the suffix _ref, and the log10 rate ratios.

--paths adds, under "paths", the transition paths of time-ordered Langevin samples (TransitionPathEvaluator; needs
--folded-pdb; order parameter, cores, frame time and trajectories are those of --kinetics: --kinetics-cv, --kinetics-cores,
--frame-time, --traj-lengths / --parallel-sim): the number of folding and unfolding paths and their mean and median path times,
the shares of frames on paths and on loops, the largest p(TP | cv) over --paths-bins bins (50) with the bin it lies in, and the
cv at which the empirical committor crosses 1 / 2.  With HELDOUT.pt (as for --kinetics) the same numbers for it with the suffix
_ref, log10_path_time_ratio_folding / _unfolding, ptp_max_diff and committor_rmsd.

--relaxation adds, under "relaxation", how fast an observable decorrelates along time-ordered Langevin samples and how many
independent samples they hold (RelaxationEvaluator): the autocorrelation function of Q (--relaxation-cv q, the default), of
the RMSD to the folded structure (rmsd; both need --folded-pdb) or of the components of MOL's TICA model (tic) for the lags
0 .. --max-lag, inside the trajectories of --traj-lengths / --parallel-sim; its integrated autocorrelation time and 1 / e time
in units of --frame-time, the effective sample size and the standard error of the mean.  With HELDOUT.pt (as for --kinetics)
the same numbers for it with the suffix _ref, and log10_tau_int_ratio.

--msm adds, under "msm", a Markov state model of time-ordered Langevin samples (MsmEvaluator): --msm-states k-means
microstates in the space of MOL's TICA model, sliding-window counts at --msm-lag frames inside the trajectories of
--traj-lengths / --parallel-sim, the largest strongly connected set, the reversible maximum-likelihood transition matrix and
its slowest implied timescales in units of --frame-time.  With HELDOUT.pt (as for --kinetics) the microstates are fitted on
it, and the same numbers for it come with the suffix _ref, with log10_timescale_ratio and stationary_js.  --msm-lagtimes
a,b,c adds "implied_timescales": the timescales (frames x --frame-time) of the samples' model at each of these lag times.
--msm-bootstrap B adds bootstrap error bars (B resamples of the trajectories, or of blocks of --msm-block-frames frames):
timescales_lo / _hi at --msm-confidence (0.95), timescales_std, bootstrap_failed, with HELDOUT.pt their _ref counterparts and
log10_timescale_ratio_lo / _hi, and "timescales_lo" / "timescales_hi" in "implied_timescales".
--msm-eigensolver device takes every spectrum from dff_sym_eig_topk on the GPU (all resamples of a bootstrap batch in one call)
instead of numpy on the host, the default; --msm-eigenvectors N adds "eigenvectors": the N slowest right eigenvectors of the
samples' model on the full microstate index ("right"), their eigenvalues and the active set.

--ck adds the validity check of the Markov state model (ChapmanKolmogorovEvaluator): microstates and lag time as for --msm
(--ck-states K, --ck-lag L), --ck-sets M metastable sets from the model's leading eigenvectors (3), and for every multiple k of
--ck-multiples (1,2,3,4,5) the set-to-set probabilities that T(L)^k predicts against those of the model estimated at lag k L,
with the model's autocorrelation of the first TIC against the measured one; --ck-bootstrap B adds percentile intervals.  With
HELDOUT.pt also for that MD data, which then defines the sets.  Needs --parallel-sim.

--hmm adds a hidden Markov model of the microstate trajectory (HmmEvaluator) under "hmm": --hmm-states K microstates as for
--msm, --hmm-hidden M hidden states (1..8), --hmm-lag L frames; the implied timescales of the hidden transition matrix, the
hidden states' populations and lifetimes in units of --frame-time, the E-steps spent and the log-likelihood per frame.  With
HELDOUT.pt also for that MD data, with the ratios of timescales and lifetimes and the Jensen-Shannon divergence of the
populations, the hidden states compared in the order of their populations.  Needs --parallel-sim.
--hmm-path posterior|viterbi adds the dwell statistics of the hidden states ("hidden_path", "mean_dwell", "n_transitions"): of the
argmax of the posterior marginals, taken on the frame-ordered series, or of the Viterbi path (HiddenMarkovModel.viterbi), taken
inside the chains of the lag, one step being --hmm-lag frames.
--hmm-bootstrap B adds error bars from B bootstrap refits on the GPU (bootstrap_hmm, warm-started from the fitted model, whole
trajectories resampled or with --hmm-block-frames N blocks of N >= 2 L frames, draws seeded by --hmm-bootstrap-seed S):
"timescales_std", "lifetimes_std", "hidden_populations_std", "timescales_lo" / "timescales_hi" (95 %) and "bootstrap_failed".

--js-bootstrap B [--block-frames F] [--js-blocks N] adds, under "js_bootstrap", block-bootstrap error bars of the JS metrics
above (Evaluator.eval_bootstrap: the units' histograms once, B resamples scored on the GPU by dff_resampled_js): every key of
the plain evaluation with "_lo" / "_hi" (95 % percentile interval), "_std" and "_bias" (mean over the resamples - point; a JS
between finite histograms is biased upward), and "n_units", "n_resamples".  With --parallel-sim P the units are the P
trajectories, or their blocks of F frames; without it the samples count as independent and are cut into N (256) blocks.
"""
import argparse
import json
import os

import numpy as np
import torch

import dff_amd  # noqa: F401
from dff_amd import evaluate


def traj_lengths(a, n):
    if a.traj_lengths is not None and a.parallel_sim is not None:
        raise SystemExit("--traj-lengths and --parallel-sim exclude each other")
    L = a.traj_lengths if a.traj_lengths is not None else (n // a.parallel_sim if a.parallel_sim else None)
    if L is None:
        return None
    if L < 1 or n % L:
        raise SystemExit(f"{n} frames do not split into trajectories of {L} frames")
    return [L] * (n // L)


def tica_path(a):
    """MOL's saved TICA model in SAVED_REF_DIR: the .npz when there is one, else the reference's pickle"""
    stem = os.path.join(a.saved_ref_dir, f"saved_TICA_{a.mol.upper()}_{a.evalset}")
    return stem + ".npz" if os.path.exists(stem + ".npz") else stem + ".pickle"


def clean(v):
    """v as JSON can carry it: a non-finite number becomes None, a list goes element by element"""
    if isinstance(v, list):
        return [clean(u) for u in v]
    return None if not np.isfinite(v) else float(v)


def cleaned(res):
    """an evaluator's dict of numbers and lists of numbers, every value through clean()"""
    return {k: clean(v) for k, v in res.items()}


def number(parse, ok, message, unparsed=None):
    """an argparse type: parse(text), int or float, refused with `message` unless ok(value); text that does not parse is
    refused with `unparsed`, or with `message` too when there is none ({text!r} in either stands for the text)"""
    def convert(text):
        try:
            v = parse(text)
        except ValueError:
            raise argparse.ArgumentTypeError((unparsed or message).format(text=text))
        if not ok(v):
            raise argparse.ArgumentTypeError(message.format(text=text))
        return v
    return convert


NOT_A_NUMBER, NOT_AN_INTEGER = "not a number: {text!r}", "not an integer: {text!r}"


def transitions(a, x):
    mol = a.mol.lower()
    fit = torch.load(a.centers_fit_data, map_location="cpu").float() if a.centers_fit_data else None
    st = evaluate.StateTransitionEvaluator(mol, tica_path(a), n_clusters=a.n_clusters, fit_data=fit, device=a.device)
    r = st.eval(x, traj_lengths=traj_lengths(a, len(x)), lagtimes=[int(v) for v in a.lagtimes.split(",")])
    return {"centers": st.centers.tolist(), "lagtimes": r["lagtimes"], "populations": r["populations"].tolist(),
            "count_matrices": r["count_matrices"].tolist(), "transition_matrices": r["transition_matrices"].tolist(),
            "timescales": [clean(list(t)) for t in r["timescales"]]}


def rmsd_thresholds(text):
    """"1,2,4" -> (1.0, 2.0, 4.0): positive, comma-separated"""
    try:
        t = tuple(float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of numbers: {text!r}")
    if not t or min(t) <= 0:
        raise argparse.ArgumentTypeError("thresholds must be positive")
    return t


def subsample(x, k):
    """at most k evenly spaced frames of x, the first and the last among them (all of x when k is None or >= len(x))"""
    if k is None or k >= len(x):
        return x
    return x[torch.linspace(0, len(x) - 1, k).round().long()]


def coverage(a, x):
    ref = torch.load(a.coverage, map_location="cpu").float()
    ev = evaluate.EnsembleCoverageEvaluator(subsample(ref, a.coverage_subsample), a.mol.lower(), a.rmsd_thresholds,
                                            device=a.device)
    return ev.eval(subsample(x, a.coverage_subsample))


def flexibility(a, x):
    ref = torch.load(a.flexibility, map_location="cpu").float()
    ev = evaluate.FlexibilityEvaluator(ref, a.mol.lower(), a.folded_pdb, device=a.device)
    res = ev.eval(x)
    res["rmsf_samples"] = ev.profiles["samples"]["rmsf"].tolist()
    res["rmsf_refs"] = ev.profiles["refs"]["rmsf"].tolist()
    return res


cluster_cutoff = number(float, lambda v: np.isfinite(v) and v >= 0, "the cutoff must be finite and >= 0", NOT_A_NUMBER)


def clusters(a, x):
    ref = torch.load(a.clusters, map_location="cpu").float()
    ev = evaluate.RmsdClusterEvaluator(ref, a.mol.lower(), a.cluster_cutoff, stride=a.cluster_stride, device=a.device)
    res = ev.eval(x)
    res["cutoff"] = ev.cutoff
    res["centers"] = (ev.clusters.centers * a.cluster_stride).tolist()          # frame indices of HELDOUT
    return res


def cores(text):
    """"0.2,0.9" -> (0.2, 0.9): two finite numbers, the first below the second"""
    try:
        lo, hi = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"not two comma-separated numbers: {text!r}")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise argparse.ArgumentTypeError("the cores must be finite with LO < HI")
    return lo, hi


frame_time = number(float, lambda v: np.isfinite(v) and v > 0, "the frame time must be finite and > 0", NOT_A_NUMBER)


def kinetics_cores(a):
    if a.kinetics_cores is not None:
        return a.kinetics_cores
    if a.kinetics_cv != "q":
        raise SystemExit("--kinetics-cv rmsd needs --kinetics-cores LO,HI (Angstrom)")
    return 0.2, 0.9


def ordered_frames(path):
    """(frames, trajectory lengths or None) of a .pt of MD frames in time order, or of a list of such trajectories"""
    ref = torch.load(path, map_location="cpu")
    if isinstance(ref, torch.Tensor):
        return ref.float(), None
    trajs = [torch.as_tensor(t).float() for t in ref]
    return torch.cat(trajs), [len(t) for t in trajs]


def kinetics(a, x):
    lo, hi = kinetics_cores(a)
    ref, ref_lengths = ordered_frames(a.kinetics) if a.kinetics else (None, None)
    ev = evaluate.FoldingKineticsEvaluator(a.mol.lower(), a.folded_pdb, cv=a.kinetics_cv, lo=lo, hi=hi, frame_time=a.frame_time,
                                           ref_data=ref, ref_traj_lengths=ref_lengths, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"cv": a.kinetics_cv, "lo": lo, "hi": hi, "frame_time": a.frame_time})
    return res


def paths_arguments(a):
    """refused: --paths without --folded-pdb, --paths-bins without --paths"""
    if a.paths is None:
        if a.paths_bins is not None:
            raise SystemExit("--paths-bins needs --paths")
        return
    if not a.folded_pdb:
        raise SystemExit("--paths needs --folded-pdb")


def paths(a, x):
    lo, hi = kinetics_cores(a)
    ref, ref_lengths = ordered_frames(a.paths) if a.paths else (None, None)
    ev = evaluate.TransitionPathEvaluator(a.mol.lower(), a.folded_pdb, cv=a.kinetics_cv, lo=lo, hi=hi, frame_time=a.frame_time,
                                          nbins=a.paths_bins or 50, ref_data=ref, ref_traj_lengths=ref_lengths, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"cv": a.kinetics_cv, "lo": lo, "hi": hi, "frame_time": a.frame_time, "bins": a.paths_bins or 50})
    return res


paths_bins = number(int, lambda v: 1 <= v <= 65536, "the number of bins must be 1..65536", NOT_AN_INTEGER)
max_lag = number(int, lambda v: 1 <= v <= 65535, "the largest lag must be 1..65535", NOT_AN_INTEGER)


def relaxation_max_lag(a):
    if a.max_lag is None:
        raise SystemExit("--relaxation needs --max-lag L (frames)")
    return a.max_lag


def relaxation(a, x):
    L = relaxation_max_lag(a)
    ref, ref_lengths = ordered_frames(a.relaxation) if a.relaxation else (None, None)
    tica = tica_path(a) if a.relaxation_cv == "tic" else None
    ev = evaluate.RelaxationEvaluator(a.mol.lower(), a.folded_pdb, cv=a.relaxation_cv, tica=tica, max_lag=L,
                                      frame_time=a.frame_time, ref_data=ref, ref_traj_lengths=ref_lengths, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"cv": a.relaxation_cv, "max_lag": L, "frame_time": a.frame_time})
    return res


msm_states = number(int, lambda v: 1 <= v <= evaluate.MSM_MAX_STATES,
                    f"the number of microstates must be 1..{evaluate.MSM_MAX_STATES}", NOT_AN_INTEGER)
msm_lag = number(int, lambda v: v >= 1, "a lag time must be >= 1 frame", NOT_AN_INTEGER)


def msm_lagtimes(text):
    try:
        return [msm_lag(v) for v in text.split(",")]
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError(f"expected comma-separated lag times >= 1, got {text!r}")


def msm_arguments(a):
    if a.msm_states is None or a.msm_lag is None:
        raise SystemExit("--msm needs --msm-states K and --msm-lag L (frames)")
    return a.msm_states, a.msm_lag


msm_bootstrap = number(int, lambda v: v >= 1, "expected a number of resamples >= 1, got {text!r}")
msm_confidence = number(float, lambda v: 0 < v < 1, "expected a confidence level in (0, 1), got {text!r}")


msm_eigenvectors = number(int, lambda v: 1 <= v < evaluate.SPECTRUM_MAX_K, "expected a number of eigenvectors in 1..31, got {text!r}")


def msm_bootstrap_arguments(a):
    """keyword arguments of MsmEvaluator for --msm-bootstrap; its options are refused without it, and it without --msm"""
    if a.msm_bootstrap is None:
        if a.msm_block_frames is not None or a.msm_confidence is not None:
            raise SystemExit("--msm-block-frames and --msm-confidence need --msm-bootstrap B")
        return {}
    if a.msm is None:
        raise SystemExit("--msm-bootstrap needs --msm")
    return {"n_bootstrap": a.msm_bootstrap, "block_frames": a.msm_block_frames,
            "confidence": 0.95 if a.msm_confidence is None else a.msm_confidence}


def msm_spectrum_arguments(a):
    """(eigensolver, eigenvectors) of --msm; both options are refused without it"""
    if a.msm is None and (a.msm_eigensolver is not None or a.msm_eigenvectors is not None):
        raise SystemExit("--msm-eigensolver and --msm-eigenvectors need --msm")
    return a.msm_eigensolver or "host", a.msm_eigenvectors


def msm(a, x):
    K, lag = msm_arguments(a)
    boot = msm_bootstrap_arguments(a)
    solver, n_vectors = msm_spectrum_arguments(a)
    ref, ref_lengths = ordered_frames(a.msm) if a.msm else (None, None)
    ev = evaluate.MsmEvaluator(a.mol.lower(), tica_path(a), n_microstates=K, lagtime=lag, frame_time=a.frame_time, ref_data=ref,
                               ref_traj_lengths=ref_lengths, eigensolver=solver, device=a.device, **boot)
    lengths = traj_lengths(a, len(x))
    res = cleaned(ev.eval(x, lengths))
    res.update({"n_microstates": K, "lagtime": lag, "frame_time": a.frame_time, "eigensolver": solver})
    if n_vectors:                                # the slowest right eigenvectors of the point model, on the full microstate index
        sp = evaluate.msm_spectrum(ev.models["samples"], k=n_vectors, vectors=True, device=a.device)
        res["eigenvectors"] = {"eigenvalues": clean(list(sp.eigenvalues[0, 1:])), "right": [clean(list(row)) for row in sp.right[0, 1:]],
                               "active_set": [int(i) for i in ev.models["samples"].active_set]}
    if boot:
        res.update({"n_bootstrap": boot["n_bootstrap"], "block_frames": boot["block_frames"], "confidence": boot["confidence"]})
    table = lambda m: [clean([v * a.frame_time for v in row]) for row in m]     # noqa: E731
    if a.msm_lagtimes and boot:
        its, lo, hi = evaluate.implied_timescales_bootstrap(ev.labels["samples"], a.msm_lagtimes, lengths, K, k=ev.n_timescales,
                                                            n_resamples=boot["n_bootstrap"], block_frames=boot["block_frames"],
                                                            confidence=boot["confidence"], eigensolver=solver, device=a.device)
        res["implied_timescales"] = {"lagtimes": a.msm_lagtimes, "timescales": table(its), "timescales_lo": table(lo),
                                     "timescales_hi": table(hi)}
    elif a.msm_lagtimes:
        its = evaluate.implied_timescales(ev.labels["samples"], a.msm_lagtimes, lengths, K, k=ev.n_timescales, eigensolver=solver,
                                          device=a.device)
        res["implied_timescales"] = {"lagtimes": a.msm_lagtimes, "timescales": table(its)}
    return res


def passage_arguments(a):
    """(states, lag, cv, (lo, hi)) of --passage, None without it; refused without --passage-states / --passage-lag, --folded-pdb, --parallel-sim,
    and (for the RMSD) --passage-cores; the options of --passage are refused without it"""
    if a.passage is None:
        if any(v is not None for v in (a.passage_states, a.passage_lag, a.passage_cv, a.passage_cores, a.passage_bootstrap)):
            raise SystemExit("--passage-states, --passage-lag, --passage-cv, --passage-cores and --passage-bootstrap need --passage")
        return None
    if a.passage_states is None or a.passage_lag is None:
        raise SystemExit("--passage needs --passage-states K and --passage-lag L (frames)")
    if not a.folded_pdb:
        raise SystemExit("--passage needs --folded-pdb")
    if a.parallel_sim is None:
        raise SystemExit("--passage needs --parallel-sim (the trajectories of the samples)")
    cv = a.passage_cv or "q"
    if a.passage_cores is None and cv != "q":
        raise SystemExit("--passage-cv rmsd needs --passage-cores LO,HI (Angstrom)")
    return a.passage_states, a.passage_lag, cv, a.passage_cores or (0.2, 0.9)


def passage(a, x):
    K, lag, cv, (lo, hi) = passage_arguments(a)
    ref, ref_lengths = ordered_frames(a.passage) if a.passage else (None, None)
    ev = evaluate.MsmPassageEvaluator(a.mol.lower(), tica_path(a), a.folded_pdb, n_microstates=K, lagtime=lag, cv=cv, lo=lo, hi=hi,
                                      frame_time=a.frame_time, ref_data=ref, ref_traj_lengths=ref_lengths,
                                      n_bootstrap=a.passage_bootstrap or 0, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"n_microstates": K, "lagtime": lag, "cv": cv, "lo": lo, "hi": hi, "frame_time": a.frame_time,
                "n_bootstrap": a.passage_bootstrap or 0})
    return res


ck_sets = number(int, lambda v: 1 <= v <= evaluate.PROPAGATE_MAX_ROWS, "expected a number of metastable sets in 1..16, got {text!r}")


def ck_multiples(text):
    try:
        ks = [int(v) for v in text.split(",")]
    except ValueError:
        ks = []
    if not ks or any(k < 1 for k in ks) or len(set(ks)) != len(ks):
        raise argparse.ArgumentTypeError(f"expected distinct comma-separated multiples >= 1, got {text!r}")
    return ks


def ck_arguments(a):
    """(states, lag, sets, multiples, resamples) of --ck, None without it; refused without --ck-states / --ck-lag and
    --parallel-sim; the options of --ck are refused without it"""
    if a.ck is None:
        if any(v is not None for v in (a.ck_states, a.ck_lag, a.ck_sets, a.ck_multiples, a.ck_bootstrap)):
            raise SystemExit("--ck-states, --ck-lag, --ck-sets, --ck-multiples and --ck-bootstrap need --ck")
        return None
    if a.ck_states is None or a.ck_lag is None:
        raise SystemExit("--ck needs --ck-states K and --ck-lag L (frames)")
    if a.parallel_sim is None:
        raise SystemExit("--ck needs --parallel-sim (the trajectories of the samples)")
    return a.ck_states, a.ck_lag, a.ck_sets or 3, a.ck_multiples or [1, 2, 3, 4, 5], a.ck_bootstrap or 0


def ck(a, x):
    K, lag, n_sets, multiples, boots = ck_arguments(a)
    ref, ref_lengths = ordered_frames(a.ck) if a.ck else (None, None)
    ev = evaluate.ChapmanKolmogorovEvaluator(a.mol.lower(), tica_path(a), n_microstates=K, lagtime=lag, n_sets=n_sets,
                                             multiples=multiples, frame_time=a.frame_time, ref_data=ref,
                                             ref_traj_lengths=ref_lengths, n_bootstrap=boots, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"n_microstates": K, "lagtime": lag, "multiples": multiples, "n_bootstrap": boots,
                "sets": [[int(i) for i in s] for s in ev.sets]})
    return res


hmm_hidden = number(int, lambda v: 1 <= v <= evaluate.HMM_MAX_HIDDEN, "expected a number of hidden states in 1..8, got {text!r}")


def hmm_arguments(a):
    """(states, hidden, lag) of --hmm, None without it; refused without --hmm-states / --hmm-hidden / --hmm-lag and
    --parallel-sim; the options of --hmm are refused without it"""
    if a.hmm is None:
        if any(v is not None for v in (a.hmm_states, a.hmm_hidden, a.hmm_lag)):
            raise SystemExit("--hmm-states, --hmm-hidden and --hmm-lag need --hmm")
        if getattr(a, "hmm_path", None) is not None:
            raise SystemExit("--hmm-path needs --hmm")
        if any(getattr(a, k, None) is not None for k in ("hmm_bootstrap", "hmm_block_frames", "hmm_bootstrap_seed")):
            raise SystemExit("--hmm-bootstrap, --hmm-block-frames and --hmm-bootstrap-seed need --hmm")
        return None
    if getattr(a, "hmm_bootstrap", None) is None and (getattr(a, "hmm_block_frames", None) is not None
                                                       or getattr(a, "hmm_bootstrap_seed", None) is not None):
        raise SystemExit("--hmm-block-frames and --hmm-bootstrap-seed need --hmm-bootstrap B")
    if a.hmm_states is None or a.hmm_hidden is None or a.hmm_lag is None:
        raise SystemExit("--hmm needs --hmm-states K, --hmm-hidden M and --hmm-lag L (frames)")
    if a.parallel_sim is None:
        raise SystemExit("--hmm needs --parallel-sim (the trajectories of the samples)")
    return a.hmm_states, a.hmm_hidden, a.hmm_lag


def hmm(a, x):
    K, M, lag = hmm_arguments(a)
    ref, ref_lengths = ordered_frames(a.hmm) if a.hmm else (None, None)
    ev = evaluate.HmmEvaluator(a.mol.lower(), tica_path(a), n_microstates=K, n_hidden=M, lagtime=lag, frame_time=a.frame_time,
                               ref_data=ref, ref_traj_lengths=ref_lengths, path=a.hmm_path or "posterior",
                               n_bootstrap=a.hmm_bootstrap or 0, block_frames=a.hmm_block_frames,
                               bootstrap_seed=a.hmm_bootstrap_seed or 0, device=a.device)
    res = cleaned(ev.eval(x, traj_lengths(a, len(x))))
    res.update({"n_microstates": K, "n_hidden": M, "lagtime": lag, "frame_time": a.frame_time})
    if a.hmm_path is not None:                                      # the dwell statistics of the chosen state series
        for name, suffix in (("samples", ""), ("refs", "_ref")):
            if name in ev.dwell:
                res.update(hmm_dwell(ev.dwell[name], M, a.hmm_path, suffix))
    return res


def hmm_dwell(dwell, n_hidden, path, suffix=""):
    """what --hmm-path adds under "hmm": the state series the dwells were taken on, the mean completed dwell of every hidden
    state (in units of --frame-time; null without a completed dwell) and the number of transitions between hidden states"""
    mean = [dwell["mean_dwell"].get(i, float("nan")) for i in range(n_hidden)]
    res = cleaned({"mean_dwell" + suffix: mean, "n_transitions" + suffix: float(sum(dwell["events"].values()))})
    res["hidden_path" + suffix] = path
    return res


def write_aligned(a, x):
    folded = evaluate.folded_ca(a.folded_pdb, a.mol.lower())
    torch.save(evaluate.superpose(x, folded, device=a.device).cpu(), a.write_aligned)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("samples", help="sample-{mode}.pt written by sample.py")
    ap.add_argument("mol", help="molecule name as sample.py's --mol (alanine_dipeptide_*, chignolin, ...)")
    ap.add_argument("saved_ref_dir", help="directory of saved references")
    ap.add_argument("--ref-data", default=None, help="reference structures (.pt, (n, N, 3) Angstrom) where no saved "
                                                     "reference exists (PWD at offset 0)")
    ap.add_argument("--evalset", default="testset")
    ap.add_argument("--folded-pdb", default=None, help="folded PDB: also report the RMSD curve and the contact BCE")
    ap.add_argument("--tica-fit-data", default=None, help="time-ordered trajectories (.pt: (n, N, 3) Angstrom or a list "
                                                          "of them) to fit a TICA model on where none is saved")
    ap.add_argument("--lagtime", type=int, default=100, help="TICA lag time in frames (with --tica-fit-data)")
    ap.add_argument("--transitions", action="store_true", help="also report state populations, transition counts and "
                                                               "probabilities (time-ordered Langevin samples)")
    ap.add_argument("--traj-lengths", type=int, default=None, help="frames per trajectory of the samples")
    ap.add_argument("--parallel-sim", type=int, default=None, help="number of equal-length simulations in the samples")
    ap.add_argument("--lagtimes", default="1", help="comma-separated lag times in frames (with --transitions)")
    ap.add_argument("--n-clusters", type=int, default=None, help="fit this many state centres on --centers-fit-data")
    ap.add_argument("--centers-fit-data", default=None, help="structures (.pt, (n, N, 3) Angstrom) to fit the state "
                                                             "centres on instead of the presets")
    ap.add_argument("--coverage", default=None, metavar="REF.pt",
                    help="ensemble (.pt, (m, N, 3) Angstrom) to report novelty / coverage / diversity against")
    ap.add_argument("--rmsd-thresholds", type=rmsd_thresholds, default=(1.0, 2.0, 4.0),
                    help="comma-separated RMSD thresholds in Angstrom (with --coverage)")
    ap.add_argument("--coverage-subsample", type=int, default=None, metavar="K",
                    help="keep at most K evenly spaced frames of each ensemble (with --coverage)")
    ap.add_argument("--flexibility", default=None, metavar="HELDOUT.pt",
                    help="ensemble (.pt, (m, N, 3) Angstrom) to compare the per-bead RMSF and the mean structure with")
    ap.add_argument("--write-aligned", default=None, metavar="OUT.pt",
                    help="save the samples superposed on the folded structure (needs --folded-pdb)")
    ap.add_argument("--clusters", default=None, metavar="HELDOUT.pt",
                    help="ensemble (.pt, (m, N, 3) Angstrom) to cluster by RMSD; report its clusters' populations in the samples")
    ap.add_argument("--cluster-cutoff", type=cluster_cutoff, default=2.0, help="RMSD cutoff in Angstrom (with --clusters)")
    ap.add_argument("--cluster-stride", type=int, default=1, metavar="K",
                    help="cluster every K-th frame of the ensemble (with --clusters)")
    ap.add_argument("--kinetics", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report folding / unfolding counts, rates and dwell times (time-ordered Langevin samples; needs "
                         "--folded-pdb); with HELDOUT.pt also for that MD data")
    ap.add_argument("--kinetics-cv", choices=("q", "rmsd"), default="q",
                    help="order parameter: fraction of native contacts or RMSD to the folded structure (with --kinetics)")
    ap.add_argument("--kinetics-cores", type=cores, default=None, metavar="LO,HI",
                    help="the two cores cv <= LO and cv >= HI (with --kinetics; 0.2,0.9 for q)")
    ap.add_argument("--frame-time", type=frame_time, default=1.0, metavar="T",
                    help="time between two frames, the unit of the rates and dwell times (with --kinetics) and of the "
                         "relaxation times (with --relaxation) and the implied timescales (with --msm)")
    ap.add_argument("--paths", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report transition-path times, p(TP | cv) and the empirical committor (time-ordered Langevin "
                         "samples; needs --folded-pdb; cv, cores and frame time as for --kinetics); with HELDOUT.pt also for that MD data")
    ap.add_argument("--paths-bins", type=paths_bins, default=None, metavar="N",
                    help="bins of the order parameter for p(TP | cv) and the committor (with --paths; 50)")
    ap.add_argument("--relaxation", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report autocorrelation times, effective sample size and standard error of an observable "
                         "(time-ordered Langevin samples; needs --max-lag); with HELDOUT.pt also for that MD data")
    ap.add_argument("--relaxation-cv", choices=("q", "rmsd", "tic"), default="q",
                    help="observable: fraction of native contacts, RMSD to the folded structure (both need --folded-pdb) or "
                         "the TICs of MOL's saved TICA model (with --relaxation)")
    ap.add_argument("--max-lag", type=max_lag, default=None, metavar="L", help="largest lag in frames (with --relaxation)")
    ap.add_argument("--msm", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report a Markov state model's implied timescales (time-ordered Langevin samples; needs "
                         "--msm-states and --msm-lag); with HELDOUT.pt also for that MD data, on microstates fitted on it")
    ap.add_argument("--msm-states", type=msm_states, default=None, metavar="K", help="k-means microstates (with --msm)")
    ap.add_argument("--msm-lag", type=msm_lag, default=None, metavar="L", help="lag time in frames (with --msm)")
    ap.add_argument("--msm-lagtimes", type=msm_lagtimes, default=None, metavar="a,b,c",
                    help="also the implied timescales at these lag times in frames (with --msm)")
    ap.add_argument("--msm-bootstrap", type=msm_bootstrap, default=None, metavar="B",
                    help="bootstrap error bars of the implied timescales from B resamples (with --msm)")
    ap.add_argument("--msm-block-frames", type=msm_lag, default=None, metavar="F",
                    help="resample blocks of F frames instead of whole trajectories (with --msm-bootstrap)")
    ap.add_argument("--msm-confidence", type=msm_confidence, default=None, metavar="C",
                    help="confidence level of the percentile intervals, default 0.95 (with --msm-bootstrap)")
    ap.add_argument("--passage", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report mean first-passage times, rates and the committor between the folded and the unfolded "
                         "microstates of a Markov state model (time-ordered Langevin samples; needs --folded-pdb, --parallel-sim, "
                         "--passage-states and --passage-lag); with HELDOUT.pt also for that MD data, which then defines the states")
    ap.add_argument("--msm-eigensolver", choices=("host", "device"), default=None,
                    help="where the spectra of the Markov models are computed: numpy on the host (default) or dff_sym_eig_topk on "
                         "the GPU, all resamples of a bootstrap batch in one call (with --msm)")
    ap.add_argument("--msm-eigenvectors", type=msm_eigenvectors, default=None, metavar="N",
                    help="also the N slowest right eigenvectors of the model, under \"eigenvectors\" (with --msm)")
    ap.add_argument("--passage-states", type=msm_states, default=None, metavar="K", help="k-means microstates (with --passage)")
    ap.add_argument("--passage-lag", type=msm_lag, default=None, metavar="L", help="lag time in frames (with --passage)")
    ap.add_argument("--passage-cv", choices=("q", "rmsd"), default=None,
                    help="order parameter that sorts the microstates: fraction of native contacts (default) or RMSD (with --passage)")
    ap.add_argument("--passage-cores", type=cores, default=None, metavar="LO,HI",
                    help="a microstate is in a set when its mean cv is <= LO or >= HI (with --passage; 0.2,0.9 for q)")
    ap.add_argument("--passage-bootstrap", type=msm_bootstrap, default=None, metavar="B",
                    help="bootstrap error bars of the times and rates from B resamples of the trajectories (with --passage)")
    ap.add_argument("--ck", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report the Chapman-Kolmogorov test of a Markov state model on its metastable sets and its predicted "
                         "against the measured autocorrelation of the first TIC (time-ordered Langevin samples; needs --parallel-sim, "
                         "--ck-states and --ck-lag); with HELDOUT.pt also for that MD data, which then defines the sets")
    ap.add_argument("--ck-states", type=msm_states, default=None, metavar="K", help="k-means microstates (with --ck)")
    ap.add_argument("--ck-lag", type=msm_lag, default=None, metavar="L", help="lag time in frames (with --ck)")
    ap.add_argument("--ck-sets", type=ck_sets, default=None, metavar="M", help="metastable sets (with --ck; 3)")
    ap.add_argument("--ck-multiples", type=ck_multiples, default=None, metavar="1,2,3,4,5",
                    help="multiples of the lag time that are tested (with --ck)")
    ap.add_argument("--ck-bootstrap", type=msm_bootstrap, default=None, metavar="B",
                    help="percentile intervals of the test from B resamples of the trajectories (with --ck)")
    ap.add_argument("--hmm", nargs="?", const="", default=None, metavar="HELDOUT.pt",
                    help="also report a hidden Markov model of the microstate trajectory: timescales, populations and lifetimes of "
                         "its hidden states (time-ordered Langevin samples; needs --parallel-sim, --hmm-states, --hmm-hidden and "
                         "--hmm-lag); with HELDOUT.pt also for that MD data")
    ap.add_argument("--hmm-states", type=msm_states, default=None, metavar="K", help="k-means microstates (with --hmm)")
    ap.add_argument("--hmm-hidden", type=hmm_hidden, default=None, metavar="M", help="hidden states, 1..8 (with --hmm)")
    ap.add_argument("--hmm-lag", type=msm_lag, default=None, metavar="L", help="lag time in frames (with --hmm)")
    ap.add_argument("--hmm-bootstrap", type=number(int, lambda v: v >= 1, "expected a number of resamples >= 1, got {text!r}"),
                    default=None, metavar="B",
                    help="with --hmm: error bars of the timescales, lifetimes and populations from B bootstrap refits on the GPU "
                         "(bootstrap_hmm: timescales_std, lifetimes_std, hidden_populations_std, timescales_lo / _hi, bootstrap_failed)")
    ap.add_argument("--hmm-block-frames", type=number(int, lambda v: v >= 2, "expected a block length >= 2 frames, got {text!r}"),
                    default=None, metavar="N",
                    help="with --hmm-bootstrap: resample blocks of N frames (at least 2 --hmm-lag) instead of whole trajectories")
    ap.add_argument("--hmm-bootstrap-seed", type=int, default=None, metavar="S", help="with --hmm-bootstrap: the seed of the draws (0)")
    ap.add_argument("--hmm-path", choices=("posterior", "viterbi"), default=None,
                    help="with --hmm: the per-frame hidden states whose dwell statistics are reported -- the argmax of the posterior "
                         "marginals on the frame-ordered series, or the Viterbi path with the dwells taken inside the lagged chains")
    ap.add_argument("--js-bootstrap", type=number(int, lambda v: 1 <= v, "expected a number of resamples >= 1, got {text!r}"),
                    default=None, metavar="B",
                    help="also report block-bootstrap error bars of the JS metrics from B resamples (Evaluator.eval_bootstrap), "
                         "under \"js_bootstrap\": <key>, <key>_lo / _hi (95 %%), _std, _bias, n_units, n_resamples; the units are "
                         "the trajectories of --parallel-sim or their blocks, else --js-blocks blocks of the samples as given")
    ap.add_argument("--block-frames", type=number(int, lambda v: v >= 1, "expected a block length >= 1 frame, got {text!r}"),
                    default=None, metavar="F",
                    help="with --js-bootstrap and --parallel-sim: resample blocks of F frames instead of whole trajectories")
    ap.add_argument("--js-blocks", type=number(int, lambda v: v >= 1, "expected a number of blocks >= 1, got {text!r}"),
                    default=None, metavar="N",
                    help="with --js-bootstrap and without --parallel-sim: independent samples in N consecutive blocks (256)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def js_bootstrap_arguments(a):
    """the options of --js-bootstrap are refused without it, --block-frames without the trajectories it cuts"""
    if a.js_bootstrap is None:
        if a.block_frames is not None or a.js_blocks is not None:
            raise SystemExit("--block-frames and --js-blocks need --js-bootstrap")
        return
    if a.block_frames is not None and a.parallel_sim is None:
        raise SystemExit("--block-frames needs --parallel-sim (the trajectories it cuts into blocks)")
    if a.js_blocks is not None and a.parallel_sim is not None:
        raise SystemExit("--js-blocks is for independent samples: with --parallel-sim the units are the trajectories or --block-frames")


def main():
    ap = build_parser()
    a = ap.parse_args()
    if a.coverage_subsample is not None and a.coverage_subsample < 1:
        ap.error("--coverage-subsample must be >= 1")
    if a.cluster_stride < 1:
        ap.error("--cluster-stride must be >= 1")
    if a.write_aligned and not a.folded_pdb:
        ap.error("--write-aligned needs --folded-pdb")
    if a.kinetics is not None and not a.folded_pdb:
        ap.error("--kinetics needs --folded-pdb")
    paths_arguments(a)
    if a.relaxation is not None and a.relaxation_cv != "tic" and not a.folded_pdb:
        ap.error("--relaxation with --relaxation-cv q or rmsd needs --folded-pdb")
    if a.relaxation is not None:
        relaxation_max_lag(a)
    if a.msm is not None:
        msm_arguments(a)
    msm_bootstrap_arguments(a)
    msm_spectrum_arguments(a)
    passage_arguments(a)
    ck_arguments(a)
    hmm_arguments(a)
    js_bootstrap_arguments(a)
    x = torch.load(a.samples, map_location="cpu").float().contiguous()
    ref = torch.load(a.ref_data, map_location="cpu").float() if a.ref_data else None
    fit = torch.load(a.tica_fit_data, map_location="cpu") if a.tica_fit_data else None
    if isinstance(fit, torch.Tensor):
        fit = fit.float()
    elif fit is not None:
        fit = [torch.as_tensor(t).float() for t in fit]
    ev = evaluate.Evaluator(ref, None, a.mol, evalsetname=a.evalset, saved_ref_dir=a.saved_ref_dir,
                            tica_fit_data=fit, tica_lagtime=a.lagtime, device=a.device)
    res = ev.eval(x, 0)
    if a.js_bootstrap is not None:
        lengths = [len(x) // a.parallel_sim] * a.parallel_sim if a.parallel_sim else None
        if lengths is not None and sum(lengths) != len(x):
            raise SystemExit(f"{len(x)} frames do not split into {a.parallel_sim} equal trajectories")
        res["js_bootstrap"] = cleaned(ev.eval_bootstrap(x, traj_lengths=lengths, block_frames=a.block_frames,
                                                        n_blocks=a.js_blocks or 256, n_resamples=a.js_bootstrap))
    if a.folded_pdb:
        mol = a.mol.lower()
        re = evaluate.RmsdEvaluator(mol, a.folded_pdb, saved_ref_dir=a.saved_ref_dir, device=a.device)
        rmsd = re.rmsd(x)
        res["RMSD mean"] = float(np.nanmean(rmsd))
        curve = evaluate.rmsd_curve(rmsd, evaluate.RMSD_NBINS_REF, evaluate.RMSD_CUTOFF_REF.get(mol))
        res["RMSD curve"] = {"bin_mids": curve["bin_mids"].tolist(),
                             "energies": clean(list(curve["energies"]))}
        _, mean = evaluate.ContactEvaluator(mol, a.folded_pdb, device=a.device).contact_bce(x)
        res["Contact BCE"] = float(mean)
    if a.transitions:
        res["Transitions"] = transitions(a, x)
    if a.coverage:
        res["coverage"] = coverage(a, x)
    if a.flexibility:
        res["flexibility"] = flexibility(a, x)
    if a.clusters:
        res["clusters"] = clusters(a, x)
    if a.kinetics is not None:
        res["kinetics"] = kinetics(a, x)
    if a.paths is not None:
        res["paths"] = paths(a, x)
    if a.relaxation is not None:
        res["relaxation"] = relaxation(a, x)
    if a.msm is not None:
        res["msm"] = msm(a, x)
    if a.passage is not None:
        res["passage"] = passage(a, x)
    if a.ck is not None:
        res["ck"] = ck(a, x)
    if a.hmm is not None:
        res["hmm"] = hmm(a, x)
    if a.write_aligned:
        write_aligned(a, x)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
