"""The host stand-ins that more than one test file puts behind a seam of dff_amd.evaluate (reversible_sweeper, spectral_solver,
hmm_estep_solver, hmm_viterbi_solver): the oracle's numpy statement of what the device solver computes, with the solver's
signature.  Not a test and not a conftest; a test file imports the classes it needs and keeps its own `on_host` fixture, which
says what it replaces.  A stand-in that only one file uses, or that differs from these, stays in its file."""
import numpy as np
import torch

import eig_cases as ec
import hmm_cases as hc
import viterbi_cases as vc
from dff_amd import binding
from oracle import msm as oracle


class OracleSweeps:
    """behind evaluate.reversible_sweeper: the reversible estimator on the oracle's numpy sweeps"""

    def __init__(self, S, c, device):
        self.S, self.c = np.array(S), np.array(c)

    def __call__(self, x, n):
        return oracle.sweeps(self.S, self.c, np.array(x), n)


class HostSpectral:
    """behind evaluate.spectral_solver: eig_cases.host_topk"""

    def __init__(self, device):
        pass

    def __call__(self, a, ks, k, vectors):
        return ec.host_topk(np.asarray(a), ks, k, vectors)


class HostEstep:
    """behind evaluate.hmm_estep_solver: hmm_cases.host_estep at the library's chunk; `calls` counts the E-steps since a test
    last reset it"""
    calls = 0

    def __init__(self, device):
        pass

    def __call__(self, labels, lengths, lag, A, B, p0, want_post=False):
        HostEstep.calls += 1
        stats, cl, post, status = hc.host_estep(np.asarray(labels), lengths, lag, A, B, p0, binding.hmm_chunk())
        return stats, (cl if want_post else None), (torch.from_numpy(post) if want_post else None), status


class HostViterbi:
    """behind evaluate.hmm_viterbi_solver: viterbi_cases.host_viterbi at the library's chunk, on labels from the host or the
    device; `calls` logs (lag, chain_order, la, lb, lp) of every call since a test last reset it"""
    calls = []

    def __init__(self, device):
        pass

    def __call__(self, labels, lengths, lag, la, lb, lp, chain_order=False):
        HostViterbi.calls.append((lag, bool(chain_order), np.array(la), np.array(lb), np.array(lp)))
        lab = np.asarray(torch.as_tensor(labels).cpu())
        path, cl, status = vc.host_viterbi(lab, lengths, lag, la, lb, lp, binding.hmm_chunk(), chain_order)
        return torch.from_numpy(path), cl, status
