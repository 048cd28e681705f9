#!/usr/bin/env python3
"""Record the trp-cage TICA covariances of the reference's saved model, for the host test of the TICA decomposition.

Run once, from any directory, with a checkout of the reference project (the tests never read it):

    python tests/golden/make_golden_tica_fit.py REFERENCE_ROOT

Reads evaluate/saved_references/saved_TICA_TRP_CAGE_testset.pickle through the restricted unpickler of
two-for-one-diffusion_amd/evaluate.py (no deeptime, no code from the pickle runs) and writes DATA only:
  tica_trp_cage_cov.npz   cov_00_triu / cov_0t_triu   upper triangles of deeptime's C00 / C0t, np.triu_indices(F) order
                          mean                        mean_0 (F,)
                          singular_values             the model's singular values (F,)
                          sqrt_inv_cov_lead           the leading NCOL columns of the instantaneous whitening's
                                                      sqrt_inv_cov (the kinetic-map coefficients)
                          lagtime, epsilon            the fitted model's settings
The chignolin model is tested from its own pickle (tests/golden/saved_TICA_CHIGNOLIN_testset.pickle).
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else sys.exit("usage: make_golden_tica_fit.py REFERENCE_ROOT")
OUT = os.path.dirname(os.path.abspath(__file__))
NCOL = 8
sys.path.insert(0, REPO)

from dff_amd.evaluate import restricted_load  # noqa: E402


def main():
    tica = restricted_load(os.path.join(REF, "evaluate", "saved_references", "saved_TICA_TRP_CAGE_testset.pickle"))[0]
    model, cov = tica._model, tica._model._cov
    c00, c0t = np.asarray(cov._cov_00, np.float64), np.asarray(cov._cov_0t, np.float64)
    iu = np.triu_indices(c00.shape[0])
    np.savez(os.path.join(OUT, "tica_trp_cage_cov.npz"),
             cov_00_triu=c00[iu], cov_0t_triu=c0t[iu], mean=np.asarray(cov._mean_0, np.float64),
             singular_values=np.asarray(model._singular_values, np.float64),
             sqrt_inv_cov_lead=np.asarray(model._whitening_instantaneous.sqrt_inv_cov, np.float64)[:, :NCOL],
             lagtime=np.int64(cov._lagtime), epsilon=np.float64(tica._epsilon))
    print("wrote", os.path.join(OUT, "tica_trp_cage_cov.npz"))


if __name__ == "__main__":
    main()
