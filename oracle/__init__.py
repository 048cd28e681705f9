"""oracle/ -- TEST INFRASTRUCTURE ONLY.

CPU restatements of the reference's sampling hot path (microsoft/two-for-one-diffusion):

* ``reference_twin``  -- op-for-op PyTorch-CPU twin of ``models/graph_transformer.py``,
  ``models/ddpm.py`` (sampling half), ``dynamics/langevin.py`` and
  ``dynamics/langevin_cgnet.py`` in the reference's own *materialised* formulation
  (N x N x 512 edge tensor, ``torch.autograd`` for the force).  This is the parity oracle
  and the thing ``bench.py`` times as ``cpu_baseline`` (kind "port").
* ``kernel_model``    -- float64 numpy statement of the *factorised* algorithm the HIP
  kernels implement (edge tensor folded away, hand-written VJP), exposing every
  intermediate the kernel stashes, for stage-by-stage debugging of the device code.
* ``synth``           -- deterministic synthetic weights (splitmix64; no torch RNG) in the
  reference's state-dict layout.  The shipped checkpoints are absent from the reference
  mount (``/root/reference/.MISSING_LARGE_BLOBS:7-15``), so parity is pinned on these.

* ``pwd_metric``      -- numpy restatement of the reference's pairwise-distance Jensen-Shannon
  metric in torch's float32 arithmetic, pinned by ``tests/golden/pwd_*.npz``.
* ``noise``           -- the in-kernel noise stream on the host: Philox4x32-10 and Box-Muller.
* ``struct_metric``   -- float64 numpy oracles of the structure kernels: dihedrals, TIC features
  and projection, contacts (torch's float32 formula), and the one Kabsch superposition by SVD
  (``kabsch64`` per frame, ``kabsch64_batch``, ``kabsch_matrix``, ``superpose64`` / ``stats64``
  with Horn's eigenvalue gap).
* ``tica_fit``        -- float64 sums of ``dff_tica_moments`` and the model comparisons of the
  TICA tests.
* ``states``          -- float64 restatements of the nearest-centre rule, Lloyd's loop and the
  transition counts (deeptime's documented semantics).
* ``frames``          -- the seeded input generators of the analysis tests (rotations, walks,
  needles, chains, Ornstein-Uhlenbeck trajectories, blobs, labels).
* ``cluster``         -- the neighbour bit-matrix and the gromos clustering from float64 pair RMSDs.
* ``kinetics``        -- native-contact Q, core states and label runs by plain loops.
* ``autocorr``        -- lagged sums and autocorrelation estimates by a loop over trajectories and lags.
* ``msm``             -- Markov state models from scratch in float64: nearest centre, transition counts, the largest
  connected set, the reversible estimator's sweeps.
* ``msm_bootstrap``   -- the bootstrap of ``msm``: weighted counts pair by pair, the pipeline per resample, and the numpy
  stand-ins the host tests put behind the device seams.
* ``passage``         -- the Dirichlet problem of ``dff_msm_dirichlet_solve`` in numpy: the fp64 system, a longdouble-refined
  truth, error measures, and the kernel's elimination as the stand-in behind ``evaluate.dirichlet_solver``.

The analysis modules need numpy and torch-CPU only and never import ``dff_amd``.

Pinning: the reference has no tests / golden vectors for this path.  The
twin is pinned against the reference ITSELF, imported in the build container, by
``tests/golden/make_golden.py``; the resulting input/output vectors are committed under
``tests/golden/*.npz`` and ``tests/test_oracle_golden.py`` checks the twin against them on
every run (CPU, no reference needed).

Nothing under ``two-for-one-diffusion_amd/`` may import this package: only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg use it, as the checker.
"""
