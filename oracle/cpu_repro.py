"""Host-independent float32 arithmetic on the CPU, for the tests that hold the twin to the reference bit for bit.

torch's CPU results depend on the host: the thread count splits reductions, the ATen kernels are picked per ISA (AVX2 /
AVX-512) and MKL's GEMMs per ISA and thread count.  Under PIN_ENV -- one thread, ATen's portable kernels, MKL's
conditional bitwise reproducible path, no oneDNN -- the same program gives the same bits on any x86-64 host.  The
golden float32 vectors of the reference (tests/golden/make_golden*.py) are recorded under it, and the twin is compared
against them under it.

The variables must be in the environment before torch starts, so `call()` runs the function in a fresh interpreter;
a generator script calls `pin()` before it imports torch.
"""
import os
import pickle
import subprocess
import sys
import tempfile

PIN_ENV = {"OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1", "ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pin():
    """Pin this process (before torch is imported)."""
    assert "torch" not in sys.modules or all(os.environ.get(k) == v for k, v in PIN_ENV.items()), \
        "cpu_repro.pin() must run before torch is imported"
    os.environ.update(PIN_ENV)
    import torch
    torch.set_num_threads(1)
    torch.backends.mkldnn.enabled = False


def call(fn, *args, **kwargs):
    """fn(*args, **kwargs) -- fn a module-level function, arguments and result picklable (numpy arrays, tensors) --
    computed in a pinned child interpreter."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.pkl"), os.path.join(d, "out.pkl")
        with open(src, "wb") as f:
            pickle.dump((fn.__module__, fn.__qualname__, args, kwargs), f)
        env = {k: v for k, v in os.environ.items() if k not in ("GOMP_CPU_AFFINITY", "KMP_AFFINITY")}
        env.update(PIN_ENV)
        r = subprocess.run([sys.executable, "-s", "-c", "import sys; sys.path.insert(0, sys.argv[1]); "
                            "from oracle import cpu_repro; cpu_repro._child(sys.argv[2], sys.argv[3])", ROOT, src, dst],
                           env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"pinned call of {fn.__qualname__} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        with open(dst, "rb") as f:
            return pickle.load(f)


def _child(src, dst):
    pin()
    import importlib
    with open(src, "rb") as f:
        mod, name, args, kwargs = pickle.load(f)
    fn = importlib.import_module(mod)
    for part in name.split("."):
        fn = getattr(fn, part)
    out = fn(*args, **kwargs)
    with open(dst, "wb") as f:
        pickle.dump(out, f)


def twin_p_sample_loop(p, x_start, noises, t_start, n_layers):
    """reference_twin.p_sample_loop with the noise schedule built in the (pinned) calling process."""
    from oracle import reference_twin as twin
    return twin.p_sample_loop(p, twin.make_schedule(), x_start, noises, t_start, n_layers)
