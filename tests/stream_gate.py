"""The stream-order protocol: how a test shows that an ABI call is ordered on the caller's stream, and only on it
(include/dff.h: "calls enqueue on `stream` ... and do not synchronise"; README: "the launch path never synchronises").
tests/test_stream_order.py runs it on every call; a later kernel's test file runs it on its own (tests/test_superpose.py).

Every other GPU test runs on PyTorch's default stream, where a memset, a copy or a launch that went to the null stream, or a
stray device synchronisation, changes nothing.  Here every call runs on a side stream behind a GATE: torch.cuda._sleep, a
device-side spin that involves none of this project's code.  Behind the gate, on the same stream, the real inputs are copied
over buffers that hold POISON (a legal input that gives another output: NaN coordinates, constant labels / levels / bin counts,
other finite constants for limits, means and matrices -- never an index out of range) and the outputs are filled with a
SENTINEL (123.0, 0x7b7b7b7b).  Anything the call enqueues elsewhere runs during the gate: a misplaced kernel reads poison or
is overwritten by the sentinel fill, a misplaced zeroing memset leaves sentinel + counts, a copy not ordered after its producer
copies stale data.  The result must equal the default-stream result bit for bit (run twice there, so that a non-deterministic
call cannot pass by luck), no sentinel may survive where the call writes, and -- for every call that is not in BLOCKING -- the
call must have returned while the gate was still spinning (the gate's event not yet complete): it synchronised nothing.  The
failure of a misordered call is deterministic; nothing here tries to win a race.  test_stream_order.py::test_control_* shows
that the harness itself sees work on the wrong stream.

The gate is a stimulus, not a tolerance: about 100 ms against the tens of microseconds of an enqueue; a calibration that gives
less than 50 ms fails every test with "gate too short".
MEASURED on the MI355X: _sleep of 2 000 000 cycles = 0.847 ms, of 20 000 000 cycles = 8.335 ms -> 2.404e6 cycles / ms (the 2.4 GHz
shader clock); the gate of 240 362 198 cycles = 100.0 ms.
MEASURED on the MI355X: every call of test_stream_order.py returned inside its gate except the cold model calls (BLOCKING); a
test takes 0.25 - 0.45 s (two gates and a model upload for the model calls), the file 18 s.

The fixtures `gate` and `side` are imported by name.  Pytest does not rewrite the asserts of this module: each carries its
message."""
import pytest
import torch

# Calls that must block the host, with the reason (include/dff.h says so for each).  Everything else is asserted to return
# while its gate is still spinning.  A WARM dff_score / dff_langevin_run / dff_ddpm_run may not be listed here.
BLOCKING = {
    ("dff_score", "cold"): "the first call at a batch size grows the model's scratch (hipFree / hipMalloc)",
    ("dff_langevin_run", "cold"): "the first call at a noise level builds the layer-0 table: allocations, a host-to-device copy of "
                                  "the levels and stream synchronisations between its chunks",
    ("dff_ddpm_run", "cold"): "as dff_langevin_run, one table entry per noise level",
}

GATE_MS = 100.0          # the gate aimed at
GATE_MIN_MS = 50.0       # "gate too short" below this
F_SENTINEL = 123.0
I_SENTINEL = 0x7B7B7B7B


# ------------------------------------------------------------------------------------------------ the gate
class Gate:
    def __init__(self, rate, cycles, ms):
        self.rate, self.cycles, self.ms = rate, cycles, ms


def time_sleep(stream, cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def gate():
    """torch.cuda._sleep alone at two cycle counts -> cycles per millisecond -> the cycle count of a GATE_MS gate, timed once."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    s = torch.cuda.Stream()
    time_sleep(s, 1000)                        # (loads the spin kernel)
    c1, c2 = 2_000_000, 20_000_000
    t1, t2 = time_sleep(s, c1), time_sleep(s, c2)
    rate = (c2 - c1) / max(t2 - t1, 1e-6)      # cycles per ms
    cycles = int(rate * GATE_MS)
    ms = time_sleep(s, cycles)
    print(f"[stream] _sleep: {c1} cycles = {t1:.3f} ms, {c2} cycles = {t2:.3f} ms -> {rate:.4g} cycles / ms; "
          f"gate of {cycles} cycles = {ms:.1f} ms")
    return Gate(rate, cycles, ms)


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream()


# ------------------------------------------------------------------------------------------------ one gated call
class Spec:
    """One call: `ins` name -> (real device tensor, poison: a scalar or a tensor), `outs` name -> (shape, dtype) of the pure
    outputs, `inout` the inputs the call also writes, `work` name -> workspace tensor, fn(nat, bufs) the call itself on the
    current stream (nat: the model, None for the stateless calls), `unwritten` the outputs whose sentinel may survive,
    wrap(nat, bufs) -> name -> tensor: the binding's allocating wrapper of the same call, when it reads nothing back."""

    def __init__(self, name, ins, outs, fn, inout=(), work=None, unwritten=(), wrap=None):
        self.name, self.ins, self.outs, self.fn, self.inout = name, ins, outs, fn, tuple(inout)
        self.work, self.unwritten, self.wrap = work or {}, tuple(unwritten), wrap

    @property
    def results(self):
        return tuple(self.outs) + self.inout


def sentinel(dtype):
    return F_SENTINEL if dtype.is_floating_point else (0x7B if dtype == torch.uint8 else I_SENTINEL)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def poisoned(real, poison):
    if isinstance(poison, torch.Tensor):
        assert poison.shape == real.shape and poison.dtype == real.dtype, \
            f"poison {tuple(poison.shape)} {poison.dtype} for an input {tuple(real.shape)} {real.dtype}"
        return poison.clone()
    return torch.full_like(real, poison)


def device_of(spec):
    """Where a Spec's buffers live: the GPU for every ABI call; the CPU for the stand-in calls of tests/test_fence.py's controls."""
    return next(iter(spec.ins.values()))[0].device


def reference(spec, nat=None):
    """Step 1: the call on the default stream with the real inputs, twice, bit-equal -> name -> result."""
    dev = device_of(spec)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    runs = []
    for _ in range(2):
        bufs = {k: real.clone() for k, (real, _) in spec.ins.items()}
        for k, (shape, dtype) in spec.outs.items():
            bufs[k] = torch.full(shape, sentinel(dtype), dtype=dtype, device=dev)
        bufs.update(spec.work)
        spec.fn(nat, bufs)
        sync()
        runs.append({k: bufs[k].clone() for k in spec.results})
    for k in spec.results:
        assert bits_equal(runs[0][k], runs[1][k]), f"{spec.name}: {k} differs between two default-stream calls"
    sync()
    return runs[0]


class Run:
    """Steps 2 - 4 of one gated call, split so that two of them can be in flight on two streams."""

    def __init__(self, spec, nat=None):
        self.spec, self.nat = spec, nat
        self.real = {k: real.clone() for k, (real, _) in spec.ins.items()}
        self.bufs = {k: poisoned(real, poison) for k, (real, poison) in spec.ins.items()}
        for k, (shape, dtype) in spec.outs.items():
            self.bufs[k] = torch.zeros(shape, dtype=dtype, device="cuda")
        self.bufs.update(spec.work)
        self.got = {k: torch.empty_like(self.bufs[k]) for k in spec.results}
        self.wrapped = None
        self.ev_gate, self.ev_done = torch.cuda.Event(), torch.cuda.Event()
        self.returned_early = None

    def enqueue(self, stream, gate):
        assert gate.ms >= GATE_MIN_MS, f"gate too short: {gate.ms:.1f} ms ({gate.cycles} cycles at {gate.rate:.4g} cycles / ms)"
        spec = self.spec
        with torch.cuda.stream(stream):
            torch.cuda._sleep(gate.cycles)
            self.ev_gate.record()
            for k in spec.ins:
                self.bufs[k].copy_(self.real[k])
            for k, (_, dtype) in spec.outs.items():
                self.bufs[k].fill_(sentinel(dtype))
            for k in spec.work:         # a workspace arrives dirty: zeros are what a minimum over keys cannot recover from
                self.bufs[k].zero_()
            spec.fn(self.nat, self.bufs)
            self.returned_early = not self.ev_gate.query()      # step 5: before anything else touches the device
            for k in spec.results:
                self.got[k].copy_(self.bufs[k])
            if spec.wrap is not None:
                self.wrapped = spec.wrap(self.nat, self.bufs)
            self.ev_done.record()
        return self

    def check(self, stream, ref, nonblocking, tag=""):
        spec = self.spec
        what = f"{spec.name}{tag}"
        if nonblocking:
            assert self.returned_early, f"{what}: the call returned only after the gate had finished: it synchronised"
        stream.synchronize()
        for k in spec.results:
            assert bits_equal(self.got[k], ref[k]), f"{what}: {k} on the side stream differs from the default-stream result"
        for k, (_, dtype) in spec.outs.items():
            if k not in spec.unwritten:
                assert not bool((self.got[k] == sentinel(dtype)).any()), f"{what}: a sentinel survives in {k}"
        for k, v in (self.wrapped or {}).items():
            assert bits_equal(v, ref[k]), f"{what}: {k} of the binding's wrapper differs from the default-stream result"


def gated(spec, stream, gate, ref, nat=None, nonblocking=True, tag=""):
    run = Run(spec, nat)
    torch.cuda.synchronize()
    run.enqueue(stream, gate).check(stream, ref, nonblocking, tag)
    return run


# ------------------------------------------------------------------------------------------------ the stateless (analysis) calls
N_FRAMES = 1000


def raw(name, *args):
    from dff_amd import binding
    lib = binding.load_library()
    binding._check(lib, getattr(lib, name)(*args), name)


def ptr(t):
    from dff_amd import binding
    return binding._ptr(t)


def stream_of(t):
    from dff_amd import binding
    return binding._stream(t)


def analysis_call(spec, gate, side):
    ref = reference(spec)
    gated(spec, side, gate, ref, nonblocking=(spec.name, "warm") not in BLOCKING)
    return ref
