"""The numpy statement of dff_hmm_fit_steps (include/dff.h) that tests/test_hmm_fit.py and tests/test_hmm_fit_host.py hold the
kernel and its Python layer to (not a test; no GPU).

mstep()   one M-step, in fp64.  Every sum is an explicit loop over j or s, one term after the other from +0, vectorised over i
          only: every element's order of additions is the stated one, so a kernel that keeps the order has these bits.
replay()  the step loop of the call over ANY E-step callable estep(labels, lengths, lag, A, B, p0) -> (stats packed as
          dff_hmm_estep packs them, status): the stop word, the convergence rule, the flags and the sweep count.
The E-step is never restated here: on the device replay() runs over dff_hmm_estep itself, whose bits the call must reproduce."""
import numpy as np

NAN = float("nan")


def new_state():
    return {"n_estep": 0, "stop": 0, "estep_status": 0, "flags": 0, "last_loglik": 0.0, "rev_sweeps": 0}


def ordered_sum(x, axis_len):
    """sum over the LAST axis in index order from +0 (vectorised over the others)"""
    acc = np.zeros(x.shape[:-1], np.float64)
    for k in range(axis_len):
        acc = acc + x[..., k]
    return acc


def strongly_connected(xi):
    """every state is reached from state 0 and reaches it over the edges i -> j with xi[i, j] > 0"""
    m = len(xi)
    adj = xi > 0
    fwd, bwd = {0}, {0}
    for _ in range(m):
        fwd |= {j for i in fwd for j in range(m) if adj[i, j]}
        bwd |= {i for i in range(m) if any(adj[i, j] for j in bwd)}
    return len(fwd) == m and len(bwd) == m


def flow(S, c, x):
    q = c / x
    den = q[:, None] + q[None, :]
    return np.divide(S, den, out=np.zeros_like(S), where=S != 0)


def reversible(xi, rev_tol, rev_max_sweeps):
    """(A, pi, sweeps, capped) of the reversible estimator on m >= 2 strongly connected states"""
    m = len(xi)
    S = xi + xi.T
    c = ordered_sum(xi, m)
    x = 0.5 * ordered_sum(S, m)
    sweeps, met = 0, False
    with np.errstate(all="ignore"):
        while sweeps < rev_max_sweeps:
            xn = ordered_sum(flow(S, c, x), m)
            err = np.max(np.abs(xn - x) / x)                        # np.max keeps a NaN
            x = xn
            sweeps += 1
            if err < rev_tol:
                met = True
                break
            if not np.isfinite(err):
                break
        t = flow(S, c, x)
        return t / x[:, None], x / ordered_sum(x[None, :], m)[0], sweeps, (not met and sweeps >= rev_max_sweeps)


def mstep(stats, A, B, p0, m, K, reversible_, rev_tol=1e-12, rev_max_sweeps=1_000_000):
    """-> dict: A, B, p0 (new arrays), pi (None unless a reversible step wrote it), flags (bits to OR in), sweeps, lost (True: the
    graph is not strongly connected -- stop 3, A, B, p0 are the old ones)"""
    stats = np.asarray(stats, np.float64)
    xi = stats[1:1 + m * m].reshape(m, m)
    g0 = stats[1 + m * m:1 + m * m + m]
    gs = stats[1 + m * m + m:].reshape(m, K)
    A, B, p0 = np.array(A, np.float64), np.array(B, np.float64), np.array(p0, np.float64)
    flags = 0
    occ = ordered_sum(gs, K)
    if (occ <= 0).any():
        flags |= 1
    with np.errstate(all="ignore"):
        Bn = np.where(occ[:, None] > 0, gs / occ[:, None], B)
        g = ordered_sum(g0[None, :], m)[0]
        pn = g0 / g if g > 0 else p0
        if reversible_:
            if m > 1 and not strongly_connected(xi):
                return {"A": A, "B": B, "p0": p0, "pi": None, "flags": flags, "sweeps": 0, "lost": True}
            if m == 1:
                return {"A": np.ones((1, 1)), "B": Bn, "p0": pn, "pi": np.ones(1), "flags": flags, "sweeps": 0, "lost": False}
            An, pi, sweeps, capped = reversible(xi, rev_tol, rev_max_sweeps)
            return {"A": An, "B": Bn, "p0": pn, "pi": pi, "flags": flags | (2 if capped else 0), "sweeps": sweeps, "lost": False}
        r = ordered_sum(xi, m)
        if (r <= 0).any():
            flags |= 1
        An = np.where(r[:, None] > 0, xi / r[:, None], A)
    return {"A": An, "B": Bn, "p0": pn, "pi": None, "flags": flags, "sweeps": 0, "lost": False}


def replay(estep, labels, lengths, lag, A, B, p0, reversible_, n_steps, accuracy, state=None, rev_tol=1e-12,
           rev_max_sweeps=1_000_000, pi=None):
    """the step loop of dff_hmm_fit_steps -> (A, B, p0, loglik (n_steps,), pi | None, state)"""
    A, B, p0 = np.array(A, np.float64), np.array(B, np.float64), np.array(p0, np.float64)
    m, K = B.shape
    st = dict(new_state() if state is None else state)
    ll = np.full(n_steps, NAN)
    for s in range(n_steps):
        if st["stop"]:
            continue
        stats, status = estep(labels, lengths, lag, A, B, p0)
        st["n_estep"] += 1
        st["estep_status"] = int(status)
        if status:
            st["stop"] = 2
            continue
        L = float(stats[0])
        ll[s] = L
        if st["n_estep"] > 1 and abs(L - st["last_loglik"]) < accuracy:
            st["stop"], st["last_loglik"] = 1, L
            continue
        st["last_loglik"] = L
        new = mstep(stats, A, B, p0, m, K, reversible_, rev_tol, rev_max_sweeps)
        st["flags"] |= new["flags"]
        if new["lost"]:
            st["stop"] = 3
            continue
        A, B, p0 = new["A"], new["B"], new["p0"]
        pi = new["pi"] if new["pi"] is not None else pi
        st["rev_sweeps"] += new["sweeps"]
    return A, B, p0, ll, pi, st


class ReplaySolver:
    """the stand-in behind evaluate.hmm_fit_solver: replay() over a host E-step (stats, chain_loglik, post, status)"""
    host_estep = None                                               # set by the test: hmm_cases.host_estep with the chunk bound

    def __init__(self, device):
        self.pi = None
        self.calls = 0

    def steps(self, labels, lengths, lag, A, B, p0, reversible_, n_steps, accuracy, state=None, *, rev_tol=1e-12,
              rev_max_sweeps=1_000_000):
        self.calls += 1
        if state is None:
            self.pi = None
        lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels)

        def estep(labels_, lengths_, lag_, a, b, p):
            out = type(self).host_estep(labels_, lengths_, lag_, a, b, p)
            return out[0], out[3]
        A, B, p0, ll, self.pi, st = replay(estep, lab, list(lengths), lag, A, B, p0, reversible_, n_steps, accuracy, state, rev_tol,
                                           rev_max_sweeps, self.pi)
        return A, B, p0, ll, self.pi, st
