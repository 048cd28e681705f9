"""Seeded log-parameters and label sets, the truth, the yardstick and the measure that tests/test_hmm_viterbi.py and
tests/test_hmm_viterbi_host.py hold dff_hmm_viterbi and its Python layer to (not a test).  Chains, chunk lengths, models and
labels are those of tests/hmm_cases.py.

The call: the most probable hidden path of every chain under LOG-parameters la (m, m), lb (m, K), lp (m) (include/dff.h); a
negative label is a missing observation (log-emission 0 for every state), every argmax takes the lowest index.
Truth: sequential(..., np.longdouble), the textbook recursion delta_t(j) = max_i (delta_{t-1}(i) + la[i][j]) + le_t(j), every chain on
its own.  Yardstick: the same recursion in np.float64.
chunked(): a numpy fp64 statement of the call's algorithm at the kernel's chunk length, in the header's order of additions --
max-plus chunk products, forward carries, the apply pass with back-pointers and the chunk's back map, backward carries,
backtrack.
score(): the joint log-probability of a path and its labels in long double.
Measure E, with `optimum` the score of the truth's path of the chain: for a path (optimum - score(path)) / (2^-52 |optimum|), for
chain_logprob |value - optimum| / (2^-52 |optimum|); the worst chain counts.
Bar: 8 x the larger of the two numpy E's (sequential fp64, chunked) of the same output on the same case, floored at one unit
before the factor (the rule of tests/hmm_cases.py).  The kernel is never its own reference."""
import functools

import numpy as np

import hmm_cases as hc

EPS = hc.EPS
FACTOR = hc.FACTOR
OUTPUTS = ("path", "chain_logprob")


def emission(lb, o):
    """lb[:, o], or zeros for a missing observation (and for a label >= K, which the call reports as status 3)"""
    return lb[:, o] if 0 <= o < lb.shape[1] else np.zeros(lb.shape[0], lb.dtype)


def _best(x, axis):
    """(the max along `axis`, the LOWEST index attaining it): np.argmax returns the first occurrence; the value is gathered, so
    it is the very element a strict '>' scan from index 0 keeps"""
    a = x.argmax(axis=axis)
    return np.take_along_axis(x, np.expand_dims(a, axis), axis).squeeze(axis), a


# ---------------------------------------------------------------- the textbook recursion on one chain at a chosen dtype
def sequential(obs, la, lb, lp, dtype):
    """(path int32 (L,), log-probability) of one chain; an empty chain: (empty, 0)"""
    la, lb, lp = np.asarray(la, dtype), np.asarray(lb, dtype), np.asarray(lp, dtype)
    L, m = len(obs), len(lp)
    if L == 0:
        return np.zeros(0, np.int32), dtype(0)
    with np.errstate(all="ignore"):
        d = lp + emission(lb, obs[0])
        psi = np.zeros((L, m), np.int64)
        for t in range(1, L):
            mx, psi[t] = _best(d[:, None] + la, 0)
            d = mx + emission(lb, obs[t])
    path = np.empty(L, np.int32)
    s = int(d.argmax())
    logprob = d[s]
    for t in range(L - 1, -1, -1):
        path[t] = s
        s = int(psi[t, s])
    return path, logprob


def sequential_all(labels, lengths, lag, la, lb, lp, dtype):
    """every chain on its own -> (path (n,) int32 in frame order, chain_logprob (n_traj lag,) of `dtype`)"""
    labels = np.asarray(labels)
    path, cl = np.zeros(len(labels), np.int32), []
    for idx in hc.chains(lengths, lag):
        p, v = sequential(labels[idx], la, lb, lp, dtype)
        path[idx] = p
        cl.append(v)
    return path, np.array(cl, dtype)


# ---------------------------------------------------------------- the chunked algorithm of the call, numpy fp64
def chunked_chain(obs, la, lb, lp, C):
    L, m = len(obs), len(lp)
    if L == 0:
        return np.zeros(0, np.int32), 0.0
    nch = (L + C - 1) // C
    ninf = -np.inf
    with np.errstate(all="ignore"):
        # (1) chunk products
        prods = []
        for k in range(nch):
            P = np.where(np.eye(m, dtype=bool), 0.0, ninf)
            for t in range(max(k * C, 1), min(L, (k + 1) * C)):
                P = _best(P[:, :, None] + la[None, :, :], 1)[0] + emission(lb, obs[t])[None, :]
            prods.append(P)
        # (2) forward carries
        din, d = [], lp + emission(lb, obs[0])
        for k in range(nch):
            din.append(d)
            d = _best(d[:, None] + prods[k], 0)[0]
        # (3) apply
        psi = np.zeros((L, m), np.int64)
        origin = []
        for k in range(nch):
            d, org = din[k], np.arange(m)
            for t in range(max(k * C, 1), min(L, (k + 1) * C)):
                mx, psi[t] = _best(d[:, None] + la, 0)
                d = mx + emission(lb, obs[t])
                org = org[psi[t]]
            origin.append(org)
        s = int(d.argmax())
        logprob = float(d[s])
    # (4) backward carries
    end = [0] * nch
    for k in range(nch - 1, -1, -1):
        end[k] = s
        s = int(origin[k][s])
    # (5) backtrack
    path = np.empty(L, np.int32)
    for k in range(nch):
        s, t0 = end[k], k * C
        for t in range(min(L, (k + 1) * C) - 1, t0 - 1, -1):
            path[t] = s
            if t > t0:
                s = int(psi[t, s])
    return path, logprob


def chunked(labels, lengths, lag, la, lb, lp, chunk):
    la, lb, lp = np.asarray(la, np.float64), np.asarray(lb, np.float64), np.asarray(lp, np.float64)
    labels = np.asarray(labels)
    path, cl = np.zeros(len(labels), np.int32), []
    for idx in hc.chains(lengths, lag):
        p, v = chunked_chain(labels[idx], la, lb, lp, int(chunk))
        path[idx] = p
        cl.append(v)
    return path, np.array(cl, np.float64)


def chain_order(lengths, lag):
    """the frame index of every position of the chain-ordered path: the chains back to back, r-major, f-minor"""
    ch = hc.chains(lengths, lag)
    return np.concatenate(ch) if ch else np.zeros(0, np.int64)


# ---------------------------------------------------------------- the call's contract on the host (the tests' stand-in)
def host_viterbi(labels, lengths, lag, la, lb, lp, chunk=128, chain_order_=False):
    """dff_hmm_viterbi on numpy -> (path (n,) int32, chain_logprob (n_traj lag,), status)"""
    la, lb, lp = np.asarray(la, np.float64), np.asarray(lb, np.float64), np.asarray(lp, np.float64)
    labels = np.asarray(labels)
    K = lb.shape[1]
    bad = lambda x: bool((np.isnan(x) | (x == np.inf)).any())      # noqa: E731
    status = 1 if bad(la) or bad(lb) or bad(lp) else (3 if (labels >= K).any() else 0)
    if status == 0:
        path, cl = chunked(labels, lengths, lag, la, lb, lp, chunk)
        full = np.array([len(c) > 0 for c in hc.chains(lengths, lag)], bool)
        if (cl[full] == -np.inf).any():
            status = 2
    if status:
        return np.full(len(labels), -1, np.int32), np.full(len(lengths) * lag, np.nan), status
    return (path[chain_order(lengths, lag)] if chain_order_ else path), cl, 0


# ---------------------------------------------------------------- the score, the measure and the bar
def score(path, obs, la, lb, lp):
    """ln P(path, observations) of one chain in long double"""
    la, lb, lp = (np.asarray(x, np.longdouble) for x in (la, lb, lp))
    if len(obs) == 0:
        return np.longdouble(0)
    with np.errstate(all="ignore"):
        v = lp[path[0]] + emission(lb, obs[0])[path[0]]
        for t in range(1, len(obs)):
            v = v + la[path[t - 1], path[t]] + emission(lb, obs[t])[path[t]]
    return v


def scores(path, labels, lengths, lag, la, lb, lp):
    labels = np.asarray(labels)
    return np.array([score(path[idx], labels[idx], la, lb, lp) for idx in hc.chains(lengths, lag)], np.longdouble)


def _units(diff, optimum):
    unit = EPS * np.abs(optimum)
    with np.errstate(all="ignore"):
        e = np.where(unit > 0, diff / np.where(unit > 0, unit, 1), np.where(diff != 0, np.inf, 0.0))
    return float(e.max()) if e.size else 0.0


def measure_path(path, ref):
    """E of a path in frame order against a reference() record: how far its chains' scores fall short of the optimum"""
    got = scores(path, ref["labels"], ref["lengths"], ref["lag"], ref["la"], ref["lb"], ref["lp"])
    return _units(ref["optimum"] - got, ref["optimum"])


def measure_logprob(cl, ref):
    return _units(np.abs(np.asarray(cl, np.longdouble) - ref["optimum"]), ref["optimum"])


def bars(ref):
    return {k: FACTOR * max(ref["e_seq"][k], ref["e_chunked"][k], 1.0) for k in OUTPUTS}


# ---------------------------------------------------------------- inputs
def log_model(A, B, p0):
    with np.errstate(divide="ignore"):
        return np.log(A), np.log(B), np.log(p0)


def exact_parameters(m, K, seed=0):
    """integer log-parameters in -6 .. 0: every sum is exact in fp64 and ties are frequent.  For m > 1, 15 % of the entries of la
    and lb are -inf; the diagonal of la is 0 and row 0 of lb is finite, so staying in state 0 emits everything: no chain is
    impossible."""
    rng = np.random.default_rng(1000 * m + K + 7919 * seed)
    la = (-rng.integers(0, 7, (m, m))).astype(np.float64)
    lb = (-rng.integers(0, 7, (m, K))).astype(np.float64)
    lp = (-rng.integers(0, 7, m)).astype(np.float64)
    if m > 1:
        la[rng.random((m, m)) < 0.15] = -np.inf
        hole = rng.random((m, K)) < 0.15
        hole[0] = False
        lb[hole] = -np.inf
    la[np.arange(m), np.arange(m)] = 0.0
    return la, lb, lp


def exact_inputs(m, K, lag, disjoint, C):
    """(labels with missing observations, lengths, la, lb, lp) of one case of hc.CASES"""
    labels, lengths = hc.case_inputs(m, K, lag, disjoint, C)[:2]
    return (hc.with_missing(labels, lengths, lag, C, seed=m + K),) + (lengths,) + exact_parameters(m, K)


def reference_of(labels, lengths, lag, la, lb, lp, C):
    """inputs, the long-double truth, the chunked statement and the two numpy E's per output"""
    labels = np.array(labels, np.int32)
    tpath, _ = sequential_all(labels, lengths, lag, la, lb, lp, np.longdouble)
    ref = {"labels": labels, "lengths": lengths, "lag": lag, "la": la, "lb": lb, "lp": lp, "truth_path": tpath}
    ref["optimum"] = scores(tpath, labels, lengths, lag, la, lb, lp)
    seq = sequential_all(labels, lengths, lag, la, lb, lp, np.float64)
    chk = chunked(labels, lengths, lag, la, lb, lp, C)
    ref["sequential"], ref["chunked"] = seq, chk
    ref["e_seq"] = {"path": measure_path(seq[0], ref), "chain_logprob": measure_logprob(seq[1], ref)}
    ref["e_chunked"] = {"path": measure_path(chk[0], ref), "chain_logprob": measure_logprob(chk[1], ref)}
    for v in (labels, tpath, ref["optimum"], seq[0], seq[1], chk[0], chk[1]):
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(m, K, lag, disjoint, C, missing=False):
    """one case of hc.CASES on its hc.case_inputs model (logs taken on the host), computed once"""
    labels, lengths, A, B, p0 = hc.case_inputs(m, K, lag, disjoint, C)
    if missing:
        labels = hc.with_missing(labels, lengths, lag, C, seed=m)
    return reference_of(labels, lengths, lag, *log_model(A, B, p0), C)


@functools.lru_cache(maxsize=None)
def exact_reference(m, K, lag, disjoint, C):
    return reference_of(*exact_inputs(m, K, lag, disjoint, C)[:2], lag, *exact_inputs(m, K, lag, disjoint, C)[2:], C)
