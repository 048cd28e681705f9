"""Seeded hidden Markov models and label sets, the truth, the yardstick and the measure that tests/test_hmm.py and
tests/test_hmm_host.py hold dff_hmm_estep and its Python layer to (not a test).

The call: one E-step of Baum-Welch over all chains of the labels (include/dff.h).  Chain (r, f) at lag tau: the frames f, f + tau,
... of trajectory r; a negative label is a missing observation (emission factor 1, no emission count).
Truth: sequential(..., np.longdouble), the textbook scaled forward-backward, every chain on its own.
Yardstick: the same recursion in np.float64.
chunked(): a numpy fp64 statement of the call's chunked algorithm at the kernel's chunk length -- chunk products row by row with
power-of-two scales, the two carries, the apply pass with its self-normalised gamma and xi, the ordered reductions.
Measure: E of an output = max |value - truth| / (2^-52 x the truth's largest magnitude over that output); for the log-likelihoods
the unit is 2^-52 |l| (every chain's own l for chain_loglik).
Bar: 8 x the larger of the two numpy E's (sequential fp64, chunked) of the same output on the same case, that larger E floored at
one unit before the factor: never below 8 units (the rule of tests/propagate_cases.py).  The kernel is never its own reference."""
import functools

import numpy as np

EPS = 2.0 ** -52
FACTOR = 8.0
NOEXP = -(1 << 28)
OUTPUTS = ("loglik", "xi", "gamma0", "gamma_sym", "chain_loglik", "post")


# ---------------------------------------------------------------- chains
def chains(lengths, lag):
    """the frame indices of every chain, r-major, f-minor; empty chains included"""
    out, o = [], 0
    for n in lengths:
        for f in range(lag):
            out.append(np.arange(o + f, o + n, lag, dtype=np.int64))
        o += int(n)
    return out


def plan(lengths, lag, chunk):
    """(n_chains, n_chunks) by counting"""
    ch = chains(lengths, lag)
    return len(ch), sum((len(c) + chunk - 1) // chunk for c in ch)


def emission(B, o):
    """B[:, o], or ones for a missing observation (and for a label >= K, which the call reports as status 3)"""
    return B[:, o] if 0 <= o < B.shape[1] else np.ones(B.shape[0], B.dtype)


def pack(res):
    return np.concatenate([[res["loglik"]], np.ravel(res["xi"]), res["gamma0"], np.ravel(res["gamma_sym"])]).astype(np.float64)


def unpack(stats, m, K):
    s = np.asarray(stats)
    return {"loglik": s[0], "xi": s[1:1 + m * m].reshape(m, m), "gamma0": s[1 + m * m:1 + m * m + m],
            "gamma_sym": s[1 + m * m + m:].reshape(m, K)}


# ---------------------------------------------------------------- the sequential recursion at a chosen dtype
def sequential(labels, lengths, lag, A, B, p0, dtype):
    A, B, p0 = np.asarray(A, dtype), np.asarray(B, dtype), np.asarray(p0, dtype)
    m, K = B.shape
    n = len(labels)
    post = np.zeros((n, m), dtype)
    xi, gamma0, gsym = np.zeros((m, m), dtype), np.zeros(m, dtype), np.zeros((m, K), dtype)
    lls = []
    with np.errstate(all="ignore"):
        for idx in chains(lengths, lag):
            L = len(idx)
            if L == 0:
                lls.append(dtype(0))
                continue
            obs = labels[idx]
            al = np.zeros((L, m), dtype)
            a = p0 * emission(B, obs[0])
            ll = dtype(0)
            for t in range(L):
                if t:
                    a = (a @ A) * emission(B, obs[t])
                s = a.sum()
                ll = ll + np.log(s)
                a = a / s
                al[t] = a
            lls.append(ll)
            be = np.ones(m, dtype)
            for t in range(L - 1, -1, -1):
                g = al[t] * be
                g = g / g.sum()
                post[idx[t]] = g
                if 0 <= obs[t] < K:
                    gsym[:, obs[t]] += g
                if t == 0:
                    gamma0 += g
                    break
                w = emission(B, obs[t]) * be
                x = al[t - 1][:, None] * A * w[None, :]
                xi += x / x.sum()
                be = A @ w
                be = be / be.sum()
    lls = np.array(lls, dtype)
    return {"loglik": lls.sum(), "xi": xi, "gamma0": gamma0, "gamma_sym": gsym, "chain_loglik": lls, "post": post}


# ---------------------------------------------------------------- the chunked algorithm of the call, numpy fp64
def _pow2(v):
    """(v 2^-e, e) with e the exponent of sum(v) (0.5 <= sum 2^-e < 1); (zeros, NOEXP) when the sum is not positive and finite"""
    s = v.sum()
    if not (s > 0 and np.isfinite(s)):
        return np.zeros_like(v), NOEXP
    e = int(np.frexp(s)[1])
    return np.ldexp(v, -e), e


def _shift(v, e):
    return np.ldexp(v, int(np.clip(e, -4000, 4000)))


def chunked(labels, lengths, lag, A, B, p0, chunk):
    A, B, p0 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(p0, np.float64)
    m, K = B.shape
    n, C = len(labels), int(chunk)
    post = np.zeros((n, m))
    xi_parts, lls, gamma0 = [], [], np.zeros(m)
    with np.errstate(all="ignore"):
        for idx in chains(lengths, lag):
            L = len(idx)
            if L == 0:
                lls.append(0.0)
                continue
            obs = labels[idx]
            nch = (L + C - 1) // C
            # (1) chunk products, row by row, one power-of-two scale per row and step
            prods, pexps = [], []
            for k in range(nch):
                P, e = np.eye(m), np.zeros(m, np.int64)
                for t in range(max(k * C, 1), min(L, (k + 1) * C)):
                    P = (P @ A) * emission(B, obs[t])[None, :]
                    for i in range(m):
                        if e[i] != NOEXP:
                            P[i], de = _pow2(P[i])
                            e[i] = NOEXP if de == NOEXP else e[i] + de
                prods.append(P)
                pexps.append(e)
            # (2) carries
            ain, bout = [None] * nch, [None] * nch
            v, E = _pow2(p0 * emission(B, obs[0]))
            gone = E == NOEXP
            for k in range(nch):
                ain[k] = v
                reach = [pexps[k][i] for i in range(m) if v[i] > 0 and pexps[k][i] != NOEXP]
                if not reach:
                    gone = True
                    break
                emax = max(reach)
                vs = np.array([0.0 if pexps[k][i] == NOEXP else _shift(v[i], pexps[k][i] - emax) for i in range(m)])
                v, de = _pow2(vs @ prods[k])
                if de == NOEXP:
                    gone = True
                    break
                E += emax + de
            s1 = v.sum()
            gone = gone or not (s1 > 0 and np.isfinite(s1))
            lls.append(np.nan if gone else float(E) * np.log(2.0) + np.log(s1))
            if gone:
                xi_parts.extend([np.full((m, m), np.nan)] * nch)
                post[idx] = np.nan
                continue
            v = np.ones(m)
            for k in range(nch - 1, -1, -1):
                bout[k] = v
                if k == 0:
                    break
                y = prods[k] @ v
                reach = [pexps[k][i] for i in range(m) if y[i] > 0 and pexps[k][i] != NOEXP]
                emax = max(reach) if reach else 0
                y = np.array([0.0 if pexps[k][i] == NOEXP or not reach else _shift(y[i], pexps[k][i] - emax) for i in range(m)])
                v, _ = _pow2(y)
            # (3) apply
            for k in range(nch):
                t0, t1 = k * C, min(L, (k + 1) * C)
                u = np.zeros((t1 - t0 + 1, m))                       # slot 0: the alpha entering, slot s + 1: frame t0 + s
                u[0] = ain[k] if k else 0.0
                for s in range(t1 - t0):
                    b = emission(B, obs[t0 + s])
                    u[s + 1] = p0 * b if t0 + s == 0 else (u[s] @ A) * b / u[s].sum()
                beta, xi, wpend = bout[k], np.zeros((m, m)), None
                for s in range(t1 - t0 - 1, -2, -1):
                    if s == -1 and k == 0:
                        break
                    G = u[s + 1] @ beta
                    if s >= 0:
                        post[idx[t0 + s]] = u[s + 1] * beta / G
                    if wpend is not None:
                        xi += (u[s + 1][:, None] * A) * (wpend / G)[None, :]
                    wpend = None
                    if s >= 0 and t0 + s >= 1:
                        wpend = emission(B, obs[t0 + s]) * beta / beta.sum()
                        beta = A @ wpend
                xi_parts.append(xi)
            gamma0 += post[idx[0]]
    # (4) reductions, in order
    xi = np.zeros((m, m))
    for x in xi_parts:
        xi = xi + x
    gsym = np.zeros((m, K))
    lab = np.asarray(labels)
    for g0 in range(0, n, 1024):
        part = np.zeros((m, K))
        sl = slice(g0, min(n, g0 + 1024))
        ok = (lab[sl] >= 0) & (lab[sl] < K)
        np.add.at(part.T, lab[sl][ok], post[sl][ok])
        gsym = gsym + part
    lls = np.array(lls)
    ll = 0.0
    for x in lls:
        ll = ll + x
    return {"loglik": ll, "xi": xi, "gamma0": gamma0, "gamma_sym": gsym, "chain_loglik": lls, "post": post}


# ---------------------------------------------------------------- the call's contract on the host (the tests' stand-in)
def host_estep(labels, lengths, lag, A, B, p0, chunk=128):
    """dff_hmm_estep on numpy -> (stats packed (1 + m m + m + m K), chain_loglik, post (n, m), status)"""
    A, B, p0 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(p0, np.float64)
    labels = np.asarray(labels)
    m, K = B.shape
    n_chains = len(lengths) * lag
    bad = lambda x: not (np.isfinite(x).all() and (x >= 0).all())   # noqa: E731
    status = 1 if bad(A) or bad(B) or bad(p0) else (3 if (labels >= K).any() else 0)
    res = None
    if status == 0:
        res = chunked(labels, lengths, lag, A, B, p0, chunk)
        if np.isnan(res["chain_loglik"]).any():
            status = 2
    if status:
        nan = np.nan
        return np.full(1 + m * m + m + m * K, nan), np.full(n_chains, nan), np.full((len(labels), m), nan), status
    return pack(res), res["chain_loglik"], res["post"], 0


# ---------------------------------------------------------------- the measure and the bar
def measure(value, truth, name):
    v, t = np.asarray(value, np.longdouble), np.asarray(truth, np.longdouble)
    if v.size == 0:
        return 0.0
    if name == "chain_loglik":
        unit = EPS * np.abs(t)
        d = np.abs(v - t)
        return float(np.max(np.where(unit > 0, d / np.where(unit > 0, unit, 1), np.where(d > 0, np.inf, 0.0))))
    big = np.abs(t).max()
    if big == 0:
        return 0.0 if np.abs(v).max() == 0 else float("inf")
    return float(np.abs(v - t).max() / (EPS * big))


def bars(ref):
    """{output: bar} of a reference() record"""
    return {k: FACTOR * max(ref["e_seq"][k], ref["e_chunked"][k], 1.0) for k in OUTPUTS}


# ---------------------------------------------------------------- models and labels
def model(m, K, seed=0, disjoint=False):
    """(A (m, m) metastable and row-stochastic, B (m, K) row-stochastic, p0 (m)).  disjoint: hidden state i emits only the
    symbols s with s mod m == i (exact zeros elsewhere), where K >= m.  The call normalises nothing, and two things are left
    unnormalised on purpose: p0 (sum != 1) and, at K = 1, B (entries != 1) -- otherwise a chain of missing observations, and every
    chain at K = 1, has the log-likelihood ln 1 = 0, of which no relative error exists."""
    rng = np.random.default_rng(100 * m + K + 7919 * seed)
    A = rng.uniform(0.01, 0.05, (m, m)) + np.diag(rng.uniform(0.8, 0.95, m))
    A /= A.sum(axis=1)[:, None]
    B = rng.uniform(0.05, 1.0, (m, K))
    if disjoint and K >= m:
        B *= (np.arange(K)[None, :] % m == np.arange(m)[:, None])
    if K > 1:
        B /= B.sum(axis=1)[:, None]
    p0 = rng.uniform(0.2, 1.0, m)
    return A, B, p0 * (0.7 / p0.sum())


def simulate(A, B, p0, lengths, seed=0):
    """labels int32 of trajectories of the model, one after the other"""
    rng = np.random.default_rng(seed)
    cA, cB, m, K = np.cumsum(A, axis=1), np.cumsum(B / B.sum(axis=1)[:, None], axis=1), B.shape[0], B.shape[1]
    out = []
    for n in lengths:
        h = min(int(np.searchsorted(np.cumsum(p0) / p0.sum(), rng.random())), m - 1)
        r = rng.random((int(n), 2))
        lab = np.empty(int(n), np.int32)
        for t in range(int(n)):
            lab[t] = min(int(np.searchsorted(cB[h], r[t, 0])), K - 1)
            h = min(int(np.searchsorted(cA[h], r[t, 1])), m - 1)
        out.append(lab)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def lengths_for(lag, C):
    """trajectories whose chains have 0, 1, 2, C - 1, C, C + 1 and 2 C + 1 frames, empty trajectories among them, one shorter than
    the lag when lag > 1, and at lag 1 one chain of 20 C"""
    L = [0, 1, 2, lag * (C - 1), 0, lag * C, lag * C + 1, lag * (2 * C + 1) + (lag > 1), max(lag - 1, 0)]
    if lag == 1:
        L.append(20 * C)
    return L


CASES = tuple([(m, K, lag, False) for m, K, lag in ((1, 1, 1), (1, 5, 3), (1, 1024, 1), (2, 1, 7), (2, 5, 1), (2, 1024, 3),
                                                      (3, 1, 1), (3, 5, 7), (3, 1024, 1), (8, 1, 3), (8, 5, 1), (8, 1024, 7),
                                                      (8, 1024, 1), (2, 5, 3))]
              + [(3, 5, 1, True), (8, 1024, 3, True), (2, 5, 7, True)])


def case_inputs(m, K, lag, disjoint, C):
    A, B, p0 = model(m, K, disjoint=disjoint)
    lengths = lengths_for(lag, C)
    if disjoint:                                                   # labels the model can emit: drawn from it, trajectory by trajectory
        labels = simulate(A, B, p0, lengths, seed=m + K + lag)
    else:
        labels = np.random.default_rng(31 * m + K + lag).integers(0, K, sum(lengths)).astype(np.int32)
    return labels, lengths, A, B, p0


@functools.lru_cache(maxsize=None)
def reference(m, K, lag, disjoint, C):
    """one case, computed once: inputs, truth, and the two numpy E's per output"""
    labels, lengths, A, B, p0 = case_inputs(m, K, lag, disjoint, C)
    return reference_of(labels, lengths, lag, A, B, p0, C)


def reference_of(labels, lengths, lag, A, B, p0, C):
    truth = sequential(labels, lengths, lag, A, B, p0, np.longdouble)
    seq = sequential(labels, lengths, lag, A, B, p0, np.float64)
    chk = chunked(labels, lengths, lag, A, B, p0, C)
    for v in truth.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    labels.setflags(write=False)
    return {"labels": labels, "lengths": lengths, "lag": lag, "A": A, "B": B, "p0": p0, "truth": truth, "chunked": chk,
            "e_seq": {k: measure(seq[k], truth[k], k) for k in OUTPUTS},
            "e_chunked": {k: measure(chk[k], truth[k], k) for k in OUTPUTS}}


def with_missing(labels, lengths, lag, C, seed=0):
    """labels with -1 scattered, at a chain's first and last frame, over a whole chunk and over a whole chain"""
    lab = np.array(labels, np.int32)
    rng = np.random.default_rng(seed)
    lab[rng.random(len(lab)) < 0.05] = -1
    ch = [c for c in chains(lengths, lag) if len(c)]
    longest = max(ch, key=len)
    lab[longest[0]] = lab[longest[-1]] = -1
    if len(longest) >= 2 * C:
        lab[longest[C:2 * C]] = -1                                   # the chain's second chunk
    whole = [c for c in ch if 1 < len(c) <= C + 1 and c is not longest]
    if whole:
        lab[whole[-1]] = -1
    return lab
