"""ORACLE (test infrastructure only) of dff_autocorr and of evaluate.autocorrelation: deliberately naive numpy -- a Python loop
over trajectories and lags with masked vector sums in float64.  Nothing here imports dff_amd."""
import numpy as np


def starts_of(lengths, n):
    lengths = [int(n)] if lengths is None else [int(v) for v in lengths]
    assert sum(lengths) == n and min(lengths, default=0) >= 0
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def lagged_sums(series, max_lag, lengths=None, shift=None):
    """dict of sxy, sx, sy, sabs, sgx, sgy float64 (max_lag + 1, d) and count int64 (max_lag + 1,) over the pairs (t, t + l)
    of one trajectory whose two frames are finite in every component; g = series - shift.  sabs = sum |g_t g_{t+l}|,
    sgx = sum |g_t|, sgy = sum |g_{t+l}|: what the summation error bounds scale with."""
    x = np.asarray(series, np.float64)
    x = x[:, None] if x.ndim == 1 else x
    n, d = x.shape
    sh = np.zeros(d) if shift is None else np.asarray(shift, np.float64).reshape(d)
    usable = np.isfinite(x).all(1)
    g = np.where(usable[:, None], x - sh, 0.0)
    out = {k: np.zeros((max_lag + 1, d)) for k in ("sxy", "sx", "sy", "sabs", "sgx", "sgy")}
    out["count"] = np.zeros(max_lag + 1, np.int64)
    s = starts_of(lengths, n)
    for a, b in zip(s[:-1], s[1:]):
        for l in range(min(max_lag, b - a - 1) + 1):
            m = usable[a:b - l] & usable[a + l:b]
            u, w = g[a:b - l][m], g[a + l:b][m]
            out["count"][l] += m.sum()
            out["sx"][l] += u.sum(0)
            out["sy"][l] += w.sum(0)
            out["sxy"][l] += (u * w).sum(0)
            out["sabs"][l] += np.abs(u * w).sum(0)
            out["sgx"][l] += np.abs(u).sum(0)
            out["sgy"][l] += np.abs(w).sum(0)
    return out


def usable_mean(series):
    x = np.asarray(series, np.float64)
    x = x[:, None] if x.ndim == 1 else x
    usable = np.isfinite(x).all(1)
    return x[usable].sum(0) / max(usable.sum(), 1)


def estimate(sums, estimator="per_lag"):
    """C(l) (max_lag + 1, d) from lagged_sums: per_lag subtracts each end's own mean, global the lag-0 mean from both"""
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = sums["count"].astype(np.float64)[:, None]
        if estimator == "per_lag":
            return sums["sxy"] / cnt - (sums["sx"] / cnt) * (sums["sy"] / cnt)
        m0 = sums["sx"][:1] / cnt[:1]
        return sums["sxy"] / cnt - m0 * (sums["sx"] + sums["sy"]) / cnt + m0 * m0


class Acf:
    """the fields of evaluate.Autocorrelation from the oracle's sums"""

    def __init__(self, series, max_lag, lengths=None, estimator="per_lag"):
        shift = usable_mean(series)
        sums = lagged_sums(series, max_lag, lengths, shift)
        self.cov = estimate(sums, estimator)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.acf = self.cov / self.cov[:1]
            self.mean = shift + sums["sx"][0] / sums["count"][0]
        self.counts = sums["count"]
        self.variance = self.cov[0]
        self.sums = sums
