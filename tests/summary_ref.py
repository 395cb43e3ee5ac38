"""numpy restatement of the summary contract (include/hhmm_summary.h) -- test helper.

Cell quantile at probability p over S values x (R's default, type 7):
    if any x is NaN: q = NaN
    y = x sorted ascending
    h = (S - 1) * p;  lo = floor(h);  hi = ceil(h);  q = y[lo]
    if h > lo and y[hi] != y[lo]:  g = h - lo;  q = (1 - g) * y[lo] + g * y[hi]
in fp64 as written.  np.quantile agrees with this only to within 2 ulp (it
interpolates as y[lo] + g * (y[hi] - y[lo])), np.median exactly, so the GPU is
compared against this restatement bit for bit.  Argmax: 1-based first k that
maximises the quantile, NaN skipped, 0 when all K are NaN (R's which.max).
"""
import numpy as np


def cell_quantile(x, p):
    """One cell, one probability, straight from the contract."""
    x = np.asarray(x).astype(np.float64)
    if np.isnan(x).any():
        return np.float64(np.nan)
    y = np.sort(x)
    h = np.float64(x.size - 1) * np.float64(p)
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    q = y[lo]
    if h > lo and y[hi] != y[lo]:
        g = h - np.float64(lo)
        with np.errstate(invalid="ignore"):
            q = (np.float64(1.0) - g) * y[lo] + g * y[hi]
    return np.float64(q)


def quantiles(values, S, probs, T=None, fill=np.nan):
    """values [P, T] or [P, T, K], p = s + S*n  ->  [N, T, K, Q] ([N, T, Q]);
    steps t >= T[n] hold `fill`."""
    v = np.asarray(values).astype(np.float64)
    kaxis = v.ndim == 3
    if not kaxis:
        v = v[:, :, None]
    P, Tm, K = v.shape
    N = P // S
    x = v.reshape((S, N, Tm, K), order="F")
    has_nan = np.isnan(x).any(axis=0)
    y = np.sort(np.where(np.isnan(x), np.inf, x), axis=0)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    out = np.full((N, Tm, K, probs.size), fill, dtype=np.float64)
    for j, p in enumerate(probs):
        h = np.float64(S - 1) * np.float64(p)
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        q = y[lo].copy()
        if h > lo:
            g = h - np.float64(lo)
            with np.errstate(invalid="ignore"):
                interp = (np.float64(1.0) - g) * y[lo] + g * y[hi]
            q = np.where(y[hi] != y[lo], interp, y[lo])
        q[has_nan] = np.nan
        out[..., j] = q
    if T is not None:
        past = np.arange(Tm)[None, :] >= np.asarray(T).reshape(-1, 1)
        out[past] = fill
    return out if kaxis else out[:, :, 0, :]


def argmax(q, T=None, fill=0):
    """q [N, T, K] (the quantiles at one probability) -> [N, T] int32."""
    q = np.asarray(q, dtype=np.float64)
    N, Tm, K = q.shape
    best = np.zeros((N, Tm), dtype=np.int32)
    bestv = np.zeros((N, Tm))
    for k in range(K):
        v = q[:, :, k]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(v) & ((best == 0) | (v > bestv))
        best[take] = k + 1
        bestv[take] = v[take]
    if T is not None:
        past = np.arange(Tm)[None, :] >= np.asarray(T).reshape(-1, 1)
        best[past] = fill
    return best
