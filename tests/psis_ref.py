"""Numpy restatement of the PSIS contract (include/hhmm_psis.h): test
infrastructure.  The cell rules one after the other as the header numbers them,
on plain arrays of D members, and the two kinds (LOO, LFO) on an lp_t array;
`predictive()` is the whole path on tests/pointwise_ref.py.
tests/test_psis_ref.py pins it to scipy's generalised Pareto and to a
hand-worked cell.
"""
import math

import numpy as np

import pointwise_ref


def tail_length(D):
    """M = min(floor(D / 5), c), c the smallest integer with c^2 >= 9 D."""
    c = math.isqrt(9 * D)
    if c * c < 9 * D:
        c += 1
    return min(D // 5, c)


def fit_points(M):
    """m = 30 + floor(sqrt(M)) profile points."""
    return 30 + math.isqrt(M)


def xstar_rank(M):
    """x* = x_{(M + 2) div 4}, 1-based among the ascending exceedances."""
    return (M + 2) // 4


def gpd_fit(x):
    """(k, sigma) of the Zhang-Stephens fit with PSIS's prior to the ascending exceedances x."""
    x = np.asarray(x, dtype=np.float64)
    M = x.size
    m = fit_points(M)
    xstar = x[xstar_rank(M) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xstar)
        kj = np.mean(np.log1p(-theta[:, None] * x[None, :]), axis=1)
        L = M * (np.log(-theta / kj) - kj - 1.0)
        omega = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
        th = np.sum(theta * omega)
        k = np.mean(np.log1p(-th * x))
        sigma = -k / th
        k = (k * M + 5.0) / (M + 10.0)
    return k, sigma


def gpd_quantiles(k, sigma, M):
    """q_i, i = 1..M, at p_i = (i - 0.5) / M."""
    p = (np.arange(1, M + 1) - 0.5) / M
    lg = np.log1p(-p)
    if k == 0.0:
        return -sigma * lg
    return sigma * np.expm1(-k * lg) / k


def cell(r, l):
    """(elpd, khat, neff) of one cell of D members (r_d, l_d)."""
    r, l = np.array(r, dtype=np.float64), np.asarray(l, dtype=np.float64)
    D = r.size
    if not (np.isfinite(r).all() and np.isfinite(l).all()):
        return np.nan, np.nan, np.nan
    r = r - r.max()
    M = tail_length(D)
    order = np.lexsort((np.arange(D), r))            # ascending by (r_d, d)
    w, khat = r.copy(), np.inf
    if M >= 5:
        tail, cut = r[order[D - M:]], r[order[D - M - 1]]
        with np.errstate(all="ignore"):
            x = np.exp(tail) - np.exp(cut)
            if x[0] != x[-1]:
                k, sigma = gpd_fit(x)
                if np.isfinite(k) and np.isfinite(sigma):
                    q = gpd_quantiles(k, sigma, M)
                    w[order[D - M:]] = np.minimum(np.log(np.exp(cut) + q), 0.0)
                    khat = k
    a, b = np.max(w + l), np.max(w)
    ew = np.exp(w - b)
    elpd = (a + np.log(np.sum(np.exp((w + l) - a)))) - (b + np.log(np.sum(ew)))
    neff = np.sum(ew) ** 2 / np.sum(np.exp(2.0 * (w - b)))
    return elpd, khat, neff


def cells(lr, lp, N, T=None):
    """{elpd_t, khat_t, neff_t} (N, T_max) of hhmm_amd.psis_cells(); steps t >= T[n] are NaN."""
    lr, lp = np.asarray(lr, dtype=np.float64), np.asarray(lp, dtype=np.float64)
    P, Tmax = lr.shape
    D = P // N
    Tn = np.full(N, Tmax) if T is None else np.asarray(T).reshape(N)
    out = {name: np.full((N, Tmax), np.nan) for name in ("elpd_t", "khat_t", "neff_t")}
    for n in range(N):
        for t in range(Tn[n]):
            rows = slice(n * D, (n + 1) * D)
            out["elpd_t"][n, t], out["khat_t"][n, t], out["neff_t"][n, t] = cell(lr[rows, t], lp[rows, t])
    return out


def log_ratios(lp_t, N, kind, T=None):
    """r (P, T_max) of the kind from lp_t (P, T_max); NaN past T[n]."""
    lp_t = np.asarray(lp_t, dtype=np.float64)
    P, Tmax = lp_t.shape
    D = P // N
    Tn = np.full(N, Tmax) if T is None else np.asarray(T).reshape(N)
    r = np.full((P, Tmax), np.nan)
    for p in range(P):
        t_end = Tn[p // D]
        if kind == "loo":
            r[p, :t_end] = -lp_t[p, :t_end]
        else:
            acc = 0.0
            for t in range(t_end - 1, -1, -1):   # l_T + l_{T-1} + ... + l_t, one addition per step from +0.0
                with np.errstate(invalid="ignore"):
                    acc = acc + lp_t[p, t]
                r[p, t] = -acc
    return r


def from_lp(lp_t, N, kind, T=None):
    """The three cell arrays of the kind from lp_t."""
    return cells(log_ratios(lp_t, N, kind, T), lp_t, N, T)


def predictive(model, data, draws, pairing="grid", kind="loo"):
    """The arrays of hhmm_amd.psis_predictive(per_draw=True)."""
    out = pointwise_ref.pointwise(model, data, draws, pairing)
    N = out["lpd_t"].shape[0]
    T = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else None
    out.update(from_lp(out["lp_t"], N, kind, T))
    return out
