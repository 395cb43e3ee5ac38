"""Numpy restatement of the pointwise contract (include/hhmm_pointwise.h): test
infrastructure.  A log-space forward with logsumexp per pair on
estep_ref.log_emissions (the CODED likelihood, Q2 row included), l_t as the
difference of consecutive log forward sums, and the three reductions over the
draws of each series exactly as the header tabulates them.
tests/test_pointwise_ref.py pins it to the CPU oracle.
"""
import numpy as np

import estep_ref


def lp_series(model, x, par):
    """[T] l_t = log p(x_t | x_{1:t-1}) of one series under one parameter set."""
    x = np.asarray(x)
    T = x.shape[0]
    le = estep_ref.log_emissions(model, x, par)
    with np.errstate(divide="ignore", invalid="ignore"):
        lA, lp = np.log(par["A_ij"]), np.log(par["p_1k"])
        la = lp + le[0]
        tot = np.empty(T)
        tot[0] = estep_ref._lse(la, 0)
        for t in range(1, T):
            la = estep_ref._lse(la[:, None] + lA, 0) + le[t]
            tot[t] = estep_ref._lse(la, 0)
        return np.concatenate([tot[:1], tot[1:] - tot[:-1]]), tot[-1]


def reduce_draws(l):
    """(lpd, mean, var) over axis 0 of l [D, ...]: the header's formulas in IEEE arithmetic."""
    D = l.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.fmax.reduce(l, axis=0)                       # the largest member, NaN ignored
        m = np.where(np.isfinite(m), m, 0.0)                # every member -inf (or NaN): no shift
        lpd = m + np.log(np.sum(np.exp(l - m), axis=0) / D)
        mean = np.sum(l, axis=0) / D
        var = np.sum((l - mean) ** 2, axis=0) / (D - 1) if D > 1 else np.full(l.shape[1:], np.nan)
    return lpd, mean, var


def pointwise(model, data, draws, pairing="grid"):
    """The arrays of hhmm_amd.pointwise_predictive(per_draw=True); steps t >= T[n] are NaN."""
    x = np.asarray(data["x"])
    if x.ndim == 1:
        x = x.reshape(1, -1)
    N, Tmax = x.shape
    S = np.asarray(draws["p_1k"]).shape[0]
    Tn = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else np.full(N, Tmax)
    P = N * S if pairing == "grid" else (S if pairing == "block" else N)
    D = P // N
    out = {"loglik": np.empty(P), "lp_t": np.full((P, Tmax), np.nan)}
    for name in ("lpd_t", "mean_t", "var_t"):
        out[name] = np.full((N, Tmax), np.nan)
    for p in range(P):
        n, d = estep_ref.pair_coords(pairing, p, S, N)
        assert n == p // D
        par = {name: np.asarray(v, dtype=np.float64)[d] for name, v in draws.items()}
        out["lp_t"][p, :Tn[n]], out["loglik"][p] = lp_series(model, x[n, :Tn[n]], par)
    for n in range(N):
        t = Tn[n]
        out["lpd_t"][n, :t], out["mean_t"][n, :t], out["var_t"][n, :t] = reduce_draws(out["lp_t"][n * D:(n + 1) * D, :t])
    return out
