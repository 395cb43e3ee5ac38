"""Numpy restatement of the IOHMM E-step contract (include/hhmm_estep_io.h):
test infrastructure.  The coded path weight of iohmm-reg / -mix / -hmix /
-hmix-lite factorises over the steps (the "transition" softmax(u_t' w_k) is
indexed by the previous state only), so per pair
    lw_t(k) = oblik_t(k) + log A_{t+1}(k)   (+ log p_1k(k) at t = 1, no log A at t = T)
    c_t = LSE_k lw_t(k),  loglik = sum_t c_t,  q_t = softmax_k lw_t
and the statistics are sums over t weighted by q_t (and, for the mixtures, by
the component responsibilities).  tests/test_estep_io_ref.py pins it to the CPU
oracle.
"""
import numpy as np

from estep_ref import _lse, normal_lpdf, pair_coords

MIX = ("iohmm-mix", "iohmm-hmix", "iohmm-hmix-lite")


def log_emissions(model, x, u, par):
    """(oblik [T, K], comp [T, K, L] or None): comp = log lambda_kl + normal_lpdf(x_t | mu_kl, s_kl)."""
    if model == "iohmm-reg":
        return normal_lpdf(x[:, None], u @ par["b_km"].T, par["s_k"][None, :]), None
    comp = np.log(par["lambda_kl"])[None] + normal_lpdf(x[:, None, None], par["mu_kl"][None], par["s_kl"][None])
    return _lse(comp, 2), comp


def posteriors(model, x, u, par):
    """(c [T], q [T, K], A [T, K], oblik, comp) of one series under one parameter set; A[0] is unused."""
    T = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ob, comp = log_emissions(model, x, u, par)
        v = u @ par["w_km"].T
        lA = v - _lse(v, 1)[:, None]
        lw = ob.copy()
        lw[0] += np.log(par["p_1k"])
        lw[:T - 1] += lA[1:]
        c = _lse(lw, 1)
        q = np.exp(lw - c[:, None])
    return c, q, np.exp(lA), ob, comp


def pair_stats(model, x, u, par):
    """The statistics of one pair as {name: array} (loglik a float)."""
    c, q, A, ob, comp = posteriors(model, x, u, par)
    st = {"loglik": c.sum(), "n_1k": q[0], "gw_km": (q[:-1] - A[1:]).T @ u[1:]}
    if model == "iohmm-reg":
        st["n_k"] = q.sum(axis=0)
        uu = np.einsum("tk,tm,tn->kmn", q, u, u)
        iu = np.triu_indices(u.shape[1], 1)
        uu[:, iu[1], iu[0]] = uu[:, iu[0], iu[1]]  # the lower triangle mirrors the upper
        st["uu_kmm"] = uu
        st["ux_km"] = np.einsum("tk,tm,t->km", q, u, x)
        st["xx_k"] = q.T @ (x * x)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.where(q[:, :, None] == 0, 0.0, q[:, :, None] * np.exp(comp - ob[:, :, None]))
        st["n_kl"] = r.sum(axis=0)
        st["sx_kl"] = np.einsum("tkl,t->kl", r, x)
        st["sxx_kl"] = np.einsum("tkl,t->kl", r, x * x)
    return st


def series(data):
    """(x [N, Tmax], u [N, Tmax, M], T [N])."""
    x = np.asarray(data["x_t"], dtype=np.float64)
    u = np.asarray(data["u_tm"], dtype=np.float64)
    if x.ndim == 1:
        x, u = x[None], u[None]
    N = x.shape[0]
    Tn = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else np.full(N, x.shape[1])
    return x, u, Tn


def estep(model, data, draws, pairing="grid"):
    """The statistics of hhmm_amd.estep_io for every pair, pair-major like the engine."""
    x, u, Tn = series(data)
    N, S = x.shape[0], np.asarray(draws["p_1k"]).shape[0]
    P = N * S if pairing == "grid" else (S if pairing == "block" else N)
    out = {}
    for p in range(P):
        n, d = pair_coords(pairing, p, S, N)
        par = {name: np.asarray(v, dtype=np.float64)[d] for name, v in draws.items()}
        st = pair_stats(model, x[n, :Tn[n]], u[n, :Tn[n]], par)
        for name, v in st.items():
            if p == 0:
                out[name] = np.empty((P,) + np.shape(v))
            out[name][p] = v if name == "loglik" or np.isfinite(st["loglik"]) else np.nan
    return out
