"""Numpy restatement of the E-step contract (include/hhmm_estep.h): test
infrastructure.  A log-space forward-backward with logsumexp per pair, under
the CODED likelihood of hmm.stan / hmm-multinom.stan, returning the
log-likelihood, gamma, the summed pairwise posterior and the emission
statistics exactly as the header's table defines them -- including the Q2 row
(hmm.stan:30: x_1 enters every state with sum_k normal_lpdf(x_1 | mu_k,
sigma_k), so it counts with weight 1 for every state).
tests/test_estep_ref.py pins it to the CPU oracle.
"""
import numpy as np

_LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def _lse(v, axis):
    m = np.max(v, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(v - m), axis=axis))


def normal_lpdf(x, mu, sigma):
    z = (x - mu) / sigma
    return -_LOG_SQRT_2PI - np.log(sigma) - 0.5 * z * z


def log_emissions(model, x, par):
    """[T, K] log emission of every step under the coded likelihood."""
    x = np.asarray(x)
    if model == "hmm-multinom":
        with np.errstate(divide="ignore"):
            return np.log(par["phi_k"])[:, x - 1].T
    le = normal_lpdf(x[:, None], par["mu_k"][None, :], par["sigma_k"][None, :])
    le[0, :] = le[0, :].sum()  # Q2
    return le


def forward_backward(model, x, par):
    """(loglik, gamma [T, K], sum_t xi_t [K, K]) of one series under one parameter set."""
    x = np.asarray(x)
    T, K = x.shape[0], par["p_1k"].shape[0]
    le = log_emissions(model, x, par)
    with np.errstate(divide="ignore", invalid="ignore"):
        lA, lp = np.log(par["A_ij"]), np.log(par["p_1k"])
        la = np.empty((T, K))
        lb = np.zeros((T, K))
        la[0] = lp + le[0]
        for t in range(1, T):
            la[t] = _lse(la[t - 1][:, None] + lA, 0) + le[t]
        for t in range(T - 2, -1, -1):
            lb[t] = _lse(lA + (le[t + 1] + lb[t + 1])[None, :], 1)
        ll = _lse(la[T - 1], 0)
        gamma = np.exp(la + lb - ll)
        xi = np.zeros((K, K))
        for t in range(1, T):
            xi += np.exp(la[t - 1][:, None] + lA + (le[t] + lb[t])[None, :] - ll)
    return ll, gamma, xi


def pair_coords(pairing, p, S, N):
    if pairing == "zip":
        return p, p
    if pairing == "block":
        return p // (S // N), p
    return p // S, p % S


def estep(model, data, draws, pairing="grid"):
    """The statistics of hhmm_amd.estep for every pair, pair-major like the engine."""
    x = np.asarray(data["x"])
    if x.ndim == 1:
        x = x.reshape(1, -1)
    N, K = x.shape[0], int(data["K"])
    L = int(data.get("L", 0))
    S = np.asarray(draws["p_1k"]).shape[0]
    Tn = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else np.full(N, x.shape[1])
    P = N * S if pairing == "grid" else (S if pairing == "block" else N)
    out = {"loglik": np.empty(P), "n_1k": np.empty((P, K)), "xi_ij": np.empty((P, K, K))}
    if model == "hmm-multinom":
        out["c_kl"] = np.empty((P, K, L))
    else:
        out.update({name: np.empty((P, K)) for name in ("w_k", "s1_k", "s2_k")})
    for p in range(P):
        n, d = pair_coords(pairing, p, S, N)
        par = {name: np.asarray(v, dtype=np.float64)[d] for name, v in draws.items()}
        xs = x[n, :Tn[n]]
        ll, g, xi = forward_backward(model, xs, par)
        st = {"n_1k": g[0], "xi_ij": xi}
        if model == "hmm-multinom":
            st["c_kl"] = np.stack([g[xs == l + 1].sum(axis=0) for l in range(L)], axis=1)
        else:
            xr = xs.astype(np.float64)
            st["w_k"] = 1.0 + g[1:].sum(axis=0)
            st["s1_k"] = xr[0] + (g[1:] * xr[1:, None]).sum(axis=0)
            st["s2_k"] = xr[0] ** 2 + (g[1:] * xr[1:, None] ** 2).sum(axis=0)
        out["loglik"][p] = ll
        for name, v in st.items():
            out[name][p] = v if np.isfinite(ll) else np.nan
    return out
