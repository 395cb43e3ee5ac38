"""Numpy restatement of the expected draw statistics (include/hhmm_expect.h).
TEST INFRASTRUCTURE ONLY.

A log-space forward pass with the programs' forward masks and its ADJOINT
backward pass, with logsumexp, per pair; it shares no code with the engine and
takes its masks from tests/draw_stats_ref.py (trans_on / init_on), the
definitions the draw statistics are pinned to.  With M_t(i, j) = A(i, j) where
the mask is on at (t, j) and 1 elsewhere:

    alpha_1(k) = e_1(k) p(k) [init on] ,  alpha_t(j) = e_t(j) sum_i alpha_{t-1}(i) M_t(i, j)
    beta_T = 1 ,                          beta_{t-1}(i) = sum_j M_t(i, j) e_t(j) beta_t(j)

tests/test_expected_stats.py pins it to the weighted mean of
draw_stats_ref.counts over all K^T paths.
"""
import numpy as np

import draw_stats_ref as dsr

MODELS = ("hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009")


def _lse(v, axis):
    m = np.max(v, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(v - m), axis=axis))


def expand(model, par):
    """(p_1k [K], A_ij [K, K], phi_k [K, L]) of one parameter set."""
    if model == "hhmm-tayal2009":
        p, A = dsr.tayal_expand(float(par["p_11"]), np.asarray(par["A_row"], dtype=np.float64))
        return p, A, np.asarray(par["phi_k"], dtype=np.float64)
    return tuple(np.asarray(par[k], dtype=np.float64) for k in ("p_1k", "A_ij", "phi_k"))


def masks(model, aux, T, K):
    """(init [K], trans [T, K]) booleans: the factor is applied at (t, state)."""
    a = [None] * T if aux is None else [int(v) for v in aux]
    init = np.array([dsr.init_on(model, a[0], j) for j in range(1, K + 1)])
    trans = np.array([[dsr.trans_on(model, a[t], j) for j in range(1, K + 1)] for t in range(T)])
    return init, trans.reshape(T, K)


def forward_backward(model, x, aux, p, A, phi):
    """(loglik, n1 [K], xi [K, K], gamma [T, K]) of one series under one parameter set."""
    x = np.asarray(x)
    T, K = x.shape[0], A.shape[0]
    init, on = masks(model, aux, T, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        lA, lp, le = np.log(A), np.log(p), np.log(phi)[:, x - 1].T
        la = np.empty((T, K))
        lb = np.zeros((T, K))
        la[0] = le[0] + np.where(init, lp, 0.0)
        for t in range(1, T):
            la[t] = _lse(la[t - 1][:, None] + np.where(on[t][None, :], lA, 0.0), 0) + le[t]
        for t in range(T - 1, 0, -1):
            lb[t - 1] = _lse(np.where(on[t][None, :], lA, 0.0) + (le[t] + lb[t])[None, :], 1)
        ll = _lse(la[T - 1], 0)
        gamma = np.exp(la + lb - ll)
        xi = np.zeros((K, K))
        for t in range(1, T):
            term = np.exp(la[t - 1][:, None] + lA + (le[t] + lb[t])[None, :] - ll)
            xi += np.where(on[t][None, :], term, 0.0)
        n1 = np.where(init, gamma[0], 0.0)
    return ll, n1, xi, gamma


def loglik(model, x, aux, par):
    return forward_backward(model, x, aux, *expand(model, par))[0]


def series_stats(model, L, x, aux, par):
    """{loglik, n_1k, xi_ij, c_kl} of one series; NaN statistics when loglik is not finite."""
    x = np.asarray(x)
    ll, n1, xi, g = forward_backward(model, x, aux, *expand(model, par))
    c = np.stack([g[x == l + 1].sum(axis=0) for l in range(L)], axis=1)
    st = {"n_1k": n1, "xi_ij": xi, "c_kl": c}
    if not np.isfinite(ll):
        st = {k: np.full(v.shape, np.nan) for k, v in st.items()}
    st["loglik"] = ll
    return st


def pair_coords(pairing, p, S, N):
    if pairing == "zip":
        return p, p
    if pairing == "block":
        return p // (S // N), p
    return p // S, p % S


def expected_stats(model, data, draws, pairing="grid"):
    """The statistics of hhmm_amd.expected_stats for every pair, pair-major like the engine."""
    x = np.atleast_2d(np.asarray(data["x"]))
    N, K, L = x.shape[0], int(data["K"]), int(data["L"])
    aux = None
    if model != "hmm-multinom":
        aux = np.atleast_2d(np.asarray(data["g"] if model == "hmm-multinom-semisup" else data["sign"]))
    S = np.asarray(draws["phi_k"]).shape[0]
    Tn = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else np.full(N, x.shape[1])
    P = N * S if pairing == "grid" else (S if pairing == "block" else N)
    out = {"loglik": np.empty(P), "n_1k": np.empty((P, K)), "xi_ij": np.empty((P, K, K)), "c_kl": np.empty((P, K, L))}
    for q in range(P):
        n, d = pair_coords(pairing, q, S, N)
        par = {name: np.asarray(v, dtype=np.float64)[d] for name, v in draws.items()}
        st = series_stats(model, L, x[n, :Tn[n]], None if aux is None else aux[n, :Tn[n]], par)
        for name, v in st.items():
            out[name][q] = v
    return out
