"""Batched E-step of the input-output HMM programs on the GPU
(include/hhmm_estep_io.h) and what follows from it: score and an EM point fit.

The coded transition A_t = softmax(u_t' w_k) of iohmm-reg / -mix / -hmix /
-hmix-lite is indexed by the previous state only, so the coded path weight is a
product of per-step factors and the posterior of z_t under it is q_t =
softmax_k(oblik_t(k) + log A_{t+1}(k)) -- one forward sweep, no backward pass.
`estep_io()` returns the sums over t per (series, draw) pair:

  every model  loglik (P,), n_1k (P, K) = q_1, gw_km (P, K, M) = dl/dw_km
  iohmm-reg    n_k (P, K), uu_kmm (P, K, M, M), ux_km (P, K, M), xx_k (P, K)
  mixtures     n_kl, sx_kl, sxx_kl (P, K, L), weighted by the component
               responsibilities r_t(k, l)

  score_io()   the gradient of the model-block log-likelihood (Fisher's
               identity; the priors of the model blocks are not part of it);
  m_step_io()  one generalised EM update: closed forms for p_1k and the
               emission parameters, and for w_km one step on Boehning's
               quadratic lower bound of the multinomial logit (a data-only
               curvature, so the step is closed form and the iteration monotone);
  em_io()      iterates it, with the contract of hhmm_amd.baum_welch.
"""
import numpy as np

from . import _abi, _stats
from .api import load_library
from .estep import _ratio, pair_draw

MODELS = ("iohmm-reg", "iohmm-mix", "iohmm-hmix", "iohmm-hmix-lite")
S_MIN = 1e-4  # real<lower=0.0001> s_k (iohmm-reg.stan:23)


def _check_model(model, what):
    if model not in MODELS:
        raise ValueError(f"{what} covers {MODELS}, not {model!r}")


def stat_shapes(model, P, K, M, L):
    """{name: shape} of the statistics estep_io() returns for `model`."""
    shapes = {"loglik": (P,), "n_1k": (P, K), "gw_km": (P, K, M)}
    if model == "iohmm-reg":
        shapes.update({"n_k": (P, K), "uu_kmm": (P, K, M, M), "ux_km": (P, K, M), "xx_k": (P, K)})
    else:
        shapes.update({"n_kl": (P, K, L), "sx_kl": (P, K, L), "sxx_kl": (P, K, L)})
    return shapes


def prepare(model, data, draws, pairing="grid", device=-1):
    """(PreparedRequest, EstepIoResult, {name: array}) with the shape checks."""
    _check_model(model, "the IOHMM E-step")
    M = int(data["M"])
    u = np.asarray(data["u_tm"])
    if u.shape[-1] != M:
        raise ValueError(f"u_tm must have M = {M} columns, got shape {u.shape}")
    if u.shape[:-1] != np.shape(data["x_t"]):
        raise ValueError(f"u_tm {u.shape} does not match x_t {np.shape(data['x_t'])}")

    def param_shapes(S, K, L):
        if model == "iohmm-reg":
            return {"p_1k": (S, K), "w_km": (S, K, M), "b_km": (S, K, M), "s_k": (S, K)}
        return {"p_1k": (S, K), "w_km": (S, K, M), "lambda_kl": (S, K, L), "mu_kl": (S, K, L), "s_kl": (S, K, L)}

    return _stats.request(model, data, draws, pairing, device, param_shapes,
                          lambda P, K, L: stat_shapes(model, P, K, M, L), _abi.EstepIoResult)


def estep_io(model, data, draws, pairing="grid", device=-1, lib=None, return_status=False):
    """Expected sufficient statistics of every (series, draw) pair.

    data: the keys of gqs (x_t, u_tm, K, M, L).  Returns {name: array} (see
    the module docstring).  A pair whose log-likelihood is -inf or NaN has NaN
    statistics."""
    lib = lib or load_library()
    return _stats.call(lib, "estep_io", *prepare(model, data, draws, pairing, device), return_status)


def score_io(model, draws, stats, pairing, S, N):
    """Gradient of loglik with respect to the constrained parameters, per pair.

    {name: (P, ...)} for p_1k, w_km and b_km, s_k (iohmm-reg) or lambda_kl,
    mu_kl, s_kl (mixtures), from the statistics of estep_io().  The simplex
    parameters are treated as free coordinates, as in hhmm_amd.score."""
    _check_model(model, "score_io")
    P = stats["loglik"].shape[0]
    d = pair_draw(pairing, P, S, N)
    g = {"p_1k": _ratio(stats["n_1k"], np.asarray(draws["p_1k"])[d]), "w_km": np.array(stats["gw_km"])}
    if model == "iohmm-reg":
        b, s = np.asarray(draws["b_km"], dtype=np.float64)[d], np.asarray(draws["s_k"], dtype=np.float64)[d]
        uu, ux = stats["uu_kmm"], stats["ux_km"]
        uub = np.einsum("pkmn,pkn->pkm", uu, b)
        g["b_km"] = (ux - uub) / (s ** 2)[..., None]
        rss = stats["xx_k"] - 2 * (b * ux).sum(axis=-1) + (b * uub).sum(axis=-1)
        g["s_k"] = -stats["n_k"] / s + rss / s ** 3
    else:
        mu, s = np.asarray(draws["mu_kl"], dtype=np.float64)[d], np.asarray(draws["s_kl"], dtype=np.float64)[d]
        n, sx, sxx = stats["n_kl"], stats["sx_kl"], stats["sxx_kl"]
        g["lambda_kl"] = _ratio(n, np.asarray(draws["lambda_kl"])[d])
        g["mu_kl"] = (sx - mu * n) / s ** 2
        g["s_kl"] = -n / s + (sxx - 2 * mu * sx + mu ** 2 * n) / s ** 3
    return g


def input_scatter(data, P):
    """(P, M, M): S_u = sum_{t=2..T_n} u_t u_t' of every pair's series."""
    u = np.asarray(data["u_tm"], dtype=np.float64)
    if u.ndim == 2:
        u = u[None]
    N, Tmax = u.shape[0], u.shape[1]
    Tn = np.asarray(data["T"]).reshape(N) if "T" in data and np.ndim(data["T"]) > 0 else np.full(N, Tmax)
    su = np.stack([u[n, 1:Tn[n]].T @ u[n, 1:Tn[n]] for n in range(N)])
    return su[np.arange(P) // (P // N)]  # P / N consecutive pairs per series under every pairing


def m_step_io(model, stats, prev, data, pairing, s_min=S_MIN):
    """One generalised EM update from the statistics of estep_io(): per-pair parameters.

    prev: {name: (P, ...)} the parameters the statistics were computed under.
    p_1k = n_1k.  iohmm-reg: b_k = pinv(uu_k) ux_k, s_k = sqrt(max(RSS_k / n_k,
    s_min^2)) with the residual sum of squares at the new b_k.  Mixtures:
    lambda_kl = n_kl / sum_l n_kl, mu = sx / n, s = sqrt(max(sxx / n - mu^2,
    s_min^2)), then the components of each state sorted by mu (ordered[L]
    mu_kl; lambda, mu and s permuted together).  A state or component whose
    count is 0 keeps its `prev` values.  w_k <- w_k + 2 pinv(S_u) gw_k with
    S_u = sum_{t>=2} u_t u_t' of the pair's series: Boehning's bound diag(A) -
    AA' <= (I - 11'/K) / 2 on the curvature of the multinomial logit; gw sums
    to 0 over k, so the common-shift direction of w is untouched.  A pair whose
    log-likelihood is not finite gets NaN parameters."""
    _check_model(model, "m_step_io")
    if pairing not in ("grid", "zip", "block"):
        raise ValueError(f"unknown pairing {pairing!r}")
    P = stats["loglik"].shape[0]
    ok = np.isfinite(stats["loglik"])
    new = {"p_1k": np.array(stats["n_1k"])}
    gw = np.where(ok[:, None, None], stats["gw_km"], 0.0)
    step = 2.0 * np.einsum("pmn,pkn->pkm", np.linalg.pinv(input_scatter(data, P)), gw)
    new["w_km"] = np.where(ok[:, None, None], np.asarray(prev["w_km"], dtype=np.float64) + step, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        if model == "iohmm-reg":
            n, ux = stats["n_k"], stats["ux_km"]
            uu = np.where(ok[:, None, None, None], stats["uu_kmm"], 0.0)
            b = np.einsum("pkmn,pkn->pkm", np.linalg.pinv(uu), np.where(ok[:, None, None], ux, 0.0))
            rss = stats["xx_k"] - 2 * (b * ux).sum(axis=-1) + (b * np.einsum("pkmn,pkn->pkm", uu, b)).sum(axis=-1)
            s = np.sqrt(np.maximum(rss / n, s_min ** 2))
            keep = n == 0
            new["b_km"] = np.where(keep[..., None], prev["b_km"], np.where(ok[:, None, None], b, np.nan))
            new["s_k"] = np.where(keep, prev["s_k"], np.where(ok[:, None], s, np.nan))
        else:
            n, sx, sxx = stats["n_kl"], stats["sx_kl"], stats["sxx_kl"]
            tot = n.sum(axis=-1, keepdims=True)
            lam = np.where(tot == 0, prev["lambda_kl"], n / tot)
            mu = sx / n
            s = np.sqrt(np.maximum(sxx / n - mu ** 2, s_min ** 2))
            keep = n == 0
            mu, s = np.where(keep, prev["mu_kl"], mu), np.where(keep, prev["s_kl"], s)
            order = np.argsort(mu, axis=-1, kind="stable")
            new["lambda_kl"] = np.take_along_axis(lam, order, axis=-1)
            new["mu_kl"] = np.take_along_axis(mu, order, axis=-1)
            new["s_kl"] = np.take_along_axis(s, order, axis=-1)
    return new


def em_io(model, data, init, n_iter, pairing="zip", device=-1, lib=None, s_min=S_MIN):
    """n_iter generalised EM iterations from the per-pair parameters `init`.

    init: {name: (P, ...)} draw arrays as estep_io() takes them (pairing "zip":
    one start per series; "block": S / N starts for each series); arrays the
    likelihood does not read (hypermu_k) pass through unchanged.  Returns
    (params, trace): the parameters after the last M-step and the (n_iter, P)
    log-likelihoods of the parameters each iteration started from -- under
    exact arithmetic a non-decreasing sequence per pair."""
    _check_model(model, "em_io")
    if pairing not in ("zip", "block"):
        raise ValueError("em_io: every pair carries its own parameters, pairing is 'zip' or 'block'")
    lib = lib or load_library()
    params = {k: np.array(v, dtype=np.float64) for k, v in init.items()}
    trace = []
    for _ in range(int(n_iter)):
        stats = estep_io(model, data, params, pairing, device, lib)
        trace.append(np.array(stats["loglik"]))
        params.update(m_step_io(model, stats, params, data, pairing, s_min))
    return params, np.array(trace).reshape(int(n_iter), -1)
