"""Pointwise predictive densities on the GPU (include/hhmm_pointwise.h) and WAIC.

`pointwise_predictive()` runs one forward sweep per (series, draw) pair, forms
the one-step-ahead predictive log density of every step,

    l_t(n, d) = log p(x_t | x_{1:t-1}, theta_d),    sum_t l_t = loglik,

and reduces it over the draws of each series on the device: three (N, T_max)
arrays come back instead of unalpha_tk (P, T, K).  `waic()` is plain arithmetic
on them -- the answer to "how many states does the data support" after fits at
K = 2, 3, 4, ...  `per_draw=True` also returns l_t itself, (P, T_max), the
input of PSIS and leave-future-out cross-validation.

l_t follows the CODED likelihood of each Stan program (hmm.stan:30, quirk Q2:
l_1 = sum_j normal_lpdf(x_1 | mu_j, sigma_j) + log sum_k p_1k).  hmm and
hmm-multinom at K <= 32: hhmm_pointwise up to K = 8 (a lane per pair),
hhmm_pointwise_large above (a group of 16 or 32 lanes per pair, and a second
kernel that reduces l_t over the draws); the masked and IOHMM programs' coded
step weights are not predictive densities.
"""
import numpy as np

from . import _abi, _stats
from .api import load_library

MODELS = ("hmm", "hmm-multinom")
HIGH_VAR = 0.4  # var_t above this: the usual WAIC reliability warning
MAX_K_LANE = 8  # hhmm_pointwise: the lane-per-pair kernel (csrc kMaxK)


def entry_name(K):
    """The library entry pointwise_predictive() calls at K states: "pointwise"
    up to MAX_K_LANE, "pointwise_large" above (K > 32 reaches the library,
    which rejects it)."""
    return "pointwise" if int(K) <= MAX_K_LANE else "pointwise_large"


def tile_draws(model, K, L=0):
    """Draws of one series that one workgroup of hhmm_pointwise (K <= 8) reduces
    (0: the table does not fit LDS).

    More draws per series spread over ceil(D / tile_draws) workgroups, whose
    partials a finish kernel merges (hhmm_pointwise_workspace_size)."""
    slab = L * ((K + 1) // 2) * 1024 if model == "hmm-multinom" else 0
    waves = 4
    while waves and (slab + 6144) * waves > 160 * 1024:
        waves -= 1
    return 64 * waves


def prepare(model, data, draws, pairing="grid", per_draw=False, device=-1):
    """(PreparedRequest, PointwiseResult, {name: array}) with the shape checks; the arrays are NaN-filled."""
    if model not in MODELS:
        raise ValueError(f"the pointwise predictive densities cover {MODELS}, not {model!r}")

    def param_shapes(S, K, L):
        if model == "hmm-multinom":
            return {"p_1k": (S, K), "A_ij": (S, K, K), "phi_k": (S, K, L)}
        return {"p_1k": (S, K), "A_ij": (S, K, K), "mu_k": (S, K), "sigma_k": (S, K)}

    pr, res, out = _stats.request(model, data, draws, pairing, device, param_shapes,
                                  lambda P, K, L: {"loglik": (P,)}, result_cls=_abi.PointwiseResult)
    shapes = {name: (pr.N, pr.Tmax) for name in ("lpd_t", "mean_t", "var_t")}
    if per_draw:
        shapes["lp_t"] = (pr.P, pr.Tmax)
    for name, shape in shapes.items():
        out[name] = np.full(shape, np.nan, dtype=np.float64, order="F")
        setattr(res, name, out[name].ctypes.data)
    return pr, res, out


def pointwise_predictive(model, data, draws, pairing="grid", per_draw=False, device=-1, lib=None,
                         return_status=False):
    """Per-step predictive log densities of every series, reduced over its draws.

    Returns {name: array}: loglik (P,), and per series and step (N, T_max)
    lpd_t = log mean_d exp l_t, mean_t = mean_d l_t and var_t = the sample
    variance of l_t over the draws (NaN with one draw per series); with
    `per_draw` also lp_t (P, T_max), l_t itself.  Steps t >= T[n] are NaN.  The
    draws of series n are S under "grid", S / N under "block" and 1 under "zip"
    pairing; its pairs are consecutive.  K <= 32; hhmm_pointwise_large above 8."""
    lib = lib or load_library()
    pr, res, out = prepare(model, data, draws, pairing, per_draw, device)
    return _stats.call(lib, entry_name(pr.K), pr, res, out, return_status)


def waic(stats, T=None):
    """WAIC of every series from the arrays of pointwise_predictive().

    `T`: the series' lengths (default: T_max for every series; ragged series
    need theirs, the steps past them are NaN).  Returns {name: (N,)}:
      elpd_waic   sum_t (lpd_t - var_t)
      p_waic      sum_t var_t, the effective number of parameters
      waic        -2 elpd_waic
      se          sqrt(T_n var_t(lpd_t - var_t)), the sample variance over the steps (NaN at T_n = 1)
      n_high_var  steps with var_t > 0.4: where the estimate is unreliable"""
    lpd, var = np.asarray(stats["lpd_t"], dtype=np.float64), np.asarray(stats["var_t"], dtype=np.float64)
    N, Tmax = lpd.shape
    Tn = np.full(N, Tmax) if T is None else np.asarray(T).reshape(N)
    out = {name: np.empty(N) for name in ("elpd_waic", "p_waic", "waic", "se")}
    out["n_high_var"] = np.zeros(N, dtype=np.int64)
    for n in range(N):
        pw, v = lpd[n, :Tn[n]] - var[n, :Tn[n]], var[n, :Tn[n]]
        out["elpd_waic"][n] = pw.sum()
        out["p_waic"][n] = v.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            out["se"][n] = np.sqrt(Tn[n] * np.var(pw, ddof=1)) if Tn[n] > 1 else np.nan
        out["n_high_var"][n] = int((v > HIGH_VAR).sum())
    out["waic"] = -2.0 * out["elpd_waic"]
    return out
