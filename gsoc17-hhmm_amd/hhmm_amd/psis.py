"""PSIS-LOO and leave-future-out cross-validation on the GPU (include/hhmm_psis.h).

`psis_predictive()` runs the forward sweep of `pointwise_predictive()` and, on
the device, Pareto-smooths the importance ratios of every cell (n, t) over the
D draws of series n.  The two kinds differ in the log ratios only:

    loo   r_d = -l_t(n, d)                              leave x_t out
    lfo   r_d = -(l_T + l_{T-1} + ... + l_t)(n, d)      leave x_{t:T} out

`lfo` is the "backward" approximate leave-future-out CV of Buerkner, Gabry and
Vehtari: the draws, conditioned on all of x_{1:T}, are re-weighted towards the
posterior given x_{1:t-1}.  Three (N, T_max) arrays come back beside those of
pointwise_predictive(): elpd_t, the Pareto shape khat_t and the effective
number of draws neff_t.  `loo()` and `lfo()` are plain arithmetic on them.
`psis_cells()` applies the same cell operation to caller-supplied log ratios
(M-step-ahead LFO, any other importance sampling).

hmm and hmm-multinom at K <= 32, D <= 16384 draws per series.
"""
import ctypes as C

import numpy as np

from . import _abi, pointwise
from .api import HHMMError, _f64, _i32, load_library
from . import _stats

KINDS = ("loo", "lfo")
BAD_K = 0.7  # khat_t above this: the estimate of the step is unreliable (LFO: a refit is due)
MAX_DRAWS = _abi.PSIS_MAX_DRAWS
CELL_ARRAYS = ("elpd_t", "khat_t", "neff_t")


def prepare(model, data, draws, pairing="grid", per_draw=False, device=-1):
    """(PreparedRequest, PsisResult, {name: array}) with the shape checks; the arrays are NaN-filled."""
    if model not in pointwise.MODELS:
        raise ValueError(f"PSIS covers {pointwise.MODELS}, not {model!r}")

    def param_shapes(S, K, L):
        if model == "hmm-multinom":
            return {"p_1k": (S, K), "A_ij": (S, K, K), "phi_k": (S, K, L)}
        return {"p_1k": (S, K), "A_ij": (S, K, K), "mu_k": (S, K), "sigma_k": (S, K)}

    pr, res, out = _stats.request(model, data, draws, pairing, device, param_shapes,
                                  lambda P, K, L: {"loglik": (P,)}, result_cls=_abi.PsisResult)
    shapes = {name: (pr.N, pr.Tmax) for name in ("lpd_t", "mean_t", "var_t") + CELL_ARRAYS}
    if per_draw:
        shapes["lp_t"] = (pr.P, pr.Tmax)
    for name, shape in shapes.items():
        out[name] = np.full(shape, np.nan, dtype=np.float64, order="F")
        setattr(res, name, out[name].ctypes.data)
    return pr, res, out


def psis_predictive(model, data, draws, pairing="grid", kind="loo", per_draw=False, device=-1, lib=None,
                    return_status=False):
    """The arrays of pointwise_predictive() plus, per series and step (N, T_max),
    elpd_t (the PSIS estimate of the step's log predictive density with x_t --
    "loo" -- or x_{t:T} -- "lfo" -- left out), khat_t (the Pareto shape of the
    cell's importance ratios; +inf where D < 25 draws leave no tail to fit) and
    neff_t (the effective number of draws).  A cell with a non-finite member is
    NaN in all three; steps t >= T[n] are NaN."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    lib = lib or load_library()
    pr, res, out = prepare(model, data, draws, pairing, per_draw, device)
    return _stats.call(lib, "psis_" + kind, pr, res, out, return_status)


def psis_cells(lr, lp, N, T=None, device=-1, lib=None):
    """The cell operation on caller-supplied members: lr and lp (N * D, T_max)
    hold the log ratios and the targets, the D members of series n in the rows
    n * D .. n * D + D - 1.  Returns {elpd_t, khat_t, neff_t}, each (N, T_max);
    with `T` (N,) the steps t >= T[n] are NaN."""
    lib = lib or load_library()
    lr, lp = _f64(lr), _f64(lp)
    if lr.ndim != 2 or lr.shape != lp.shape:
        raise ValueError(f"lr and lp must have the same shape (N * D, T_max), got {lr.shape} and {lp.shape}")
    N = int(N)
    P, Tmax = lr.shape
    if N < 1 or P < N or P % N:
        raise ValueError(f"{P} rows do not split into N = {N} series")
    req = _abi.PsisCellsRequest()
    req.n_series, req.n_draws, req.T_max = N, P // N, Tmax
    req.lr, req.lp = lr.ctypes.data, lp.ctypes.data
    if T is not None:
        Tn = _i32(np.asarray(T).reshape(-1))
        if Tn.shape != (N,):
            raise ValueError(f"T must have shape {(N,)}, got {Tn.shape}")
        req.T = Tn.ctypes.data
    out = {name: np.full((N, Tmax), np.nan, dtype=np.float64, order="F") for name in CELL_ARRAYS}
    st = lib.hhmm_psis_cells(C.byref(req), *(out[name].ctypes.data for name in CELL_ARRAYS), device)
    if st < 0:
        raise HHMMError(st, lib.hhmm_last_error().decode())
    return out


def _sums(stats, T, first, tag):
    elpd, lpd, kh = (np.asarray(stats[name], dtype=np.float64) for name in ("elpd_t", "lpd_t", "khat_t"))
    N, Tmax = elpd.shape
    Tn = np.full(N, Tmax) if T is None else np.asarray(T).reshape(N)
    out = {name: np.empty(N) for name in ("elpd_" + tag, "p_" + tag, tag + "ic", "se", "max_khat")}
    out["n_bad_k"] = np.zeros(N, dtype=np.int64)
    for n in range(N):
        sl = slice(first, Tn[n])
        e, k, cnt = elpd[n, sl], kh[n, sl], max(int(Tn[n]) - first, 0)
        out["elpd_" + tag][n] = e.sum()
        out["p_" + tag][n] = (lpd[n, sl] - e).sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            out["se"][n] = np.sqrt(cnt * np.var(e, ddof=1)) if cnt > 1 else np.nan
        out["max_khat"][n] = k.max() if cnt else np.nan
        out["n_bad_k"][n] = int((k > BAD_K).sum())
    out[tag + "ic"] = -2.0 * out["elpd_" + tag]
    return out, kh, Tn


def loo(stats, T=None):
    """PSIS-LOO of every series from the arrays of psis_predictive(kind="loo").

    `T`: the series' lengths (default: T_max for every series).  Returns {name: (N,)}:
      elpd_loo   sum_t elpd_t
      p_loo      sum_t (lpd_t - elpd_t), the effective number of parameters
      looic      -2 elpd_loo
      se         sqrt(T_n var_t(elpd_t)), the sample variance over the steps (NaN at T_n = 1)
      max_khat   the largest khat_t
      n_bad_k    steps with khat_t > 0.7 (BAD_K): where the estimate is unreliable"""
    return _sums(stats, T, 0, "loo")[0]


def lfo(stats, T=None, first=1):
    """Leave-future-out CV of every series from the arrays of psis_predictive(kind="lfo").

    The sums of loo() over the steps t > `first` (1-based): the first `first`
    observations are the minimum a fit needs, and the cell at t = 1 re-weights
    to the prior, so `first` >= 1.  Returns elpd_lfo, p_lfo, lfoic, se (over the
    T_n - first summed steps), max_khat and n_bad_k, and
      refit_at   the 0-based index of the first step the backward pass meets
                 (the largest t) whose khat_t > 0.7: the draws conditioned on
                 all the data do not reach back past it and a refit is due
                 there; -1 where no step exceeds it"""
    first = int(first)
    if first < 1:
        raise ValueError("first must be at least 1: the LFO cell at t = 1 re-weights to the prior")
    out, kh, Tn = _sums(stats, T, first, "lfo")
    out["refit_at"] = np.full(kh.shape[0], -1, dtype=np.int64)
    for n in range(kh.shape[0]):
        hit = np.nonzero(kh[n, first:Tn[n]] > BAD_K)[0]
        if hit.size:
            out["refit_at"][n] = first + hit[-1]
    return out
