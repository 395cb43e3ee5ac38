"""Summaries over the draws, computed on the GPU (include/hhmm_summary.h).

Every consumer in the reference reduces what extract() returns over the draws
and drops them:
    apply(apply(alpha_tk, c(2, 3), median), 1, which.max)   # tayal2009/main.R:131-132, R/wf-trade.R:119-120
    apply(alpha, c(2, 3), quantile(x, c(0.1, 0.5, 0.9)))     # common/R/plots.R:261-271
    apply(zstar, 2, median)                                  # plots.R:328,448
`quantiles()` is that reduction on an array already on the host;
`gqs_summary()` is gqs() followed by it, with the per-draw [P, T, K] arrays
never leaving the device.  Quantiles are R's default type 7, exact; the hard
state is which.max over k of one quantile (1-based, 0 when all are NaN).
"""
import ctypes as C

import numpy as np

from . import _abi
from .api import HHMMError, PreparedRequest, load_library

_INT_OUTPUTS = {"zstar_t", "z_ffbs", "hatz_t", "hatl_t"}
_PAIR_OUTPUTS = ("loglik", "logp_zstar")


def _probs(probs):
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if p.ndim != 1:
        raise ValueError("probs must be a scalar or a vector")
    return p


def make_request(values, S, probs, T=None, argmax_prob=None):
    """(request, kept arrays, (N, T_max, K, Q), trailing K axis?) with the shape checks."""
    v = np.asarray(values)
    if v.ndim not in (2, 3):
        raise ValueError(f"values must be [P, T] or [P, T, K], got shape {v.shape}")
    S = int(S)
    if S < 1 or v.shape[0] % S:
        raise ValueError(f"the leading extent {v.shape[0]} is not a multiple of S = {S} draws per series")
    N, Tm = v.shape[0] // S, v.shape[1]
    K = v.shape[2] if v.ndim == 3 else 1
    keep = []
    req = _abi.SummaryRequest()
    if np.issubdtype(v.dtype, np.integer):
        vv = np.asfortranarray(v, dtype=np.int32)
        req.values_i32 = vv.ctypes.data
    else:
        vv = np.asfortranarray(v, dtype=np.float64)
        req.values_f64 = vv.ctypes.data
    keep.append(vv)
    req.n_series, req.n_draws, req.T_max, req.K = N, S, Tm, K
    if T is not None:
        Tv = np.ascontiguousarray(np.asarray(T).reshape(-1), dtype=np.int32)
        if Tv.shape != (N,):
            raise ValueError(f"T must hold one length per series ({N}), got {Tv.shape[0]}")
        if (Tv < 1).any() or (Tv > Tm).any():
            raise ValueError(f"T outside 1..T_max = {Tm}")
        keep.append(Tv)
        req.T = Tv.ctypes.data
    p = _probs(probs)
    req.n_probs = p.size
    for j, x in enumerate(p[:_abi.SUMMARY_MAX_PROBS]):
        req.probs[j] = x
    req.argmax_prob = -1.0 if argmax_prob is None else float(argmax_prob)
    return req, keep, (N, Tm, K, p.size), v.ndim == 3


def quantiles(values, S, probs, T=None, argmax_prob=None, device=-1, lib=None, out=None, out_argmax=None):
    """Type-7 quantiles over the S draws of every cell of a pair-major array.

    values: [P, T] or [P, T, K] with P = N * S, pair p = s + S*n (float64, or
    an integer array, converted to double per value).  Returns [N, T, K, Q]
    ([N, T, Q] for a 2-D input); with `argmax_prob` also the [N, T] int32 hard
    state at that probability.  Steps t >= T[n] keep the fill of `out` /
    `out_argmax` (NaN / 0 when not given)."""
    lib = lib or load_library()
    req, _keep, (N, Tm, K, Q), kaxis = make_request(values, S, probs, T, argmax_prob)
    shape = (N, Tm, K, Q) if kaxis else (N, Tm, Q)
    q = np.full(shape, np.nan, order="F") if out is None else out
    if q.shape != shape or q.dtype != np.float64 or not q.flags.f_contiguous:
        raise ValueError(f"out must be a Fortran-ordered float64 array of shape {shape}")
    am = None
    if argmax_prob is not None:
        am = np.zeros((N, Tm), dtype=np.int32, order="F") if out_argmax is None else out_argmax
        if am.shape != (N, Tm) or am.dtype != np.int32 or not am.flags.f_contiguous:
            raise ValueError(f"out_argmax must be a Fortran-ordered int32 array of shape {(N, Tm)}")
    st = lib.hhmm_summary(C.byref(req), q.ctypes.data, None if am is None else am.ctypes.data, int(device))
    if st < 0:
        raise HHMMError(st, lib.hhmm_last_error().decode())
    return q if am is None else (q, am)


def gqs_summary(model, data, draws, pars, probs=(0.1, 0.5, 0.9), hard=(), argmax_prob=0.5, pairing="grid",
                device=-1, lib=None, uniforms=None, flags=0, hat_rand=None):
    """gqs() reduced over the draws on the device.

    pars: output names as in gqs().  The per-step ones come back as quantiles,
    {name: [N, T, K, Q]} ([N, T, Q] without a K axis; T = T_oos_max for the
    tayal-lite zstar_t and *_oos); those named in `hard` also as
    {"hard_" + name: [N, T] int32}, the 1-based argmax over k of the quantile
    at `argmax_prob`.  The [P] outputs (loglik, logp_zstar), "pair_status" [P]
    and "status" come back as gqs(return_status=True) gives them.  Steps past
    a series' end hold NaN (hard state: 0).  pairing: "grid" or "block"."""
    lib = lib or load_library()
    pars = list(pars)
    for name in list(pars) + list(hard):
        if name not in _abi.OUT:
            raise ValueError(f"unknown output {name!r}")
    step = [n for n in pars if n not in _PAIR_OUTPUTS]
    for name in hard:
        if name not in step:
            raise ValueError(f"hard state of {name!r} asked but it is not among the summarised pars")
        if _abi.RESULT_ARRAYS[name][1] not in ("PTK", "PToK"):
            raise ValueError(f"{name!r} has no K axis to take a hard state over")
    if pairing not in ("grid", "block"):
        raise ValueError("gqs_summary reduces over draws: pairing is 'grid' or 'block'")
    pr = PreparedRequest(model, data, draws, [n for n in pars if n in _PAIR_OUTPUTS], pairing, device, None, flags,
                         None)
    N, Tm, K, P = pr.N, pr.Tmax, pr.K, pr.P
    if "z_ffbs" in step:
        if uniforms is None:
            raise ValueError("z_ffbs (FFBS) needs uniforms of shape (P, T_max)")
        uu = np.asfortranarray(uniforms, dtype=np.float64)
        if uu.shape != (P, Tm):
            raise ValueError(f"uniforms must have shape {(P, Tm)}, got {uu.shape}")
        pr.req.ffbs_u = pr._ptr(uu)
    if {"hatz_t", "hatl_t", "hatx_t"} & set(step):
        if hat_rand is None:
            raise ValueError("hatz_t / hatl_t / hatx_t need hat_rand of shape (P, T_max, 3)")
        hr = np.asfortranarray(hat_rand, dtype=np.float64)
        if hr.shape != (P, Tm, 3):
            raise ValueError(f"hat_rand must have shape {(P, Tm, 3)}, got {hr.shape}")
        pr.req.hat_rand = pr._ptr(hr)
    p = _probs(probs)
    spec = _abi.SummarySpec()
    spec.n_probs = p.size
    for j, x in enumerate(p[:_abi.SUMMARY_MAX_PROBS]):
        spec.probs[j] = x
    spec.argmax_prob = float(argmax_prob) if hard else -1.0
    res = _abi.SummaryResult()
    out = dict(pr.out)
    Q = p.size
    for name in step:
        bit = _abi.OUT[name].bit_length() - 1
        spec.summarise |= _abi.OUT[name]
        code = _abi.RESULT_ARRAYS[name][1]
        Td = pr.T_oos_max if code == "PToK" or (code == "PTz" and model == "hhmm-tayal2009-lite") else Tm
        shape = (N, Td, K, Q) if code in ("PTK", "PToK") else (N, Td, Q)
        q = np.full(shape, np.nan, order="F")
        res.quantiles[bit] = q.ctypes.data
        out[name] = q
        if name in hard:
            spec.argmax |= _abi.OUT[name]
            am = np.zeros((N, Td), dtype=np.int32, order="F")
            res.argmax[bit] = am.ctypes.data
            out["hard_" + name] = am
    st = lib.hhmm_run_summary(C.byref(pr.req), C.byref(spec), C.byref(pr.res), C.byref(res))
    if st < 0:
        raise HHMMError(st, lib.hhmm_last_error().decode())
    out["pair_status"] = pr.status
    out["status"] = st
    return out
