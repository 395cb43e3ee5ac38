"""Baum-Welch on the GPU's E-step: an EM point fit per (series, start).

The reference initialises its chains with k-means (iohmm-mix/R/iohmm-mix-init.R)
and fits every walk-forward window by NUTS; an EM fit from the batched E-step
(hhmm_amd.estep; hhmm_amd.expected_stats for the masked programs,
hmm-multinom-semisup and hhmm-tayal2009) is a better initialiser and a quick
point fit.  Every pair carries its own parameters, so S starts per series run
as one batch; the M-step is plain numpy on the [P, K..] statistics.
"""
import numpy as np

from .api import load_library
from .estep import FIT_MODELS, MODELS, estep, m_step
from .expect import expected_stats


def baum_welch(model, data, init, n_iter, pairing="zip", device=-1, lib=None, schedule="auto", flags=0):
    """n_iter EM iterations from the per-pair parameters `init`.

    init: {name: (P, ...)} draw arrays as estep() / expected_stats() take them
    (pairing "zip": one start per series; "block": S / N starts for each
    series).  Returns (params, trace): the parameters after the last M-step
    and the (n_iter, P) log-likelihoods of the parameters each iteration
    started from -- under exact arithmetic a non-decreasing sequence per pair.
    hmm and hmm-multinom at K <= 32 (hhmm_estep_large above 8).  schedule and
    flags go to every E-step (estep(): "scan" runs it in parallel over T, for
    one or a few long series).
    A pair whose log-likelihood is not finite keeps NaN parameters from then
    on."""
    if model not in FIT_MODELS:
        raise ValueError(f"baum_welch covers {FIT_MODELS}, not {model!r}")
    if pairing not in ("zip", "block"):
        raise ValueError("baum_welch: every pair carries its own parameters, pairing is 'zip' or 'block'")
    lib = lib or load_library()
    e_step = estep if model in MODELS else expected_stats
    params = {k: np.array(v, dtype=np.float64) for k, v in init.items()}
    trace = []
    for _ in range(int(n_iter)):
        stats = e_step(model, data, params, pairing, device, lib, schedule=schedule, flags=flags)
        trace.append(np.array(stats["loglik"]))
        params = m_step(model, stats, params)
    return params, np.array(trace).reshape(int(n_iter), -1)
