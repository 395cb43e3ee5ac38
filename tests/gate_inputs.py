"""Inputs on both sides of the renormalisation gate, one binade wide.

The lane kernels (renorm_sparse_safe, csrc/hhmm_fbchunk.h) and the large-K
kernels (lk_setup, csrc/hhmm_large.h) renormalise their filters only every 4
(8 < K <= 32: every 8) steps in a wave whose pairs all have

    b = phi_min * min(min_i rowmax_i(A), min_i colmax_i(A)) >= 2^-39,

and every step otherwise.  gate_b restates b from the draw arrays the kernels
read.  The builders start from synth.hmm_multinom and move one parameter so
that b sits at 2^-38.5 (`inside`: the sparse cadence, each step shrinking the
state by up to that factor) or at 2^-39.5 (`outside`: per-step
renormalisation); `mixed` alternates the two over the first 64 draws (so a
wave of 64 lanes, and every group of a large-K wave, holds both) and keeps
every later draw inside (a wave that stays sparse).  The factor sqrt(2) on
either side of the bound keeps the route independent of last-bit rounding of
the product.  Every row of phi_k and A_ij stays a simplex to within 4 ulp.
"""
import functools
import math

import numpy as np

from hhmm_amd import synth

BOUND = 2.0 ** -39
TARGET = {"inside": 2.0 ** -38.5, "outside": 2.0 ** -39.5}
SIDES = ("inside", "outside", "mixed")
RUN = slice(60, 100)                 # the run of 40 copies of symbol L (T >= 100)


def gate_b(draws):
    """b of every draw, from phi_k (S, K, L) and A_ij (S, K, K) as the kernels form it."""
    A = np.asarray(draws["A_ij"], dtype=np.float64)
    phi = np.asarray(draws["phi_k"], dtype=np.float64)
    tmin = np.minimum(A.max(axis=2).min(axis=1), A.max(axis=1).min(axis=1))
    return phi.min(axis=(1, 2)) * tmin


def _tmin(A):
    return np.minimum(A.max(axis=2).min(axis=1), A.max(axis=1).min(axis=1))


def targets(side, S):
    """The b each draw is built to have."""
    t = np.full(S, TARGET["inside"])
    if side == "outside":
        t[:] = TARGET["outside"]
    elif side == "mixed":
        t[1:64:2] = TARGET["outside"]
    elif side != "inside":
        raise KeyError(side)
    return t


def _base(K, L, P, T, pairing, N):
    if pairing == "zip":
        data, draws = synth.hmm_multinom(N=P, S=P, T=T, K=K, L=L)
    else:
        assert pairing == "grid" and P % N == 0
        data, draws = synth.hmm_multinom(N=N, S=P // N, T=T, K=K, L=L)
    return data, {k: np.array(v, dtype=np.float64) for k, v in draws.items()}


def _set_column(rows, col, value):
    """rows[..., col] = value with the other entries of each row rescaled to keep the row sum 1."""
    value = np.broadcast_to(value, rows[..., col].shape)
    rest = rows.sum(axis=-1) - rows[..., col]
    scale = (1.0 - value) / rest
    rows *= scale[..., None]
    rows[..., col] = value
    # the rounding left over goes to each row's largest entry, so the exact row sum is 1 to an ulp or two
    flat = rows.reshape(-1, rows.shape[-1])
    for r in flat:
        big = int(np.argmax(np.where(np.arange(r.size) == col, -1.0, r)))
        r[big] += 1.0 - math.fsum(r)


def simplex_error_ulps(rows):
    """Largest |exact row sum - 1| in units of 2^-52."""
    flat = np.asarray(rows).reshape(-1, np.asarray(rows).shape[-1])
    return max(abs(math.fsum(r) - 1.0) for r in flat) / 2.0 ** -52


def _with_run(data, L, T):
    assert T >= RUN.stop
    x = np.array(data["x"])
    x[:, RUN] = L
    data["x"] = x
    return data


@functools.lru_cache(maxsize=None)
def rare_symbol(side, K=4, L=9, P=130, T=120, pairing="zip", N=2):
    """Symbol L has probability v = target / tmin under every state, and every series a run of 40 of it."""
    data, draws = _base(K, L, P, T, pairing, N)
    v = targets(side, draws["phi_k"].shape[0]) / _tmin(draws["A_ij"])
    _set_column(draws["phi_k"], L - 1, v[:, None])
    return _with_run(data, L, T), draws


@functools.lru_cache(maxsize=None)
def one_likely_state(side, K=4, L=9, P=130, T=120, pairing="zip", N=2):
    """Symbol L has probability 0.3 under state 1 and v under the others: over the run of 40 the components of
    the filter diverge by about 2^-38 a step.  K >= 2."""
    assert K >= 2
    data, draws = _base(K, L, P, T, pairing, N)
    S = draws["phi_k"].shape[0]
    v = targets(side, S) / _tmin(draws["A_ij"])
    col = np.repeat(v[:, None], K, axis=1)
    col[:, 0] = 0.3
    _set_column(draws["phi_k"], L - 1, col)
    return _with_run(data, L, T), draws


@functools.lru_cache(maxsize=None)
def rare_state(side, K=4, L=9, P=130, T=120, pairing="zip", N=2):
    """Column K of A is c = target / phi_min (its column max, the smallest of A's row and column maxima), the
    other columns rescaled: a state nothing moves into.  K >= 2."""
    assert K >= 2
    data, draws = _base(K, L, P, T, pairing, N)
    c = targets(side, draws["A_ij"].shape[0]) / draws["phi_k"].min(axis=(1, 2))
    _set_column(draws["A_ij"], K - 1, c[:, None])
    return data, draws


BUILDERS = {"rare_symbol": rare_symbol, "one_likely_state": one_likely_state, "rare_state": rare_state}
