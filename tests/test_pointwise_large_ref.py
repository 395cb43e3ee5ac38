"""Pins tests/pointwise_ref.py to the CPU oracle at K > 8, as
tests/test_pointwise_ref.py does at K <= 8: l_t is the oracle's loglik of the
series truncated to t steps minus that of t - 1 steps (0 steps: 0), and
sum_t l_t is the oracle's loglik.  The reference is K-agnostic; these are the
shapes of the state-parallel instances (K = 12: a group of 16 lanes, K = 23: of
32), 1e-9 relative to max(1, |value|).

Measured: the worst l_t discrepancy is 7.5e-15 (hmm-multinom, K = 12, L = 9)
and 5.0e-14 (hmm, K = 23).
"""
import numpy as np
import pytest

import pointwise_ref
from test_estep_large import make

TOL = 1e-9
CASES = {"multinom_K12": ("hmm-multinom", lambda: make("hmm-multinom", 2, 3, 37, 12, 9)),
         "gauss_K23": ("hmm", lambda: make("hmm", 2, 3, 37, 23))}


def _close(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    model, mk = CASES[request.param]
    data, draws = mk()
    ref = pointwise_ref.pointwise(model, data, draws, "grid")
    assert all(np.isfinite(v).all() for v in ref.values())
    return model, data, draws, ref


def test_lp_t_is_the_oracles_loglik_of_the_truncated_series(oracle, case):
    model, data, draws, ref = case
    x = np.asarray(data["x"])
    N, T = x.shape
    S = draws["p_1k"].shape[0]
    for n in range(N):
        # series i of this request: the first i + 1 steps of series n
        trunc = dict(data, x=np.tile(x[n], (T, 1)), T=np.arange(1, T + 1, dtype=np.int32))
        ll = oracle.gqs(model, trunc, draws, pars=["loglik"])["loglik"].reshape(T, S)  # p = s + S * i
        want = np.diff(ll, axis=0, prepend=0.0).T                                        # [S, T]
        w = _close(ref["lp_t"][n * S:(n + 1) * S], want)
        print(f"{model} K={data['K']} series {n}: worst l_t discrepancy {w:.2e}")
        assert w < TOL


def test_lp_t_sums_to_the_oracles_loglik(oracle, case):
    model, data, draws, ref = case
    want = oracle.gqs(model, data, draws, pars=["loglik"])["loglik"]
    assert _close(ref["loglik"], want) < TOL
    assert _close(ref["lp_t"].sum(axis=1), want) < TOL
