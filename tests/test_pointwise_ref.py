"""Pins tests/pointwise_ref.py (the numpy restatement the GPU pointwise entry
is compared with) to the CPU oracle: l_t is the oracle's loglik of the series
truncated to t steps minus that of t - 1 steps (the definition of a one-step-
ahead predictive density; 0 steps: 0), and sum_t l_t is the oracle's loglik.
The four cases of tests/test_estep_ref.py, 1e-9 relative to max(1, |value|).

Measured on a numpy prototype (N = 2, D = 70, T = 3000, both models): the
log-space cumulative-difference form and the scaled ratio form of l_t agree to
2.1e-12, the three reductions to 3e-13, a one-pass variance with the two-pass
one to 6e-14.
"""
import numpy as np
import pytest

import pointwise_ref
from test_estep_ref import CASES

TOL = 1e-9


def _close(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    model, make = CASES[request.param]
    data, draws = make()
    return model, data, draws, pointwise_ref.pointwise(model, data, draws, "grid")


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
        print(f"series {n}: worst l_t discrepancy {w:.2e}")
        assert w < TOL


def test_lp_t_sums_to_the_oracles_loglik(oracle, case):
    model, data, draws, ref = case
    want = oracle.gqs(model, data, draws, pars=["loglik"])["loglik"]
    assert _close(ref["loglik"], want) < TOL
    assert _close(ref["lp_t"].sum(axis=1), want) < TOL


def test_reductions_are_the_tabulated_formulas(case):
    _model, data, draws, ref = case
    S = draws["p_1k"].shape[0]
    for n in range(np.asarray(data["x"]).shape[0]):
        l = ref["lp_t"][n * S:(n + 1) * S]
        assert _close(ref["lpd_t"][n], np.log(np.mean(np.exp(l), axis=0))) < TOL
        assert _close(ref["mean_t"][n], l.mean(axis=0)) < TOL
        assert _close(ref["var_t"][n], l.var(axis=0, ddof=1)) < TOL


def test_non_finite_members_follow_ieee():
    inf, nan = np.inf, np.nan
    l = np.array([[-1.0, -inf, -inf, nan, -2.0], [-3.0, -2.0, -inf, -1.0, -2.0]])
    lpd, mean, var = pointwise_ref.reduce_draws(l)
    assert abs(lpd[0] - np.log(0.5 * (np.exp(-1.0) + np.exp(-3.0)))) < 1e-15 and lpd[1] == -2.0 + np.log(0.5)
    assert lpd[2] == -inf and np.isnan(lpd[3])
    assert mean[1] == -inf and mean[2] == -inf and np.isnan(mean[3])
    assert var[0] == 2.0 and np.isnan(var[1:4]).all() and var[4] == 0.0
    assert np.isnan(pointwise_ref.reduce_draws(l[:1])[2]).all()  # D = 1
