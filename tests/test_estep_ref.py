"""Pins tests/estep_ref.py (the numpy restatement the GPU E-step is compared
with) to the CPU oracle: its log-likelihood and gamma are the oracle's, its
pairwise sums have gamma's marginals, and the score built from its statistics
(hhmm_amd.estep.score, Fisher's identity with the Q2 weight) is the derivative
of the ORACLE's loglik by central differences.

Measured when the contract was prototyped (reference against reference): loglik
agrees to 3e-16 relative, gamma to 9e-13, and the worst finite-difference
discrepancy relative to max(1, |score|) was 9.0e-8 with h = 1e-6 (1e-5 for mu,
sigma); on the cases below it is 3.9e-8.  The bound 1e-6 is about 10x that.
"""
import numpy as np
import pytest

import estep_ref
from hhmm_amd import score, synth

CASES = {
    "multinom_K4_L9": ("hmm-multinom", lambda: synth.hmm_multinom(N=2, S=3, T=37, K=4, L=9)),
    "multinom_K7_L5": ("hmm-multinom", lambda: synth.hmm_multinom(N=2, S=3, T=37, K=7, L=5)),
    "gauss_K3": ("hmm", lambda: synth.hmm_gauss(N=2, S=3, T=37, K=3)),
    "gauss_K2_T100": ("hmm", lambda: synth.hmm_gauss(N=2, S=3, T=100, K=2)),
}
FD_TOL = 1e-6  # measured worst: 9.0e-8 (prototype), 3.9e-8 (these cases)


def _close(got, want, tol=1e-9):
    return np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    model, make = CASES[request.param]
    data, draws = make()
    return model, data, draws, estep_ref.estep(model, data, draws, "grid")


def test_loglik_and_gamma_are_the_oracles(oracle, case):
    model, data, draws, ref = case
    want = oracle.gqs(model, data, draws, pars=["loglik", "gamma_tk"])
    assert _close(ref["loglik"], want["loglik"]) < 1e-9
    x = np.asarray(data["x"])
    N, S = x.shape[0], draws["p_1k"].shape[0]
    for p in range(N * S):
        n, d = estep_ref.pair_coords("grid", p, S, N)
        par = {k: np.asarray(v)[d] for k, v in draws.items()}
        _ll, g, _xi = estep_ref.forward_backward(model, x[n], par)
        assert _close(g, want["gamma_tk"][p]) < 1e-9
        assert _close(ref["n_1k"][p], want["gamma_tk"][p, 0]) < 1e-9


def test_pairwise_sums_have_gammas_marginals(case):
    model, data, draws, ref = case
    x = np.asarray(data["x"])
    N, S = x.shape[0], draws["p_1k"].shape[0]
    for p in range(N * S):
        n, d = estep_ref.pair_coords("grid", p, S, N)
        par = {k: np.asarray(v)[d] for k, v in draws.items()}
        _ll, g, xi = estep_ref.forward_backward(model, x[n], par)
        assert np.allclose(xi.sum(axis=1), g[:-1].sum(axis=0), rtol=0, atol=1e-10)
        assert np.allclose(xi.sum(axis=0), g[1:].sum(axis=0), rtol=0, atol=1e-10)
        assert abs(xi.sum() - (x.shape[1] - 1)) < 1e-9
        assert np.array_equal(xi, ref["xi_ij"][p])


def _directions(model, K, L):
    """(name, index added to, index taken from or None, step)."""
    dirs = [("p_1k", (k,), ((k + 1) % K,), 1e-6) for k in range(K)]
    dirs += [("A_ij", (i, j), (i, (j + 1) % K), 1e-6) for i in range(K) for j in range(K)]
    if model == "hmm-multinom":
        dirs += [("phi_k", (k, l), (k, (l + 1) % L), 1e-6) for k in range(K) for l in range(L)]
    else:
        dirs += [(name, (k,), None, 1e-5) for name in ("mu_k", "sigma_k") for k in range(K)]
    return dirs


@pytest.mark.parametrize("pair", [0, 5])
def test_score_is_the_derivative_of_the_oracles_loglik(oracle, case, pair):
    model, data, draws, ref = case
    x = np.asarray(data["x"])
    N, S = x.shape[0], draws["p_1k"].shape[0]
    K, L = int(data["K"]), int(data.get("L", 0))
    n, d = estep_ref.pair_coords("grid", pair, S, N)
    g = score(model, draws, ref, "grid", S, N)
    dirs = _directions(model, K, L)
    pert = {k: np.repeat(np.asarray(v, dtype=np.float64)[d:d + 1], 2 * len(dirs), axis=0) for k, v in draws.items()}
    for m, (name, up, down, h) in enumerate(dirs):
        for row, sgn in ((2 * m, 1.0), (2 * m + 1, -1.0)):
            pert[name][(row,) + up] += sgn * h
            if down is not None:
                pert[name][(row,) + down] -= sgn * h
    one = dict(data, x=x[n:n + 1])
    ll = oracle.gqs(model, one, pert, pars=["loglik"])["loglik"]
    worst = 0.0
    for m, (name, up, down, h) in enumerate(dirs):
        fd = (ll[2 * m] - ll[2 * m + 1]) / (2 * h)
        want = g[name][(pair,) + up] - (g[name][(pair,) + down] if down is not None else 0.0)
        worst = max(worst, abs(fd - want) / max(1.0, abs(want)))
    print(f"worst finite-difference discrepancy {worst:.2e}")
    assert worst < FD_TOL
