"""Pins tests/estep_io_ref.py (the numpy restatement the GPU's IOHMM E-step is
compared with) to the CPU oracle: its log-likelihood is the oracle's for
iohmm-reg and the three mixture programs, and the score built from its
statistics (hhmm_amd.score_io, Fisher's identity) is the derivative of the
ORACLE's loglik by central differences.  Then the identities of the contract
and the monotone trace of the generalised EM of hhmm_amd.m_step_io on the
reference E-step.

Measured when the contract was prototyped (reference against reference): loglik
agrees to 4.3e-14 relative (reg) and 2.2e-16 (mixtures); the worst
finite-difference discrepancy relative to max(1, |score|) was 5.2e-8 (reg) and
4.5e-9 (mixtures) with h = 1e-6 for p_1k, lambda_kl and s_kl and 1e-5 for w_km,
b_km, s_k and mu_kl; the worst relative decrease over an EM run was 6e-16.  The
bounds are the project's FD_TOL = 1e-6 and 1e-12.
"""
import numpy as np
import pytest

import estep_io_ref
from hhmm_amd import m_step_io, score_io, synth

CASES = {
    "reg_K3_M4": ("iohmm-reg", lambda: synth.iohmm_reg(N=2, S=3, T=37, K=3, M=4)),
    "reg_K2_M3": ("iohmm-reg", lambda: synth.iohmm_reg(N=2, S=3, T=50, K=2, M=3)),
    "mix_K4_L3": ("iohmm-mix", lambda: synth.iohmm_mix(N=2, S=3, T=37, K=4, L=3, M=4)),
    "hmix_K3_L2": ("iohmm-hmix", lambda: synth.iohmm_mix(N=2, S=3, T=37, K=3, L=2, M=3)),
    "lite_K3_L2": ("iohmm-hmix-lite", lambda: synth.iohmm_mix(N=2, S=3, T=37, K=3, L=2, M=3)),
}
FD_TOL = 1e-6  # measured worst: 5.2e-8 (reg), 4.5e-9 (mixtures)
STEP = {"p_1k": 1e-6, "lambda_kl": 1e-6, "s_kl": 1e-6, "w_km": 1e-5, "b_km": 1e-5, "s_k": 1e-5, "mu_kl": 1e-5}


def _close(got, want):
    return np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    model, make = CASES[request.param]
    data, draws = make()
    return model, data, draws, estep_io_ref.estep(model, data, draws, "grid")


def test_loglik_is_the_oracles(oracle, case):
    model, data, draws, ref = case
    want = oracle.gqs(model, data, draws, pars=["loglik"])["loglik"]
    w = _close(ref["loglik"], want)
    print(f"{model}: loglik against the oracle {w:.2e}")
    assert w < 1e-9


def _directions(model, K, M, L):
    """(name, index added to, index taken from or None): simplex parameters move along a tangent."""
    dirs = [("p_1k", (k,), ((k + 1) % K,)) for k in range(K)]
    dirs += [("w_km", (k, m), None) for k in range(K) for m in range(M)]
    if model == "iohmm-reg":
        dirs += [("b_km", (k, m), None) for k in range(K) for m in range(M)]
        dirs += [("s_k", (k,), None) for k in range(K)]
    else:
        dirs += [("lambda_kl", (k, l), (k, (l + 1) % L)) for k in range(K) for l in range(L)]
        dirs += [(name, (k, l), None) for name in ("mu_kl", "s_kl") for k in range(K) for l in range(L)]
    return dirs


@pytest.mark.parametrize("pair", [0, 5])
def test_score_is_the_derivative_of_the_oracles_loglik(oracle, case, pair):
    model, data, draws, ref = case
    x, u, _Tn = estep_io_ref.series(data)
    N, S = x.shape[0], draws["p_1k"].shape[0]
    K, M, L = int(data["K"]), int(data["M"]), int(data.get("L", 0))
    n, d = estep_io_ref.pair_coords("grid", pair, S, N)
    g = score_io(model, draws, ref, "grid", S, N)
    dirs = _directions(model, K, M, L)
    pert = {k: np.repeat(np.asarray(v, dtype=np.float64)[d:d + 1], 2 * len(dirs), axis=0) for k, v in draws.items()}
    for m, (name, up, down) in enumerate(dirs):
        for row, sgn in ((2 * m, 1.0), (2 * m + 1, -1.0)):
            pert[name][(row,) + up] += sgn * STEP[name]
            if down is not None:
                pert[name][(row,) + down] -= sgn * STEP[name]
    one = dict(data, x_t=x[n:n + 1], u_tm=u[n:n + 1])
    ll = oracle.gqs(model, one, pert, pars=["loglik"])["loglik"]
    worst = 0.0
    for m, (name, up, down) in enumerate(dirs):
        fd = (ll[2 * m] - ll[2 * m + 1]) / (2 * STEP[name])
        want = g[name][(pair,) + up] - (g[name][(pair,) + down] if down is not None else 0.0)
        worst = max(worst, abs(fd - want) / max(1.0, abs(want)))
    print(f"{model}: worst finite-difference discrepancy {worst:.2e}")
    assert worst < FD_TOL


def test_identities(case):
    model, data, _draws, ref = case
    T = np.shape(data["x_t"])[-1]
    assert np.allclose(ref["n_1k"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.allclose(ref["gw_km"].sum(axis=1), 0.0, rtol=0, atol=1e-10)
    if model == "iohmm-reg":
        assert np.allclose(ref["n_k"].sum(axis=1), T, rtol=1e-12, atol=0)
        assert np.array_equal(ref["uu_kmm"], ref["uu_kmm"].transpose(0, 1, 3, 2))
    else:
        assert np.allclose(ref["n_kl"].sum(axis=(1, 2)), T, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["reg_K3_M4", "mix_K4_L3"])
def test_a_single_step_has_no_transition(name):
    model, make = CASES[name]
    data, draws = make()
    one = dict(data, x_t=np.asarray(data["x_t"])[:, :1], u_tm=np.asarray(data["u_tm"])[:, :1])
    ref = estep_io_ref.estep(model, one, draws, "grid")
    assert not ref["gw_km"].any()
    if model == "iohmm-reg":
        assert np.array_equal(ref["n_k"], ref["n_1k"])
    else:
        assert np.allclose(ref["n_kl"].sum(axis=2), ref["n_1k"], rtol=0, atol=1e-15)


def _random_start(model, g, P, K, M, L, x):
    """Per-pair starts spread over the data's range, wide enough that the s_min floor stays away."""
    init = {"p_1k": g.dirichlet(np.full(K, 5.0), size=P), "w_km": g.normal(0.0, 0.3, size=(P, K, M))}
    if model == "iohmm-reg":
        init["b_km"] = g.normal(0.0, 1.0, size=(P, K, M))
        init["s_k"] = np.full((P, K), float(np.std(x))) * np.exp(g.normal(0.0, 0.1, size=(P, K)))
    else:
        lo, hi = np.quantile(x, [0.05, 0.95])
        init["lambda_kl"] = g.dirichlet(np.full(L, 5.0), size=(P, K))
        init["mu_kl"] = np.sort(g.uniform(lo, hi, size=(P, K, L)), axis=2)
        init["s_kl"] = np.full((P, K, L), float(np.std(x))) * np.exp(g.normal(0.0, 0.1, size=(P, K, L)))
    return init


EM_CASES = {
    "reg": ("iohmm-reg", lambda: synth.iohmm_reg(N=2, S=1, T=300, K=3, M=4), 3, 4, 0),
    "mix": ("iohmm-mix", lambda: synth.iohmm_mix(N=2, S=1, T=200, K=3, L=2, M=3), 3, 3, 2),
}


@pytest.mark.parametrize("name", sorted(EM_CASES))
def test_em_on_the_reference_estep_never_decreases(name):
    model, make, K, M, L = EM_CASES[name]
    data, _true = make()
    g = np.random.Generator(np.random.Philox(key=77))
    P = np.shape(data["x_t"])[0]
    params = _random_start(model, g, P, K, M, L, np.asarray(data["x_t"]))
    s_min, trace = 1e-4, []
    for _ in range(12):
        stats = estep_io_ref.estep(model, data, params, "zip")
        trace.append(stats["loglik"].copy())
        params.update(m_step_io(model, stats, params, data, "zip", s_min))
        sname = "s_k" if model == "iohmm-reg" else "s_kl"
        assert (params[sname] > s_min).all(), "the s_min floor must not bind in this test"
    trace = np.array(trace)
    drop = np.max((trace[:-1] - trace[1:]) / np.maximum(1.0, np.abs(trace[:-1])))
    print(f"{model}: worst relative decrease {max(drop, 0.0):.1e}; loglik {trace[0]} -> {trace[-1]}")
    assert drop <= 1e-12
    assert (trace[-1] > trace[0]).all()
    if model != "iohmm-reg":
        assert (np.diff(params["mu_kl"], axis=2) >= 0).all()
