"""hhmm_amd.em_io on the GPU's IOHMM E-step: the generalised EM of
hhmm_amd.m_step_io (closed forms for p_1k and the emission parameters, one
step on Boehning's bound for w_km) started from random parameters.  The trace
is non-decreasing within the E-step's own tolerance (1e-9 relative to max(1,
|loglik|)), the fit improves, the mixture means come back ordered, and the
statistics of the first iteration are the reference's (tests/estep_io_ref.py).
"""
import numpy as np
import pytest

import estep_io_ref
import hhmm_amd
from hhmm_amd import synth
from test_estep_io import worst

TOL = 1e-9
N_ITER = 10


def _start(model, g, P, K, M, L, x):
    """Per-pair random starts spread over the data's range."""
    init = {"p_1k": g.dirichlet(np.full(K, 5.0), size=P), "w_km": g.normal(0.0, 0.3, size=(P, K, M))}
    if model == "iohmm-reg":
        init["b_km"] = g.normal(0.0, 1.0, size=(P, K, M))
        init["s_k"] = np.full((P, K), float(np.std(x))) * np.exp(g.normal(0.0, 0.1, size=(P, K)))
    else:
        lo, hi = np.quantile(x, [0.05, 0.95])
        init["lambda_kl"] = g.dirichlet(np.full(L, 5.0), size=(P, K))
        init["mu_kl"] = np.sort(g.uniform(lo, hi, size=(P, K, L)), axis=2)
        init["s_kl"] = np.full((P, K, L), float(np.std(x))) * np.exp(g.normal(0.0, 0.1, size=(P, K, L)))
        init["hypermu_k"] = np.sort(g.normal(0.0, 1.0, size=(P, K)), axis=1)  # not read by the likelihood
    return init


CASES = {
    "reg": ("iohmm-reg", lambda: synth.iohmm_reg(N=4, S=1, T=300, K=3, M=4), 3, 4, 0),
    "mix": ("iohmm-mix", lambda: synth.iohmm_mix(N=4, S=1, T=200, K=3, L=2, M=3), 3, 3, 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_em_io_improves_monotonically(engine, name):
    model, make, K, M, L = CASES[name]
    data, _true = make()
    P = np.shape(data["x_t"])[0]
    init = _start(model, np.random.Generator(np.random.Philox(key=99)), P, K, M, L, np.asarray(data["x_t"]))
    first = hhmm_amd.estep_io(model, data, init, "zip", lib=engine)
    w = worst(first, estep_io_ref.estep(model, data, init, "zip"))
    print(f"{model}: first iteration's statistics against the reference {w:.2e}")
    assert w <= TOL
    params, trace = hhmm_amd.em_io(model, data, init, N_ITER, pairing="zip", lib=engine)
    assert trace.shape == (N_ITER, P) and np.isfinite(trace).all()
    assert np.array_equal(trace[0], first["loglik"])
    drop = np.max((trace[:-1] - trace[1:]) / np.maximum(1.0, np.abs(trace[:-1])))
    print(f"{model}: worst relative decrease {max(drop, 0.0):.1e}; loglik {trace[0]} -> {trace[-1]}")
    assert drop <= TOL
    assert (trace[-1] > trace[0]).all()
    assert set(params) == set(init) and all(np.isfinite(v).all() for v in params.values())
    assert np.allclose(params["p_1k"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    if model != "iohmm-reg":
        assert (np.diff(params["mu_kl"], axis=2) >= 0).all()
        assert np.allclose(params["lambda_kl"].sum(axis=2), 1.0, rtol=0, atol=1e-12)
        assert np.array_equal(params["hypermu_k"], init["hypermu_k"])
