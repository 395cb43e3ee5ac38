"""Baum-Welch on the GPU's E-step (hhmm_amd.em.baum_welch, hhmm_amd.m_step).

EM never lowers the likelihood it climbs -- here the CODED likelihood, whose
Gaussian M-step takes x_1 with weight 1 for every state (quirk Q2).  The slack
1e-9 |l| of the monotonicity check is the parity tolerance of the
log-likelihood, not a tuning knob.  On these inputs the numpy reference EM
(tests/estep_ref.py with hhmm_amd.m_step) rose at every step, by at least 4e-10
relative, and ended 7 to 35 log units above its start.
"""
import numpy as np
import pytest

import estep_ref
import hhmm_amd
from hhmm_amd import synth

CASES = {
    "hmm-multinom": lambda: synth.hmm_multinom(N=8, S=8, T=64, K=4, L=9),
    "hmm": lambda: synth.hmm_gauss(N=8, S=8, T=64, K=3),
}


def _close(got, want):
    return max(float(np.max(np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k])))) for k in want)


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(CASES))
def test_gpu_baum_welch_never_lowers_the_likelihood(engine, model):
    data, draws = CASES[model]()
    params, trace = hhmm_amd.baum_welch(model, data, draws, 15, pairing="zip", lib=engine)
    assert trace.shape == (15, 8) and np.isfinite(trace).all()
    assert all(np.isfinite(v).all() for v in params.values())
    assert (trace[1:] >= trace[:-1] - 1e-9 * np.abs(trace[:-1])).all(), np.diff(trace, axis=0).min()
    assert (trace[-1] - trace[0] >= 5.0).all(), trace[-1] - trace[0]
    for name in ("p_1k", "A_ij") + (("phi_k",) if model == "hmm-multinom" else ()):
        assert np.allclose(params[name].sum(axis=-1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(CASES))
def test_gpu_one_m_step_is_the_references(engine, model):
    data, draws = CASES[model]()
    got = hhmm_amd.m_step(model, hhmm_amd.estep(model, data, draws, "zip", lib=engine), draws)
    want = hhmm_amd.m_step(model, estep_ref.estep(model, data, draws, "zip"), draws)
    assert set(got) == set(want)
    assert _close(got, want) <= 1e-9


@pytest.mark.gpu
def test_gpu_row_without_expected_count_keeps_its_values(engine):
    data, draws = CASES["hmm-multinom"]()
    draws = {k: np.array(v) for k, v in draws.items()}
    draws["A_ij"][:, :, 3] = 0.0      # state 4 is never entered nor started in: its rows get no count
    draws["A_ij"] /= draws["A_ij"].sum(axis=2, keepdims=True)
    draws["p_1k"][:, 3] = 0.0
    draws["p_1k"] /= draws["p_1k"].sum(axis=1, keepdims=True)
    params, trace = hhmm_amd.baum_welch("hmm-multinom", data, draws, 3, pairing="zip", lib=engine)
    assert np.isfinite(trace).all()
    assert np.array_equal(params["A_ij"][:, 3, :], draws["A_ij"][:, 3, :])
    assert np.array_equal(params["phi_k"][:, 3, :], draws["phi_k"][:, 3, :])
    assert not params["A_ij"][:, :3, 3].any() and np.allclose(params["A_ij"][:, :3, :].sum(axis=2), 1.0)
