"""Baum-Welch, the M-step and the score on the GPU's E-step at 8 < K <= 32
(hhmm_estep_large through hhmm_amd.estep): the arithmetic of hhmm_amd.m_step /
score / em.baum_welch is K-agnostic, so what is checked is that the statistics
arrive -- one M-step against the reference's statistics (tests/estep_ref.py),
and EM's own invariant: it never lowers the likelihood it climbs (the CODED
likelihood; slack 1e-9 |l|, the parity tolerance of the log-likelihood, as in
tests/test_em.py).

Baum-Welch runs on hmm-multinom only.  With 12 or 23 Gaussian states on 70
points the likelihood of hmm.stan is unbounded (a state that owns one point
drives its sigma to 0), and EM goes there: the numpy reference EM
(tests/estep_ref.py with hhmm_amd.m_step) on synth.hmm_gauss(N=4, S=4, T=70)
has sigma at m_step's floor of 1e-150 after two iterations at K = 12 and after
one at K = 23, where its own trace then reads -1e272 and -4.5e277 -- no
sequence to test monotonicity on.  hmm is covered by the M-step and the score.
"""
import numpy as np
import pytest

import estep_ref
import hhmm_amd
from hhmm_amd import synth

SIMPLEX = {"hmm-multinom": ("p_1k", "A_ij", "phi_k"), "hmm": ("p_1k", "A_ij")}


def case(model, K, N=4, T=70):
    if model == "hmm-multinom":
        return synth.hmm_multinom(N=N, S=N, T=T, K=K, L=9)
    return synth.hmm_gauss(N=N, S=N, T=T, K=K)


def _close(got, want):
    return max(float(np.max(np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k])))) for k in want)


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(SIMPLEX))
def test_gpu_one_m_step_is_the_references(engine, model):
    data, draws = case(model, 12)
    got = hhmm_amd.m_step(model, hhmm_amd.estep(model, data, draws, "zip", lib=engine), draws)
    want = hhmm_amd.m_step(model, estep_ref.estep(model, data, draws, "zip"), draws)
    assert set(got) == set(want)
    assert _close(got, want) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 23])
def test_gpu_baum_welch_never_lowers_the_likelihood(engine, K):
    model = "hmm-multinom"
    data, draws = case(model, K)
    params, trace = hhmm_amd.baum_welch(model, data, draws, 6, pairing="zip", lib=engine)
    assert trace.shape == (6, 4) and np.isfinite(trace).all()
    assert all(np.isfinite(v).all() for v in params.values())
    assert (trace[1:] >= trace[:-1] - 1e-9 * np.abs(trace[:-1])).all(), np.diff(trace, axis=0).min()
    for name in SIMPLEX[model]:
        assert np.allclose(params[name].sum(axis=-1), 1.0, rtol=0, atol=1e-12), name


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(SIMPLEX))
def test_gpu_score_is_finite_and_has_the_parameters_shapes(engine, model):
    data, draws = case(model, 12)
    stats = hhmm_amd.estep(model, data, draws, "zip", lib=engine)
    g = hhmm_amd.score(model, draws, stats, "zip", 4, 4)
    assert set(g) == set(draws)
    for name, v in g.items():
        assert v.shape == np.shape(draws[name]) and np.isfinite(v).all(), name
