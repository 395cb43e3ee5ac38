"""Baum-Welch for the masked programs (hhmm_amd.baum_welch on hhmm_amd.expected_stats).

EM never lowers the likelihood it climbs -- here the CODED likelihood of
hmm-multinom-semisup and hhmm-tayal2009, whose E-step is the adjoint sweep of
include/hhmm_expect.h; Tayal's M-step updates the parameters the program has
(p_11, the two rows of A_row, phi_k).  The slack 1e-9 |l| of the monotonicity
check is the parity tolerance of the log-likelihood, not a tuning knob.  On
these inputs the numpy reference EM (tests/expect_ref.py with hhmm_amd.m_step,
15 iterations) never fell: hhmm-tayal2009 ended 18.8 to 46.1 log units above
its start, its smallest step 2.8e-14 (3.5e-16 relative: a pair that had
converged), with p_11 on the boundary (0 or 1) and every log-likelihood finite;
hmm-multinom-semisup ended 43.0 to 65.8 above, its smallest step 0.044 (1.3e-3
relative).  The GPU fit must gain at least half the reference's smallest gain:
the factor absorbs nothing numerical, it only states that EM climbed.
"""
import numpy as np
import pytest

import expect_ref
import hhmm_amd
from hhmm_amd import synth

CASES = {
    "hhmm-tayal2009": lambda: synth.tayal(N=8, S=8, T=64, L=9),
    "hmm-multinom-semisup": lambda: synth.hmm_multinom_semisup(N=8, S=8, T=64),
}
REF_MIN_GAIN = {"hhmm-tayal2009": 18.8, "hmm-multinom-semisup": 42.9}
SIMPLEX = {"hhmm-tayal2009": ("A_row", "phi_k"), "hmm-multinom-semisup": ("p_1k", "A_ij", "phi_k")}


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
    gain = trace[-1] - trace[0]
    print(model, "gain", float(gain.min()), "to", float(gain.max()), "smallest step", float(np.diff(trace, axis=0).min()))
    assert (gain >= 0.5 * REF_MIN_GAIN[model]).all(), gain
    for name in SIMPLEX[model]:
        assert np.allclose(params[name].sum(axis=-1), 1.0, rtol=0, atol=1e-12), name
    if model == "hhmm-tayal2009":
        assert set(params) == {"p_11", "A_row", "phi_k"} and params["A_row"].shape == (8, 2, 2)
        assert ((params["p_11"] >= 0.0) & (params["p_11"] <= 1.0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(CASES))
def test_gpu_one_m_step_is_the_references(engine, model):
    data, draws = CASES[model]()
    got = hhmm_amd.m_step(model, hhmm_amd.expected_stats(model, data, draws, "zip", lib=engine), draws)
    want = hhmm_amd.m_step(model, expect_ref.expected_stats(model, data, draws, "zip"), draws)
    assert set(got) == set(want)
    assert _close(got, want) <= 1e-9
