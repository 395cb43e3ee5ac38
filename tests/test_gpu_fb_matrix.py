"""GPU: every K <= 8 forward-backward and Viterbi kernel of the HMM family
against the CPU oracle, at the loop edges of its sweeps.

The table is tests/fb_matrix.py (shapes and rows in its docstring): one case
per (forward-backward kernel, decoder) pair that a (model, K) has, on a batch
whose lengths sit at every edge of fb_sweep's chunk loops, ragged inside a
wave.  Each case asserts its launch plan first (tests/hot_plan.py), then
compares every output it asked for, and pair_status, with the oracle at
tests/tolerances.py: floats to 1e-9, zstar_t / z_ffbs / pair_status exact, NaN
and infinities in the same places, every pair and every step.
tests/test_fb_matrix_plan.py walks the same table on the CPU and shows that
it covers every kernel the plan function can name at these shapes."""
import pytest

import fb_matrix as fm
from hot_plan import run_planned

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", fm.CASES, ids=[c.id for c in fm.CASES])
def test_fb_matrix(engine, oracle, case):
    data, draws, uu = fm.inputs(case.key)
    ref = fm.reference(case.key, tuple(case.pars))
    got, _ = run_planned(engine, oracle, case.model, data, draws, case.pars, case.flags, case.pairing, case.plan,
                         uniforms=uu if "z_ffbs" in case.pars else None, tag=case.id,
                         ref=ref)
    assert set(got) == set(case.pars) | {"pair_status", "status"}
    assert got["status"] == ref["status"]
