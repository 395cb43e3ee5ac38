"""CPU: every shape of tests/test_gpu_row_cursors.py plans the phased sweep.

hhmm_selftest_plan touches no device, so the shapes that module runs on the
GPU are checked here first: with its flags each request gives the phased
plan's words, the packed-symbol region included (L = 9 packs 4 bits)."""
import pytest

import test_gpu_row_cursors as rc
from hot_plan import C2, plan_of

SHAPES = [(P, T) for T in rc.EDGE_T for P in rc.EDGE_P] + [(65, 40), (65, 57), (70, 40), (70, 33), (140000, 1000)]


@pytest.mark.parametrize("P,T", SHAPES)
def test_shape_plans_the_phased_sweep(engine, P, T):
    got = plan_of(engine, rc.MODEL, rc.K, rc.L, P, T, C2, rc.FLAGS)
    assert {k: got[k] for k in rc.PLAN} == dict(rc.PLAN), got
    assert "xpk" in got["regions"] and "bp" in got["regions"]
