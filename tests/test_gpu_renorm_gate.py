"""GPU: the renormalisation gate from one binade on either side of its bound.

renorm_sparse_safe (csrc/hhmm_fbchunk.h) lets a wave renormalise its filter
every kBigRenorm = 4 steps when every pair of it has b >= 2^-39; lk_setup
(csrc/hhmm_large.h, 8 < K <= 32) does the same with a cadence of 8.  The
other gate tests sit 60 binades or more on the dense side (a symbol of
probability 1e-30 or less) or at b ~ 1e-2 on the sparse side.  Here
tests/gate_inputs.py puts b at 2^-38.5 (`inside`: the sparse code path, the
state shrinking by up to 2^-38.5 a step, so the exponent counters move by
about 150 per renormalisation, checkpoints are rescaled under that shrink and
beta and the recomputed alpha carry very different exponents), at 2^-39.5
(`outside`: per-step renormalisation) and both within one wave (`mixed`, a
second wave all inside).  tests/test_gate_inputs.py shows on the CPU that no
gamma of these inputs is below 1e-240, so the 1e-250 floor of
tests/tolerances.py excuses nothing.

Every kernel that reads the gate runs every builder on every side against the
CPU oracle at tests/tolerances.py, plan-pinned where the request has a plan
(K <= 8): the four K = 4 schedules of the C2 request, fb_kernel FB_BIG alone,
phase 1 of the T-scan (forced, 32-step chunks), lk_fb_kernel and the forced
large-K scan at K = 12 and 23, and the statistics entries at K = 12 against
their own references at their own files' bound.  T = 120, 130 pairs, zip;
one grid batch per builder and kernel family.  CASES is walked without a
device by tests/test_hot_plan.py."""
import collections
import functools

import numpy as np
import pytest

import gate_inputs
from hhmm_amd import _abi, synth
from hot_plan import C2, LANES, SCHEDULES, run_planned

pytestmark = pytest.mark.gpu

MODEL = "hmm-multinom"
LG = ["loglik", "gamma_tk"]
FULL = ["loglik", "alpha_tk", "beta_tk", "gamma_tk"]
SCAN32 = _abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(5)
P, T = 130, 120

Case = collections.namedtuple("Case", "id builder side K pars flags pairing plan")


def inputs(case):
    """(data, draws) of a case: gate_inputs caches them, and they are only read."""
    return gate_inputs.BUILDERS[case.builder](case.side, K=case.K, L=9, P=P, T=T, pairing=case.pairing, N=2)


@functools.lru_cache(maxsize=None)
def reference(builder, side, K, pars, pairing):
    import pyoracle
    data, draws = gate_inputs.BUILDERS[builder](side, K=K, L=9, P=P, T=T, pairing=pairing, N=2)
    return pyoracle.gqs(MODEL, data, draws, pars=list(pars), pairing=pairing, return_status=True, nthreads=8)


def _cases():
    out = []
    big = dict(schedule="separate", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="none", scan_cl="0")
    scan = dict(schedule="separate", fb="scan", fb_mode="FULL", scan_cl="32", scan_nc="4")
    none = dict(schedule="none")                   # 8 < K <= 32 plans for itself (hhmm_large.h)

    def family(b, side, pairing, tag=""):
        rows = [(f"{sid}", 4, C2, flags, plan) for sid, flags, plan in SCHEDULES]
        rows += [(f"fb-big-K{K}", K, LG, LANES, big) for K in (2, 3, 4)]
        rows += [(f"tscan-K{K}", K, FULL, SCAN32, scan) for K in (2, 4, 8)]
        for K in (12, 23):
            rows += [(f"large-K{K}-gamma", K, C2, 0, none), (f"large-K{K}-full", K, FULL, 0, none),
                     (f"large-K{K}-scan", K, FULL, SCAN32, none)]
        return [Case(f"{b}-{side}{tag}-{rid}", b, side, K, pars, flags, pairing, plan)
                for rid, K, pars, flags, plan in rows]

    for b in gate_inputs.BUILDERS:
        for side in gate_inputs.SIDES:
            out += family(b, side, "zip")
        # one grid batch per builder and kernel family: 2 series x 65 draws, waves straddling the series
        keep = ("phased", "fb-big-K4", "tscan-K4", "large-K12-full", "large-K12-scan")
        out += [c for c in family(b, "mixed", "grid", "-grid") if c.id.rsplit("-grid-", 1)[1] in keep]
    return out


CASES = _cases()
STATS = [(b, side) for b in gate_inputs.BUILDERS for side in gate_inputs.SIDES]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gate(engine, oracle, case):
    data, draws = inputs(case)
    got, _ = run_planned(engine, oracle, MODEL, data, draws, case.pars, case.flags, case.pairing, case.plan,
                         tag=case.id, ref=reference(case.builder, case.side, case.K, tuple(case.pars), case.pairing))
    assert all(np.isfinite(got[k]).all() for k in case.pars if k != "zstar_t") and got["status"] == 0


def _stats_inputs(builder, side):
    return gate_inputs.BUILDERS[builder](side, K=12, L=9, P=P, T=T, pairing="zip", N=2)


@pytest.mark.parametrize("builder,side", STATS, ids=[f"{b}-{s}" for b, s in STATS])
def test_gate_estep_large(engine, builder, side):
    """estep_large_kernel (lk_setup's gate) against tests/estep_ref.py at tests/test_estep_large.py's bound."""
    from test_estep_large import check
    data, draws = _stats_inputs(builder, side)
    check(engine, MODEL, data, draws, "zip")


@pytest.mark.parametrize("builder,side", STATS, ids=[f"{b}-{s}" for b, s in STATS])
def test_gate_pointwise_large(engine, builder, side):
    """pointwise_large_kernel against tests/pointwise_ref.py at tests/test_pointwise_large.py's bound."""
    from test_pointwise_large import check
    data, draws = _stats_inputs(builder, side)
    check(engine, MODEL, data, draws, "zip")


@pytest.mark.parametrize("builder,side", STATS, ids=[f"{b}-{s}" for b, s in STATS])
def test_gate_draw_stats_large(engine, builder, side):
    """draw_stats_large_kernel: the counts of the engine's own FFBS path exact, loglik at
    tests/test_draw_stats_large.py's bound, host and device entries bit-identical."""
    from test_draw_stats_large import check
    data, draws = _stats_inputs(builder, side)
    check(engine, MODEL, data, draws, synth.ffbs_uniforms(P, T, seed=12), "zip")
