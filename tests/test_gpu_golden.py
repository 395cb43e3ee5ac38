"""GPU: every committed golden fixture (tests/golden/*.npz) through the HIP
path.  The fixtures hold seeded inputs and the oracle's outputs (made by
tests/golden/make_golden.py after the independent Python transcription
agreed); here the gfx950 engine must reproduce them: paths, statuses and
pair_status bit-exact, floats within tests/tolerances.py.  The HMM-family
fixtures also run through the parallel scan over T (forced 8-step chunks,
which a 4-step request rounds up to at K <= 4), the exact T-parallel Viterbi
(forced) and, for hmm-multinom's hot outputs, the phased sweep, so each
schedule meets the same vectors.  Every HMM-family case asserts the launch
plan of its request first (tests/hot_plan.py, want_plan below)."""
import numpy as np
import pytest

from hhmm_amd import _abi
from hot_plan import SCHEDULE_PLAN, assert_plan
from test_golden import MODELS, load
from tolerances import compare

pytestmark = pytest.mark.gpu

HMM_FAMILY = {"hmm", "hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009", "hhmm-tayal2009-lite"}
SCHEDULES = {
    "default": 0,
    "scan8": _abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(3),
    "scan4": _abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(2),
    "vscan": _abi.FLAG_VIT_SCAN,
    "vit-lanes": _abi.FLAG_VIT_LANES,
    "vit-states": _abi.FLAG_VIT_STATES,
    "vfb": _abi.FLAG_VIT_LANES | _abi.FLAG_VFB,
    # the hot request alone (hmm-multinom only): the one output set HHMM_FLAG_VFB plans the phased sweep for
    "phased-c2": _abi.FLAG_VIT_LANES | _abi.FLAG_VFB,
}
C2 = ["loglik", "gamma_tk", "zstar_t", "logp_zstar"]


def _cases():
    for m in MODELS:
        for name in SCHEDULES:
            if (name != "default" and m not in HMM_FAMILY) or (name == "phased-c2" and m != "hmm-multinom"):
                continue
            yield m, name


def want_plan(model, schedule, K):
    """The plan words of a fixture's request under a schedule (6 pairs x T = 16, every declared output).
    The fixtures ask for log-scale outputs, so the sequential forward-backward is the log-space recursion
    and `vfb` plans no phased sweep: the flag must be ignored, and the run is `vit-lanes` again.  A forced
    T-scan drops the log-scale outputs; at K <= 4 its chunks are whole 8-step fb chunks, so `scan4` rounds
    up to the 8 steps of `scan8`; tayal-lite has no backward sweep and no T-scan.  The T-parallel decoder
    exists at K = 2 and 4 (hmm's fixture is K = 3: the state-parallel decoder)."""
    if schedule == "phased-c2":
        return SCHEDULE_PLAN["phased"]
    lite, scan = model.endswith("-lite"), schedule.startswith("scan")
    vit = {"vit-lanes": "lanes", "vfb": "lanes", "vscan": "vscan" if K in (2, 4) else "states"}.get(schedule, "states")
    return dict(schedule="lite" if lite else "separate", vit=vit,
                fb=("linear" if lite else "scan") if scan else "log", scan_cl="8" if scan and not lite else "0",
                vs_nc="1" if vit == "vscan" else "0")


@pytest.mark.parametrize("model,schedule", list(_cases()), ids=[f"{m}-{s}" for m, s in _cases()])
def test_engine_reproduces_golden(engine, model, schedule):
    import hhmm_amd
    data, draws, outs = load(model)
    flags = SCHEDULES[schedule]
    pars = [k for k in outs if k != "pair_status"]
    if schedule.startswith("scan"):
        # the T-scan evaluates the probability-space profile (log-scale outputs stay sequential)
        pars = [k for k in pars if k not in ("unalpha_tk", "unbeta_tk", "unalpha_tk_oos")]
    if schedule == "phased-c2":
        pars = C2
    if model in HMM_FAMILY:
        assert_plan(engine, model, data, draws, pars, flags, "grid", want_plan(model, schedule, int(data["K"])))
    got = hhmm_amd.gqs(model, data, draws, pars=pars, lib=engine, return_status=True, flags=flags)
    for k in pars + ["pair_status"]:
        compare(k, got[k], outs[k])
