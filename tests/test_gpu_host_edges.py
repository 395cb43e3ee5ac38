"""GPU: the smallest requests through hhmm_run -- the layer that turns a
caller's request into device shards, chunks and kernel launches.

* One draw (S = 1: R evaluating a few series at a posterior mean) under GRID
  pairing with fewer series than devices.  make_shards gives such a request a
  draws-shaped shard holding its single draw; split_shard must keep it whole
  (tests/test_shard_plan.py pins the plan on host buffers, this file the
  device run).  Over the device sets {0,0,0} and {0}*8 and in 1, 2 and 3 forced
  host chunks on one device, every output and pair_status is bit-identical to
  hhmm_run_device on the whole request and within tests/tolerances.py of the
  oracle.
* One pair (N = 1, S = 1) at T = 1, 2, 37 for every model, whole and in two
  forced chunks, against the oracle with every declared output.
* P = 63, 64, 65 under ZIP pairing: a final wave with one idle lane, none, and
  a second wave of one lane."""
import ctypes as C
import functools

import numpy as np
import pytest

from hhmm_amd import _abi, synth
from hot_plan import SCHEDULE_PLAN, assert_plan
from test_gpu_host_pipeline import _dev, _host
from test_gpu_invalid_data import C2_PARS
from test_gpu_parity import DEVICE_MODELS
from tolerances import compare_all

pytestmark = pytest.mark.gpu


@pytest.fixture
def devset(engine):
    def use(ords):
        arr = (C.c_int32 * len(ords))(*ords)
        assert engine.hhmm_init_devices(arr, len(ords)) == 0, engine.hhmm_last_error().decode()
    yield use
    assert engine.hhmm_init(1) == 0


ONE_DRAW = {
    "hmm-multinom": (dict(K=4, L=9), C2_PARS),
    "iohmm-reg": (dict(K=3), ["loglik", "gamma_tk", "zstar_t", "logp_zstar"]),
}
RAGGED = {2: [64, 1], 4: [64, 1, 33, 64], 7: [64, 17, 1, 64, 2, 63, 40]}


@functools.lru_cache(maxsize=None)
def _one_draw(model, N):
    """The request and the oracle's outputs, computed once per (model, N) and only read."""
    kw, pars = ONE_DRAW[model]
    data, draws = synth.GENERATORS[model](N=N, S=1, T=64, **kw)
    data["T"] = np.array(RAGGED[N], dtype=np.int32)
    import pyoracle
    ref = pyoracle.gqs(model, data, draws, pars=pars, return_status=True)
    return data, draws, pars, ref


def _check_one_draw(engine, model, N, got):
    data, draws, pars, ref = _one_draw(model, N)
    want = _dev(engine, model, data, draws, pars, "grid")
    for k in pars + ["pair_status"]:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=True), k
    compare_all(got, ref, pars + ["pair_status"])


@pytest.mark.parametrize("N", [2, 4, 7])
@pytest.mark.parametrize("shards", [3, 8])
@pytest.mark.parametrize("model", list(ONE_DRAW))
def test_one_draw_over_the_device_set(engine, oracle, devset, model, shards, N):
    """N < shards: one draws-shaped shard of a single draw; N >= shards (7 over 3): series shards."""
    data, draws, pars, _ = _one_draw(model, N)
    devset([0] * shards)
    got = _host(engine, model, data, draws, pars, "grid", 0, device=_abi.DEVICE_SET)
    _check_one_draw(engine, model, N, got)


@pytest.mark.parametrize("N", [2, 4, 7])
@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("model", list(ONE_DRAW))
def test_one_draw_in_host_chunks(engine, oracle, model, chunks, N):
    data, draws, pars, _ = _one_draw(model, N)
    got = _host(engine, model, data, draws, pars, "grid", chunks)
    _check_one_draw(engine, model, N, got)


@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("model", DEVICE_MODELS)
def test_one_pair_every_model(engine, oracle, model, T):
    """P = 1: one lane of one wave runs every declared output, whole and in two forced chunks."""
    data, draws = synth.GENERATORS[model](N=1, S=1, T=T)
    pars = synth.PARS[model]
    ref = oracle.gqs(model, data, draws, pars=pars, return_status=True)
    for chunks in (1, 2):
        got = _host(engine, model, data, draws, pars, "grid", chunks)
        assert got["loglik"].shape == (1,)
        compare_all(got, ref, pars + ["pair_status"])
        assert got["status"] == ref["status"], chunks


# At K = 4 a batch this small decodes state-parallel whatever the schedule flag (use_vit_states:
# P < 131072), so the first two rows both run fb_kernel + viterbi_sp_kernel.  FLAG_VIT_LANES puts the
# batch on the lane-per-pair kernels, whose last wave is the padded one: the phased sweep (vfb_kernel,
# launched per wave) and fb_kernel beside viterbi_kernel.
_LANES = _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF | _abi.FLAG_VIT_LANES
_STATES = dict(schedule="separate", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="states")
# (id, flags, the plan words asserted before the run)
WAVE_SCHEDULES = [("default", 0, _STATES), ("vfb-off", _abi.FLAG_VFB_OFF, _STATES),
                  ("lanes-phased-sweep", _LANES, SCHEDULE_PLAN["phased"]),
                  ("lanes-two-kernels", _LANES | _abi.FLAG_VFB_OFF, SCHEDULE_PLAN["two-kernels"])]


@pytest.mark.parametrize("flags,plan", [s[1:] for s in WAVE_SCHEDULES], ids=[s[0] for s in WAVE_SCHEDULES])
@pytest.mark.parametrize("P", [63, 64, 65])
def test_padded_final_wave(engine, oracle, P, flags, plan):
    import hhmm_amd
    data, draws = synth.hmm_multinom(N=P, S=P, T=64, K=4, L=9)
    assert_plan(engine, "hmm-multinom", data, draws, C2_PARS, flags, "zip", plan)
    got = hhmm_amd.gqs("hmm-multinom", data, draws, pars=C2_PARS, pairing="zip", lib=engine, return_status=True,
                       flags=flags)
    ref = oracle.gqs("hmm-multinom", data, draws, pars=C2_PARS, pairing="zip", return_status=True)
    compare_all(got, ref, C2_PARS + ["pair_status"])
