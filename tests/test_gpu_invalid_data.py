"""The device entry enforces the data block's bounds pair by pair.

Stan rejects a data block whose int arrays leave their declared bounds:
int<lower=1,upper=L> x[T] (hmm/stan/hmm-multinom.stan:11), int<lower=1,upper=2>
sign[T] (tayal2009/stan/hhmm-tayal2009.stan:11-12; -lite.stan:11-16 for the
out-of-sample arrays), int<lower=1,upper=G> g[T] (hmm-multinom-semisup.stan:7-14).
hhmm_run checks them on the host and rejects the request (tests/test_abi.py).
hhmm_run_device cannot read its device arrays on the host: it flags each pair
whose series breaks a bound with HHMM_PAIR_INVALID_DATA and computes every other
pair as usual.  Each case corrupts one value of one series (and one ragged length)
and checks (a) exactly that series' pairs are flagged, (b) every other pair matches
the oracle on the clean data (tests/tolerances.py)."""
import numpy as np
import pytest

from hhmm_amd import _abi, synth
from hot_plan import SCHEDULE_PLAN, assert_plan
from tolerances import compare

pytestmark = pytest.mark.gpu

INVALID_DATA = _abi.PAIR_INVALID_DATA


def _run(engine, oracle, model, data, bad_data, draws, pars, bad_series, pairing="grid", flags=0):
    from devrun import DeviceRequest
    r = DeviceRequest(engine, model, bad_data, draws, pars, pairing=pairing, flags=flags)
    r.run()
    status = r.status.cpu().numpy()
    N = np.asarray(data["x"]).shape[0]
    S = np.asarray(next(iter(draws.values()))).shape[0]
    pairs = np.arange(r.P)
    series = pairs // S if pairing == "grid" else pairs
    flagged = np.isin(series, bad_series)
    assert (status[flagged] == INVALID_DATA).all(), status[flagged]
    assert (status[~flagged] == 0).all(), np.flatnonzero(status[~flagged])
    ok = pairs[~flagged]
    ref = oracle.gqs(model, data, draws, pars=pars, pairing=pairing, return_status=True, nthreads=8)
    for name in pars:
        compare(name, r.host_pairs(name, ok), np.asarray(ref[name])[ok])
    assert N == len(np.unique(series)) or pairing != "grid"
    return status


def _corrupt(data, key, n, t, v):
    bad = dict(data)
    a = np.array(data[key], copy=True)
    a[n, t] = v
    bad[key] = a
    return bad


C2_PARS = ["loglik", "gamma_tk", "zstar_t", "logp_zstar"]


_STATES = dict(schedule="separate", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="states", checked_inline="1")
C2_ROWS = [
    # (id, flags, the plan words pinned).  512 pairs at K = 4 decode state-parallel (use_vit_states: P < 131072)
    # whatever HHMM_FLAG_VFB / VFB_OFF say, so the first two rows are fb_kernel (which checks x inline) beside
    # viterbi_sp_kernel; HHMM_FLAG_VIT_LANES puts the batch on the lane-per-pair schedules of the full C2 batch.
    ("default-dispatch", 0, _STATES),
    ("two-kernels", _abi.FLAG_VFB_OFF, _STATES),
    ("fused", _abi.FLAG_FUSED | _abi.FLAG_VIT_LANES, dict(SCHEDULE_PLAN["fused"], checked_inline="0")),
    ("split", _abi.FLAG_FB_SPLIT | _abi.FLAG_VIT_LANES, dict(SCHEDULE_PLAN["split"], checked_inline="1")),
    ("lanes-phased-sweep", _abi.FLAG_VIT_LANES, dict(SCHEDULE_PLAN["phased"], checked_inline="1")),
    ("lanes-two-kernels", _abi.FLAG_VIT_LANES | _abi.FLAG_VFB_OFF,
     dict(SCHEDULE_PLAN["two-kernels"], checked_inline="1")),
]


@pytest.mark.parametrize("flags,plan", [r[1:] for r in C2_ROWS], ids=[r[0] for r in C2_ROWS])
def test_multinom_symbol_out_of_range(engine, oracle, flags, plan):
    """C2's request at 512 pairs x T = 200, each row pinned to its plan (tests/hot_plan.py).
    Without flags, and with the phased sweep switched off, this batch runs fb_kernel, which
    checks x as it packs the symbols, beside the state-parallel decoder.  With VIT_LANES it
    runs the schedules of the full batch: the phased sweep (phase 1 checks x while it packs),
    fb_kernel beside viterbi_kernel (both check inline), the fused sweep (the plan's
    checked_inline = 0: the check pass runs) and the split schedule (1: its forward launch
    checks x)."""
    data, draws = synth.hmm_multinom(N=512, S=512, T=200, K=4, L=9)
    bad = _corrupt(data, "x", 37, 101, 10)       # L + 1
    bad = _corrupt(bad, "x", 200, 0, 0)          # below 1
    bad = _corrupt(bad, "x", 311, 199, -7)
    assert_plan(engine, "hmm-multinom", data, draws, C2_PARS, flags, "zip", plan)
    _run(engine, oracle, "hmm-multinom", data, bad, draws, C2_PARS, [37, 200, 311], pairing="zip", flags=flags)


def test_multinom_grid_ragged_length(engine, oracle):
    """GRID pairing: every draw of the broken series is flagged; a T[n] past T_max too.
    A step past a series' own length is padding and is not checked."""
    data, draws = synth.hmm_multinom(N=6, S=64, T=300, K=4, L=9)
    T = np.array([300, 250, 300, 120, 300, 300], dtype=np.int32)
    data = dict(data, T=T)
    bad = dict(data, T=T.copy())
    bad["T"][4] = 301
    bad = _corrupt(bad, "x", 1, 20, 99)
    bad = _corrupt(bad, "x", 3, 200, 0)          # t >= T[3]: padding, not a violation
    _run(engine, oracle, "hmm-multinom", data, bad, draws, ["loglik", "gamma_tk", "zstar_t"], [1, 4])


def test_semisup_group_out_of_range(engine, oracle):
    data, draws = synth.hmm_multinom_semisup(N=8, S=32, T=150)
    bad = _corrupt(data, "g", 5, 77, 3)          # G + 1
    _run(engine, oracle, "hmm-multinom-semisup", data, bad, draws, ["loglik", "gamma_tk", "zstar_t"], [5])


def test_tayal_sign_out_of_range(engine, oracle):
    data, draws = synth.tayal(N=4, S=32, T=400)
    bad = _corrupt(data, "sign", 2, 399, 0)
    bad = _corrupt(bad, "x", 0, 3, 12)
    _run(engine, oracle, "hhmm-tayal2009", data, bad, draws, ["loglik", "gamma_tk", "zstar_t"], [0, 2])


def test_tayal_lite_out_of_sample(engine, oracle):
    data, draws = synth.tayal(N=4, S=16, T=300, T_oos=120)
    bad = _corrupt(data, "sign_oos", 1, 50, 3)
    bad = _corrupt(bad, "x_oos", 3, 0, 10)
    _run(engine, oracle, "hhmm-tayal2009-lite", data, bad, draws,
         ["loglik", "alpha_tk", "alpha_tk_oos", "zstar_t"], [1, 3])


def test_tayal_long_series_scan(engine, oracle):
    """One series under many draws, long T: the T-scan and the V-scan (C5's dispatch)."""
    data, draws = synth.tayal(N=2, S=8, T=40_000)
    bad = _corrupt(data, "x", 1, 39_999, 0)
    # alpha / beta, not gamma: past t ~ 2000 the Q6 masks underflow gamma's overlap to
    # NaN at the subnormal edge (tests/test_gpu_configs.py compare_tayal_gamma)
    _run(engine, oracle, "hhmm-tayal2009", data, bad, draws, ["loglik", "alpha_tk", "beta_tk", "zstar_t"], [1])


def test_large_k_symbol_out_of_range(engine, oracle):
    data, draws = synth.hmm_multinom(N=6, S=16, T=200, K=12, L=9)
    bad = _corrupt(data, "x", 2, 150, 10)
    _run(engine, oracle, "hmm-multinom", data, bad, draws, ["loglik", "gamma_tk", "zstar_t"], [2])


_LANES = _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF | _abi.FLAG_VIT_LANES
def _sep(fb, mode, vit, inline):
    return dict(schedule="separate", fb=fb, fb_mode=mode, vit=vit, checked_inline=inline)


SCHEDULES = [
    # (id, outputs, flags, the plan words pinned): which kernels read x, hence which check runs
    ("fb", ["loglik", "gamma_tk"], _LANES, _sep("linear", "GAMMA|PACK|BIG", "none", "1")),     # fb_kernel, inline
    ("forward", ["loglik"], _LANES, _sep("linear", "FWD", "none", "1")),           # fb_kernel forward only, inline
    ("alpha-beta", ["alpha_tk", "beta_tk"], _LANES, _sep("linear", "FULL", "none", "1")),  # fb_kernel FB_FULL, inline
    ("log-space", ["unalpha_tk"], _LANES, _sep("log", "FWD", "none", "0")),        # fb_log_kernel: check pass
    ("viterbi", ["zstar_t", "logp_zstar"], _LANES, _sep("none", "-", "lanes", "1")),    # viterbi_kernel, inline
    ("viterbi-states", ["zstar_t"], _abi.FLAG_VIT_STATES, _sep("none", "-", "states", "0")),  # viterbi_sp_kernel: pass
    ("two", C2_PARS, _LANES | _abi.FLAG_VFB_OFF,                                   # both inline, two streams
     dict(SCHEDULE_PLAN["two-kernels"], checked_inline="1", side_stream="1")),
    ("split", C2_PARS, _LANES | _abi.FLAG_FB_SPLIT, dict(SCHEDULE_PLAN["split"], checked_inline="1")),  # forward launch
    ("fused", C2_PARS, _LANES | _abi.FLAG_FUSED, dict(SCHEDULE_PLAN["fused"], checked_inline="0")),     # check pass
    ("scan", ["loglik", "gamma_tk"], _abi.FLAG_SCAN_FORCE,                         # T-scan: check pass
     dict(_sep("scan", "GAMMA", "none", "0"), scan_cl="64", scan_nc="4")),
]


@pytest.mark.parametrize("outs,flags,plan", [s[1:] for s in SCHEDULES], ids=[s[0] for s in SCHEDULES])
def test_multinom_schedules_ragged(engine, oracle, outs, flags, plan):
    """Every schedule of the hmm-multinom request flags the same series: the sweeps
    that read x over whole series check it inline (fb_sweep, viterbi_block, the phased
    sweep), the others leave it to data_check_kernel.  Ragged lengths put violations
    in a wave's full chunks, in its partial chunks, and in the padding past a
    series' own length (not a violation).  Each row asserts its plan first."""
    N, T = 300, 203
    data, draws = synth.hmm_multinom(N=N, S=N, T=T, K=4, L=9, seed=11)
    rng = np.random.default_rng(5)
    Tn = rng.integers(150, T + 1, size=N).astype(np.int32)
    Tn[17] = 161
    Tn[29] = 170
    data = dict(data, T=Tn)
    bad = dict(data, T=Tn.copy())
    bad["T"][60] = T + 1                          # length past T_max
    bad = _corrupt(bad, "x", 5, 3, 10)            # a full chunk (every lane's steps valid)
    bad = _corrupt(bad, "x", 17, 160, 0)          # the series' last step (a partial chunk)
    bad = _corrupt(bad, "x", 29, 170, 0)          # t = T[29]: padding, not a violation
    bad = _corrupt(bad, "x", 41, 100, -3)
    bad = _corrupt(bad, "x", 299, 149, 12)        # the last pair (the final wave's padded lanes)
    assert_plan(engine, "hmm-multinom", data, draws, outs, flags, "zip", plan)
    _run(engine, oracle, "hmm-multinom", data, bad, draws, outs, [5, 17, 41, 60, 299], pairing="zip", flags=flags)


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# The phased sweep (vfb_kernel) is a lane-per-pair schedule: at K <= 4 a batch below 131072 pairs decodes
# state-parallel instead (use_vit_states) and the request falls back to fb_kernel + viterbi_sp_kernel, so
# FLAG_VIT_LANES (_LANES) is what puts this small batch on it; the default dispatch runs beside it.
EXTREME_SCHEDULES = [s for s in SCHEDULES if s[0] in ("fb", "log-space")] + [
    ("phased-sweep", C2_PARS, _LANES, dict(SCHEDULE_PLAN["phased"], checked_inline="1")),  # vfb_kernel: inline
    ("default-dispatch", C2_PARS, 0, _STATES),                      # fb_kernel inline + viterbi_sp_kernel
]


@pytest.mark.parametrize("outs,flags,plan", [s[1:] for s in EXTREME_SCHEDULES],
                         ids=[s[0] for s in EXTREME_SCHEDULES])
def test_multinom_extreme_symbols(engine, oracle, outs, flags, plan):
    """The ends of int32 on the three checks that differ (inline in fb_sweep, the
    separate check pass, inline in the phased sweep, whose 4-bit packed symbols
    then feed its other phases) and on the default dispatch of this batch:
    INT32_MIN is R's NA_integer_, where `x - 1` wraps (formed in unsigned
    arithmetic), and INT32_MAX the largest index a table lookup could form.
    The kernels clamp the symbol before they index with it, so the series is
    flagged and nothing else changes; the same value in padding is no violation."""
    N, T = 130, 70
    data, draws = synth.hmm_multinom(N=N, S=N, T=T, K=4, L=9, seed=12)
    Tn = np.random.default_rng(6).integers(40, T + 1, size=N).astype(np.int32)
    Tn[3], Tn[70], Tn[129] = T, 55, 41
    data = dict(data, T=Tn)
    bad = _corrupt(data, "x", 3, 0, INT32_MIN)            # step 0 (the init row)
    bad = _corrupt(bad, "x", 70, 54, INT32_MAX)           # the series' last valid step
    bad = _corrupt(bad, "x", 129, 41, INT32_MIN)          # t = T[129]: padding, in the final (two-lane) wave
    assert_plan(engine, "hmm-multinom", data, draws, outs, flags, "zip", plan)
    _run(engine, oracle, "hmm-multinom", data, bad, draws, outs, [3, 70], pairing="zip", flags=flags)


def test_multinom_check_past_grid_y_limit(engine, oracle):
    """T_max above 65535 strips of 64 steps (4,194,240) -- the check
    kernel caps grid.y and loops over strips, so the launch still succeeds and a bad
    symbol past the cap is found (the long series runs the parallel scan over T)."""
    T = 4_300_000
    data, draws = synth.hmm_multinom(N=2, S=1, T=64, K=4, L=9)
    data = dict(data, x=np.random.default_rng(11).integers(1, 10, size=(2, T)).astype(np.int32))
    bad = _corrupt(data, "x", 1, 4_250_000, 10)   # in the strips past the cap
    from devrun import DeviceRequest
    got = DeviceRequest(engine, "hmm-multinom", bad, draws, ["loglik"])
    got.run()
    clean = DeviceRequest(engine, "hmm-multinom", data, draws, ["loglik"])
    clean.run()
    assert list(got.status.cpu().numpy()) == [0, INVALID_DATA]
    assert list(clean.status.cpu().numpy()) == [0, 0]
    # the clean series' pair is computed as usual (the oracle's 77 s at this T is
    # spared: the same device path on the clean data is the reference here)
    assert got.host_pairs("loglik", [0])[0] == clean.host_pairs("loglik", [0])[0]
    assert np.isfinite(clean.host_pairs("loglik", [0, 1])).all()
