"""hhmm_run_summary / gqs_summary on the GPU: the engine's outputs reduced over
the draws on the device (include/hhmm_summary.h).

* against the engine itself: gqs_summary == the numpy restatement
  (tests/summary_ref.py) applied to gqs()'s per-draw outputs, bit for bit;
* independent of the number of series ranges and of a device set;
* against the CPU oracle: the restatement applied to oracle.gqs, within the
  output's own tolerance (a quantile of values that agree within a relative
  eps agrees within eps: order statistics and convex combinations of two of
  them are monotone in every value), integers exactly; hard states are checked
  against the returned quantiles, not the oracle (near ties may differ);
* a failed pair is summarised as it is; the walk-forward's filtered states.
"""
import ctypes as C

import numpy as np
import pytest

import summary_ref
from hhmm_amd import _abi, synth, walkforward
from tolerances import INT, compare

pytestmark = pytest.mark.gpu

SEQ = _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF
PROBS = (0.1, 0.5, 0.9)
PAIR = ("loglik", "logp_zstar")
_cache = {}


def _multinom():
    data, draws = synth.GENERATORS["hmm-multinom"](N=3, S=250, T=40)
    return dict(model="hmm-multinom", data=data, draws=draws, pairing="grid", S=250,
                pars=["loglik", "alpha_tk", "gamma_tk", "zstar_t", "logp_zstar"], hard=("alpha_tk",), kw={})


def _tayal_lite():
    N, B = 3, 64
    data, draws = synth.GENERATORS["hhmm-tayal2009-lite"](N=N, S=N * B, T=60, T_oos=48)
    data["T"] = np.array([60, 17, 1], dtype=np.int32)
    data["T_oos"] = np.array([5, 48, 1], dtype=np.int32)
    return dict(model="hhmm-tayal2009-lite", data=data, draws=draws, pairing="block", S=B,
                pars=["loglik", "alpha_tk", "alpha_tk_oos", "zstar_t"], hard=("alpha_tk", "alpha_tk_oos"), kw={})


def _hmix():
    data, draws = synth.GENERATORS["iohmm-hmix"](N=2, S=96, T=50)
    kw = {"uniforms": synth.ffbs_uniforms(192, 50, seed=11), "hat_rand": synth.hat_rand(192, 50, seed=12)}
    return dict(model="iohmm-hmix", data=data, draws=draws, pairing="grid", S=96,
                pars=["loglik", "gamma_tk", "oblik_t", "z_ffbs", "hatx_t"], hard=(), kw=kw)


CASES = {"hmm-multinom": _multinom, "tayal-lite-block": _tayal_lite, "iohmm-hmix": _hmix}


def _case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def _lengths(c, name):
    oos = name.endswith("_oos") or (name == "zstar_t" and c["model"] == "hhmm-tayal2009-lite")
    return c["data"].get("T_oos" if oos else "T")


def restate(c, full):
    """What gqs_summary must return, from per-draw outputs `full` (gqs or oracle)."""
    want = {}
    for name in c["pars"]:
        if name in PAIR:
            want[name] = np.asarray(full[name])
            continue
        T = _lengths(c, name)
        want[name] = summary_ref.quantiles(full[name], c["S"], PROBS, T=T)
        if name in c["hard"]:
            want["hard_" + name] = summary_ref.argmax(want[name][..., PROBS.index(0.5)], T=T)
    return want


def _summary(engine, c, flags=SEQ, device=-1):
    import hhmm_amd
    return hhmm_amd.gqs_summary(c["model"], c["data"], c["draws"], c["pars"], probs=PROBS, hard=c["hard"],
                                pairing=c["pairing"], flags=flags, device=device, lib=engine, **c["kw"])


def _full(engine, c):
    key = ("full", c["model"])
    if key not in _cache:
        import hhmm_amd
        _cache[key] = hhmm_amd.gqs(c["model"], c["data"], c["draws"], pars=c["pars"], pairing=c["pairing"],
                                   lib=engine, return_status=True, flags=SEQ, **c["kw"])
    return _cache[key]


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_restatement_of_gqs(engine, name):
    c = _case(name)
    full = _full(engine, c)
    got = _summary(engine, c)
    want = restate(c, full)
    assert got["status"] == full["status"] == 0
    assert set(want) <= set(got)
    _same(got, want, sorted(want))
    assert np.array_equal(got["pair_status"], full["pair_status"])
    for k in c["hard"]:
        assert got["hard_" + k].dtype == np.int32
        assert np.array_equal(got["hard_" + k], summary_ref.argmax(got[k][..., 1], T=_lengths(c, k)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_independent_of_series_ranges(engine, name):
    c = _case(name)
    one = _summary(engine, c, flags=SEQ | _abi.flag_host_chunks(1))
    three = _summary(engine, c, flags=SEQ | _abi.flag_host_chunks(3))
    keys = [k for k in one if k != "status"]
    _same(one, three, keys)
    _same(one, _summary(engine, c), keys)


@pytest.mark.parametrize("N", [3, 1])
def test_device_set_repeated(engine, N):
    data, draws = synth.GENERATORS["hmm-multinom"](N=N, S=250, T=40)
    c = dict(_case("hmm-multinom"), data=data, draws=draws)
    want = _summary(engine, c)
    assert engine.hhmm_init_devices((C.c_int32 * 2)(0, 0), 2) == 0
    try:
        got = _summary(engine, c, device=_abi.DEVICE_SET)
    finally:
        assert engine.hhmm_init(1) == 0
    _same(got, want, [k for k in want if k != "status"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_oracle(engine, oracle, name):
    c = _case(name)
    ref = oracle.gqs(c["model"], c["data"], c["draws"], pars=c["pars"], pairing=c["pairing"], **c["kw"])
    want = restate(c, ref)
    got = _summary(engine, c)
    for k in c["pars"]:
        if k in INT or k in ("hatx_t",):   # integer paths / draws, and hatx_t (bit-exact against the oracle: test_fitted)
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        else:
            compare(k, got[k], want[k])


def test_failed_pair_is_summarised_as_it_is(engine):
    """All delta_T = -inf for series 0 (a symbol no state emits): its zstar_t is 0 for every
    draw, flagged in pair_status; the summary holds those zeros."""
    import hhmm_amd
    data, draws = synth.hmm_multinom(N=2, S=4, T=60, K=4, L=5)
    draws["phi_k"][:, :, 4] = 0.0
    draws["phi_k"] /= draws["phi_k"].sum(axis=2, keepdims=True)
    data["x"][1][data["x"][1] == 5] = 1
    data["x"][0, 30] = 5
    pars = ["zstar_t", "logp_zstar"]
    full = hhmm_amd.gqs("hmm-multinom", data, draws, pars=pars, lib=engine, return_status=True, flags=SEQ)
    got = hhmm_amd.gqs_summary("hmm-multinom", data, draws, pars, probs=PROBS, lib=engine, flags=SEQ)
    assert full["status"] == got["status"] == _abi.WARN_PAIR_FAILURES
    assert (got["pair_status"][:4] == _abi.PAIR_INVALID_BACKPOINTER).all() and (got["pair_status"][4:] == 0).all()
    assert np.array_equal(got["pair_status"], full["pair_status"])
    assert (got["zstar_t"][0] == 0).all() and (got["zstar_t"][1] >= 1).all()
    assert np.array_equal(got["zstar_t"], summary_ref.quantiles(full["zstar_t"], 4, PROBS))
    assert np.array_equal(got["logp_zstar"], full["logp_zstar"], equal_nan=True)


def test_walkforward_filtered_states(engine):
    """wf-trade.R:119-120 per window, over the window's own steps."""
    c = _case("tayal-lite-block")
    full = _full(engine, c)
    states = walkforward.filtered_states(_summary(engine, c), c["data"])
    B = c["S"]
    assert len(states) == 3
    for n, st in enumerate(states):
        for key, name, T in (("state.filtered.ins", "alpha_tk", c["data"]["T"][n]),
                             ("state.filtered.oos", "alpha_tk_oos", c["data"]["T_oos"][n])):
            a = full[name][n * B:(n + 1) * B, :T]          # this window's extract(): [B, T_n, K]
            assert st[key].shape == (T,)
            assert np.array_equal(st[key], np.median(a, axis=0).argmax(axis=1) + 1), (n, key)
