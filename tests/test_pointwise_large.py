"""Pointwise predictive densities at 8 < K <= 32 (include/hhmm_pointwise.h,
hhmm_pointwise_large): l_t of every (series, draw) pair from the state-parallel
forward kernel and its reductions over the draws of each series from the
reduction kernel (csrc/hhmm_pointwise_large.hip), against the numpy restatement
of the contract (tests/pointwise_ref.py, K-agnostic, pinned to the CPU oracle at
these K by tests/test_pointwise_large_ref.py), to 1e-9 relative to
max(1, |reference|) with NaN and the infinities in the same places.

CPU: symbols, the argument checks (they come before the device check), the
workspace size and the routing of hhmm_amd.pointwise_predictive by K.  gpu: the
host entry (hhmm_pointwise_large) unless stated, and the device entry on
torch's stream.

Shapes: a group of G = 16 lanes owns a pair up to K = 16, G = 32 above; the
compile-time state loops run 16, 24 or 32 entries, so K = 9, 16 | 17, 24 | 25,
32 are both sides of every instance edge.  The filter renormalises every 8
steps and l_t leaves the group once per observation block of G steps, so T
covers 1, 2, the cadence edges 7 8 9, the block edges 16 17 and 32 33, and 70 (a
last block of 6 steps after two full ones at G = 32).  The reduction gives a
cell 4 lanes up to D = 16 draws, 16 up to 64, a wave up to 256 and the
workgroup above: D covers both sides of 16 | 17, 64 | 65 and 256 | 257.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import hhmm_amd
import pointwise_ref
from hhmm_amd import _abi, _stats
from test_estep import INT32_MIN
from test_estep_large import FAMILIES, KS, TOL, TS, make, worst

_pw = sys.modules["hhmm_amd.pointwise"]
ENTRIES = ("hhmm_pointwise_large", "hhmm_pointwise_large_device", "hhmm_pointwise_large_workspace_size")
REDUCED = ("lpd_t", "mean_t", "var_t")
# (pairing, N, S): D = 1, 1, 1 and 2 draws per series
PAIRINGS = [("grid", 1, 5), ("grid", 5, 1), ("zip", 5, 5), ("block", 5, 10)]


def check(engine, model, data, draws, pairing="grid"):
    got = hhmm_amd.pointwise_predictive(model, data, draws, pairing, per_draw=True, lib=engine, return_status=True)
    want = pointwise_ref.pointwise(model, data, draws, pairing)
    w = worst(got, want)
    print(f"{model} K={data['K']} {pairing}: worst discrepancy {w:.2e}")
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    return got, want


def rows(stats, keep, names=("loglik", "lp_t")):
    return {k: stats[k][keep] for k in names}


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ENTRIES:
        assert getattr(engine, name).restype is C.c_int
    assert callable(_pw.entry_name)


def _poke(field, value):
    def f(pr, res):
        obj, name = (pr.req, field) if "." not in field else (getattr(pr.req, field.split(".")[0]), field.split(".")[1])
        setattr(obj, name, value)
    return f


def _null(field):
    def f(pr, res):
        setattr(res, field, None)
    return f


# name -> (model, K, L, change to the prepared request, expected status, word of the message)
BAD = {
    "K8": ("hmm-multinom", 12, 9, _poke("data.K", 8), _abi.ERR_UNSUPPORTED, "K = 8"),
    "K8_gauss": ("hmm", 12, 0, _poke("data.K", 8), _abi.ERR_UNSUPPORTED, "K = 8"),
    "K33": ("hmm-multinom", 12, 9, _poke("data.K", 33), _abi.ERR_UNSUPPORTED, "K = 33"),
    "K33_gauss": ("hmm", 12, 0, _poke("data.K", 33), _abi.ERR_UNSUPPORTED, "K = 33"),
    "model_semisup": ("hmm-multinom", 12, 9, _poke("model", 3), _abi.ERR_UNSUPPORTED, "model"),
    "model_tayal": ("hmm-multinom", 12, 9, _poke("model", 8), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm": ("hmm", 12, 0, _poke("model", 4), _abi.ERR_UNSUPPORTED, "model"),
    "device_set": ("hmm-multinom", 12, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "abi": ("hmm", 12, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
    "null_loglik": ("hmm", 12, 0, _null("loglik"), _abi.ERR_INVALID_ARGUMENT, "loglik"),
    "null_lpd_t": ("hmm-multinom", 12, 9, _null("lpd_t"), _abi.ERR_INVALID_ARGUMENT, "lpd_t must"),
    "null_mean_t": ("hmm-multinom", 12, 9, _null("mean_t"), _abi.ERR_INVALID_ARGUMENT, "mean_t must"),
    "null_var_t": ("hmm", 12, 0, _null("var_t"), _abi.ERR_INVALID_ARGUMENT, "var_t must"),
    # two slots and the [L][G] table of one group against 160 KiB: L <= 1278 at G = 16, L <= 638 at G = 32
    "lds_G16": ("hmm-multinom", 12, 1279, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "L = 1279"),
    "lds_G32": ("hmm-multinom", 25, 639, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "L = 639"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _pw.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_pointwise_large(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_pointwise_large_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)
    if case.startswith("K8"):
        assert "hhmm_pointwise " in msg, msg
    if case.startswith("lds"):
        assert "LDS" in msg, msg


@pytest.mark.parametrize("entry", ["host", "device"])
def test_null_request_and_null_result_are_invalid_arguments(engine, entry):
    res = _abi.PointwiseResult()
    data, draws = make("hmm", 2, 2, 5, 12)
    pr, _res, _out = _pw.prepare("hmm", data, draws, "grid")
    if entry == "host":
        st = [engine.hhmm_pointwise_large(None, C.byref(res)), engine.hhmm_last_error().decode(),
              engine.hhmm_pointwise_large(C.byref(pr.req), None), engine.hhmm_last_error().decode()]
    else:
        st = [engine.hhmm_pointwise_large_device(None, C.byref(res), None, 0, None), engine.hhmm_last_error().decode(),
              engine.hhmm_pointwise_large_device(C.byref(pr.req), None, None, 0, None),
              engine.hhmm_last_error().decode()]
    assert st[0] == _abi.ERR_INVALID_ARGUMENT and "request" in st[1]
    assert st[2] == _abi.ERR_INVALID_ARGUMENT and "result" in st[3]


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 12, 1278), ("hmm-multinom", 25, 638), ("hmm", 32, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  The largest L of either group size."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _pw.prepare(model, data, draws, "grid", per_draw=True)
    st = engine.hhmm_pointwise_large(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()


@pytest.mark.parametrize("K,Tmax,P", [(9, 1, 1), (23, 70, 5), (32, 1000, 3)])
def test_workspace_is_l_t(engine, K, Tmax, P):
    """P * T_max * 8 bytes whatever the result holds: the size is a function of the request."""
    data, draws = make("hmm-multinom", P, P, Tmax, K, 3)
    for per_draw in (False, True):
        pr, _res, _out = _pw.prepare("hmm-multinom", data, draws, "zip", per_draw=per_draw)
        ws = C.c_size_t(0)
        assert engine.hhmm_pointwise_large_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
        assert ws.value == P * Tmax * 8


def test_workspace_size_rejects_the_lane_kernels_K(engine):
    data, draws = make("hmm-multinom", 2, 2, 5, 8, 3)
    pr, _res, _out = _pw.prepare("hmm-multinom", data, draws, "zip")
    ws = C.c_size_t(0)
    assert engine.hhmm_pointwise_large_workspace_size(C.byref(pr.req), C.byref(ws)) == _abi.ERR_UNSUPPORTED
    assert "K = 8" in engine.hhmm_last_error().decode()


def test_python_routing_by_K(monkeypatch):
    assert [_pw.entry_name(K) for K in (1, 8, 9, 32, 33)] == ["pointwise", "pointwise", "pointwise_large",
                                                              "pointwise_large", "pointwise_large"]
    data, draws = make("hmm-multinom", 3, 5, 6, 12, 9)
    pr, _res, out = _pw.prepare("hmm-multinom", data, draws, "grid", per_draw=True)
    assert pr.P == 15 and pr.K == 12
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "lpd_t": (3, 6), "mean_t": (3, 6), "var_t": (3, 6),
                                                     "lp_t": (15, 6)}
    called = []
    monkeypatch.setattr(_stats, "call", lambda lib, entry, pr, res, out, rs: called.append((entry, pr.K)) or out)
    for K in (8, 9):
        d, w = make("hmm-multinom", 2, 2, 5, K, 3)
        hhmm_amd.pointwise_predictive("hmm-multinom", d, w, lib=object())
    assert called == [("pointwise", 8), ("pointwise_large", 9)]


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("model,L", FAMILIES)
def test_gpu_parity(engine, model, L, K, T):
    for i, (pairing, N, S) in enumerate(PAIRINGS):
        data, draws = make(model, N, S, T, K, L, seed=1000 * K + 10 * T + i)
        got, _want = check(engine, model, data, draws, pairing)
        assert np.allclose(got["lp_t"].sum(axis=1), got["loglik"], rtol=1e-9, atol=1e-9)


_DRAW_CASES = {}


def _draw_case(K, D):
    """N = 2, T = 11, L = 9 under D draws per series and its reference; made once per (K, D)."""
    if (K, D) not in _DRAW_CASES:
        data, draws = make("hmm-multinom", 2, D, 11, K, 9, seed=D)
        _DRAW_CASES[K, D] = data, draws, pointwise_ref.pointwise("hmm-multinom", data, draws)
    return _DRAW_CASES[K, D]


@pytest.mark.gpu
@pytest.mark.parametrize("K,D", [(12, D) for D in (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)] +
                         [(23, D) for D in (7, 8, 9, 300)])
def test_gpu_draw_count_edges_of_the_reducer(engine, K, D):
    """Both sides of the reducer's width edges (16 | 17, 64 | 65, 256 | 257), members that leave lanes idle
    (D < the width) and several members per lane (1000 over 256 lanes)."""
    data, draws, want = _draw_case(K, D)
    got = hhmm_amd.pointwise_predictive("hmm-multinom", data, draws, per_draw=True, lib=engine)
    w = worst(got, want)
    print(f"K = {K}, D = {D}: worst discrepancy {w:.2e}")
    assert w <= TOL
    if D == 1:
        assert np.isnan(got["var_t"]).all() and np.array_equal(got["lpd_t"], got["mean_t"])
    if D in (1000, 300):  # no atomics, a fixed order: the same bits again
        again = hhmm_amd.pointwise_predictive("hmm-multinom", data, draws, per_draw=True, lib=engine)
        for name, v in got.items():
            assert np.array_equal(again[name], v, equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 23])
@pytest.mark.parametrize("model,L", [("hmm", 0), ("hmm-multinom", 9)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, L, K):
    lens = np.array([70, 1, 33, 8, 9], dtype=np.int32)
    N, S = 5, 3
    data, draws = make(model, N, S, 70, K, L, seed=K)
    for n in range(N):  # padding must not matter: garbage symbols / values past T[n]
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    got, _want = check(engine, model, data, draws)
    for n in range(N):  # cells and lp_t at t >= T[n] keep the NaN fill
        for name in REDUCED:
            assert np.isnan(got[name][n, lens[n]:]).all() and np.isfinite(got[name][n, :lens[n]]).all()
        assert np.isnan(got["lp_t"][S * n:S * n + S, lens[n]:]).all()
        assert np.isfinite(got["lp_t"][S * n:S * n + S, :lens[n]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", [(12, 17), (12, 21), (23, 9), (23, 11)])
@pytest.mark.parametrize("model,L", [("hmm", 0), ("hmm-multinom", 9)])
def test_gpu_past_one_workgroup_and_a_last_wave_with_one_group(engine, model, L, K, P):
    """256 threads hold 16 groups at K = 12 and 8 at K = 23: P = 17 / 9 start a second workgroup with one live
    group; P = 21 / 11 leave its second wave with one."""
    data, draws = make(model, P, P, 19, K, L, seed=P)
    check(engine, model, data, draws, "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("K,L", [(12, 1278), (12, 300), (25, 638), (23, 150)])
def test_gpu_tables_that_shrink_the_workgroup(engine, K, L):
    """The largest L of either group size (one group per workgroup, its table and slots 160 KiB) and an L
    between (four groups per workgroup: one wave at K = 12, L = 300, two at K = 23, L = 150)."""
    data, draws = make("hmm-multinom", 3, 3, 19, K, L, seed=L)
    check(engine, "hmm-multinom", data, draws, "zip")


@pytest.mark.gpu
def test_gpu_dense_cadence_for_a_tiny_symbol(engine):
    """phi = 1e-200 under every state of draw 1 breaks the bound of the eight-step renormalisation: the waves that
    hold its pairs renormalise every step, and l_t stays finite."""
    N, S, K, L = 2, 4, 12, 9
    data, draws = make("hmm-multinom", N, S, 40, K, L, seed=5)
    x = data["x"]
    x[x == L] = 1
    x[:, [3, 4, 20, 39]] = L
    clean, _want = check(engine, "hmm-multinom", data, draws)
    draws["phi_k"][1, :, L - 1] = 1e-200
    got, want = check(engine, "hmm-multinom", data, draws)
    hit = np.arange(N * S) % S == 1
    # l_t at the four steps is log(1e-200) to rounding: every state emits the symbol with that probability
    assert np.isfinite(got["lp_t"][hit]).all() and (got["lp_t"][hit][:, [3, 4, 20, 39]] < -199 * np.log(10)).all()
    assert (got["loglik"][hit] < -4 * 200 * np.log(10)).all() and np.isfinite(want["loglik"]).all()
    w = worst(rows(got, ~hit), rows(clean, ~hit))  # the other pairs: what they were without it
    assert w <= TOL, w


@pytest.mark.gpu
def test_gpu_structural_zeros_stay_finite(engine):
    K = 12
    data, draws = make("hmm-multinom", 3, 4, 41, K, 9, seed=3)
    band = np.abs(np.subtract.outer(np.arange(K), np.arange(K))) <= 2
    draws["A_ij"] = draws["A_ij"] * band
    draws["A_ij"] /= draws["A_ij"].sum(axis=2, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "lp_t") + REDUCED)


@pytest.mark.gpu
def test_gpu_impossible_symbol_is_minus_inf_then_nan_for_that_pair(engine):
    N, S, K, L, T = 3, 5, 12, 9, 27
    data, draws = make("hmm-multinom", N, S, T, K, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf and np.isfinite(np.delete(got["loglik"], p)).all()
    lp = got["lp_t"]
    assert np.isfinite(lp[p, :9]).all() and lp[p, 9] == -np.inf and np.isnan(lp[p, 10:]).all()
    assert np.isfinite(np.delete(lp, p, axis=0)).all()
    # the step itself: a -inf member; after it: a NaN member
    assert np.isfinite(got["lpd_t"][1, 9]) and got["mean_t"][1, 9] == -np.inf and np.isnan(got["var_t"][1, 9])
    for name in REDUCED:
        assert np.isnan(got[name][1, 10:]).all() and np.isfinite(got[name][1, :9]).all()
        assert np.isfinite(got[name][[0, 2]]).all()


@pytest.mark.gpu
def test_gpu_every_draw_impossible_is_minus_inf_not_nan(engine):
    """A cell whose members are all -inf: lpd_t = -inf (never NaN), mean_t = -inf, var_t = NaN; also at t = 1."""
    K, L = 12, 9
    data, draws = make("hmm-multinom", 2, 3, 6, K, L, seed=5)
    x = data["x"]
    x[x == L] = 1
    x[0, 0] = L
    x[1, 4] = L
    draws["phi_k"][:, :, L - 1] = 0.0
    draws["phi_k"] /= draws["phi_k"].sum(axis=2, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    for n, t in ((0, 0), (1, 4)):
        assert got["lpd_t"][n, t] == -np.inf and got["mean_t"][n, t] == -np.inf and np.isnan(got["var_t"][n, t])
        assert all(np.isnan(got[name][n, t + 1:]).all() for name in REDUCED)


@pytest.mark.gpu
@pytest.mark.parametrize("model,L", [("hmm-multinom", 9), ("hmm", 0)])
def test_gpu_nan_draw_is_nan_in_every_cell(engine, model, L):
    """The NaN enters with the first transition: l_1 of that draw is finite.  Its wave renormalises every step
    (a NaN parameter makes it dense), so the other pairs are the clean run's to the tolerance, not to the bit."""
    N, S, K = 3, 5, 12
    data, draws = make(model, N, S, 20, K, L, seed=13)
    clean, _want = check(engine, model, data, draws)
    draws["A_ij"][1, 0, 1] = np.nan
    got, _want = check(engine, model, data, draws)
    hit = np.arange(N * S) % S == 1
    assert np.isnan(got["loglik"][hit]).all() and np.isfinite(got["loglik"][~hit]).all()
    assert np.isnan(got["lp_t"][hit][:, 1:]).all() and np.isfinite(got["lp_t"][hit][:, 0]).all()
    assert worst(rows(got, ~hit), rows(clean, ~hit)) <= TOL
    for name in REDUCED:
        assert np.isnan(got[name][:, 1:]).all() and np.isfinite(got[name][:, 0]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,D", [("hmm-multinom", 12, 9, 70), ("hmm", 12, 0, 70), ("hmm-multinom", 23, 9, 20),
                                         ("hmm", 23, 0, 20), ("hmm-multinom", 12, 9, 300)])
def test_gpu_per_draw_output(engine, model, K, L, D):
    data, draws = make(model, 2, D, 19, K, L, seed=29)
    full = hhmm_amd.pointwise_predictive(model, data, draws, per_draw=True, lib=engine)
    lean = hhmm_amd.pointwise_predictive(model, data, draws, per_draw=False, lib=engine)
    assert "lp_t" not in lean
    for name, v in lean.items():  # the same kernels: l_t through the workspace instead of lp_t
        assert np.array_equal(full[name], v, equal_nan=True), name
    for n in range(2):  # the reductions again, on the host, from lp_t
        host = dict(zip(REDUCED, pointwise_ref.reduce_draws(full["lp_t"][n * D:(n + 1) * D])))
        assert worst({k: full[k][n] for k in REDUCED}, host) <= TOL
    ua = hhmm_amd.gqs(model, data, draws, pars=["unalpha_tk"], lib=engine)["unalpha_tk"]
    tot = pointwise_ref.estep_ref._lse(ua, 2)  # log sum_k exp(unalpha_tk): [P, T]
    assert worst({"lp_t": full["lp_t"]}, {"lp_t": np.diff(tot, axis=1, prepend=0.0)}) <= TOL


def _device(engine, model, data, draws, pairing="grid"):
    from stats_devrun import _Device
    return _Device(engine, "pointwise_large", _pw.prepare(model, data, draws, pairing, per_draw=True))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,pairing,N,S", [("hmm-multinom", 12, 9, "grid", 5, 30),
                                                   ("hmm", 23, 0, "block", 4, 72)])
def test_gpu_device_entry_is_the_host_entry(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 23, K, L, seed=17)
    data["T"] = np.array([23, 1, 9, 17, 8][:N], dtype=np.int32)
    host = hhmm_amd.pointwise_predictive(model, data, draws, pairing, per_draw=True, lib=engine)
    dv = _device(engine, model, data, draws, pairing)
    assert dv.run() == 0
    got = dv.stats()
    assert not got["pair_status"].any()
    for name, v in host.items():
        assert np.array_equal(got[name], v, equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_gpu_device_entry_flags_invalid_data(engine, bad):
    N, S, K, L = 4, 20, 12, 9
    data, draws = make("hmm-multinom", N, S, 15, K, L, seed=19)
    clean = _device(engine, "hmm-multinom", data, draws)
    assert clean.run() == 0
    want = clean.stats()
    data["x"][2, 6] = bad
    dv = _device(engine, "hmm-multinom", data, draws)
    assert dv.run() == 0
    got = dv.stats()
    hit = np.arange(N * S) // S == 2
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in ("loglik", "lp_t"):
        assert np.array_equal(got[name][~hit], want[name][~hit]), name
    for name in REDUCED:
        assert np.array_equal(got[name][[0, 1, 3]], want[name][[0, 1, 3]]), name


@pytest.mark.gpu
def test_gpu_device_entry_flags_a_length_outside_the_data_block(engine):
    data, draws = make("hmm", 3, 4, 9, 12, seed=23)
    data["T"] = np.array([9, 10, 0], dtype=np.int32)
    dv = _device(engine, "hmm", data, draws)
    assert dv.run() == 0
    got = dv.stats()
    assert got["pair_status"].tolist() == [0] * 4 + [_abi.PAIR_INVALID_DATA] * 8
    want = pointwise_ref.pointwise("hmm", dict(data, T=np.array([9, 9, 9])), draws)
    assert worst({k: got[k][:4] for k in ("loglik", "lp_t")}, {k: want[k][:4] for k in ("loglik", "lp_t")}) <= TOL
    assert worst({k: got[k][:1] for k in REDUCED}, {k: want[k][:1] for k in REDUCED}) <= TOL


@pytest.mark.gpu
def test_gpu_gibbs_to_waic_end_to_end(engine):
    """gibbs at K = 9 on two short series -> stack_chains -> pointwise_predictive(block) -> waic."""
    N, B, T, K, L = 2, 8, 30, 9, 4
    data, init = make("hmm-multinom", N, N * B, T, K, L, seed=71)
    draws, trace = hhmm_amd.gibbs("hmm-multinom", data, init, 6, burn=2, seed=3, pairing="block", lib=engine)
    assert trace.shape == (6, N * B) and draws["phi_k"].shape == (4, N * B, K, L)
    stacked = hhmm_amd.stack_chains(draws, N)
    got, want = check(engine, "hmm-multinom", data, stacked, "block")
    assert got["lp_t"].shape == (N * 4 * B, T) and want["lpd_t"].shape == (N, T)
    w = hhmm_amd.waic(got)
    assert all(np.isfinite(w[k]).all() for k in ("elpd_waic", "p_waic", "waic", "se"))
