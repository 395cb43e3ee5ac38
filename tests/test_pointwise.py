"""Pointwise predictive densities (include/hhmm_pointwise.h): l_t of every
(series, draw) pair and its reductions over the draws of each series, against
the numpy restatement of the contract (tests/pointwise_ref.py, pinned to the
CPU oracle by tests/test_pointwise_ref.py), to 1e-9 relative to
max(1, |reference|) with NaN and the infinities in the same places.

CPU: symbols, struct layout, Python shape checks, the argument checks (they
come before the device check) and the arithmetic of waic().  gpu: the host
entry (hhmm_pointwise) unless stated, and the device entry on torch's stream.

Shapes: C = fb_chunk(K) is 8 at K <= 4 and 4 above; T covers the chunk edges,
D the wave, the workgroup's coverage (tile_draws) and the multi-tile finish.
"""
import ctypes as C
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import hhmm_amd
import pointwise_ref
from hhmm_amd import _abi, synth
from test_estep import INT32_MIN, TOL, fb_chunk, make, worst

REPO = pathlib.Path(__file__).resolve().parent.parent
_pw = sys.modules["hhmm_amd.pointwise"]
REDUCED = ("lpd_t", "mean_t", "var_t")


def check(engine, model, data, draws, pairing="grid"):
    got = hhmm_amd.pointwise_predictive(model, data, draws, pairing, per_draw=True, lib=engine, return_status=True)
    want = pointwise_ref.pointwise(model, data, draws, pairing)
    w = worst(got, want)
    print(f"{model} {pairing}: worst discrepancy {w:.2e}")
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    return got, want


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ("hhmm_pointwise", "hhmm_pointwise_device", "hhmm_pointwise_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    for name in ("pointwise_predictive", "waic"):
        assert callable(getattr(hhmm_amd, name))


def test_struct_layout_matches_header(tmp_path):
    cls = _abi.PointwiseResult
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hhmm_pointwise.h"', "int main(void){",
           'printf("sizeof %zu\\n", sizeof(hhmm_pointwise_result));']
    for f, _ in cls._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(hhmm_pointwise_result, {f}));')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(REPO / "include"), str(c), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    lay = {r.split()[0]: int(r.split()[1]) for r in rows if r}
    assert lay["sizeof"] == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert lay[f] == getattr(cls, f).offset, f


def test_python_shape_checks():
    data, draws = make("hmm-multinom", 3, 6, 7, 4, 9)
    pr, res, out = _pw.prepare("hmm-multinom", data, draws, "grid")
    assert pr.P == 18 and not res.lp_t
    assert {k: v.shape for k, v in out.items()} == {"loglik": (18,), "lpd_t": (3, 7), "mean_t": (3, 7), "var_t": (3, 7)}
    assert all(np.isnan(v).all() for v in out.values())
    _pr, res, out = _pw.prepare("hmm-multinom", data, draws, "block", per_draw=True)
    assert out["lp_t"].shape == (6, 7) and out["lpd_t"].shape == (3, 7) and res.lp_t
    gd, gw = make("hmm", 6, 6, 5, 3)
    _pr, _res, out = _pw.prepare("hmm", gd, gw, "zip", per_draw=True)
    assert out["lp_t"].shape == (6, 5) and out["var_t"].shape == (6, 5)
    with pytest.raises(ValueError):
        _pw.prepare("hhmm-tayal2009", data, draws)
    with pytest.raises(ValueError):
        _pw.prepare("hmm-multinom", data, draws, "zip")                       # N != S
    with pytest.raises(ValueError):
        _pw.prepare("hmm-multinom", data, dict(draws, p_1k=draws["p_1k"][:4], A_ij=draws["A_ij"][:4],
                                               phi_k=draws["phi_k"][:4]), "block")  # S % N
    with pytest.raises(ValueError):
        _pw.prepare("hmm-multinom", data, dict(draws, phi_k=draws["phi_k"][:, :, :8]))
    with pytest.raises(ValueError):
        _pw.prepare("hmm", gd, {k: v for k, v in gw.items() if k != "sigma_k"})


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
    "model_semisup": ("hmm-multinom", 4, 9, _poke("model", 3), _abi.ERR_UNSUPPORTED, "model"),
    "model_tayal": ("hmm-multinom", 4, 9, _poke("model", 8), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm": ("hmm", 3, 0, _poke("model", 4), _abi.ERR_UNSUPPORTED, "model"),
    "K9": ("hmm-multinom", 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K9_gauss": ("hmm", 3, 0, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": ("hmm-multinom", 4, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "lds": ("hmm-multinom", 8, 39, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),      # 39 * 4 = 156 > 154
    "lds_odd_K": ("hmm-multinom", 7, 39, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "null_loglik": ("hmm", 3, 0, _null("loglik"), _abi.ERR_INVALID_ARGUMENT, "loglik"),
    "null_lpd_t": ("hmm-multinom", 4, 9, _null("lpd_t"), _abi.ERR_INVALID_ARGUMENT, "lpd_t must"),
    "null_mean_t": ("hmm-multinom", 4, 9, _null("mean_t"), _abi.ERR_INVALID_ARGUMENT, "mean_t must"),
    "null_var_t": ("hmm", 3, 0, _null("var_t"), _abi.ERR_INVALID_ARGUMENT, "var_t must"),
    "abi": ("hmm", 3, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _pw.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_pointwise(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_pointwise_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 7, 38), ("hmm", 3, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  L * ceil(K / 2) = 152 <= 154 still fits."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _pw.prepare(model, data, draws, "grid", per_draw=True)
    st = engine.hhmm_pointwise(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws = C.c_size_t(1)
    assert engine.hhmm_pointwise_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == 0  # two draws: one workgroup


@pytest.mark.parametrize("model,K,L,cover", [("hmm-multinom", 4, 9, 256), ("hmm-multinom", 4, 23, 192),
                                             ("hmm-multinom", 8, 16, 128), ("hmm-multinom", 8, 38, 64),
                                             ("hmm", 8, 0, 256)])
def test_workspace_size_is_the_documented_value(engine, model, K, L, cover):
    """0 while one workgroup covers the draws of a series, then tiles * 5 * N * T_max * 8 bytes."""
    assert _pw.tile_draws(model, K, L) == cover
    N, T = 2, 5
    for D, tiles in ((cover, 1), (cover + 1, 2), (2 * cover + 1, 3)):
        data, draws = make(model, N, 1, T, K, L)
        draws = {k: np.repeat(v, D, axis=0) for k, v in draws.items()}
        pr, _res, _out = _pw.prepare(model, data, draws, "grid")
        ws = C.c_size_t(1)
        assert engine.hhmm_pointwise_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
        assert ws.value == (0 if tiles == 1 else tiles * 5 * N * T * 8), (D, ws.value)
    pr, _res, _out = _pw.prepare(model, data, {k: np.repeat(v[:1], 2 * (cover + 1), axis=0) for k, v in draws.items()},
                                 "block")
    assert engine.hhmm_pointwise_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == 2 * 5 * N * T * 8  # block: D = S / N = cover + 1


def test_waic_arithmetic():
    nan = np.nan
    stats = {"lpd_t": np.array([[-1.0, -2.0, -3.0, -4.0], [-1.0, -1.5, nan, nan]]),
             "var_t": np.array([[0.5, 0.25, 0.4, 0.0], [0.41, 0.5, nan, nan]])}
    w = hhmm_amd.waic(stats, T=[4, 2])
    near = dict(rtol=1e-14, atol=0)
    assert np.allclose(w["elpd_waic"], [-11.15, -3.41], **near) and np.allclose(w["p_waic"], [1.15, 0.91], **near)
    assert np.array_equal(w["waic"], -2.0 * w["elpd_waic"])
    assert w["n_high_var"].tolist() == [1, 2]  # 0.4 itself does not count
    pw0, pw1 = np.array([-1.5, -2.25, -3.4, -4.0]), np.array([-1.41, -2.0])
    assert np.allclose(w["se"], [np.sqrt(4 * pw0.var(ddof=1)), np.sqrt(2 * pw1.var(ddof=1))], rtol=1e-15, atol=0)
    full = hhmm_amd.waic({k: v[:1] for k, v in stats.items()})  # no T: every step
    assert np.array_equal(full["elpd_waic"], w["elpd_waic"][:1]) and full["n_high_var"].tolist() == [1]
    one = hhmm_amd.waic({k: v[:1, :1] for k, v in stats.items()})
    assert one["elpd_waic"].tolist() == [-1.5] and np.isnan(one["se"][0])


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 9, 16])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_gpu_multinom_every_K_and_L(engine, K, L):
    data, draws = make("hmm-multinom", 3, 5, 2 * fb_chunk(K) + 1, K, L, seed=K * 100 + L)
    check(engine, "hmm-multinom", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_gpu_gauss_every_K(engine, K):
    data, draws = make("hmm", 3, 5, 2 * fb_chunk(K) + 1, K, seed=K)
    check(engine, "hmm", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 5, 3), ("hmm", 3, 0), ("hmm", 8, 0)])
@pytest.mark.parametrize("Tsel", ["1", "2", "C-1", "C", "C+1", "2C+1", "61"])
def test_gpu_chunk_edges_in_T(engine, model, K, L, Tsel):
    c = fb_chunk(K)
    T = {"1": 1, "2": 2, "C-1": c - 1, "C": c, "C+1": c + 1, "2C+1": 2 * c + 1, "61": 61}[Tsel]
    data, draws = make(model, 2, 3, T, K, L, seed=T)
    got, _want = check(engine, model, data, draws)
    assert np.allclose(got["lp_t"].sum(axis=1), got["loglik"], rtol=1e-9, atol=1e-9)


def _tile_case(D):
    """N = 2, T = 11, K = 4, L = 9 under D draws per series; made once per D."""
    data, draws = make("hmm-multinom", 2, D, 11, 4, 9, seed=D)
    return data, draws, pointwise_ref.pointwise("hmm-multinom", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 256, 257, 577])
def test_gpu_draw_tile_edges(engine, D):
    """The wave (64), the workgroup's coverage (tile_draws = 256 here) and one more, and three tiles (577)."""
    assert _pw.tile_draws("hmm-multinom", 4, 9) == 256
    data, draws, want = _tile_case(D)
    got = hhmm_amd.pointwise_predictive("hmm-multinom", data, draws, per_draw=True, lib=engine)
    w = worst(got, want)
    print(f"D = {D}: worst discrepancy {w:.2e}")
    assert w <= TOL
    if D == 1:
        assert np.isnan(got["var_t"]).all() and np.array_equal(got["lpd_t"], got["mean_t"])
    if D == 577:  # no atomics, a fixed merge order: the same bits again
        again = hhmm_amd.pointwise_predictive("hmm-multinom", data, draws, per_draw=True, lib=engine)
        for name, v in got.items():
            assert np.array_equal(again[name], v, equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("D", [129, 300])
def test_gpu_draw_tiles_of_a_two_wave_workgroup(engine, D):
    """K = 8, L = 16: two waves per workgroup (tile_draws = 128), C = 4; the Gaussian kernel past one tile."""
    assert _pw.tile_draws("hmm-multinom", 8, 16) == 128
    data, draws = make("hmm-multinom", 2, D, 9, 8, 16, seed=D)
    check(engine, "hmm-multinom", data, draws)
    data, draws = make("hmm", 2, D, 9, 5, seed=D)
    check(engine, "hmm", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("K,L,D", [(4, 23, 193), (8, 38, 65)])
def test_gpu_draw_tiles_of_the_three_and_one_wave_workgroups(engine, K, L, D):
    """The other LDS classes: three waves (tile_draws = 192) and one (64), each one draw past its tile."""
    assert _pw.tile_draws("hmm-multinom", K, L) == D - 1
    data, draws = make("hmm-multinom", 2, D, 9, K, L, seed=D)
    check(engine, "hmm-multinom", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 3, 5), ("hmm", 2, 0)])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 13, K, L, seed=N * S)
    got, _want = check(engine, model, data, draws, pairing)
    if pairing == "zip":
        assert np.isnan(got["var_t"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 6, 4), ("hmm", 3, 0)])
def test_gpu_ragged_lengths(engine, model, K, L):
    c, Tmax = fb_chunk(K), 19
    lens = np.array([1, 2, c, c + 1, Tmax], dtype=np.int32)
    N = lens.size
    data, draws = make(model, N, 3, Tmax, K, L, seed=7)
    for n in range(N):  # padding rows must not matter: garbage symbols / values
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    got, _want = check(engine, model, data, draws)
    for n in range(N):  # cells at t >= T[n] keep the NaN fill
        for name in REDUCED:
            assert np.isnan(got[name][n, lens[n]:]).all() and np.isfinite(got[name][n, :lens[n]]).all()
        assert np.isnan(got["lp_t"][3 * n:3 * n + 3, lens[n]:]).all()


@pytest.mark.gpu
def test_gpu_long_series_keeps_its_scale(engine):
    T = 3000
    data, draws = synth.hmm_multinom(N=2, S=2, T=T, K=4, L=9)
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert (got["loglik"] < -2000).all() and (got["loglik"] > -8000).all()  # exp(loglik) underflows fp64
    assert np.allclose(got["lp_t"].sum(axis=1), got["loglik"], rtol=1e-9, atol=0)


@pytest.mark.gpu
def test_gpu_structural_zeros_stay_finite(engine):
    data, draws = make("hmm-multinom", 3, 4, 21, 4, 9, seed=3)
    A = draws["A_ij"]
    A[:, 1, 2] = 0.0
    A[:, :, 3] = 0.0        # state 4 is never entered ...
    A /= A.sum(axis=2, keepdims=True)
    draws["p_1k"] = np.tile([0.5, 0.5, 0.0, 0.0], (4, 1))  # ... nor started in
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "lp_t") + REDUCED)


@pytest.mark.gpu
def test_gpu_impossible_symbol_is_minus_inf_then_nan_for_that_pair(engine):
    N, S, L, T = 3, 5, 9, 17
    data, draws = make("hmm-multinom", N, S, T, 4, L, seed=11)
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
    L = 9
    data, draws = make("hmm-multinom", 2, 3, 6, 4, L, seed=5)
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
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm", 3, 0)])
def test_gpu_nan_draw_is_nan_in_every_cell(engine, model, K, L):
    N, S = 3, 5
    data, draws = make(model, N, S, 20, K, L, seed=13)
    draws["A_ij"][1, 0, 1] = np.nan
    got, _want = check(engine, model, data, draws)
    hit = np.arange(N * S) % S == 1
    assert np.isnan(got["loglik"][hit]).all() and np.isfinite(got["loglik"][~hit]).all()
    assert np.isnan(got["lp_t"][hit][:, 1:]).all() and np.isfinite(got["lp_t"][~hit]).all()
    for name in REDUCED:  # the NaN enters with the first transition
        assert np.isnan(got[name][:, 1:]).all() and np.isfinite(got[name][:, 0]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,D", [("hmm-multinom", 4, 9, 70), ("hmm", 5, 0, 70), ("hmm-multinom", 4, 9, 300)])
def test_gpu_per_draw_output(engine, model, K, L, D):
    data, draws = make(model, 2, D, 2 * fb_chunk(K) + 3, K, L, seed=29)
    full = hhmm_amd.pointwise_predictive(model, data, draws, per_draw=True, lib=engine)
    lean = hhmm_amd.pointwise_predictive(model, data, draws, per_draw=False, lib=engine)
    assert "lp_t" not in lean
    for name, v in lean.items():  # the same kernel, the stores skipped
        assert np.array_equal(full[name], v, equal_nan=True), name
    for n in range(2):  # the reductions again, on the host, from lp_t
        host = dict(zip(REDUCED, pointwise_ref.reduce_draws(full["lp_t"][n * D:(n + 1) * D])))
        assert worst({k: full[k][n] for k in REDUCED}, host) <= TOL
    ua = hhmm_amd.gqs(model, data, draws, pars=["unalpha_tk"], lib=engine)["unalpha_tk"]
    tot = pointwise_ref.estep_ref._lse(ua, 2)  # log sum_k exp(unalpha_tk): [P, T]
    assert worst({"lp_t": full["lp_t"]}, {"lp_t": np.diff(tot, axis=1, prepend=0.0)}) <= TOL


def _device(engine, model, data, draws, pairing="grid"):
    from stats_devrun import _Device
    return _Device(engine, "pointwise", _pw.prepare(model, data, draws, pairing, per_draw=True))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,pairing,N,S", [("hmm-multinom", 4, 9, "grid", 5, 30), ("hmm", 5, 0, "block", 4, 72),
                                                   ("hmm-multinom", 4, 9, "grid", 2, 300)])
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
    N, S, L = 4, 20, 9
    data, draws = make("hmm-multinom", N, S, 15, 4, L, seed=19)
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
    data, draws = make("hmm", 3, 4, 9, 3, seed=23)
    data["T"] = np.array([9, 10, 0], dtype=np.int32)
    dv = _device(engine, "hmm", data, draws)
    assert dv.run() == 0
    got = dv.stats()
    assert got["pair_status"].tolist() == [0] * 4 + [_abi.PAIR_INVALID_DATA] * 8
    want = pointwise_ref.pointwise("hmm", dict(data, T=np.array([9, 9, 9])), draws)
    assert worst({k: got[k][:4] for k in ("loglik", "lp_t")}, {k: want[k][:4] for k in ("loglik", "lp_t")}) <= TOL
    assert worst({k: got[k][:1] for k in REDUCED}, {k: want[k][:1] for k in REDUCED}) <= TOL
