"""IOHMM E-step (include/hhmm_estep_io.h): expected sufficient statistics and
the transition-weight gradient per (series, draw) pair against the numpy
restatement of the contract (tests/estep_io_ref.py, pinned to the CPU oracle by
tests/test_estep_io_ref.py), to 1e-9 relative to max(1, |reference|) -- the
project's parity tolerance -- with NaN and infinities in the same places.

CPU: symbols, struct layout, Python shape checks, the argument checks (they
come before the device check, so they answer INVALID_ARGUMENT / UNSUPPORTED
with no GPU) and the M-step's arithmetic.  gpu: the host entry (hhmm_estep_io)
unless stated, and the device entry (hhmm_estep_io_device on torch's stream).

Shapes: M <= 4 and M > 4 are the kernel's two input classes (an odd M pads its
class), K * MMAX > 32 moves gw from registers into the LDS slab (reg K = 5 at
M = 5, 8; mix (5, 2, 5)), T = 1 has no transition and T = 2 exactly one, P
covers the partial last wave; T = 3000 is the long series of the sibling
entries' files.  Batches past one workgroup: tests/test_stats_geometry.py.
"""
import ctypes as C
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import estep_io_ref
import hhmm_amd
from hhmm_amd import _abi

REPO = pathlib.Path(__file__).resolve().parent.parent
_eio = sys.modules["hhmm_amd.estep_io"]
TOL = 1e-9
MIX = ("iohmm-mix", "iohmm-hmix", "iohmm-hmix-lite")
REG_STATS = ("loglik", "n_1k", "gw_km", "n_k", "uu_kmm", "ux_km", "xx_k")
MIX_STATS = ("loglik", "n_1k", "gw_km", "n_kl", "sx_kl", "sxx_kl")


def make(model, N, S, T, K, M, L=0, seed=0):
    """Random parameters and series (no structure needed: any x has positive density)."""
    g = np.random.Generator(np.random.Philox(key=4000 + seed))
    data = {"K": K, "M": M, "x_t": g.normal(0.0, 2.0, size=(N, T)), "u_tm": g.normal(0.0, 1.0, size=(N, T, M))}
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "w_km": g.normal(0.0, 0.7, size=(S, K, M))}
    if model == "iohmm-reg":
        draws["b_km"] = g.normal(0.0, 1.0, size=(S, K, M))
        draws["s_k"] = np.exp(g.normal(0.0, 0.3, size=(S, K)))
    else:
        data["L"] = L
        draws["lambda_kl"] = g.dirichlet(np.full(L, 2.0), size=(S, K))
        draws["mu_kl"] = np.sort(g.normal(0.0, 2.0, size=(S, K, L)), axis=2)
        draws["s_kl"] = np.exp(g.normal(0.0, 0.3, size=(S, K, L)))
    return data, draws


def worst(got, want):
    """Largest |got - want| / max(1, |want|) over the statistics; NaN and infinities must coincide."""
    w = 0.0
    for name, ref in want.items():
        out = got[name]
        assert out.shape == ref.shape, (name, out.shape, ref.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(out), np.isnan(ref)), name
        assert np.array_equal(out[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), name
        if fin.any():
            w = max(w, float(np.max(np.abs(out[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))))
    return w


def check(engine, model, data, draws, pairing="grid"):
    got = hhmm_amd.estep_io(model, data, draws, pairing, lib=engine, return_status=True)
    want = estep_io_ref.estep(model, data, draws, pairing)
    assert set(want) == set(REG_STATS if model == "iohmm-reg" else MIX_STATS)
    w = worst(got, want)
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    if model == "iohmm-reg":
        assert np.array_equal(got["uu_kmm"], got["uu_kmm"].transpose(0, 1, 3, 2), equal_nan=True)
    return got, want


class DeviceEstepIo:
    """hhmm_estep_io_device on torch's stream, in the style of stats_devrun.py."""

    def __init__(self, lib, model, data, draws, pairing="grid"):
        from stats_devrun import _Device
        self._d = _Device(lib, "estep_io", _eio.prepare(model, data, draws, pairing))

    def run(self):
        return self._d.run()

    def stats(self):
        return self._d.stats()


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ("hhmm_estep_io", "hhmm_estep_io_device", "hhmm_estep_io_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    for name in ("estep_io", "score_io", "m_step_io", "em_io"):
        assert callable(getattr(hhmm_amd, name))


def test_struct_layout_matches_header(tmp_path):
    cls = _abi.EstepIoResult
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hhmm_estep_io.h"', "int main(void){",
           'printf("sizeof %zu\\n", sizeof(hhmm_estep_io_result));']
    for f, _ in cls._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(hhmm_estep_io_result, {f}));')
    src.append('printf("abi %u\\n", HHMM_ABI_VERSION);')
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
    assert lay["abi"] == _abi.ABI_VERSION == 2


def test_python_shape_checks():
    data, draws = make("iohmm-reg", 3, 5, 6, 4, 3)
    pr, _res, out = _eio.prepare("iohmm-reg", data, draws, "grid")
    assert pr.P == 15
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "n_1k": (15, 4), "gw_km": (15, 4, 3),
                                                     "n_k": (15, 4), "uu_kmm": (15, 4, 3, 3), "ux_km": (15, 4, 3),
                                                     "xx_k": (15, 4)}
    md, mw = make("iohmm-hmix", 6, 6, 5, 3, 2, 4)
    _pr, _res, out = _eio.prepare("iohmm-hmix", md, mw, "zip")
    assert {k: v.shape for k, v in out.items()} == {"loglik": (6,), "n_1k": (6, 3), "gw_km": (6, 3, 2),
                                                     "n_kl": (6, 3, 4), "sx_kl": (6, 3, 4), "sxx_kl": (6, 3, 4)}
    with pytest.raises(ValueError):
        _eio.prepare("hmm", data, draws)
    with pytest.raises(ValueError):
        _eio.prepare("iohmm-reg", data, draws, "zip")                            # N != S
    with pytest.raises(ValueError):
        _eio.prepare("iohmm-reg", data, draws, "block")                          # S % N
    with pytest.raises(ValueError):
        _eio.prepare("iohmm-reg", data, dict(draws, b_km=draws["b_km"][:, :, :2]))
    with pytest.raises(ValueError):
        _eio.prepare("iohmm-reg", dict(data, M=2), draws)                        # u_tm has 3 columns
    with pytest.raises(ValueError):
        _eio.prepare("iohmm-mix", md, {k: v for k, v in mw.items() if k != "s_kl"})
    with pytest.raises(ValueError):
        hhmm_amd.em_io("iohmm-reg", data, draws, 1, pairing="grid")
    with pytest.raises(ValueError):
        hhmm_amd.score_io("hmm", {}, {}, "grid", 1, 1)
    with pytest.raises(ValueError):
        hhmm_amd.m_step_io("hmm-multinom", {}, {}, {}, "zip")


def _poke(*changes):
    def f(pr, res):
        for field, value in changes:
            obj, name = (pr.req, field) if "." not in field else (getattr(pr.req, field.split(".")[0]),
                                                                   field.split(".")[1])
            setattr(obj, name, value)
    return f


def _null(field):
    def f(pr, res):
        setattr(res, field, None)
    return f


def _both(*fs):
    def f(pr, res):
        for g in fs:
            g(pr, res)
    return f


# name -> (model, K, M, L, change to the prepared request, expected status, word of the message)
BAD = {
    "abi": ("iohmm-reg", 3, 4, 0, _poke(("abi_version", 1)), _abi.ERR_INVALID_ARGUMENT, "abi"),
    "model_unknown": ("iohmm-reg", 3, 4, 0, _poke(("model", 10)), _abi.ERR_INVALID_ARGUMENT, "model id"),
    "model_hmm": ("iohmm-reg", 3, 4, 0, _poke(("model", 1)), _abi.ERR_UNSUPPORTED, "4..7"),
    "model_multinom": ("iohmm-mix", 3, 4, 2, _poke(("model", 2)), _abi.ERR_UNSUPPORTED, "4..7"),
    "model_tayal": ("iohmm-mix", 4, 4, 2, _poke(("model", 8)), _abi.ERR_UNSUPPORTED, "4..7"),
    "model_before_K": ("iohmm-reg", 3, 4, 0, _poke(("model", 1), ("data.K", 9)), _abi.ERR_UNSUPPORTED, "4..7"),
    "K9": ("iohmm-reg", 3, 4, 0, _poke(("data.K", 9)), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K9_mix": ("iohmm-hmix-lite", 3, 4, 2, _poke(("data.K", 9)), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K_before_device_set": ("iohmm-reg", 3, 4, 0, _poke(("data.K", 9), ("device", _abi.DEVICE_SET)),
                            _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": ("iohmm-mix", 3, 4, 2, _poke(("device", _abi.DEVICE_SET)), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "device_set_before_lds": ("iohmm-reg", 8, 8, 0, _poke(("device", _abi.DEVICE_SET)), _abi.ERR_UNSUPPORTED,
                              "DEVICE_SET"),
    "M9": ("iohmm-reg", 3, 4, 0, _poke(("data.M", 9)), _abi.ERR_UNSUPPORTED, "M = 9"),
    "L9": ("iohmm-mix", 3, 4, 2, _poke(("data.L", 9)), _abi.ERR_UNSUPPORTED, "L = 9"),
    "lds_reg_K8_M8": ("iohmm-reg", 8, 8, 0, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_reg_K6_M5": ("iohmm-reg", 6, 5, 0, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_mix_K8_L6": ("iohmm-mix", 8, 4, 6, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_mix_K5_L8_M8": ("iohmm-hmix", 5, 8, 8, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_before_null": ("iohmm-reg", 8, 8, 0, _null("loglik"), _abi.ERR_UNSUPPORTED, "LDS"),
    "null_loglik": ("iohmm-reg", 3, 4, 0, _null("loglik"), _abi.ERR_INVALID_ARGUMENT, "loglik"),
    "null_gw": ("iohmm-mix", 3, 4, 2, _null("gw_km"), _abi.ERR_INVALID_ARGUMENT, "gw_km"),
    "null_uu": ("iohmm-reg", 3, 4, 0, _null("uu_kmm"), _abi.ERR_INVALID_ARGUMENT, "uu_kmm"),
    "null_sxx": ("iohmm-hmix", 3, 4, 2, _null("sxx_kl"), _abi.ERR_INVALID_ARGUMENT, "sxx_kl"),
    "null_draw": ("iohmm-reg", 3, 4, 0, _poke(("draws.w_km", None)), _abi.ERR_INVALID_ARGUMENT, "w_km"),
    "pairing": ("iohmm-reg", 3, 4, 0, _poke(("pairing", 7)), _abi.ERR_INVALID_ARGUMENT, "pairing"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, M, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, M, L)
    pr, res, _out = _eio.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_estep_io(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_estep_io_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_null_request_and_result(engine, entry):
    data, draws = make("iohmm-reg", 2, 2, 5, 3, 4)
    pr, res, _out = _eio.prepare("iohmm-reg", data, draws, "grid")
    for req, rs, word in ((None, C.byref(res), "request"), (C.byref(pr.req), None, "result")):
        if entry == "host":
            st = engine.hhmm_estep_io(req, rs)
        else:
            st = engine.hhmm_estep_io_device(req, rs, None, 0, None)
        assert st == _abi.ERR_INVALID_ARGUMENT and word in engine.hhmm_last_error().decode()


def test_host_entry_validates_the_data_block(engine):
    data, draws = make("iohmm-reg", 2, 2, 5, 3, 4)
    data["T"] = np.array([5, 6], dtype=np.int32)  # T[n] outside 1..T_max
    pr, res, _out = _eio.prepare("iohmm-reg", data, draws, "grid")
    assert engine.hhmm_estep_io(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "T[1]" in engine.hhmm_last_error().decode()


@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-reg", 8, 4, 0), ("iohmm-reg", 5, 8, 0),
                                         ("iohmm-mix", 8, 4, 5), ("iohmm-hmix", 4, 8, 8),
                                         ("iohmm-hmix-lite", 5, 5, 7)])
def test_good_request_passes_the_argument_checks(engine, model, K, M, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  The shapes are the largest of their classes."""
    data, draws = make(model, 2, 2, 5, K, M, L)
    pr, res, _out = _eio.prepare(model, data, draws, "grid")
    st = engine.hhmm_estep_io(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws = C.c_size_t(77)
    assert engine.hhmm_estep_io_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == 0  # one forward sweep: no checkpoints


def _one_pair_data(T=4, M=2):
    u = np.zeros((1, T, M))
    u[0, 1:, 0] = [1.0, 2.0, 3.0][:T - 1]
    u[0, 1:, 1] = 1.0
    return {"K": 2, "M": M, "x_t": np.zeros((1, T)), "u_tm": u}


def test_m_step_w_follows_boehnings_bound():
    data = _one_pair_data()
    u = data["u_tm"][0]
    su = u[1:].T @ u[1:]
    gw = np.array([[[0.5, -0.25], [-0.5, 0.25]]])
    stats = {"loglik": np.zeros(1), "n_1k": np.array([[0.25, 0.75]]), "gw_km": gw, "n_k": np.array([[1.0, 3.0]]),
             "uu_kmm": np.tile(np.eye(2), (1, 2, 1, 1)), "ux_km": np.array([[[1.0, 2.0], [3.0, 6.0]]]),
             "xx_k": np.array([[9.0, 60.0]])}
    prev = {"p_1k": np.array([[0.5, 0.5]]), "w_km": np.array([[[0.1, 0.2], [0.3, 0.4]]]),
            "b_km": np.zeros((1, 2, 2)), "s_k": np.ones((1, 2))}
    new = hhmm_amd.m_step_io("iohmm-reg", stats, prev, data, "zip")
    assert np.array_equal(new["p_1k"], stats["n_1k"])
    want_w = prev["w_km"][0] + 2.0 * (np.linalg.pinv(su) @ gw[0].T).T
    assert np.allclose(new["w_km"][0], want_w, rtol=1e-13, atol=0)
    assert np.allclose(new["w_km"].sum(axis=1), prev["w_km"].sum(axis=1), rtol=1e-13)  # the common shift stays
    # b = pinv(I) ux; RSS = xx - |ux|^2: (9 - 5) / 1 and (60 - 45) / 3
    assert np.allclose(new["b_km"], stats["ux_km"], rtol=1e-13)
    assert np.allclose(new["s_k"], [[2.0, np.sqrt(5.0)]], rtol=1e-13)


def test_m_step_reg_zero_count_keeps_prev_and_floor_applies():
    data = _one_pair_data()
    stats = {"loglik": np.zeros(1), "n_1k": np.array([[1.0, 0.0]]), "gw_km": np.zeros((1, 2, 2)),
             "n_k": np.array([[4.0, 0.0]]), "uu_kmm": np.stack([np.eye(2), np.zeros((2, 2))])[None],
             "ux_km": np.array([[[1.0, 2.0], [0.0, 0.0]]]), "xx_k": np.array([[5.0, 0.0]])}
    prev = {"p_1k": np.array([[0.5, 0.5]]), "w_km": np.zeros((1, 2, 2)), "b_km": np.full((1, 2, 2), 7.0),
            "s_k": np.array([[3.0, 4.0]])}
    new = hhmm_amd.m_step_io("iohmm-reg", stats, prev, data, "zip")
    assert new["b_km"].tolist() == [[[1.0, 2.0], [7.0, 7.0]]]
    assert new["s_k"][0, 1] == 4.0 and abs(new["s_k"][0, 0] - 1e-4) < 1e-18  # n = 0: prev; RSS = 0: the floor
    assert np.array_equal(new["w_km"], prev["w_km"])     # gw = 0
    new = hhmm_amd.m_step_io("iohmm-reg", stats, prev, data, "zip", s_min=0.5)
    assert new["s_k"].tolist() == [[0.5, 4.0]]


def test_m_step_mix_sorts_components_and_keeps_empty_ones():
    data = dict(_one_pair_data(), L=3)
    n = np.array([[[2.0, 0.0, 6.0], [0.0, 0.0, 0.0]]])
    stats = {"loglik": np.zeros(1), "n_1k": np.array([[1.0, 0.0]]), "gw_km": np.zeros((1, 2, 2)), "n_kl": n,
             "sx_kl": np.array([[[8.0, 0.0, 6.0], [0.0, 0.0, 0.0]]]),
             "sxx_kl": np.array([[[40.0, 0.0, 6.0], [0.0, 0.0, 0.0]]])}
    prev = {"p_1k": np.array([[0.5, 0.5]]), "w_km": np.zeros((1, 2, 2)),
            "lambda_kl": np.array([[[0.2, 0.3, 0.5], [0.1, 0.2, 0.7]]]),
            "mu_kl": np.array([[[0.0, 2.5, 9.0], [1.0, 2.0, 3.0]]]), "s_kl": np.array([[[1.0, 1.5, 2.0], [4.0, 5.0, 6.0]]])}
    new = hhmm_amd.m_step_io("iohmm-mix", stats, prev, data, "zip")
    # state 0: mu = (4, prev 2.5, 1) -> sorted (1, 2.5, 4); s = (2, prev 1.5, floor); lambda = (.25, 0, .75)
    assert new["mu_kl"][0, 0].tolist() == [1.0, 2.5, 4.0]
    assert new["lambda_kl"][0, 0].tolist() == [0.75, 0.0, 0.25]
    assert new["s_kl"][0, 0, 1:].tolist() == [1.5, 2.0] and abs(new["s_kl"][0, 0, 0] - 1e-4) < 1e-18
    # state 1 saw nothing: everything as before
    for name in ("lambda_kl", "mu_kl", "s_kl"):
        assert new[name][0, 1].tolist() == prev[name][0, 1].tolist()


def test_m_step_nan_pair_gets_nan_parameters():
    data = _one_pair_data()
    nan = np.full
    stats = {"loglik": np.array([-np.inf]), "n_1k": nan((1, 2), np.nan), "gw_km": nan((1, 2, 2), np.nan),
             "n_k": nan((1, 2), np.nan), "uu_kmm": nan((1, 2, 2, 2), np.nan), "ux_km": nan((1, 2, 2), np.nan),
             "xx_k": nan((1, 2), np.nan)}
    prev = {"p_1k": np.array([[0.5, 0.5]]), "w_km": np.zeros((1, 2, 2)), "b_km": np.zeros((1, 2, 2)),
            "s_k": np.ones((1, 2))}
    new = hhmm_amd.m_step_io("iohmm-reg", stats, prev, data, "zip")
    assert all(np.isnan(v).all() for v in new.values())


# ---------------------------------------------------------------- GPU

# every K and M inside the LDS fit BAD pins (M > 4 needs K <= 5); M = 3, 6 and 7 pad their MMAX class, K = 6 and 7
# at M <= 4 are the 3- and 2-wave classes
REG_SHAPES = [(K, M) for K in range(1, 9) for M in range(1, 9) if M <= 4 or K <= 5]
MIX_SHAPES = [(1, 1, 1), (2, 3, 4), (4, 3, 4), (5, 2, 5), (8, 3, 4), (4, 8, 8),
              (3, 2, 3), (6, 2, 3), (7, 2, 4), (2, 3, 6), (3, 2, 7), (4, 8, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,M", REG_SHAPES)
def test_gpu_reg_every_K_and_M(engine, K, M):
    data, draws = make("iohmm-reg", 3, 5, 5, K, M, seed=K * 10 + M)
    check(engine, "iohmm-reg", data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MIX)
@pytest.mark.parametrize("K,L,M", MIX_SHAPES)
def test_gpu_mix_every_shape_and_model_id(engine, model, K, L, M):
    data, draws = make(model, 3, 5, 5, K, M, L, seed=K * 100 + L * 10 + M)
    check(engine, model, data, draws)


@pytest.mark.gpu
def test_gpu_reg_K8_M8_matches_or_is_rejected_for_lds(engine):
    data, draws = make("iohmm-reg", 3, 5, 5, 8, 8, seed=88)
    try:
        check(engine, "iohmm-reg", data, draws)
    except hhmm_amd.HHMMError as e:
        assert e.status == _abi.ERR_UNSUPPORTED and "LDS" in str(e)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-reg", 5, 5, 0), ("iohmm-mix", 4, 4, 3),
                                         ("iohmm-hmix-lite", 5, 5, 2)])
@pytest.mark.parametrize("T", [1, 2, 3, 61])
def test_gpu_lengths(engine, model, K, M, L, T):
    data, draws = make(model, 2, 3, T, K, M, L, seed=T)
    got, _want = check(engine, model, data, draws)
    if T == 1:
        assert not got["gw_km"].any()
        if model == "iohmm-reg":
            assert np.array_equal(got["n_k"], got["n_1k"])
    assert np.allclose(got["n_1k"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.allclose(got["gw_km"].sum(axis=1), 0.0, rtol=0, atol=1e-9)
    count = got["n_k"].sum(axis=1) if model == "iohmm-reg" else got["n_kl"].sum(axis=(1, 2))
    assert np.allclose(count, T, rtol=1e-12, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-hmix", 3, 3, 2)])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_gpu_partial_last_wave(engine, model, K, M, L, P):
    data, draws = make(model, P, P, 7, K, M, L, seed=P)
    check(engine, model, data, draws, "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 2, 3, 0), ("iohmm-mix", 3, 4, 2)])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, model, K, M, L, pairing, N, S):
    data, draws = make(model, N, S, 9, K, M, L, seed=N * S)
    check(engine, model, data, draws, pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 4, 4, 0), ("iohmm-reg", 5, 8, 0), ("iohmm-hmix", 3, 4, 3)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, K, M, L):
    Tmax = 13
    lens = np.array([1, 2, 3, 8, Tmax] * 4, dtype=np.int32)
    N = lens.size
    data, draws = make(model, N, 3, Tmax, K, M, L, seed=7)
    for n in range(N):  # padding must not matter: garbage values, NaN inputs
        data["x_t"][n, lens[n]:] = 1e300
        data["u_tm"][n, lens[n]:] = np.nan
    data["T"] = lens
    got, _want = check(engine, model, data, draws)
    assert all(np.isfinite(got[k]).all() for k in got if k not in ("status", "pair_status"))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-mix", 3, 3, 2)])
def test_gpu_long_series_keeps_its_scale(engine, model, K, M, L):
    """T = 3000: exp(loglik) underflows fp64 (log of the smallest subnormal is -744.4).  Every step is in log
    space on its own and the sums have 3000 terms of order one, so the parity tolerance holds as it stands."""
    T = 3000
    data, draws = make(model, 2, 2, T, K, M, L, seed=30)
    got, _want = check(engine, model, data, draws)
    assert (got["loglik"] < -745.0).all() and np.isfinite(got["loglik"]).all()
    count = got["n_k"].sum(axis=1) if model == "iohmm-reg" else got["n_kl"].sum(axis=(1, 2))
    assert np.max(np.abs(count - T)) <= TOL * T
    assert np.allclose(got["gw_km"].sum(axis=1), 0.0, rtol=0, atol=TOL * T)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-mix", 3, 4, 2)])
def test_gpu_outlier_step_keeps_a_finite_loglik(engine, model, K, M, L):
    """|x - mean| / s is about 60 for every state: each density underflows in linear space."""
    data, draws = make(model, 2, 4, 12, K, M, L, seed=60)
    if model == "iohmm-reg":
        draws["s_k"][:] = 1.0
        draws["b_km"] *= 0.1
    else:
        draws["s_kl"][:] = 1.0
        draws["mu_kl"] *= 0.1
    data["x_t"][1, 5] = 60.0
    got, _want = check(engine, model, data, draws)
    assert np.isfinite(got["loglik"]).all() and (got["loglik"][4:] < -1500).all()
    assert all(np.isfinite(got[k]).all() for k in got if k not in ("status", "pair_status"))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 4, 4, 0), ("iohmm-hmix", 4, 4, 2)])
def test_gpu_zero_initial_probabilities_stay_exact(engine, model, K, M, L):
    data, draws = make(model, 3, 4, 9, K, M, L, seed=3)
    draws["p_1k"] = np.tile([0.5, 0.0, 0.5, 0.0], (4, 1))
    got, _want = check(engine, model, data, draws)
    assert not got["n_1k"][:, [1, 3]].any() and (got["n_1k"][:, [0, 2]] > 0).all()
    assert np.isfinite(got["loglik"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L,name", [("iohmm-reg", 3, 4, 0, "w_km"), ("iohmm-reg", 3, 4, 0, "s_k"),
                                              ("iohmm-mix", 3, 4, 2, "mu_kl")])
def test_gpu_nan_draw_is_nan_for_its_pairs_only(engine, model, K, M, L, name):
    N, S = 3, 5
    data, draws = make(model, N, S, 10, K, M, L, seed=13)
    draws[name][(1, 0) + (1,) * (draws[name].ndim - 2)] = np.nan
    got, _want = check(engine, model, data, draws)
    hit = np.arange(N * S) % S == 1
    for key, v in got.items():
        if key in ("pair_status", "status"):
            continue
        assert np.isnan(v[hit]).all() and np.isfinite(v[~hit]).all(), key


@pytest.mark.gpu
def test_gpu_nonpositive_scale_is_nan(engine):
    data, draws = make("iohmm-reg", 2, 3, 6, 3, 4, seed=5)
    draws["s_k"][2, 1] = -1.0
    got, _want = check(engine, "iohmm-reg", data, draws)
    assert np.isnan(got["loglik"][[2, 5]]).all() and np.isfinite(got["loglik"][[0, 1, 3, 4]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L,pairing,N,S", [("iohmm-reg", 4, 4, 0, "grid", 5, 30),
                                                     ("iohmm-reg", 5, 8, 0, "block", 4, 72),
                                                     ("iohmm-hmix-lite", 4, 5, 3, "grid", 5, 30)])
def test_gpu_device_entry_is_the_host_entry(engine, model, K, M, L, pairing, N, S):
    data, draws = make(model, N, S, 17, K, M, L, seed=17)
    data["T"] = np.array([17, 1, 9, 16, 8][:N], dtype=np.int32)
    host = hhmm_amd.estep_io(model, data, draws, pairing, lib=engine)
    dv = DeviceEstepIo(engine, model, data, draws, pairing)
    assert dv.run() == 0
    got = dv.stats()
    assert not got["pair_status"].any()
    for name, v in host.items():
        assert np.array_equal(got[name], v, equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-mix", 3, 4, 2)])
def test_gpu_device_entry_flags_a_length_outside_the_data_block(engine, model, K, M, L):
    data, draws = make(model, 3, 4, 9, K, M, L, seed=23)
    clean = DeviceEstepIo(engine, model, dict(data, T=np.array([9, 9, 9], dtype=np.int32)), draws)
    assert clean.run() == 0
    want = clean.stats()
    dv = DeviceEstepIo(engine, model, dict(data, T=np.array([9, 10, 0], dtype=np.int32)), draws)
    assert dv.run() == 0
    got = dv.stats()
    assert got["pair_status"].tolist() == [0] * 4 + [_abi.PAIR_INVALID_DATA] * 8
    for name in (REG_STATS if model == "iohmm-reg" else MIX_STATS):
        assert np.array_equal(got[name][:4], want[name][:4]), name
    ref = estep_io_ref.estep(model, data, draws)
    assert worst({k: v[:4] for k, v in got.items() if k != "pair_status"}, {k: v[:4] for k, v in ref.items()}) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,M,L", [("iohmm-reg", 3, 4, 0), ("iohmm-mix", 4, 4, 3), ("iohmm-hmix", 4, 4, 3),
                                         ("iohmm-hmix-lite", 5, 5, 2)])
def test_gpu_loglik_is_the_engines_own(engine, model, K, M, L):
    data, draws = make(model, 3, 4, 37, K, M, L, seed=31)
    st = hhmm_amd.estep_io(model, data, draws, lib=engine)
    ll = hhmm_amd.gqs(model, data, draws, pars=["loglik"], lib=engine)["loglik"]
    assert worst({"loglik": st["loglik"]}, {"loglik": ll}) <= TOL
