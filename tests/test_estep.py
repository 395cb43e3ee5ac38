"""Batched E-step (include/hhmm_estep.h): expected sufficient statistics per
(series, draw) pair against the numpy restatement of the contract
(tests/estep_ref.py, pinned to the CPU oracle by tests/test_estep_ref.py), to
1e-9 relative to max(1, |reference|) -- the project's parity tolerance.

CPU: symbols, struct layout, Python shape checks and the argument checks (they
come before the device check, so they answer INVALID_ARGUMENT / UNSUPPORTED
with no GPU).  gpu: the host entry (hhmm_estep) unless stated, and the device
entry (hhmm_estep_device on torch's stream).

Shapes: C = fb_chunk(K) is 8 at K <= 4 and 4 above; T covers the chunk edges,
P the partial last wave, K and L every template instance class and the odd /
even state pairs of the LDS tables.
"""
import ctypes as C
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import estep_ref
import hhmm_amd
from hhmm_amd import _abi, synth

REPO = pathlib.Path(__file__).resolve().parent.parent
_estep = sys.modules["hhmm_amd.estep"]
TOL = 1e-9
INT32_MIN = -2 ** 31


def fb_chunk(K):
    return 8 if K <= 4 else 4


def make(model, N, S, T, K, L=0, seed=0):
    """Random parameters and series (no structure needed: any x has positive likelihood)."""
    g = np.random.Generator(np.random.Philox(key=1000 + seed))
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K))}
    if model == "hmm-multinom":
        draws["phi_k"] = g.dirichlet(np.full(L, 2.0), size=(S, K))
        return {"K": K, "L": L, "x": g.integers(1, L + 1, size=(N, T)).astype(np.int32)}, draws
    draws["mu_k"] = np.sort(g.normal(0.0, 5.0, size=(S, K)), axis=1)
    draws["sigma_k"] = np.exp(g.normal(0.0, 0.3, size=(S, K))) * 2.0
    return {"K": K, "x": g.normal(0.0, 5.0, size=(N, T))}, draws


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
    got = hhmm_amd.estep(model, data, draws, pairing, lib=engine, return_status=True)
    want = estep_ref.estep(model, data, draws, pairing)
    w = worst(got, want)
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    return got, want


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ("hhmm_estep", "hhmm_estep_device", "hhmm_estep_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    for name in ("estep", "score", "m_step", "baum_welch"):
        assert callable(getattr(hhmm_amd, name))


def test_struct_layout_matches_header(tmp_path):
    cls = _abi.EstepResult
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hhmm_estep.h"', "int main(void){",
           'printf("sizeof %zu\\n", sizeof(hhmm_estep_result));']
    for f, _ in cls._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(hhmm_estep_result, {f}));')
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
    data, draws = make("hmm-multinom", 3, 5, 6, 4, 9)
    pr, _res, out = _estep.prepare("hmm-multinom", data, draws, "grid")
    assert pr.P == 15
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "n_1k": (15, 4), "xi_ij": (15, 4, 4),
                                                     "c_kl": (15, 4, 9)}
    gd, gw = make("hmm", 6, 6, 5, 3)
    _pr, _res, out = _estep.prepare("hmm", gd, gw, "zip")
    assert {k: v.shape for k, v in out.items()} == {"loglik": (6,), "n_1k": (6, 3), "xi_ij": (6, 3, 3), "w_k": (6, 3),
                                                     "s1_k": (6, 3), "s2_k": (6, 3)}
    with pytest.raises(ValueError):
        _estep.prepare("hhmm-tayal2009", data, draws)
    with pytest.raises(ValueError):
        _estep.prepare("hmm-multinom", data, draws, "zip")                       # N != S
    with pytest.raises(ValueError):
        _estep.prepare("hmm-multinom", data, draws, "block")                     # S % N
    with pytest.raises(ValueError):
        _estep.prepare("hmm-multinom", data, dict(draws, phi_k=draws["phi_k"][:, :, :8]))
    with pytest.raises(ValueError):
        _estep.prepare("hmm", gd, {k: v for k, v in gw.items() if k != "sigma_k"})
    with pytest.raises(ValueError):
        hhmm_amd.baum_welch("hmm", gd, gw, 1, pairing="grid")


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
    "lds": ("hmm-multinom", 8, 21, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_odd_K": ("hmm-multinom", 7, 21, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "LDS"),
    "null_xi": ("hmm-multinom", 4, 9, _null("xi_ij"), _abi.ERR_INVALID_ARGUMENT, "xi_ij"),
    "null_loglik": ("hmm", 3, 0, _null("loglik"), _abi.ERR_INVALID_ARGUMENT, "loglik"),
    "null_c_kl": ("hmm-multinom", 4, 9, _null("c_kl"), _abi.ERR_INVALID_ARGUMENT, "c_kl"),
    "null_s2_k": ("hmm", 3, 0, _null("s2_k"), _abi.ERR_INVALID_ARGUMENT, "s2_k"),
    "abi": ("hmm", 3, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_estep(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_estep_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_host_entry_rejects_symbols_outside_the_data_block(engine, bad):
    data, draws = make("hmm-multinom", 2, 2, 5, 4, 9)
    data["x"][1, 3] = bad
    pr, res, _out = _estep.prepare("hmm-multinom", data, draws, "grid")
    assert engine.hhmm_estep(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "x[1, 4]" in engine.hhmm_last_error().decode()
    data["x"][1, 3] = 1
    data["T"] = np.array([5, 6], dtype=np.int32)  # T[n] outside 1..T_max
    pr, res, _out = _estep.prepare("hmm-multinom", data, draws, "grid")
    assert engine.hhmm_estep(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 8, 20), ("hmm", 3, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  L * ceil(K / 2) = 80 is the largest table."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    st = engine.hhmm_estep(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws = C.c_size_t(0)
    assert engine.hhmm_estep_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-5 // fb_chunk(K)) * K * 4 * 8


def test_score_and_m_step_arithmetic():
    """0 / 0 -> 0 in the score; a zero row keeps its previous values in the M-step."""
    stats = {"loglik": np.zeros(1), "n_1k": np.array([[1.0, 0.0]]), "xi_ij": np.array([[[2.0, 0.0], [0.0, 0.0]]]),
             "c_kl": np.array([[[3.0, 1.0], [0.0, 0.0]]])}
    draws = {"p_1k": np.array([[1.0, 0.0]]), "A_ij": np.array([[[1.0, 0.0], [0.5, 0.5]]]),
             "phi_k": np.array([[[0.5, 0.5], [0.25, 0.75]]])}
    g = hhmm_amd.score("hmm-multinom", draws, stats, "zip", 1, 1)
    assert g["p_1k"].tolist() == [[1.0, 0.0]] and g["A_ij"].tolist() == [[[2.0, 0.0], [0.0, 0.0]]]
    assert g["phi_k"].tolist() == [[[6.0, 2.0], [0.0, 0.0]]]
    new = hhmm_amd.m_step("hmm-multinom", stats, draws)
    assert new["A_ij"].tolist() == [[[1.0, 0.0], [0.5, 0.5]]]
    assert new["phi_k"].tolist() == [[[0.75, 0.25], [0.25, 0.75]]]
    gs = {"loglik": np.zeros(1), "n_1k": np.array([[0.5, 0.5]]), "xi_ij": np.ones((1, 2, 2)),
          "w_k": np.array([[2.0, 4.0]]), "s1_k": np.array([[2.0, 8.0]]), "s2_k": np.array([[4.0, 16.0]])}
    new = hhmm_amd.m_step("hmm", gs)
    assert new["mu_k"].tolist() == [[1.0, 2.0]] and new["sigma_k"][0, 0] == 1.0
    assert new["sigma_k"][0, 1] == np.sqrt(1e-300)  # max(s2 / w - mu^2, tiny)


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
    if T == 1:
        assert not got["xi_ij"].any()
    assert np.allclose(got["xi_ij"].sum(axis=(1, 2)), T - 1, rtol=0, atol=1e-9 * max(1, T))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm", 5, 0)])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_gpu_partial_last_wave(engine, model, K, L, P):
    data, draws = make(model, P, P, 11, K, L, seed=P)
    check(engine, model, data, draws, "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 3, 5), ("hmm", 2, 0)])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 13, K, L, seed=N * S)
    check(engine, model, data, draws, pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 6, 4), ("hmm", 3, 0)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, K, L):
    c, Tmax = fb_chunk(K), 19
    lens = np.array([1, 2, c, c + 1, Tmax] * 4, dtype=np.int32)
    N = lens.size
    data, draws = make(model, N, 3, Tmax, K, L, seed=7)
    for n in range(N):  # padding rows must not matter: garbage symbols / values
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    check(engine, model, data, draws)


@pytest.mark.gpu
def test_gpu_long_series_keeps_its_scale(engine):
    T = 3000
    data, draws = synth.hmm_multinom(N=2, S=2, T=T, K=4, L=9)
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert (got["loglik"] < -2000).all() and (got["loglik"] > -8000).all()  # exp(loglik) underflows fp64
    assert np.allclose(got["xi_ij"].sum(axis=(1, 2)), T - 1, rtol=1e-9, atol=0)
    assert np.allclose(got["c_kl"].sum(axis=(1, 2)), T, rtol=1e-9, atol=0)


@pytest.mark.gpu
def test_gpu_structural_zeros_stay_exact(engine):
    data, draws = make("hmm-multinom", 3, 4, 21, 4, 9, seed=3)
    A = draws["A_ij"]
    A[:, 1, 2] = 0.0
    A[:, :, 3] = 0.0        # state 4 is never entered ...
    A /= A.sum(axis=2, keepdims=True)
    draws["p_1k"] = np.tile([0.5, 0.5, 0.0, 0.0], (4, 1))  # ... nor started in
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "n_1k", "xi_ij", "c_kl"))
    assert not got["xi_ij"][:, 1, 2].any() and not got["xi_ij"][:, :, 3].any() and not got["xi_ij"][:, 3, :].any()
    assert not got["n_1k"][:, 2:].any() and not got["c_kl"][:, 3, :].any()
    assert (got["xi_ij"][:, 0, :3] > 0).all()


@pytest.mark.gpu
def test_gpu_impossible_series_is_nan_for_that_pair_only(engine):
    N, S, L = 3, 5, 9
    data, draws = make("hmm-multinom", N, S, 17, 4, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf
    for name in ("n_1k", "xi_ij", "c_kl"):
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm", 3, 0)])
def test_gpu_nan_draw_is_nan_for_its_pairs_only(engine, model, K, L):
    N, S = 3, 5
    data, draws = make(model, N, S, 20, K, L, seed=13)
    draws["A_ij"][1, 0, 1] = np.nan
    got, _want = check(engine, model, data, draws)
    hit = np.arange(N * S) % S == 1
    for name, v in got.items():
        if name in ("pair_status", "status"):
            continue
        assert np.isnan(v[hit]).all() and np.isfinite(v[~hit]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,pairing,N,S", [("hmm-multinom", 4, 9, "grid", 5, 30), ("hmm", 5, 0, "block", 4, 72)])
def test_gpu_device_entry_is_the_host_entry(engine, model, K, L, pairing, N, S):
    from stats_devrun import DeviceEstep
    data, draws = make(model, N, S, 23, K, L, seed=17)
    data["T"] = np.array([23, 1, 9, 17, 8][:N], dtype=np.int32)
    host = hhmm_amd.estep(model, data, draws, pairing, lib=engine)
    dv = DeviceEstep(engine, model, data, draws, pairing)
    assert dv.run() == 0
    got = dv.stats()
    assert not got["pair_status"].any()
    for name, v in host.items():
        assert np.array_equal(got[name], v, equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_gpu_device_entry_flags_invalid_data(engine, bad):
    from stats_devrun import DeviceEstep
    N, S, L = 4, 20, 9
    data, draws = make("hmm-multinom", N, S, 15, 4, L, seed=19)
    clean = DeviceEstep(engine, "hmm-multinom", data, draws)
    assert clean.run() == 0
    want = clean.stats()
    data["x"][2, 6] = bad
    dv = DeviceEstep(engine, "hmm-multinom", data, draws)
    assert dv.run() == 0
    got = dv.stats()
    hit = np.arange(N * S) // S == 2
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in ("loglik", "n_1k", "xi_ij", "c_kl"):
        assert np.array_equal(got[name][~hit], want[name][~hit]), name


@pytest.mark.gpu
def test_gpu_device_entry_flags_a_length_outside_the_data_block(engine):
    from stats_devrun import DeviceEstep
    data, draws = make("hmm", 3, 4, 9, 3, seed=23)
    data["T"] = np.array([9, 10, 0], dtype=np.int32)
    dv = DeviceEstep(engine, "hmm", data, draws)
    assert dv.run() == 0
    got = dv.stats()
    assert got["pair_status"].tolist() == [0] * 4 + [_abi.PAIR_INVALID_DATA] * 8
    want = estep_ref.estep("hmm", dict(data, T=np.array([9, 9, 9])), draws)
    assert worst({k: v[:4] for k, v in got.items()}, {k: v[:4] for k, v in want.items()}) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("K,L", [(4, 9), (7, 5)])
def test_gpu_agrees_with_the_engines_gamma(engine, K, L):
    data, draws = synth.hmm_multinom(N=3, S=4, T=37, K=K, L=L)
    st = hhmm_amd.estep("hmm-multinom", data, draws, lib=engine)
    gam = hhmm_amd.gqs("hmm-multinom", data, draws, pars=["gamma_tk"], lib=engine)["gamma_tk"]
    x = np.asarray(data["x"])
    P = gam.shape[0]
    c = np.zeros((P, K, L))
    for p in range(P):
        for l in range(L):
            c[p, :, l] = gam[p, x[p // 4] == l + 1].sum(axis=0)
    assert worst({"c_kl": st["c_kl"], "n_1k": st["n_1k"]}, {"c_kl": c, "n_1k": gam[:, 0]}) <= TOL
    assert worst({"rows": st["xi_ij"].sum(axis=2), "cols": st["xi_ij"].sum(axis=1)},
                 {"rows": gam[:, :-1].sum(axis=1), "cols": gam[:, 1:].sum(axis=1)}) <= TOL
