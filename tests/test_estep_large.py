"""Batched E-step at 8 < K <= 32 (include/hhmm_estep.h, hhmm_estep_large):
expected sufficient statistics per (series, draw) pair from the state-parallel
kernel (csrc/hhmm_estep_large.hip) against the numpy restatement of the
contract (tests/estep_ref.py, K-agnostic, pinned to the CPU oracle by
tests/test_estep_ref.py), to 1e-9 relative to max(1, |reference|) -- the
project's parity tolerance; NaN and infinities must coincide.

CPU: symbols, the argument checks (they come before the device check), the
workspace size and the routing of hhmm_amd.estep by K.  gpu: the host entry
(hhmm_estep_large) unless stated, and the device entry on torch's stream.

Shapes: a group of G = 16 lanes owns a pair up to K = 16 (four pairs per wave,
16 per 256-thread workgroup), G = 32 above (two and eight); the compile-time
state loops run 16, 24 or 32 entries, so K = 9, 16 | 17, 24 | 25, 32 are both
sides of every instance edge.  Checkpoints come every 8 steps and observations
in blocks of G steps, so T covers 1, 2, the chunk edges 7 8 9, the block edges
16 17 and 32 33, and 70 (a last chunk of 6 steps after a full block pair).
"""
import ctypes as C
import sys

import numpy as np
import pytest

import estep_ref
import hhmm_amd
from hhmm_amd import _abi, _stats

_estep = sys.modules["hhmm_amd.estep"]
TOL = 1e-9
ENTRIES = ("hhmm_estep_large", "hhmm_estep_large_device", "hhmm_estep_large_workspace_size")
KS = [9, 16, 17, 24, 25, 32]
TS = [1, 2, 7, 8, 9, 16, 17, 32, 33, 70]
# (pairing, N, S): P = 5 every time
PAIRINGS = [("grid", 1, 5), ("grid", 5, 1), ("zip", 5, 5), ("block", 5, 5)]
FAMILIES = [("hmm", 0), ("hmm-multinom", 2), ("hmm-multinom", 9)]


def make(model, N, S, T, K, L=0, seed=0):
    """Random parameters and series (no structure needed: any x has positive likelihood)."""
    g = np.random.Generator(np.random.Philox(key=7000 + seed))
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
    print(f"{model} K={data['K']} {pairing}: worst {w:.3e}")
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    return got, want


def rows(stats, keep):
    return {k: v[keep] for k, v in stats.items() if k not in ("pair_status", "status")}


def device_entry(engine, model, data, draws, pairing="grid"):
    pr, res, out = _estep.prepare(model, data, draws, pairing)
    return _stats.DeviceStats(engine, "estep_large", pr, res, {name: a.shape for name, a in out.items()})


def device_run(dv):
    import torch
    assert dv.run() == 0
    torch.cuda.synchronize()
    return dv.stats()


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ENTRIES:
        assert getattr(engine, name).restype is C.c_int
    assert callable(hhmm_amd.estep)


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
    "null_xi": ("hmm-multinom", 12, 9, _null("xi_ij"), _abi.ERR_INVALID_ARGUMENT, "xi_ij"),
    "null_c_kl": ("hmm-multinom", 12, 9, _null("c_kl"), _abi.ERR_INVALID_ARGUMENT, "c_kl"),
    "null_w_k": ("hmm", 12, 0, _null("w_k"), _abi.ERR_INVALID_ARGUMENT, "w_k"),
    "device_set": ("hmm-multinom", 12, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    # two [L][G] tables and two slots of one group against 160 KiB: L <= 639 at G = 16, L <= 319 at G = 32
    "lds_G16": ("hmm-multinom", 12, 640, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "L = 640"),
    "lds_G32": ("hmm-multinom", 25, 320, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "L = 320"),
    "abi": ("hmm", 12, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_estep_large(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_estep_large_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)
    if case.startswith("K8"):
        assert "hhmm_estep " in msg, msg


@pytest.mark.parametrize("entry", ["host", "device"])
def test_null_request_is_an_invalid_argument(engine, entry):
    res = _abi.EstepResult()
    if entry == "host":
        st = engine.hhmm_estep_large(None, C.byref(res))
    else:
        st = engine.hhmm_estep_large_device(None, C.byref(res), None, 0, None)
    assert st == _abi.ERR_INVALID_ARGUMENT and "request" in engine.hhmm_last_error().decode()


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 12, 639), ("hmm-multinom", 25, 319), ("hmm", 32, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  The largest L of either group size."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    st = engine.hhmm_estep_large(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()


@pytest.mark.parametrize("K,Tmax,P", [(9, 1, 1), (23, 70, 5), (32, 1000, 3)])
def test_workspace_is_the_checkpoints(engine, K, Tmax, P):
    data, draws = make("hmm-multinom", P, P, Tmax, K, 3)
    pr, _res, _out = _estep.prepare("hmm-multinom", data, draws, "zip")
    ws = C.c_size_t(0)
    assert engine.hhmm_estep_large_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-Tmax // 8) * K * P * 8


def test_workspace_size_rejects_the_lane_kernels_K(engine):
    data, draws = make("hmm-multinom", 2, 2, 5, 8, 3)
    pr, _res, _out = _estep.prepare("hmm-multinom", data, draws, "zip")
    ws = C.c_size_t(0)
    assert engine.hhmm_estep_large_workspace_size(C.byref(pr.req), C.byref(ws)) == _abi.ERR_UNSUPPORTED
    assert "K = 8" in engine.hhmm_last_error().decode()


def test_python_shapes_and_routing_by_K(monkeypatch):
    data, draws = make("hmm-multinom", 3, 5, 6, 12, 9)
    pr, _res, out = _estep.prepare("hmm-multinom", data, draws, "grid")
    assert pr.P == 15 and pr.K == 12
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "n_1k": (15, 12), "xi_ij": (15, 12, 12),
                                                     "c_kl": (15, 12, 9)}
    gd, gw = make("hmm", 6, 6, 5, 12)
    _pr, _res, out = _estep.prepare("hmm", gd, gw, "zip")
    assert {k: v.shape for k, v in out.items()} == {"loglik": (6,), "n_1k": (6, 12), "xi_ij": (6, 12, 12),
                                                     "w_k": (6, 12), "s1_k": (6, 12), "s2_k": (6, 12)}
    assert [_estep.entry_name(K) for K in (1, 8, 9, 32, 33)] == ["estep", "estep", "estep_large", "estep_large",
                                                                  "estep_large"]
    called = []
    monkeypatch.setattr(_stats, "call", lambda lib, entry, pr, res, out, rs: called.append((entry, pr.K)) or out)
    for K in (8, 9):
        d, w = make("hmm-multinom", 2, 2, 5, K, 3)
        hhmm_amd.estep("hmm-multinom", d, w, lib=object())
    assert called == [("estep", 8), ("estep_large", 9)]


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("model,L", FAMILIES)
def test_gpu_parity(engine, model, L, K, T):
    for i, (pairing, N, S) in enumerate(PAIRINGS):
        data, draws = make(model, N, S, T, K, L, seed=1000 * K + 10 * T + i)
        got, _want = check(engine, model, data, draws, pairing)
        if T == 1:
            assert not got["xi_ij"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 23])
@pytest.mark.parametrize("model,L", [("hmm", 0), ("hmm-multinom", 9)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, L, K):
    lens = np.array([70, 1, 33, 8, 9], dtype=np.int32)
    data, draws = make(model, 5, 5, 70, K, L, seed=K)
    for n in range(5):  # padding must not matter: garbage symbols / values past T[n]
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    got = hhmm_amd.estep(model, data, draws, "zip", lib=engine, return_status=True)
    assert got["status"] == 0 and not got["pair_status"].any()
    for n in range(5):  # each pair against the reference run on its own truncated series
        own = dict(data, x=data["x"][n:n + 1, :lens[n]])
        del own["T"]
        want = estep_ref.estep(model, own, {k: v[n:n + 1] for k, v in draws.items()}, "zip")
        w = worst(rows(got, slice(n, n + 1)), want)
        print(f"{model} K={K} T={lens[n]}: worst {w:.3e}")
        assert w <= TOL, (n, w)


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", [(12, 17), (12, 21), (23, 9), (23, 11)])
@pytest.mark.parametrize("model,L", [("hmm", 0), ("hmm-multinom", 9)])
def test_gpu_past_one_workgroup_and_a_last_wave_with_one_group(engine, model, L, K, P):
    """256 threads hold 16 groups at K = 12 and 8 at K = 23: P = 17 / 9 start a second workgroup with one live
    group; P = 21 / 11 leave its second wave with one.  (hmm-multinom at 17 <= K <= 24 keeps xi in LDS and may
    launch smaller workgroups, of two groups at L = 9: every P here then ends on a wave with one live group.)"""
    data, draws = make(model, P, P, 19, K, L, seed=P)
    check(engine, model, data, draws, "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("K,L", [(12, 639), (12, 300), (25, 319), (23, 150)])
def test_gpu_tables_that_shrink_the_workgroup(engine, K, L):
    """The largest L of either group size (one group per workgroup, its two tables and slots 160 KiB) and an L
    between (two groups, half a wave, at K = 12, L = 300; one at K = 23, L = 150 with its xi rows in LDS)."""
    data, draws = make("hmm-multinom", 3, 3, 19, K, L, seed=L)
    check(engine, "hmm-multinom", data, draws, "zip")


@pytest.mark.gpu
def test_gpu_structural_zeros_stay_exact(engine):
    K = 12
    data, draws = make("hmm-multinom", 3, 4, 41, K, 9, seed=3)
    band = np.abs(np.subtract.outer(np.arange(K), np.arange(K))) <= 2
    draws["A_ij"] = draws["A_ij"] * band
    draws["A_ij"] /= draws["A_ij"].sum(axis=2, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "n_1k", "xi_ij", "c_kl"))
    assert (got["xi_ij"][:, ~band] == 0.0).all()
    assert (got["xi_ij"][:, band] > 0.0).all()


@pytest.mark.gpu
def test_gpu_dense_cadence_for_a_tiny_symbol(engine):
    """phi = 1e-200 under every state of draw 1 breaks the bound of the eight-step renormalisation: the waves that
    hold its pairs renormalise every step."""
    N, S, K, L = 2, 4, 12, 9
    data, draws = make("hmm-multinom", N, S, 40, K, L, seed=5)
    x = data["x"]
    x[x == L] = 1
    x[:, [3, 4, 20, 39]] = L
    clean, _want = check(engine, "hmm-multinom", data, draws)
    draws["phi_k"][1, :, L - 1] = 1e-200
    got, want = check(engine, "hmm-multinom", data, draws)
    hit = np.arange(N * S) % S == 1
    assert (got["loglik"][hit] < -4 * 200 * np.log(10)).all() and np.isfinite(want["loglik"]).all()
    w = worst(rows(got, ~hit), rows(clean, ~hit))  # the other pairs: what they were without it
    assert w <= TOL, w


@pytest.mark.gpu
def test_gpu_impossible_observation_is_nan_for_that_pair_only(engine):
    N, S, K, L = 3, 5, 12, 9
    data, draws = make("hmm-multinom", N, S, 27, K, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws)
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf and not got["pair_status"].any()
    for name in ("n_1k", "xi_ij", "c_kl"):
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
def test_gpu_device_entry_flags_invalid_data(engine):
    N, S, K, L, T = 5, 3, 12, 9, 21
    data, draws = make("hmm-multinom", N, S, T, K, L, seed=19)
    want = estep_ref.estep("hmm-multinom", data, draws)
    data["x"][1, 6] = 0
    data["x"][2, 17] = L + 1
    data["T"] = np.array([T, T, T, T, T + 1], dtype=np.int32)
    got = device_run(device_entry(engine, "hmm-multinom", data, draws))
    hit = np.isin(np.arange(N * S) // S, [1, 2, 4])
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    w = worst(rows(got, ~hit), rows(want, ~hit))
    assert w <= TOL, w


@pytest.mark.gpu
@pytest.mark.parametrize("model,L", [("hmm", 0), ("hmm-multinom", 9)])
def test_gpu_identities(engine, model, L):
    K, T = 23, 37
    data, draws = make(model, 2, 3, T, K, L, seed=23)
    got, _want = check(engine, model, data, draws)
    assert np.abs(got["n_1k"].sum(axis=1) - 1.0).max() <= 1e-9
    assert np.abs(got["xi_ij"].sum(axis=(1, 2)) - (T - 1)).max() <= 1e-9 * T
    if model == "hmm-multinom":
        assert np.abs(got["c_kl"].sum(axis=(1, 2)) - T).max() <= 1e-9 * T
    else:
        assert np.abs(got["w_k"].sum(axis=1) - (K + T - 1)).max() <= 1e-9 * (K + T)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,pairing,N,S", [("hmm-multinom", 23, 9, "grid", 5, 6), ("hmm", 12, 0, "block", 4, 24),
                                                   ("hmm-multinom", 32, 2, "zip", 5, 5)])
def test_gpu_device_entry_is_the_host_entry_and_repeats_its_bits(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 23, K, L, seed=17)
    data["T"] = np.array([23, 1, 9, 17, 8][:N], dtype=np.int32)
    host = hhmm_amd.estep(model, data, draws, pairing, lib=engine)
    dv = device_entry(engine, model, data, draws, pairing)
    first = device_run(dv)
    second = device_run(dv)
    assert not first["pair_status"].any()
    for name, v in host.items():
        assert np.array_equal(first[name], v, equal_nan=True), name
        assert np.array_equal(second[name], first[name], equal_nan=True), name
    again = hhmm_amd.estep(model, data, draws, pairing, lib=engine)
    for name, v in host.items():
        assert np.array_equal(again[name], v, equal_nan=True), name
