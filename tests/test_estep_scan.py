"""The E-step as a parallel scan over T (include/hhmm_estep.h hhmm_estep_scan;
csrc/hhmm_estep_scan.hip): hmm and hmm-multinom at K <= 8 against the numpy
restatement of the contract (tests/estep_ref.py, pinned to the CPU oracle by
tests/test_estep_ref.py), to 1e-9 relative to max(1, |reference|) -- the
contract of include/hhmm_estep.h; NaN and infinities must coincide.

CPU: the symbols, the argument checks (before the device check), the plan
(hhmm_estep_scan_plan touches no device), the documented workspace, and the
routing of hhmm_amd.estep / baum_welch by `schedule`.  gpu: the host entry
unless stated.  Shapes: tests/estep_scan_cases.py.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import estep_ref
import hhmm_amd
from estep_scan_cases import (KS, PAIRINGS, TOL, auto_chunk, chunk_flags, device_run, edge_lengths, fb_chunk,
                              layout_bytes, plan_of, rerun, rows, shape_pr, shape_request, worst)
from hhmm_amd import _abi, _stats
from test_estep_large import BAD as LARGE_BAD
from test_estep_large import _null, _poke, make

_estep = sys.modules["hhmm_amd.estep"]
_em = sys.modules["hhmm_amd.em"]
ENTRIES = ("hhmm_estep_scan", "hhmm_estep_scan_device", "hhmm_estep_scan_workspace_size",
           "hhmm_expected_stats_scan", "hhmm_expected_stats_scan_device", "hhmm_expected_stats_scan_workspace_size")
FAMILIES = [("hmm", 0), ("hmm-multinom", 2), ("hmm-multinom", 9)]


def check(engine, model, data, draws, pairing, flags, schedule="scan"):
    got = hhmm_amd.estep(model, data, draws, pairing, lib=engine, return_status=True, schedule=schedule, flags=flags)
    want = estep_ref.estep(model, data, draws, pairing)
    w = worst(got, want)
    print(f"{model} K={data['K']} T={np.shape(data['x'])[-1]} {pairing}: worst {w:.3e}")
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    return got, want


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ENTRIES + ("hhmm_estep_scan_plan",):
        assert getattr(engine, name).restype is C.c_int


# the table of test_estep_large.py, adapted: name -> (model, K, L, change, expected status, word of the message)
BAD = {
    "K9": ("hmm-multinom", 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K9_gauss": ("hmm", 4, 0, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K33": ("hmm-multinom", 4, 9, _poke("data.K", 33), _abi.ERR_UNSUPPORTED, "K = 33"),
    "K33_gauss": ("hmm", 4, 0, _poke("data.K", 33), _abi.ERR_UNSUPPORTED, "K = 33"),
    "model_semisup": ("hmm-multinom", 4, 9, _poke("model", 3), _abi.ERR_UNSUPPORTED, "model"),
    "model_tayal": ("hmm-multinom", 4, 9, _poke("model", 8), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm": ("hmm", 4, 0, _poke("model", 4), _abi.ERR_UNSUPPORTED, "model"),
    "null_xi": ("hmm-multinom", 4, 9, _null("xi_ij"), _abi.ERR_INVALID_ARGUMENT, "xi_ij"),
    "null_c_kl": ("hmm-multinom", 4, 9, _null("c_kl"), _abi.ERR_INVALID_ARGUMENT, "c_kl"),
    "null_w_k": ("hmm", 4, 0, _null("w_k"), _abi.ERR_INVALID_ARGUMENT, "w_k"),
    "device_set": ("hmm-multinom", 4, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    # the emission table and its count table of one wave against 160 KiB: L * ceil(K / 2) <= 80
    "lds": ("hmm-multinom", 8, 21, lambda pr, res: None, _abi.ERR_UNSUPPORTED, "L * ceil(K / 2) = 21 * 4"),
    "abi": ("hmm", 4, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


def test_the_table_is_the_large_entrys_adapted():
    assert {k.replace("K8", "K9").replace("lds_G16", "lds") for k in LARGE_BAD if k != "lds_G32"} == set(BAD)


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_estep_scan(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_estep_scan_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)
    if case.startswith("K"):
        assert "hhmm_estep_large" in msg, msg


@pytest.mark.parametrize("entry", ["host", "device"])
def test_null_request_is_an_invalid_argument(engine, entry):
    res = _abi.EstepResult()
    if entry == "host":
        st = engine.hhmm_estep_scan(None, C.byref(res))
    else:
        st = engine.hhmm_estep_scan_device(None, C.byref(res), None, 0, None)
    assert st == _abi.ERR_INVALID_ARGUMENT and "request" in engine.hhmm_last_error().decode()


def test_scan_off_has_no_scan(engine):
    data, draws = make("hmm-multinom", 2, 2, 5, 4, 9)
    pr, res, _out = _estep.prepare("hmm-multinom", data, draws, "grid")
    pr.req.flags = _abi.FLAG_SCAN_OFF
    assert engine.hhmm_estep_scan(C.byref(pr.req), C.byref(res)) == _abi.ERR_UNSUPPORTED
    assert "SCAN_OFF" in engine.hhmm_last_error().decode()


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 8, 20), ("hmm-multinom", 1, 80), ("hmm", 8, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  The largest L of the LDS limit."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _estep.prepare(model, data, draws, "grid")
    st = engine.hhmm_estep_scan(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("log2", [1, 2, 3, 4, 5, 7])
def test_plan_rounds_the_forced_chunk_to_the_checkpoint_interval(engine, K, log2):
    Cc, Tmax = fb_chunk(K), 1003
    want = max(Cc, (1 << log2) - (1 << log2) % Cc)
    for flags in (_abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(log2), _abi.flag_scan_chunk_log2(log2)):
        forced = bool(flags & _abi.FLAG_SCAN_FORCE)
        assert plan_of(engine, "hmm-multinom", K, 9, 3, Tmax, flags) == ((want, -(-Tmax // want)) if forced else (0, 0))
    # the gate open without the force flag: the same chunks
    assert plan_of(engine, "hmm", K, 0, 3, 9000, _abi.flag_scan_chunk_log2(log2)) == (want, -(-9000 // want))


@pytest.mark.parametrize("P,Tmax,cl,nc", [(1, 10 ** 6, 32, 31250), (250, 10 ** 6, 1024, 977), (8, 8192, 32, 256)])
def test_plan_left_to_choose(engine, P, Tmax, cl, nc):
    assert auto_chunk(4, P, Tmax) == (cl, nc)  # the rule as csrc/hhmm_plan.h states it
    for model in ("hmm-multinom", "hhmm-tayal2009"):
        assert plan_of(engine, model, 4, 9, P, Tmax) == (cl, nc)
    assert P * nc <= 262144 and (cl == 32 or P * -(-Tmax // (cl // 2)) > 262144)


def test_plan_gate_and_scope(engine):
    for P, Tmax, on in [(5, 3000, False), (4096, 10 ** 5, False), (4095, 8192, True), (2, 8191, False), (2, 8192, True)]:
        assert (plan_of(engine, "hmm-multinom", 4, 9, P, Tmax)[0] > 0) == on, (P, Tmax)
    assert plan_of(engine, "hmm-multinom", 4, 9, 2, 8192, _abi.FLAG_SCAN_OFF) == (0, 0)
    assert plan_of(engine, "hmm-multinom", 9, 9, 2, 8192, _abi.FLAG_SCAN_FORCE) == (0, 0)     # K > 8: estep_large
    assert plan_of(engine, "hhmm-tayal2009-lite", 4, 9, 2, 8192, _abi.FLAG_SCAN_FORCE) == (0, 0)
    assert plan_of(engine, "iohmm-reg", 4, 0, 2, 8192, _abi.FLAG_SCAN_FORCE) == (0, 0)
    # 2^29 (pair, chunk) lanes, a pair's chunks rounded up to whole waves: 2^23 pairs x 64 lanes
    assert plan_of(engine, "hmm-multinom", 4, 9, 2 ** 23, 8, chunk_flags(4, 1)[0]) == (0, 0)
    assert plan_of(engine, "hmm-multinom", 4, 9, 2 ** 23 - 1, 8, chunk_flags(4, 1)[0]) == (8, 1)


@pytest.mark.parametrize("model,K,L,P,Tmax,mult", [("hmm-multinom", 4, 9, 5, 99, 1), ("hmm-multinom", 8, 3, 1, 1000, 4),
                                                   ("hmm", 7, 0, 3, 4099, 2), ("hmm-multinom", 1, 2, 65, 8, 1)])
def test_workspace_is_the_documented_layout(engine, model, K, L, P, Tmax, mult):
    flags, cl = chunk_flags(K, mult)
    ws = C.c_size_t(0)
    r = shape_request(model, K, L, P, Tmax, flags)
    assert engine.hhmm_estep_scan_workspace_size(C.byref(r), C.byref(ws)) == 0, engine.hhmm_last_error()
    assert plan_of(engine, model, K, L, P, Tmax, flags) == (cl, -(-Tmax // cl))
    assert ws.value == layout_bytes(K, L, P, cl, -(-Tmax // cl), gauss=model == "hmm")
    if model == "hmm-multinom":  # one launch path: the expected statistics take the same workspace
        ws2 = C.c_size_t(0)
        assert engine.hhmm_expected_stats_scan_workspace_size(C.byref(r), C.byref(ws2)) == 0
        assert ws2.value == ws.value


def test_workspace_left_to_choose_follows_the_plan(engine):
    ws = C.c_size_t(0)
    r = shape_request("hmm-multinom", 4, 9, 8, 8192)  # no force flag: the entry scans all the same
    assert engine.hhmm_estep_scan_workspace_size(C.byref(r), C.byref(ws)) == 0
    assert ws.value == layout_bytes(4, 9, 8, 32, 256)
    r = shape_request("hmm-multinom", 4, 9, 5, 100)   # under the automatic gate: still a scan, of 4 C steps
    assert engine.hhmm_estep_scan_workspace_size(C.byref(r), C.byref(ws)) == 0
    assert ws.value == layout_bytes(4, 9, 5, 32, 4)


def test_workspace_size_rejects_the_large_entrys_K(engine):
    ws = C.c_size_t(0)
    r = shape_request("hmm-multinom", 9, 3, 2, 5)
    assert engine.hhmm_estep_scan_workspace_size(C.byref(r), C.byref(ws)) == _abi.ERR_UNSUPPORTED
    msg = engine.hhmm_last_error().decode()
    assert "K = 9" in msg and "hhmm_estep_large" in msg


def test_python_routing_by_schedule(engine, monkeypatch):
    resolve = _estep.resolve_schedule
    assert resolve(shape_pr("hmm-multinom", 4, 9, 5, 3000), "auto", engine) == "lanes"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 4096, 10 ** 5), "auto", engine) == "lanes"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 2, 8192), "auto", engine) == "scan"
    assert resolve(shape_pr("hmm", 8, 0, 2, 8192), "auto", engine) == "scan"
    assert resolve(shape_pr("hmm", 9, 0, 2, 8192), "auto", engine) == "lanes"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 2, 8192, _abi.FLAG_SCAN_OFF), "auto", engine) == "lanes"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 5, 100, _abi.FLAG_SCAN_FORCE), "auto", engine) == "scan"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 5, 3000), "auto", lib=object()) == "lanes"  # no call into the library
    assert resolve(shape_pr("hmm-multinom", 4, 9, 2, 8192), "lanes", engine) == "lanes"
    assert resolve(shape_pr("hmm-multinom", 4, 9, 5, 10), "scan", engine) == "scan"
    with pytest.raises(ValueError, match="estep_large"):
        resolve(shape_pr("hmm-multinom", 9, 9, 5, 10), "scan", engine)
    with pytest.raises(ValueError, match="schedule"):
        resolve(shape_pr("hmm-multinom", 4, 9, 5, 10), "chunks", engine)
    assert [_estep.entry_name(K, s) for K, s in ((8, "lanes"), (9, "lanes"), (8, "scan"))] == ["estep", "estep_large",
                                                                                             "estep_scan"]
    called = []
    monkeypatch.setattr(_stats, "call", lambda lib, entry, pr, res, out, rs: called.append((entry, pr.req.flags)) or out)
    d, w = make("hmm-multinom", 2, 2, 5, 4, 3)
    flags, _cl = chunk_flags(4, 1)
    hhmm_amd.estep("hmm-multinom", d, w, lib=engine)
    hhmm_amd.estep("hmm-multinom", d, w, lib=engine, schedule="scan", flags=flags)
    hhmm_amd.estep("hmm-multinom", d, w, lib=engine, schedule="lanes", flags=flags)
    hhmm_amd.estep("hmm-multinom", d, w, lib=engine, flags=flags)  # "auto" under the force flag
    assert called == [("estep", 0), ("estep_scan", flags), ("estep", flags), ("estep_scan", flags)]
    d9, w9 = make("hmm-multinom", 2, 2, 5, 9, 3)
    with pytest.raises(ValueError, match="estep_large"):
        hhmm_amd.estep("hmm-multinom", d9, w9, lib=engine, schedule="scan")


def test_baum_welch_forwards_the_schedule(monkeypatch):
    seen = []

    def fake(model, data, params, pairing, device, lib, schedule="auto", flags=0):
        seen.append((schedule, flags))
        d, w = make("hmm-multinom", 2, 2, 5, 4, 3)
        return estep_ref.estep("hmm-multinom", d, w, "zip")

    monkeypatch.setattr(_em, "estep", fake)
    _d, w = make("hmm-multinom", 2, 2, 5, 4, 3)
    hhmm_amd.baum_welch("hmm-multinom", {}, w, 2, lib=object(), schedule="scan", flags=7)
    hhmm_amd.baum_welch("hmm-multinom", {}, w, 1, lib=object())
    assert seen == [("scan", 7), ("scan", 7), ("auto", 0)]


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("mult", [1, 4])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("model,L", FAMILIES)
def test_gpu_parity(engine, model, L, K, mult):
    flags, cl = chunk_flags(K, mult)
    for T in edge_lengths(cl):
        for i, (pairing, N, S) in enumerate(PAIRINGS):
            data, draws = make(model, N, S, T, K, L, seed=1000 * K + 10 * T + i)
            got, _want = check(engine, model, data, draws, pairing, flags)
            if T == 1:
                assert not got["xi_ij"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [64, 65, 257])
def test_gpu_boundary_walk_edges(engine, nc):
    """One block on wave 0, the four-wave ranges, and more than one block per wave; the last chunk is short."""
    flags, cl = chunk_flags(4, 1)
    T = nc * cl - 3
    data, draws = make("hmm-multinom", 1, 2, T, 4, 9, seed=nc)
    assert plan_of(engine, "hmm-multinom", 4, 9, 2, T, flags) == (cl, nc)
    check(engine, "hmm-multinom", data, draws, "grid", flags)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65])
@pytest.mark.parametrize("model,L,K", [("hmm-multinom", 9, 4), ("hmm", 0, 7)])
def test_gpu_pair_count_edges(engine, model, L, K, P):
    flags, cl = chunk_flags(K, 1)
    data, draws = make(model, P, P, 5 * cl, K, L, seed=P)
    check(engine, model, data, draws, "zip", flags)


@pytest.mark.gpu
@pytest.mark.parametrize("model,L,K,mult", [("hmm", 0, 7, 1), ("hmm-multinom", 9, 4, 1), ("hmm-multinom", 9, 5, 4)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, L, K, mult):
    flags, cl = chunk_flags(K, mult)
    lens = np.array([3 * cl + 3, 1, cl, cl + 1, 2], dtype=np.int32)
    data, draws = make(model, 5, 5, int(lens.max()), K, L, seed=K)
    for n in range(5):  # padding must not matter: garbage symbols / values past T[n]
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    got = hhmm_amd.estep(model, data, draws, "zip", lib=engine, return_status=True, schedule="scan", flags=flags)
    assert got["status"] == 0 and not got["pair_status"].any()
    for n in range(5):  # each pair against the reference run on its own truncated series
        own = dict(data, x=data["x"][n:n + 1, :lens[n]])
        del own["T"]
        want = estep_ref.estep(model, own, {k: v[n:n + 1] for k, v in draws.items()}, "zip")
        w = worst(rows(got, slice(n, n + 1)), want)
        print(f"{model} K={K} T={lens[n]}: worst {w:.3e}")
        assert w <= TOL, (n, w)
    assert not got["xi_ij"][1].any()  # T = 1: every chunk past the pair's end adds exact zeros


@pytest.mark.gpu
def test_gpu_structural_zeros_stay_exact(engine):
    K = 5
    flags, cl = chunk_flags(K, 1)
    data, draws = make("hmm-multinom", 3, 4, 3 * cl + 3, K, 9, seed=3)
    band = np.abs(np.subtract.outer(np.arange(K), np.arange(K))) <= 1
    draws["A_ij"] = draws["A_ij"] * band
    draws["A_ij"] /= draws["A_ij"].sum(axis=2, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws, "grid", flags)
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "n_1k", "xi_ij", "c_kl"))
    assert (got["xi_ij"][:, ~band] == 0.0).all()
    assert (got["xi_ij"][:, band] > 0.0).all()


@pytest.mark.gpu
def test_gpu_impossible_observation_in_a_middle_chunk_is_nan_for_that_pair_only(engine):
    N, S, K, L = 3, 5, 4, 9
    flags, cl = chunk_flags(K, 1)
    data, draws = make("hmm-multinom", N, S, 4 * cl + 3, K, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, cl + 2] = L                         # only series 1 shows symbol L, in its second chunk ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _want = check(engine, "hmm-multinom", data, draws, "grid", flags)
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf and not got["pair_status"].any()
    for name in ("n_1k", "xi_ij", "c_kl"):
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
def test_gpu_dense_cadence_for_a_tiny_symbol(engine):
    """phi = 1e-200 under every state of draw 1 breaks renorm_sparse_safe's bound: the phase-1 waves that hold
    its pairs renormalise their chunk products every step."""
    N, S, K, L = 2, 4, 4, 9
    flags, cl = chunk_flags(K, 4)
    data, draws = make("hmm-multinom", N, S, 2 * cl + 8, K, L, seed=5)
    x = data["x"]
    x[x == L] = 1
    x[:, [3, 4, 20, 39, cl + 1]] = L
    clean, _want = check(engine, "hmm-multinom", data, draws, "grid", flags)
    draws["phi_k"][1, :, L - 1] = 1e-200
    got, want = check(engine, "hmm-multinom", data, draws, "grid", flags)
    hit = np.arange(N * S) % S == 1
    assert (got["loglik"][hit] < -5 * 200 * np.log(10)).all() and np.isfinite(want["loglik"]).all()
    w = worst(rows(got, ~hit), rows(clean, ~hit))  # the other pairs: what they were without it
    assert w <= TOL, w


@pytest.mark.gpu
def test_gpu_device_entry_flags_invalid_data(engine):
    N, S, K, L = 5, 3, 4, 9
    flags, cl = chunk_flags(K, 1)
    T = 2 * cl + 5
    data, draws = make("hmm-multinom", N, S, T, K, L, seed=19)
    want = estep_ref.estep("hmm-multinom", data, draws)
    data["x"][1, 6] = 0
    data["x"][2, cl + 9] = L + 1
    data["T"] = np.array([T, T, T, T, T + 1], dtype=np.int32)
    pr, res, out = _estep.prepare("hmm-multinom", data, draws, "grid")
    _dv, got = device_run(engine, "estep_scan", pr, res, out, flags)
    hit = np.isin(np.arange(N * S) // S, [1, 2, 4])
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    w = worst(rows(got, ~hit), rows(want, ~hit))
    assert w <= TOL, w


@pytest.mark.gpu
@pytest.mark.parametrize("model,L,K", [("hmm", 0, 8), ("hmm-multinom", 9, 4)])
def test_gpu_identities(engine, model, L, K):
    flags, cl = chunk_flags(K, 1)
    T = 5 * cl + 2
    data, draws = make(model, 2, 3, T, K, L, seed=23)
    got, _want = check(engine, model, data, draws, "grid", flags)
    assert np.abs(got["n_1k"].sum(axis=1) - 1.0).max() <= 1e-9
    assert np.abs(got["xi_ij"].sum(axis=(1, 2)) - (T - 1)).max() <= 1e-9 * T
    if model == "hmm-multinom":
        assert np.abs(got["c_kl"].sum(axis=(1, 2)) - T).max() <= 1e-9 * T
    else:
        assert np.abs(got["w_k"].sum(axis=1) - (K + T - 1)).max() <= 1e-9 * (K + T)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L,pairing,N,S", [("hmm-multinom", 4, 9, "grid", 5, 6), ("hmm", 7, 0, "block", 4, 24),
                                                   ("hmm-multinom", 8, 2, "zip", 5, 5)])
def test_gpu_scan_agrees_with_the_lanes_and_both_entries_repeat_their_bits(engine, model, K, L, pairing, N, S):
    flags, cl = chunk_flags(K, 1)
    T = 3 * cl + 3
    data, draws = make(model, N, S, T, K, L, seed=17)
    data["T"] = np.array([T, 1, cl + 1, 2 * cl, cl][:N], dtype=np.int32)
    host = hhmm_amd.estep(model, data, draws, pairing, lib=engine, schedule="scan", flags=flags)
    lanes = hhmm_amd.estep(model, data, draws, pairing, lib=engine, schedule="lanes")
    w = worst(host, lanes)  # the same request on both schedules: the tolerance, not the bits (reassociated sums)
    assert w <= TOL, w
    pr, res, out = _estep.prepare(model, data, draws, pairing)
    dv, first = device_run(engine, "estep_scan", pr, res, out, flags)
    second = rerun(dv)
    assert not first["pair_status"].any()
    for name, v in host.items():
        assert np.array_equal(first[name], v, equal_nan=True), name
        assert np.array_equal(second[name], first[name], equal_nan=True), name
    again = hhmm_amd.estep(model, data, draws, pairing, lib=engine, schedule="scan", flags=flags)
    for name, v in host.items():
        assert np.array_equal(again[name], v, equal_nan=True), name


@pytest.fixture(scope="module")
def long_series():
    """One series of 8192 steps under two starts: the smallest request schedule="auto" sends to the scan."""
    data, draws = make("hmm-multinom", 1, 2, 8192, 4, 9, seed=29)
    return data, draws


@pytest.mark.gpu
def test_gpu_auto_takes_the_scan_from_8192_steps(engine, long_series, monkeypatch):
    data, draws = long_series
    called = []
    real = _stats.call
    monkeypatch.setattr(_stats, "call", lambda lib, entry, *a: called.append(entry) or real(lib, entry, *a))
    check(engine, "hmm-multinom", data, draws, "grid", 0, schedule="auto")
    assert called == ["estep_scan"]


@pytest.mark.gpu
def test_gpu_baum_welch_on_the_scan(engine, long_series):
    data, draws = long_series
    init = {k: np.array(v) for k, v in draws.items()}
    both = dict(data, x=np.repeat(data["x"], 2, axis=0))  # zip pairing: one start per (copy of the) series
    _p, scan = hhmm_amd.baum_welch("hmm-multinom", both, init, 3, lib=engine, schedule="scan")
    _p, lanes = hhmm_amd.baum_welch("hmm-multinom", both, init, 3, lib=engine, schedule="lanes")
    assert scan.shape == (3, 2) and np.isfinite(scan).all()
    assert (np.diff(scan, axis=0) >= -1e-9 * np.abs(scan[1:])).all(), scan
    assert np.max(np.abs(scan - lanes) / np.maximum(1.0, np.abs(lanes))) <= TOL
