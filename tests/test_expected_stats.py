"""Expected draw statistics (include/hhmm_expect.h, hhmm_amd/expect.py): the E-step of the masked programs.

CPU: the numpy reference (tests/expect_ref.py: masked forward, adjoint
backward) against the weighted mean of draw_stats_ref.counts over all K^T
paths; Fisher's identity (hhmm_amd.score on the reference's statistics against
central differences of the reference's loglik); symbols, the header as C, the
Python shape checks, the argument checks (they come before the device check)
and the Tayal M-step / score arithmetic.

gpu: the kernel against the reference, 1e-9 relative to max(1, |reference|)
with NaN and infinities coinciding, through the host and the device entry
(bit-equal to each other); hmm-multinom through the new entry against
hhmm_amd.estep, bit for bit; and the Rao-Blackwell link to the sampler: the
mean of hhmm_amd.draw_stats over many uniforms is hhmm_amd.expected_stats.

Shapes: C = fb_chunk(K) is 8 at K <= 4 and 4 above; T covers the chunk edges,
P the partial last wave, K and L every template instance class.
"""
import ctypes as C
import itertools
import math
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import draw_stats_ref as dsr
import expect_ref as xr
import hhmm_amd
from hhmm_amd import _abi, synth

REPO = pathlib.Path(__file__).resolve().parent.parent
_gibbs = sys.modules["hhmm_amd.gibbs"]
SEMISUP, TAYAL = "hmm-multinom-semisup", "hhmm-tayal2009"
MASKED = [SEMISUP, TAYAL]
STATS = ("n_1k", "xi_ij", "c_kl")
TOL = 1e-9
INT32_MIN = -2 ** 31


def fb_chunk(K):
    return 8 if K <= 4 else 4


def make(model, N, S, T, K, L, seed=0):
    """Random parameters and series."""
    g = np.random.Generator(np.random.Philox(key=3000 + seed))
    data = {"K": K, "L": L, "x": g.integers(1, L + 1, size=(N, T)).astype(np.int32)}
    if model == TAYAL:
        assert K == 4
        data["sign"] = g.integers(1, 3, size=(N, T)).astype(np.int32)
        draws = {"p_11": g.uniform(0.2, 0.8, size=S), "A_row": g.dirichlet(np.full(2, 2.0), size=(S, 2)),
                 "phi_k": g.dirichlet(np.full(L, 2.0), size=(S, K))}
        return data, draws
    if model == SEMISUP:
        data["g"] = g.integers(1, 4, size=(N, T)).astype(np.int32)
        data["G"] = 3
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K)),
             "phi_k": g.dirichlet(np.full(L, 2.0), size=(S, K))}
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


# ---------------------------------------------------------------- CPU: the reference

def enumerate_stats(model, K, L, x, aux, par):
    """The weighted mean of draw_stats_ref.counts under exp(log_weight) over all K^T paths."""
    p, A, phi = xr.expand(model, par)
    tot, n1, xi, c = 0.0, np.zeros(K), np.zeros((K, K)), np.zeros((K, L))
    for z in itertools.product(range(1, K + 1), repeat=len(x)):
        lw = dsr.log_weight(model, z, x, aux, p, A, phi)
        if lw == -math.inf:
            continue
        w = math.exp(lw)
        a, b, d = dsr.counts(model, K, L, z, x, aux)
        tot, n1, xi, c = tot + w, n1 + w * a, xi + w * b, c + w * d
    if tot == 0.0:
        nan = np.nan
        return {"loglik": -math.inf, "n_1k": n1 * nan, "xi_ij": xi * nan, "c_kl": c * nan}
    return {"loglik": math.log(tot), "n_1k": n1 / tot, "xi_ij": xi / tot, "c_kl": c / tot}


X5 = np.array([1, 3, 2, 2, 1], dtype=np.int32)
AUX5 = {SEMISUP: [np.array([1, 2, 3, 1, 2]), np.array([3, 1, 1, 2, 3])],
        TAYAL: [np.array([1, 2, 1, 1, 2]), np.array([2, 1, 2, 2, 1])]}


def _par(model, seed):
    _data, draws = make(model, 1, 1, 1, 4, 3, seed=seed)
    return {k: np.array(v[0]) for k, v in draws.items()}


ENUM = [(m, T, a, "random") for m in MASKED for T in (1, 2, 5) for a in (0, 1)] + \
       [(TAYAL, T, a, kind) for T in (1, 2, 5) for a in (0, 1) for kind in ("p11=0", "p11=1", "row0=(1,0)", "row1=(1,0)")]


@pytest.mark.parametrize("model,T,a,kind", ENUM)
def test_reference_is_the_weighted_mean_over_all_paths(model, T, a, kind):
    K, L = 4, 3
    par = _par(model, seed=T + 10 * a)
    if kind.startswith("p11"):
        par["p_11"] = np.float64(kind[-1])
    if kind.startswith("row"):
        par["A_row"][int(kind[3])] = (1.0, 0.0)
    x, aux = X5[:T], AUX5[model][a][:T]
    got = xr.series_stats(model, L, x, aux, par)
    want = enumerate_stats(model, K, L, x, aux, par)
    assert np.isfinite(want["loglik"]) and abs(got["loglik"] - want["loglik"]) <= 1e-12
    for name in STATS:
        assert np.max(np.abs(got[name] - want[name])) <= 1e-12, (name, got[name], want[name])
        assert not got[name][want[name] == 0].any(), name                        # exact zeros stay exact
    assert abs(got["c_kl"].sum() - T) <= 1e-12


def test_reference_on_a_series_whose_only_paths_cross_a_structural_zero():
    """States 1 and 4 never emit symbol 1, so x = (1, 1) keeps both steps in {2, 3}; under sign_2 = 1 the
    transition into 2 or 3 takes A, and A(2..3, 2..3) is structurally zero: no path has weight."""
    par = _par(TAYAL, seed=4)
    par["phi_k"][[0, 3], 0] = 0.0
    par["phi_k"] /= par["phi_k"].sum(axis=1, keepdims=True)
    x, aux = np.array([1, 1], dtype=np.int32), np.array([1, 1])
    got = xr.series_stats(TAYAL, 3, x, aux, par)
    want = enumerate_stats(TAYAL, 4, 3, x, aux, par)
    assert got["loglik"] == -math.inf == want["loglik"]
    for name in STATS:
        assert np.isnan(got[name]).all() and np.isnan(want[name]).all()
    # one sign later the same steps are free: a finite series again
    assert np.isfinite(xr.series_stats(TAYAL, 3, x, np.array([1, 2]), par)["loglik"])


def _tangent_check(model, data, par, name, idx, a, b):
    """score[name][idx + (a,)] - score[name][idx + (b,)] against the central difference of loglik along e_a - e_b."""
    h = 1e-6
    aux = data.get("g", data.get("sign"))[0]
    x = data["x"][0]
    st = {k: np.asarray(v)[None] for k, v in xr.series_stats(model, int(data["L"]), x, aux, par).items()}
    sc = hhmm_amd.score(model, {k: np.asarray(v)[None] for k, v in par.items()}, st, "zip", 1, 1)[name][0]
    an = sc[idx + (a,)] - sc[idx + (b,)]
    ll = []
    for s in (+h, -h):
        q = {k: np.array(v) for k, v in par.items()}
        q[name][idx + (a,)] += s
        q[name][idx + (b,)] -= s
        ll.append(xr.loglik(model, x, aux, q))
    fd = (ll[0] - ll[1]) / (2 * h)
    assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (model, name, idx, a, b, fd, an)
    return an


@pytest.mark.parametrize("seed", [1, 2])
def test_fishers_identity_on_the_reference(seed):
    """h = 1e-6: the h^2 truncation plus the 1e-16 / h rounding of the difference allow a relative 1e-6."""
    data, draws = make(TAYAL, 1, 1, 12, 4, 3, seed=seed)
    par = {k: np.array(v[0]) for k, v in draws.items()}
    seen = [_tangent_check(TAYAL, data, par, "A_row", (0,), 0, 1), _tangent_check(TAYAL, data, par, "A_row", (1,), 0, 1),
            _tangent_check(TAYAL, data, par, "phi_k", (2,), 0, 2)]
    # p_11 is a free scalar: its score is the derivative itself
    h = 1e-6
    x, aux = data["x"][0], data["sign"][0]
    st = {k: np.asarray(v)[None] for k, v in xr.series_stats(TAYAL, 3, x, aux, par).items()}
    an = hhmm_amd.score(TAYAL, {k: np.asarray(v)[None] for k, v in par.items()}, st, "zip", 1, 1)["p_11"][0]
    fd = (xr.loglik(TAYAL, x, aux, dict(par, p_11=par["p_11"] + h)) -
          xr.loglik(TAYAL, x, aux, dict(par, p_11=par["p_11"] - h))) / (2 * h)
    assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (fd, an)
    data, draws = make(SEMISUP, 1, 1, 12, 4, 3, seed=seed)
    data["g"][0, :] = np.array([1, 2, 1, 3, 2, 2, 1, 1, 3, 2, 1, 2])
    par = {k: np.array(v[0]) for k, v in draws.items()}
    for i in range(4):
        seen.append(_tangent_check(SEMISUP, data, par, "A_ij", (i,), i, (i + 1) % 4))
    seen.append(_tangent_check(SEMISUP, data, par, "p_1k", (), 0, 3))
    assert max(abs(v) for v in seen) > 0.1                                       # gradients of order 1, not all ~0


# ---------------------------------------------------------------- CPU: the interfaces

def test_symbols_load(engine):
    for name in ("hhmm_expected_stats", "hhmm_expected_stats_device", "hhmm_expected_stats_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    assert callable(hhmm_amd.expected_stats)
    assert sys.modules["hhmm_amd.expect"].MODELS == _gibbs.MODELS


def test_header_compiles_as_c(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "hhmm_expect.h"\n'
                 "int main(void){ hhmm_request r; hhmm_estep_result o; size_t b = 0; (void)r; (void)o;\n"
                 "  hhmm_status (*f)(const hhmm_request *, hhmm_estep_result *) = hhmm_expected_stats;\n"
                 "  hhmm_status (*g)(const hhmm_request *, size_t *) = hhmm_expected_stats_workspace_size;\n"
                 "  hhmm_status (*h)(const hhmm_request *, hhmm_estep_result *, void *, size_t, void *) = "
                 "hhmm_expected_stats_device;\n"
                 "  return (f && g && h && HHMM_ABI_VERSION == 2) ? (int)b : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(REPO / "include"), "-c", str(c),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_python_shape_checks():
    td, tw = make(TAYAL, 6, 6, 5, 4, 3)
    with pytest.raises(ValueError):
        hhmm_amd.expected_stats(TAYAL, td, {k: v for k, v in tw.items() if k != "A_row"}, "zip")
    with pytest.raises(ValueError):
        hhmm_amd.expected_stats(TAYAL, td, dict(tw, phi_k=tw["phi_k"][:, :, :2]), "zip")
    sd, sw = make(SEMISUP, 3, 5, 6, 4, 9)
    with pytest.raises(ValueError):
        hhmm_amd.expected_stats(SEMISUP, sd, sw, "zip")                            # N != S
    with pytest.raises(ValueError):
        hhmm_amd.baum_welch(TAYAL, td, tw, 1, pairing="grid")
    with pytest.raises(ValueError):
        hhmm_amd.expected_stats("hmm", {"K": 3, "x": np.zeros((2, 5))}, {})
    with pytest.raises(ValueError):
        hhmm_amd.m_step("hhmm-tayal2009-lite", {})
    with pytest.raises(ValueError):
        hhmm_amd.score("iohmm-reg", {}, {}, "zip", 1, 1)


def _poke(field, value):
    def f(pr, res):
        obj, name = (pr.req, field) if "." not in field else (getattr(pr.req, field.split(".")[0]), field.split(".")[1])
        setattr(obj, name, value)
    return f


def _null(field):
    def f(pr, res):
        setattr(res, field, None)
    return f


def _same(pr, res):
    pass


# name -> (model, K, L, change to the prepared request, expected status, word of the message)
BAD = {
    "model_gauss": ("hmm-multinom", 4, 9, _poke("model", 1), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm_reg": ("hmm-multinom", 4, 9, _poke("model", 4), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm_mix": ("hmm-multinom", 4, 9, _poke("model", 5), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm_hmix": ("hmm-multinom", 4, 9, _poke("model", 6), _abi.ERR_UNSUPPORTED, "model"),
    "model_iohmm_hmix_lite": ("hmm-multinom", 4, 9, _poke("model", 7), _abi.ERR_UNSUPPORTED, "model"),
    "model_tayal_lite": (TAYAL, 4, 9, _poke("model", 9), _abi.ERR_UNSUPPORTED, "model"),
    "K9": ("hmm-multinom", 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K9_semisup": (SEMISUP, 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": (TAYAL, 4, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "lds_semisup": (SEMISUP, 7, 21, _same, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_tayal": (TAYAL, 4, 41, _same, _abi.ERR_UNSUPPORTED, "LDS"),
    "null_xi": (TAYAL, 4, 9, _null("xi_ij"), _abi.ERR_INVALID_ARGUMENT, "xi_ij"),
    "null_c_kl": (SEMISUP, 4, 9, _null("c_kl"), _abi.ERR_INVALID_ARGUMENT, "c_kl"),
    "abi": (TAYAL, 4, 9, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _gibbs._request(model, data, draws, "grid", -1)
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_expected_stats(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_expected_stats_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_host_entry_rejects_values_outside_the_data_block(engine, bad):
    data, draws = make(TAYAL, 2, 2, 5, 4, 9)
    data["x"][1, 3] = bad
    pr, res, _out = _gibbs._request(TAYAL, data, draws, "grid", -1)
    assert engine.hhmm_expected_stats(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "x[1, 4]" in engine.hhmm_last_error().decode()
    data["x"][1, 3] = 1
    data["sign"][0, 2] = 3 if bad == 10 else bad
    pr, res, _out = _gibbs._request(TAYAL, data, draws, "grid", -1)
    assert engine.hhmm_expected_stats(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "sign[0, 3]" in engine.hhmm_last_error().decode()


# the largest accepted tables: L * ceil(K / 2) = 80
@pytest.mark.parametrize("model,K,L", [(TAYAL, 4, 40), (SEMISUP, 7, 20), ("hmm-multinom", 4, 9)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _gibbs._request(model, data, draws, "grid", -1)
    st = engine.hhmm_expected_stats(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws = C.c_size_t(0)
    assert engine.hhmm_expected_stats_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-5 // fb_chunk(K)) * K * 4 * 8                            # the checkpoints: ceil(T / C) K P 8


def test_tayal_m_step_and_score_arithmetic():
    P = 3
    n1 = np.array([[0.25, 0.0, 0.75, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    xi = np.zeros((P, 4, 4))
    xi[0, 0, 1], xi[0, 0, 2], xi[0, 2, 0], xi[0, 2, 3] = 1.0, 3.0, 2.0, 2.0
    xi[2, 0, 1] = 5.0                                                             # pair 2: row 0 all on its first entry
    xi[:, 1, 0] = 7.0                                                             # A(2, 1) = 1 is no parameter
    c = np.ones((P, 4, 2))
    c[1, 3] = 0.0
    stats = {"loglik": np.zeros(P), "n_1k": n1, "xi_ij": xi, "c_kl": c}
    prev = {"p_11": np.array([0.5, 0.3, 0.6]), "A_row": np.full((P, 2, 2), 0.5), "phi_k": np.full((P, 4, 2), 0.5)}
    prev["A_row"][1] = [[0.9, 0.1], [0.2, 0.8]]
    prev["phi_k"][1, 3] = [0.4, 0.6]
    new = hhmm_amd.m_step(TAYAL, stats, prev)
    assert set(new) == {"p_11", "A_row", "phi_k"}
    assert np.array_equal(new["p_11"], [0.25, 0.3, 0.0])                           # a zero total keeps prev
    assert np.array_equal(new["A_row"][0], [[0.25, 0.75], [0.5, 0.5]])
    assert np.array_equal(new["A_row"][1], prev["A_row"][1])
    assert np.array_equal(new["A_row"][2], [[1.0, 0.0], [0.5, 0.5]])
    assert np.array_equal(new["phi_k"][1, 3], [0.4, 0.6]) and np.array_equal(new["phi_k"][0], np.full((4, 2), 0.5))
    # the score: 0 / 0 -> 0 at the ends of p_11 and at a zero of A_row
    draws = {"p_11": np.array([0.5, 0.0, 1.0]), "A_row": np.array([[[0.5, 0.5], [0.25, 0.75]]] * P),
             "phi_k": np.full((P, 4, 2), 0.5)}
    draws["A_row"][2, 0] = [1.0, 0.0]
    n1s = np.array([[0.25, 0.0, 0.75, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    sc = hhmm_amd.score(TAYAL, draws, dict(stats, n_1k=n1s), "zip", P, P)
    assert np.array_equal(sc["p_11"], [0.25 / 0.5 - 0.75 / 0.5, -1.0, 1.0])
    assert np.array_equal(sc["A_row"][0], [[2.0, 6.0], [8.0, 2.0 / 0.75]])
    assert np.array_equal(sc["A_row"][2], [[5.0, 0.0], [0.0, 0.0]])
    assert np.array_equal(sc["phi_k"][0], np.full((4, 2), 2.0))
    # NaN statistics give NaN parameters, not prev
    nan = {k: np.full_like(v, np.nan) for k, v in stats.items()}
    assert np.isnan(hhmm_amd.m_step(TAYAL, nan, prev)["p_11"]).all()


# ---------------------------------------------------------------- GPU

def check(engine, model, data, draws, pairing="grid"):
    """The host entry against the reference; the device entry bit-equal to the host entry."""
    from stats_devrun import DeviceExpect
    got = hhmm_amd.expected_stats(model, data, draws, pairing, lib=engine, return_status=True)
    want = xr.expected_stats(model, data, draws, pairing)
    w = worst(got, want)
    assert w <= TOL, (model, pairing, w)
    assert got["status"] == 0 and not got["pair_status"].any()
    dv = DeviceExpect(engine, model, data, draws, pairing)
    assert dv.run() == 0
    dev = dv.stats()
    assert not dev["pair_status"].any()
    for name in STATS + ("loglik",):
        assert np.array_equal(dev[name], got[name], equal_nan=True), (model, pairing, name)
    return got, want


KL = [(SEMISUP, K, L) for K in (4, 5, 6, 8) for L in (1, 2, 9, 16)] + [(TAYAL, 4, L) for L in (1, 2, 9, 16)] + \
     [(SEMISUP, 1, 3), (SEMISUP, 2, 3), (SEMISUP, 3, 3), (SEMISUP, 7, 20), (TAYAL, 4, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", KL)
def test_gpu_every_instance(engine, model, K, L):
    data, draws = make(model, 3, 5, 2 * fb_chunk(K) + 1, K, L, seed=K * 100 + L)
    check(engine, model, data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [(SEMISUP, 4, 9), (SEMISUP, 5, 3), (TAYAL, 4, 9)])
@pytest.mark.parametrize("Tsel", ["1", "2", "C-1", "C", "C+1", "2C+1", "61"])
def test_gpu_chunk_edges_in_T(engine, model, K, L, Tsel):
    c = fb_chunk(K)
    T = {"1": 1, "2": 2, "C-1": c - 1, "C": c, "C+1": c + 1, "2C+1": 2 * c + 1, "61": 61}[Tsel]
    data, draws = make(model, 2, 3, T, K, L, seed=T)
    got, _want = check(engine, model, data, draws)
    assert np.isfinite(got["loglik"]).all()
    assert np.max(np.abs(got["c_kl"].sum(axis=(1, 2)) - T)) <= TOL * T
    if T == 1:
        assert not got["xi_ij"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [(SEMISUP, 5, 3), (TAYAL, 4, 9)])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_gpu_partial_last_wave(engine, model, K, L, P):
    data, draws = make(model, P, P, 11, K, L, seed=P)
    check(engine, model, data, draws, "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [(SEMISUP, 4, 3), (TAYAL, 4, 4)])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 13, K, L, seed=N * S)
    check(engine, model, data, draws, pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [(SEMISUP, 6, 4), (TAYAL, 4, 5)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, K, L):
    c = fb_chunk(K)
    Tmax = 2 * c + 1
    lens = np.array([1, Tmax, 2, c, c + 1, Tmax, 1, c - 1] * 3, dtype=np.int32)
    N = lens.size
    data, draws = make(model, N, 2, Tmax, K, L, seed=7)
    aux = data["g"] if model == SEMISUP else data["sign"]
    for n in range(N):  # padding rows must not matter: garbage symbols, aux values outside the block's range
        data["x"][n, lens[n]:] = L + 5
        aux[n, lens[n]:] = [77, -5, 0, INT32_MIN][n % 4]
    data["T"] = lens
    check(engine, model, data, draws)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["all1", "all2", "alt1", "alt2", "mixed"])
def test_gpu_tayal_sign_patterns(engine, pattern):
    """One sign per step over the whole wave (tayal_dispatch's sign-class path) and a zip batch whose lanes
    disagree at every step (the masks per lane); sign_1 both ways.  Both against the one reference."""
    N, S, T = 2, 70, 19
    data, draws = make(TAYAL, N, S, T, 4, 5, seed=31)
    t = np.arange(T)
    if pattern != "mixed":
        row = {"all1": np.ones(T), "all2": np.full(T, 2), "alt1": 1 + t % 2, "alt2": 2 - t % 2}[pattern]
        data["sign"] = np.tile(row.astype(np.int32), (N, 1))
        check(engine, TAYAL, data, draws)
    else:
        data, draws = make(TAYAL, 140, 140, T, 4, 5, seed=33)
        data["sign"][::2, 0] = 1
        data["sign"][1::2, 0] = 2
        check(engine, TAYAL, data, draws, "zip")


@pytest.mark.gpu
def test_gpu_sign_class_path_agrees_with_the_per_lane_path(engine):
    """The same (series, draw) pairs once in a wave that shares every step's sign and once in a wave that
    does not (a second series with the opposite signs interleaved, zip).  The sign-class arms do the per-lane
    form's additions in its order, so a pair's result does not depend on the other lanes of its wave: the
    same bits (the last wave's spare lanes redo pair P - 1 and store it again, which needs that too)."""
    T, B = 19, 64
    data, draws = make(TAYAL, 1, B, T, 4, 5, seed=35)
    shared = hhmm_amd.expected_stats(TAYAL, data, draws, "grid", lib=engine)
    x2 = np.repeat(data["x"], 2 * B, axis=0)
    s2 = np.repeat(data["sign"], 2 * B, axis=0)
    s2[1::2] = 3 - s2[1::2]
    d2 = {k: np.repeat(v, 2, axis=0) for k, v in draws.items()}
    mixed = hhmm_amd.expected_stats(TAYAL, dict(data, x=x2, sign=s2), d2, "zip", lib=engine)
    for name in STATS + ("loglik",):
        assert np.array_equal(mixed[name][0::2], shared[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1, 2, 3, "mixed"])
@pytest.mark.parametrize("K", [4, 5])
def test_gpu_semisup_groups(engine, g, K):
    data, draws = make(SEMISUP, 3, 30, 19, K, 4, seed=37)
    if g != "mixed":
        data["g"][:] = g
    got, _want = check(engine, SEMISUP, data, draws)
    if g == 3:  # no transition is ever applied
        assert not got["xi_ij"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["p11=0", "p11=1", "row0=(1,0)", "row0=(0,1)", "row1=(1,0)", "row1=(0,1)"])
def test_gpu_tayal_degenerate_draws(engine, kind):
    """Exact zeros at the structural zeros (of the matrix and of the draw), finite statistics elsewhere."""
    N, S, T = 3, 40, 21
    data, draws = make(TAYAL, N, S, T, 4, 5, seed=39)
    if kind.startswith("p11"):
        draws["p_11"][:] = float(kind[-1])
    else:
        draws["A_row"][:, int(kind[3])] = (1.0, 0.0) if kind.endswith("(1,0)") else (0.0, 1.0)
    got, _want = check(engine, TAYAL, data, draws)
    for name in STATS + ("loglik",):
        assert np.isfinite(got[name]).all(), name
    A = np.array([dsr.tayal_expand(draws["p_11"][s], draws["A_row"][s])[1] for s in range(S)])
    Ap = np.tile(A, (N, 1, 1))                                                    # grid: draw p % S
    assert not got["xi_ij"][Ap == 0].any() and got["xi_ij"][Ap > 0].all()
    assert not got["n_1k"][:, [1, 3]].any()
    if kind == "p11=0":
        assert not got["n_1k"][:, 0].any()
    if kind == "p11=1":
        assert not got["n_1k"][:, 2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("model", MASKED)
def test_gpu_impossible_series_is_nan_for_that_pair_only(engine, model):
    N, S, L = 3, 5, 9
    data, draws = make(model, N, S, 17, 4, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _want = check(engine, model, data, draws)
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf
    for name in STATS:
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
def test_gpu_series_through_a_structural_zero_is_nan_for_that_pair_only(engine):
    """The CPU case above on the kernel: series 0 can only cross A(2..3, 2..3) = 0 with the mask on."""
    data, draws = make(TAYAL, 2, 3, 2, 4, 3, seed=12)
    data["x"][0] = 1
    data["sign"][:] = [[1, 1], [1, 2]]
    data["x"][1] = 1
    draws["phi_k"][:, [0, 3], 0] = 0.0
    draws["phi_k"] /= draws["phi_k"].sum(axis=2, keepdims=True)
    got, _want = check(engine, TAYAL, data, draws)
    assert (got["loglik"][:3] == -np.inf).all() and np.isfinite(got["loglik"][3:]).all()
    for name in STATS:
        assert np.isnan(got[name][:3]).all() and np.isfinite(got[name][3:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,name,idx", [(TAYAL, "A_row", (1, 0, 1)), (TAYAL, "phi_k", (1, 2, 3)),
                                            (TAYAL, "p_11", (1,)), (SEMISUP, "A_ij", (1, 0, 1)),
                                            (SEMISUP, "phi_k", (1, 2, 3))])
def test_gpu_nan_draw_is_nan_for_its_pairs_only(engine, model, name, idx):
    N, S = 3, 5
    data, draws = make(model, N, S, 20, 4, 9, seed=13)
    if model == TAYAL:
        data["sign"][:, 0] = 2               # sign_1 = 2: p_11 is used by every series
    else:
        data["g"][:, 1] = 2                  # column 2 takes A at step 2: A(1, 2) is used by every series
    data["x"][:, 5] = 4                      # phi(3, 4) is read by every series
    draws[name][idx] = np.nan
    got, _want = check(engine, model, data, draws)
    hit = np.arange(N * S) % S == 1
    for k in STATS + ("loglik",):
        assert np.isnan(got[k][hit]).all() and np.isfinite(got[k][~hit]).all(), k


def _device(engine, model, data, draws):
    from stats_devrun import DeviceExpect
    dv = DeviceExpect(engine, model, data, draws)
    assert dv.run() == 0
    return dv.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("model,field,bad", [(SEMISUP, "x", 10), (SEMISUP, "x", 0), (TAYAL, "x", INT32_MIN),
                                             (SEMISUP, "g", 4), (SEMISUP, "g", 0), (TAYAL, "sign", 3),
                                             (TAYAL, "sign", INT32_MIN), (TAYAL, "T", 0), (SEMISUP, "T", 16)])
def test_gpu_device_entry_flags_invalid_data(engine, model, field, bad):
    N, S, L = 4, 20, 9
    data, draws = make(model, N, S, 15, 4, L, seed=19)
    data["T"] = np.array([15, 9, 15, 12], dtype=np.int32)
    want = _device(engine, model, data, draws)
    assert not want["pair_status"].any()
    if field == "T":
        data["T"][2] = bad
    else:
        data[field][2, 6] = bad
    got = _device(engine, model, data, draws)
    hit = np.arange(N * S) // S == 2
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in STATS + ("loglik",):
        assert np.array_equal(got[name][~hit], want[name][~hit], equal_nan=True), name
    # a bad value in the padding of a shorter series is no violation
    if field != "T":
        data[field][2, 6] = 1
        data[field][1, 12] = bad
        assert not _device(engine, model, data, draws)["pair_status"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("K,L", [(4, 9), (5, 3), (8, 2)])
def test_gpu_hmm_multinom_is_the_estep_bit_for_bit(engine, K, L):
    data, draws = make("hmm-multinom", 3, 70, 2 * fb_chunk(K) + 3, K, L, seed=K)
    got = hhmm_amd.expected_stats("hmm-multinom", data, draws, lib=engine, return_status=True)
    want = hhmm_amd.estep("hmm-multinom", data, draws, lib=engine)
    assert got["status"] == 0 and not got["pair_status"].any()
    for name in STATS + ("loglik",):
        assert np.array_equal(got[name], want[name]), name
    dev = _device(engine, "hmm-multinom", data, draws)
    for name in STATS + ("loglik",):
        assert np.array_equal(dev[name], want[name]), name


RB_R, RB_T, RB_SEED = 2048, 12, 5


def rao_blackwell_inputs(model):
    """N = 2 series of T = 12 under R identical copies of one draw (grid: P = 2 R, fresh uniforms per pair)."""
    data, draws = make(model, 2, 1, RB_T, 4, 3, seed=RB_SEED)
    many = {k: np.repeat(v, RB_R, axis=0) for k, v in draws.items()}
    return data, draws, many, synth.ffbs_uniforms(2 * RB_R, RB_T, seed=RB_SEED)


def rao_blackwell_check(sample, expect):
    """sample: {name: (2 R, ...)} counts of one path per pair; expect: {name: (2, ...)}.  Every entry of the
    mean over a series' R pairs within 5 standard errors (sample sd / sqrt(R)) of its expectation; an entry
    whose expectation is exactly 0 is exactly 0 in every path; one with no spread (an exact integer) is equal."""
    worst_z = 0.0
    for name in STATS:
        for n in range(2):
            v, e = sample[name][n * RB_R:(n + 1) * RB_R], expect[name][n]
            assert np.isfinite(v).all() and np.isfinite(e).all(), name
            assert not v[:, e == 0].any(), name
            mean, se = v.mean(axis=0), v.std(axis=0, ddof=1) / np.sqrt(RB_R)
            flat = se == 0
            assert np.max(np.abs(mean[flat] - e[flat]), initial=0.0) <= TOL * RB_T, (name, n)
            z = np.abs(mean[~flat] - e[~flat]) / se[~flat]
            print(name, "series", n, "max |z| =", float(z.max(initial=0.0)))
            worst_z = max(worst_z, float(z.max(initial=0.0)))
    assert worst_z <= 5.0, worst_z


@pytest.mark.gpu
@pytest.mark.parametrize("model", MASKED)
def test_gpu_mean_of_the_draw_statistics_is_the_expected_statistics(engine, model):
    """Rao-Blackwell: E over the uniforms of hhmm_amd.draw_stats = hhmm_amd.expected_stats.  A condition, not
    a measurement: before this was committed the references alone were checked to pass it for this seed on
    the CPU -- the oracle's z_ffbs for these uniforms -> draw_stats_ref.counts_pairs, against expect_ref
    (rao_blackwell_check on both; max |z| 2.7 for semisup, 3.0 for Tayal)."""
    data, draws, many, u = rao_blackwell_inputs(model)
    sample = hhmm_amd.draw_stats(model, data, many, u, "grid", lib=engine)
    expect = hhmm_amd.expected_stats(model, data, draws, "grid", lib=engine)
    assert worst(expect, xr.expected_stats(model, data, draws, "grid")) <= TOL
    rao_blackwell_check(sample, expect)


@pytest.mark.gpu
def test_gpu_long_series_keeps_its_scale(engine):
    """T = 3000: exp(loglik) underflows fp64 (log of the smallest subnormal is -744.4); the scaled sweeps do not."""
    data, draws = synth.tayal(N=1, S=2, T=3000, L=9)
    got, want = check(engine, TAYAL, data, draws)
    assert (got["loglik"] < -745.0).all() and np.isfinite(got["loglik"]).all()
    assert np.max(np.abs(got["c_kl"].sum(axis=(1, 2)) - 3000)) <= TOL * 3000
