"""Draw statistics and the blocked Gibbs samplers at 8 < K <= 32 (include/hhmm_gibbs.h,
hhmm_draw_stats_large; csrc/hhmm_draw_stats_large.hip): hmm-multinom and the Gaussian hmm on groups of 16 or
32 lanes per pair.

CPU: symbols, the headers as C, the argument checks (they come before the device check), the workspace size,
the routing of hhmm_amd.draw_stats / draw_stats_gauss by K, and the samplers built from the oracle's FFBS +
the reference statistics + conditional_draw / conditional_draw_gauss at K = 9 against the exact posterior of a
T = 4 series (all 9^4 = 6561 paths enumerated, tests/draw_stats_ref.py and tests/draw_stats_gauss_ref.py),
under the cap |z| < 5 of tests/test_ffbs.py.

gpu: the kernel against the reference statistics of the path hhmm_amd.gqs(..., pars=["z_ffbs", "loglik"])
returns for the same uniforms (the FFBS contract, pinned bit for bit elsewhere), through the host and the
device entry: n_1k, xi_ij, c_kl and w_k with ==, loglik to 1e-9 relative to max(1, |v|), s1_k within
T 2^-52 sum|x_t| and s2_k within T 2^-52 sum x_t^2 of the fsum reference -- the first-order bound of T
sequential fp64 additions in any order, doubled (the bound of tests/test_draw_stats_gauss.py).  The two
entries are bit-identical to each other and on a second run.  Then hhmm_amd.gibbs and gibbs_gauss at K = 9
against the same enumeration and cap.

Shapes: a group of G = 16 lanes owns a pair up to K = 16, G = 32 above; the compile-time state loops run 16,
24 or 32 entries, so K = 9, 16 | 17, 24 | 25, 32 are both sides of every instance edge.  Checkpoints come every
8 steps and observations in blocks of G steps, so T covers 1, 2, the chunk edges 7 8 9, the block edges 16 17
and 32 33, and 70 (a last chunk of 6 steps after a full block pair).
"""
import ctypes as C
import functools
import math
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import draw_stats_gauss_ref as gref
import draw_stats_ref as dsr
import hhmm_amd
from hhmm_amd import _abi, _stats, synth

REPO = pathlib.Path(__file__).resolve().parent.parent
_gibbs = sys.modules["hhmm_amd.gibbs"]
_gg = sys.modules["hhmm_amd.gibbs_gauss"]
ENTRIES = ("hhmm_draw_stats_large", "hhmm_draw_stats_large_device", "hhmm_draw_stats_large_workspace_size")
TOL = 1e-9
ZCAP = 5.0  # tests/test_ffbs.py
KS = [9, 16, 17, 24, 25, 32]
TS = [1, 2, 7, 8, 9, 16, 17, 32, 33, 70]
# (pairing, N, S): P = 5 every time
PAIRINGS = [("grid", 1, 5), ("grid", 5, 1), ("zip", 5, 5), ("block", 5, 5)]
FAMILIES = [("hmm", 0), ("hmm-multinom", 2), ("hmm-multinom", 9)]
BOTH = [("hmm", 0), ("hmm-multinom", 9)]


def lds_max_L(K):
    """The largest L of hmm-multinom: G * (16 + 12 L + 4 K) <= 160 KiB (include/hhmm_gibbs.h)."""
    G = 16 if K <= 16 else 32
    return (160 * 1024 // G - 16 - 4 * K) // 12


def make(model, N, S, T, K, L=0, seed=0):
    """Random parameters and series; Gaussian: overlapping states, so the paths vary with the uniforms."""
    g = np.random.Generator(np.random.Philox(key=9000 + seed))
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K))}
    if model == "hmm-multinom":
        draws["phi_k"] = g.dirichlet(np.full(L, 2.0), size=(S, K))
        return {"K": K, "L": L, "x": g.integers(1, L + 1, size=(N, T)).astype(np.int32)}, draws
    mu = 1.5 * np.arange(K) - 0.75 * (K - 1)
    draws["mu_k"] = mu[None, :] + g.normal(0.0, 0.3, size=(S, K))
    draws["sigma_k"] = g.uniform(0.6, 1.6, size=(S, K))
    return {"K": K, "x": mu[g.integers(0, K, size=(N, T))] + g.normal(0.0, 1.0, size=(N, T))}, draws


def npairs(N, S, pairing):
    return N * S if pairing == "grid" else (N if pairing == "zip" else S)


def prepare(model, data, draws, u, pairing="grid"):
    if model == "hmm":
        return _gg.prepare(data, draws, u, pairing)
    return _gibbs.prepare(model, data, draws, u, pairing)


def host_entry(engine, model, data, draws, u, pairing="grid"):
    if model == "hmm":
        return hhmm_amd.draw_stats_gauss(data, draws, u, pairing, lib=engine, return_status=True)
    return hhmm_amd.draw_stats(model, data, draws, u, pairing, lib=engine, return_status=True)


def device_entry(engine, model, data, draws, u, pairing="grid"):
    pr, res, out = prepare(model, data, draws, u, pairing)
    return _stats.DeviceStats(engine, "draw_stats_large", pr, res, {name: a.shape for name, a in out.items()})


def device_run(dv):
    import torch
    assert dv.run() == 0
    torch.cuda.synchronize()
    return dv.stats()


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ENTRIES:
        assert getattr(engine, name).restype is C.c_int


def test_headers_compile_as_c(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "hhmm_gibbs.h"\n#include "hhmm_gibbs_gauss.h"\n'
                 "int main(void){ hhmm_request r; hhmm_estep_result o; size_t b = 0; (void)r; (void)o;\n"
                 "  hhmm_status (*f)(const hhmm_request *, hhmm_estep_result *) = hhmm_draw_stats_large;\n"
                 "  hhmm_status (*g)(const hhmm_request *, size_t *) = hhmm_draw_stats_large_workspace_size;\n"
                 "  hhmm_status (*h)(const hhmm_request *, hhmm_estep_result *, void *, size_t, void *) = "
                 "hhmm_draw_stats_large_device;\n"
                 "  return (f && g && h && HHMM_ABI_VERSION == 2) ? (int)b : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(REPO / "include"), "-c", str(c),
                    "-o", str(tmp_path / "use.o")], check=True)


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
    "no_uniforms": ("hmm-multinom", 12, 9, _poke("ffbs_u", None), _abi.ERR_INVALID_ARGUMENT, "ffbs_u"),
    "no_uniforms_gauss": ("hmm", 12, 0, _poke("ffbs_u", None), _abi.ERR_INVALID_ARGUMENT, "ffbs_u"),
    "device_set": ("hmm-multinom", 12, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "abi": ("hmm", 12, 0, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
    # one group's slots, phi table, count table and xi rows against 160 KiB: the first L that does not fit
    "lds_G16": ("hmm-multinom", 12, lds_max_L(12) + 1, _same, _abi.ERR_UNSUPPORTED, f"L = {lds_max_L(12) + 1}"),
    "lds_G32": ("hmm-multinom", 25, lds_max_L(25) + 1, _same, _abi.ERR_UNSUPPORTED, f"L = {lds_max_L(25) + 1}"),
}


def test_the_lds_formula_gives_the_headers_figures():
    assert lds_max_L(12) == 848 and lds_max_L(25) == 417


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = prepare(model, data, draws, synth.ffbs_uniforms(4, 5))
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_draw_stats_large(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_draw_stats_large_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)
    if case.startswith("K8"):
        assert "hhmm_draw_stats " in msg and "K <= 8" in msg, msg
    if case.startswith("lds"):
        assert "LDS" in msg, msg


@pytest.mark.parametrize("entry", ["host", "device"])
def test_null_request_is_an_invalid_argument(engine, entry):
    res = _abi.EstepResult()
    if entry == "host":
        st = engine.hhmm_draw_stats_large(None, C.byref(res))
    else:
        st = engine.hhmm_draw_stats_large_device(None, C.byref(res), None, 0, None)
    assert st == _abi.ERR_INVALID_ARGUMENT and "request" in engine.hhmm_last_error().decode()


@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 12, lds_max_L(12)), ("hmm-multinom", 25, lds_max_L(25)),
                                       ("hmm", 32, 0)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  The largest L of either group size."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = prepare(model, data, draws, synth.ffbs_uniforms(4, 5))
    st = engine.hhmm_draw_stats_large(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()


@pytest.mark.parametrize("K,Tmax,P", [(9, 1, 1), (23, 70, 5), (32, 1000, 3)])
def test_workspace_is_the_checkpoints(engine, K, Tmax, P):
    data, draws = make("hmm-multinom", P, P, Tmax, K, 3)
    pr, _res, _out = prepare("hmm-multinom", data, draws, synth.ffbs_uniforms(P, Tmax), "zip")
    ws = C.c_size_t(0)
    assert engine.hhmm_draw_stats_large_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-Tmax // 8) * K * P * 8


def test_workspace_size_rejects_the_lane_kernels_K(engine):
    data, draws = make("hmm-multinom", 2, 2, 5, 8, 3)
    pr, _res, _out = prepare("hmm-multinom", data, draws, synth.ffbs_uniforms(2, 5), "zip")
    ws = C.c_size_t(0)
    assert engine.hhmm_draw_stats_large_workspace_size(C.byref(pr.req), C.byref(ws)) == _abi.ERR_UNSUPPORTED
    assert "K = 8" in engine.hhmm_last_error().decode()


def test_existing_entries_keep_rejecting_K9_with_their_messages(engine):
    for model, entry in (("hmm-multinom", "hhmm_draw_stats"), ("hmm", "hhmm_draw_stats_gauss")):
        data, draws = make(model, 2, 2, 5, 9, 3)
        pr, res, _out = prepare(model, data, draws, synth.ffbs_uniforms(4, 5))
        assert getattr(engine, entry)(C.byref(pr.req), C.byref(res)) == _abi.ERR_UNSUPPORTED
        assert "K = 9, the lane-per-pair kernel supports K <= 8" in engine.hhmm_last_error().decode()


def test_python_routing_by_K(monkeypatch):
    assert [_gibbs.entry_name("hmm-multinom", K) for K in (1, 8, 9, 32, 33)] == \
        ["draw_stats", "draw_stats", "draw_stats_large", "draw_stats_large", "draw_stats_large"]
    assert _gibbs.entry_name("hmm-multinom-semisup", 9) == "draw_stats"            # a K <= 8 program: rejected there
    assert _gibbs.entry_name("hhmm-tayal2009", 4) == "draw_stats"
    assert [_gg.entry_name(K) for K in (1, 8, 9, 32, 33)] == \
        ["draw_stats_gauss", "draw_stats_gauss", "draw_stats_large", "draw_stats_large", "draw_stats_large"]
    called = []
    monkeypatch.setattr(_stats, "call", lambda lib, entry, pr, res, out, rs: called.append((entry, pr.K)) or out)
    for K in (8, 9):
        d, w = make("hmm-multinom", 2, 2, 5, K, 3)
        out = hhmm_amd.draw_stats("hmm-multinom", d, w, synth.ffbs_uniforms(4, 5), lib=object())
        assert out["c_kl"].shape == (4, K, 3) and out["xi_ij"].shape == (4, K, K)
        d, w = make("hmm", 2, 2, 5, K)
        out = hhmm_amd.draw_stats_gauss(d, w, synth.ffbs_uniforms(4, 5), lib=object())
        assert out["s2_k"].shape == (4, K)
    assert called == [("draw_stats", 8), ("draw_stats_gauss", 8), ("draw_stats_large", 9), ("draw_stats_large", 9)]


# ---- the exact posterior of a T = 4 series at K = 9, and the samplers against it

CHAINS, SWEEPS, K9, L3 = 4096, 40, 9, 3
X4 = np.array([2, 1, 3, 3], dtype=np.int32)
X4G = np.array([-1.2, 0.9, 1.4, -0.7])


@functools.lru_cache(maxsize=None)
def priors():
    """Fixed asymmetric priors from a seeded generator: under a label-symmetric prior every mean is 1 / K and
    the comparison shows nothing."""
    g = np.random.Generator(np.random.Philox(key=9009))
    conc = {"p_1k": g.uniform(0.5, 3.0, size=K9), "A_ij": g.uniform(0.5, 3.0, size=(K9, K9))}
    multinom = dict(conc, phi_k=g.uniform(0.5, 3.0, size=(K9, L3)))
    gauss = dict(conc, mu_sigma=(np.linspace(-2.0, 2.0, K9), g.uniform(0.5, 2.0, size=K9), np.full(K9, 3.0),
                                 g.uniform(1.0, 3.0, size=K9)))
    return multinom, gauss


@functools.lru_cache(maxsize=None)
def exact_means(model):
    """Computed once, shared by the CPU and the GPU sampler tests."""
    if model == "hmm":
        means = gref.posterior_means(X4G, priors()[1], K9)
    else:
        means = dsr.posterior_means(model, K9, L3, X4, None, priors()[0])
    for v in means.values():
        v.setflags(write=False)
    return means


def prior_draw(model, seed):
    """CHAINS starts from the prior (the conditional draw on empty statistics)."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    zero = {"n_1k": np.zeros((CHAINS, K9)), "xi_ij": np.zeros((CHAINS, K9, K9))}
    if model == "hmm":
        zero.update(w_k=np.zeros((CHAINS, K9)), s1_k=np.zeros((CHAINS, K9)), s2_k=np.zeros((CHAINS, K9)))
        new = hhmm_amd.conditional_draw_gauss(zero, priors()[1], gen)
    else:
        zero["c_kl"] = np.zeros((CHAINS, K9, L3))
        new = hhmm_amd.conditional_draw(model, zero, priors()[0], gen)
    return {k: v.numpy() for k, v in new.items()}, gen


def worst_z(model, final):
    """max |z-score| of the across-chain mean of the final draw against the exact posterior mean; final draws
    of independent chains are iid, so the standard error is the sample sd over chains / sqrt(chains)."""
    if model == "hmm":
        final = dict(final, sigma2_k=np.asarray(final["sigma_k"]) ** 2)
    worst = 0.0
    for name, want in exact_means(model).items():
        v = np.asarray(final[name], dtype=float)
        assert v.shape == (CHAINS,) + want.shape, (name, v.shape)
        se = v.std(axis=0, ddof=1) / np.sqrt(CHAINS)
        z = np.abs(v.mean(axis=0) - want) / se
        print(model, name, "max |z| =", float(z.max()))
        worst = max(worst, float(z.max()))
    return worst


def test_the_exact_means_are_not_label_symmetric():
    for model in ("hmm-multinom", "hmm"):
        m = exact_means(model)
        assert np.allclose(m["p_1k"].sum(), 1.0) and np.allclose(m["A_ij"].sum(axis=1), 1.0)
        assert np.abs(m["p_1k"] - 1.0 / K9).max() > 0.02 and np.abs(m["A_ij"] - 1.0 / K9).max() > 0.02


@pytest.mark.parametrize("model", ["hmm-multinom", "hmm"])
def test_cpu_sampler_matches_the_exact_posterior_at_K9(oracle, model):
    params, gen = prior_draw(model, seed=41)
    ug = np.random.Generator(np.random.Philox(key=43))
    x = X4G if model == "hmm" else X4
    data = {"K": K9, "x": x.reshape(1, -1)}
    if model != "hmm":
        data["L"] = L3
    for _ in range(SWEEPS):
        u = 1.0 - ug.random((CHAINS, x.size))
        z = oracle.gqs(model, data, params, pars=["z_ffbs"], pairing="block", uniforms=u, nthreads=8)["z_ffbs"]
        assert z.min() >= 1
        if model == "hmm":
            st = dict(zip(gref.NAMES, gref.stats_chains(z, x, K9)))
            new = hhmm_amd.conditional_draw_gauss(st, priors()[1], gen)
        else:
            n1, xi, c = dsr.counts_chains(model, K9, L3, z, x)
            new = hhmm_amd.conditional_draw(model, {"n_1k": n1, "xi_ij": xi, "c_kl": c}, priors()[0], gen)
        params = {k: v.numpy() for k, v in new.items()}
    w = worst_z(model, params)
    assert w < ZCAP, (model, w)


# ---------------------------------------------------------------- GPU

def bounds(data, pairing, S, P):
    """Per pair (T 2^-52 sum |x_t|, T 2^-52 sum x_t^2) over the pair's own steps."""
    x = np.atleast_2d(np.asarray(data["x"], dtype=np.float64))
    N, Tm = x.shape
    Ts = np.asarray(data["T"]).reshape(N) if "T" in data else np.full(N, Tm)
    ser = gref.pair_series(pairing, P, S, N)
    b1, b2 = np.zeros(P), np.zeros(P)
    for p in range(P):
        n = int(ser[p])
        T = int(min(max(Ts[n], 1), Tm))
        xs = np.nan_to_num(x[n, :T])
        b1[p] = T * 2.0 ** -52 * math.fsum(np.abs(xs))
        b2[p] = T * 2.0 ** -52 * math.fsum(xs * xs)
    return b1, b2


def compare(model, got, want, ref_loglik, b, tag):
    for name in ("n_1k", "xi_ij") + (("w_k",) if model == "hmm" else ("c_kl",)):
        assert got[name].shape == want[name].shape, (tag, name)
        assert np.array_equal(got[name], want[name], equal_nan=True), (tag, name)
    if model == "hmm":
        for name, bn in (("s1_k", b[0]), ("s2_k", b[1])):
            assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), (tag, name)
            err = np.abs(got[name] - want[name])
            ok = ~np.isnan(want[name])
            print(tag, name, "max err / bound =", float(np.max((err / bn[:, None])[ok], initial=0.0)))
            assert (err[ok] <= np.broadcast_to(bn[:, None], err.shape)[ok]).all(), (tag, name)
    ll = got["loglik"]
    fin = np.isfinite(ref_loglik)
    assert np.array_equal(np.isnan(ll), np.isnan(ref_loglik)), tag
    assert np.array_equal(ll[~fin & ~np.isnan(ref_loglik)], ref_loglik[~fin & ~np.isnan(ref_loglik)]), tag
    if fin.any():
        w = float(np.max(np.abs(ll[fin] - ref_loglik[fin]) / np.maximum(1.0, np.abs(ref_loglik[fin]))))
        print(tag, "loglik worst", w)
        assert w <= TOL, (tag, w)


def reference(engine, model, data, draws, u, pairing):
    """The reference statistics of the engine's own z_ffbs (the bit-exact path) and its loglik."""
    S = draws["p_1k"].shape[0]
    r = hhmm_amd.gqs(model, data, draws, pars=["z_ffbs", "loglik"], pairing=pairing, uniforms=u, lib=engine)
    if model == "hmm":
        return gref.stats_pairs(data, r["z_ffbs"], r["loglik"], pairing, S), r
    return dsr.counts_pairs(model, data, r["z_ffbs"], r["loglik"], pairing, S), r


def check(engine, model, data, draws, u, pairing="grid"):
    """Host and device entries against the reference; the two are bit-identical to each other and on a second run."""
    want, r = reference(engine, model, data, draws, u, pairing)
    P = r["loglik"].shape[0]
    b = bounds(data, pairing, draws["p_1k"].shape[0], P) if model == "hmm" else None
    host = host_entry(engine, model, data, draws, u, pairing)
    assert host["status"] == 0 and not host["pair_status"].any()
    compare(model, host, want, r["loglik"], b, (model, data["K"], pairing, "host"))
    dv = device_entry(engine, model, data, draws, u, pairing)
    first = device_run(dv)
    second = device_run(dv)
    assert not first["pair_status"].any()
    for name in list(want) + ["loglik"]:
        assert np.array_equal(first[name], host[name], equal_nan=True), name
        assert np.array_equal(second[name], first[name], equal_nan=True), name
    return host, r


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("model,L", FAMILIES)
def test_gpu_instance_edges(engine, model, L, K, T):
    data, draws = make(model, 5, 5, T, K, L, seed=1000 * K + 10 * T)
    got, _r = check(engine, model, data, draws, synth.ffbs_uniforms(5, T, seed=K + T), "zip")
    assert np.isfinite(got["n_1k"]).all()
    if T == 1:
        assert not got["xi_ij"].any()
        if model == "hmm":  # x_1 alone: every state holds it once
            assert (got["w_k"] == 1).all() and np.array_equal(got["s1_k"], data["x"][:, :1] * np.ones((1, K)))


@pytest.mark.gpu
@pytest.mark.parametrize("pairing,N,S", PAIRINGS)
@pytest.mark.parametrize("K", [12, 23])
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_pairings(engine, model, L, K, pairing, N, S):
    data, draws = make(model, N, S, 19, K, L, seed=N + 10 * S)
    check(engine, model, data, draws, synth.ffbs_uniforms(npairs(N, S, pairing), 19, seed=S), pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 23])
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_ragged_lengths_inside_one_wave(engine, model, L, K):
    lens = np.array([70, 1, 33, 8, 9], dtype=np.int32)
    data, draws = make(model, 5, 5, 70, K, L, seed=K)
    for n in range(5):  # padding must not matter: garbage symbols / values past T[n]
        data["x"][n, lens[n]:] = L + 5 if model == "hmm-multinom" else 1e300
    data["T"] = lens
    got, _r = check(engine, model, data, draws, synth.ffbs_uniforms(5, 70, seed=K), "zip")
    key = "w_k" if model == "hmm" else "c_kl"
    extra = K - 1 if model == "hmm" else 0
    assert np.array_equal(got[key].reshape(5, -1).sum(axis=1), lens + extra)


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", [(12, 17), (12, 21), (23, 9), (23, 11)])
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_past_one_workgroup_and_a_last_wave_with_one_group(engine, model, L, K, P):
    """256 threads hold 16 groups at K = 12 and 8 at K = 23: P = 17 / 9 start a second workgroup with one live
    group; P = 21 / 11 leave its second wave with one.  (Where the launch takes smaller workgroups every P here
    still ends on a wave with one live group.)"""
    data, draws = make(model, P, P, 19, K, L, seed=P)
    check(engine, model, data, draws, synth.ffbs_uniforms(P, 19, seed=P), "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("K,L", [(12, lds_max_L(12)), (12, 400), (25, lds_max_L(25)), (23, 200)])
def test_gpu_tables_that_shrink_the_workgroup(engine, K, L):
    """The largest L of either group size (one group per workgroup) and an L between (two groups, half a wave, at
    K = 12, L = 400; two, one wave, at K = 23, L = 200)."""
    data, draws = make("hmm-multinom", 3, 3, 19, K, L, seed=L)
    check(engine, "hmm-multinom", data, draws, synth.ffbs_uniforms(3, 19, seed=L), "zip")


@pytest.mark.gpu
def test_gpu_banded_transitions_count_nothing_outside_the_band(engine):
    K = 12
    data, draws = make("hmm-multinom", 3, 4, 41, K, 9, seed=3)
    band = np.abs(np.subtract.outer(np.arange(K), np.arange(K))) <= 2
    draws["A_ij"] = draws["A_ij"] * band
    draws["A_ij"] /= draws["A_ij"].sum(axis=2, keepdims=True)
    got, _r = check(engine, "hmm-multinom", data, draws, synth.ffbs_uniforms(12, 41, seed=4))
    assert all(np.isfinite(got[k]).all() for k in ("loglik", "n_1k", "xi_ij", "c_kl"))
    assert (got["xi_ij"][:, ~band] == 0.0).all() and (got["xi_ij"].sum(axis=(1, 2)) == 40).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 23, 32])
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_uniforms_at_the_ends_of_their_range(engine, model, L, K):
    N, S, T = 2, 10, 21
    data, draws = make(model, N, S, T, K, L, seed=41)
    g = np.random.Generator(np.random.Philox(key=42))
    u = synth.ffbs_uniforms(N * S, T, seed=43)
    pick = g.integers(0, 6, size=u.shape)
    for k in (1, 2, 3):
        u[pick == k] = k * 2.0 ** -1074
    u[pick == 4] = 1.0
    check(engine, model, data, draws, u)


@pytest.mark.gpu
def test_gpu_impossible_observation_is_nan_for_that_pair_only(engine):
    N, S, K, L = 3, 5, 12, 9
    data, draws = make("hmm-multinom", N, S, 27, K, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _r = check(engine, "hmm-multinom", data, draws, synth.ffbs_uniforms(N * S, 27, seed=12))
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf
    for name in ("n_1k", "xi_ij", "c_kl"):
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_nan_draw_is_nan_for_its_pairs_only(engine, model, L):
    N, S, K = 3, 5, 12
    data, draws = make(model, N, S, 20, K, L, seed=13)
    draws["A_ij"][1, 0, 1] = np.nan
    got, _r = check(engine, model, data, draws, synth.ffbs_uniforms(N * S, 20, seed=15))
    hit = np.arange(N * S) % S == 1
    for name in [k for k in got if k not in ("status", "pair_status")]:
        assert np.isnan(got[name][hit]).all() and np.isfinite(got[name][~hit]).all(), name


@pytest.mark.gpu
def test_gpu_device_entry_flags_invalid_data(engine):
    N, S, K, L, T = 5, 3, 12, 9, 21
    data, draws = make("hmm-multinom", N, S, T, K, L, seed=19)
    u = synth.ffbs_uniforms(N * S, T, seed=20)
    want = device_run(device_entry(engine, "hmm-multinom", data, draws, u))
    assert not want["pair_status"].any()
    data["x"][1, 6] = 0
    data["x"][2, 17] = L + 1
    data["T"] = np.array([T, T, T, T, T + 1], dtype=np.int32)
    got = device_run(device_entry(engine, "hmm-multinom", data, draws, u))
    hit = np.isin(np.arange(N * S) // S, [1, 2, 4])
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in ("loglik", "n_1k", "xi_ij", "c_kl"):
        assert np.array_equal(got[name][~hit], want[name][~hit], equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_identities(engine, model, L):
    K, T = 23, 37
    data, draws = make(model, 2, 3, T, K, L, seed=23)
    got, _r = check(engine, model, data, draws, synth.ffbs_uniforms(6, T, seed=24))
    assert (got["n_1k"].sum(axis=1) == 1).all() and (got["xi_ij"].sum(axis=(1, 2)) == T - 1).all()
    if model == "hmm-multinom":
        assert (got["c_kl"].sum(axis=(1, 2)) == T).all()
    else:
        assert (got["w_k"].sum(axis=1) == K + T - 1).all()


def _block_data(model):
    if model == "hmm":
        return {"K": K9, "x": X4G.reshape(1, -1)}
    return {"K": K9, "L": L3, "x": X4.reshape(1, -1)}


def run_gibbs(engine, model, data, init, n_iter, **kw):
    if model == "hmm":
        return hhmm_amd.gibbs_gauss(data, init, n_iter, lib=engine, **kw)
    return hhmm_amd.gibbs(model, data, init, n_iter, lib=engine, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["hmm-multinom", "hmm"])
def test_gpu_gibbs_matches_the_exact_posterior_at_K9(engine, model):
    init, _gen = prior_draw(model, seed=51)
    prior = priors()[1 if model == "hmm" else 0]
    draws, trace = run_gibbs(engine, model, _block_data(model), init, SWEEPS, burn=SWEEPS - 1, prior=prior, seed=53,
                          pairing="block")
    assert trace.shape == (SWEEPS, CHAINS) and np.isfinite(trace).all()
    assert all(v.shape[0] == 1 for v in draws.values())
    w = worst_z(model, {k: v[0] for k, v in draws.items()})
    assert w < ZCAP, (model, w)


@pytest.mark.gpu
@pytest.mark.parametrize("model,L", BOTH)
def test_gpu_gibbs_is_reproducible_at_large_K(engine, model, L):
    data, init = make(model, 5, 5, 11, 12, L, seed=61)
    prior = {"mu_sigma": (0.0, 0.5, 2.0, 1.0)} if model == "hmm" else None
    a, ta = run_gibbs(engine, model, data, init, 6, burn=1, thin=2, prior=prior, seed=7)
    b, tb = run_gibbs(engine, model, data, init, 6, burn=1, thin=2, prior=prior, seed=7)
    c, _tc = run_gibbs(engine, model, data, init, 6, burn=1, thin=2, prior=prior, seed=8)
    assert np.array_equal(ta, tb) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(a[k].shape[:2] == (3, 5) for k in a)                               # sweeps 1, 3, 5
    assert not np.array_equal(a["A_ij"], c["A_ij"])
    # the first sweep starts from init
    ll = hhmm_amd.gqs(model, data, init, pars=["loglik"], pairing="zip", lib=engine)["loglik"]
    assert np.max(np.abs(ta[0] - ll) / np.maximum(1.0, np.abs(ll))) <= TOL
