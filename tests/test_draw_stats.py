"""Draw statistics and the blocked Gibbs sampler (include/hhmm_gibbs.h, hhmm_amd/gibbs.py).

CPU: symbols, the header as C, Python shape checks, the argument checks (they
come before the device check), the reference counts against the oracle's FFBS
path (they must reproduce the path's coded weight), and the sampler built from
the oracle's FFBS + reference counts + conditional_draw against the exact
posterior of a T = 6 series (all K^T paths enumerated, tests/draw_stats_ref.py).

gpu: the kernel's counts must be bit-equal to the reference counts of the path
hhmm_amd.gqs(..., pars=["z_ffbs"]) returns for the same uniforms (the FFBS
contract, pinned bit for bit elsewhere), through the host and the device entry;
loglik to 1e-9 relative to max(1, |v|).  Then hhmm_amd.gibbs against the same
enumeration, under the same cap |z| < 5 that tests/test_ffbs.py uses.

Shapes: C = fb_chunk(K) is 8 at K <= 4 and 4 above; T covers the chunk edges,
P the partial last wave, K and L every template instance class.
"""
import ctypes as C
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import draw_stats_ref as dsr
import hhmm_amd
from hhmm_amd import _abi, synth

REPO = pathlib.Path(__file__).resolve().parent.parent
_gibbs = sys.modules["hhmm_amd.gibbs"]
MODELS = ["hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009"]
COUNTS = ("n_1k", "xi_ij", "c_kl")
TOL = 1e-9
ZCAP = 5.0
INT32_MIN = -2 ** 31


def fb_chunk(K):
    return 8 if K <= 4 else 4


def make(model, N, S, T, K, L, seed=0):
    """Random parameters and series."""
    g = np.random.Generator(np.random.Philox(key=2000 + seed))
    data = {"K": K, "L": L, "x": g.integers(1, L + 1, size=(N, T)).astype(np.int32)}
    if model == "hhmm-tayal2009":
        assert K == 4
        data["sign"] = g.integers(1, 3, size=(N, T)).astype(np.int32)
        draws = {"p_11": g.uniform(0.2, 0.8, size=S), "A_row": g.dirichlet(np.full(2, 2.0), size=(S, 2)),
                 "phi_k": g.dirichlet(np.full(L, 2.0), size=(S, K))}
        return data, draws
    if model == "hmm-multinom-semisup":
        data["g"] = g.integers(1, 4, size=(N, T)).astype(np.int32)
        data["G"] = 3
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K)),
             "phi_k": g.dirichlet(np.full(L, 2.0), size=(S, K))}
    return data, draws


def npairs(data, draws, pairing):
    N, S = np.atleast_2d(data["x"]).shape[0], draws["phi_k"].shape[0]
    return N * S if pairing == "grid" else (N if pairing == "zip" else S)


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ("hhmm_draw_stats", "hhmm_draw_stats_device", "hhmm_draw_stats_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    for name in ("draw_stats", "conditional_draw", "gibbs", "stack_chains"):
        assert callable(getattr(hhmm_amd, name))


def test_header_compiles_as_c(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "hhmm_gibbs.h"\n'
                 "int main(void){ hhmm_request r; hhmm_estep_result o; size_t b = 0; (void)r; (void)o;\n"
                 "  hhmm_status (*f)(const hhmm_request *, hhmm_estep_result *) = hhmm_draw_stats;\n"
                 "  hhmm_status (*g)(const hhmm_request *, size_t *) = hhmm_draw_stats_workspace_size;\n"
                 "  hhmm_status (*h)(const hhmm_request *, hhmm_estep_result *, void *, size_t, void *) = "
                 "hhmm_draw_stats_device;\n"
                 "  return (f && g && h && HHMM_ABI_VERSION == 2) ? (int)b : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(REPO / "include"), "-c", str(c),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_python_shape_checks():
    data, draws = make("hmm-multinom", 3, 5, 6, 4, 9)
    u = synth.ffbs_uniforms(15, 6)
    pr, _res, out = _gibbs.prepare("hmm-multinom", data, draws, u, "grid")
    assert pr.P == 15 and pr.req.ffbs_u
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "n_1k": (15, 4), "xi_ij": (15, 4, 4),
                                                     "c_kl": (15, 4, 9)}
    td, tw = make("hhmm-tayal2009", 6, 6, 5, 4, 3)
    _pr, _res, out = _gibbs.prepare("hhmm-tayal2009", td, tw, synth.ffbs_uniforms(6, 5), "zip")
    assert out["c_kl"].shape == (6, 4, 3)
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm", data, draws, u)
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm-multinom", data, draws, u[:5], "zip")                  # N != S
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm-multinom", data, draws, u[:5], "block")                # S % N
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm-multinom", data, dict(draws, phi_k=draws["phi_k"][:, :, :8]), u)
    with pytest.raises(ValueError):
        _gibbs.prepare("hhmm-tayal2009", td, {k: v for k, v in tw.items() if k != "A_row"},
                       synth.ffbs_uniforms(6, 5), "zip")
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm-multinom", data, draws, None)
    with pytest.raises(ValueError):
        _gibbs.prepare("hmm-multinom", data, draws, u[:, :5])
    with pytest.raises(ValueError):
        hhmm_amd.gibbs("hmm-multinom", data, draws, 1, pairing="grid")


def test_stack_chains_layout():
    n_keep, N, B = 3, 2, 4
    v = np.arange(n_keep * N * B * 5, dtype=float).reshape(n_keep, N * B, 5)
    out = hhmm_amd.stack_chains({"phi": v}, N)["phi"]
    assert out.shape == (N * n_keep * B, 5)
    S = n_keep * B
    for n in range(N):
        for k in range(n_keep):
            for b in range(B):
                assert np.array_equal(out[S * n + k * B + b], v[k, b + B * n])
    with pytest.raises(ValueError):
        hhmm_amd.stack_chains({"phi": v}, 3)


def test_conditional_draw_keeps_nan_and_structure():
    import torch
    gen = torch.Generator().manual_seed(3)
    stats = {"n_1k": np.zeros((5, 4)), "xi_ij": np.ones((5, 4, 4)), "c_kl": np.ones((5, 4, 3))}
    for v in stats.values():
        v[2] = np.nan
    for model in MODELS:
        new = hhmm_amd.conditional_draw(model, stats, None, gen)
        assert set(new) == set(_gibbs.param_shapes(model, 5, 4, 3))
        for name, t in new.items():
            t = t.numpy()
            assert t.shape == _gibbs.param_shapes(model, 5, 4, 3)[name], name
            assert np.isnan(t[2]).all() and np.isfinite(np.delete(t, 2, axis=0)).all(), name
            if name != "p_11":
                assert np.allclose(np.delete(t, 2, axis=0).sum(axis=-1), 1.0, rtol=0, atol=1e-12), name
    # a strong prior pins the draw: Dir(1e8 * m) is m to ~1e-4
    m = np.array([0.7, 0.2, 0.1])
    new = hhmm_amd.conditional_draw("hmm-multinom", {k: np.zeros_like(v) for k, v in stats.items()},
                                    {"phi_k": 1e8 * m}, gen)
    assert np.abs(new["phi_k"].numpy() - m).max() < 1e-3


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
    "model_tayal_lite": ("hhmm-tayal2009", 4, 9, _poke("model", 9), _abi.ERR_UNSUPPORTED, "model"),
    "K9": ("hmm-multinom", 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "K9_semisup": ("hmm-multinom-semisup", 4, 9, _poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": ("hhmm-tayal2009", 4, 9, _poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "lds_K8": ("hmm-multinom", 8, 25, _same, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_K7": ("hmm-multinom-semisup", 7, 26, _same, _abi.ERR_UNSUPPORTED, "LDS"),
    "lds_tayal": ("hhmm-tayal2009", 4, 53, _same, _abi.ERR_UNSUPPORTED, "LDS"),
    "no_uniforms": ("hmm-multinom", 4, 9, _poke("ffbs_u", None), _abi.ERR_INVALID_ARGUMENT, "ffbs_u"),
    "null_loglik": ("hmm-multinom", 4, 9, _null("loglik"), _abi.ERR_INVALID_ARGUMENT, "loglik"),
    "null_n_1k": ("hmm-multinom-semisup", 4, 9, _null("n_1k"), _abi.ERR_INVALID_ARGUMENT, "n_1k"),
    "null_xi": ("hhmm-tayal2009", 4, 9, _null("xi_ij"), _abi.ERR_INVALID_ARGUMENT, "xi_ij"),
    "null_c_kl": ("hmm-multinom", 4, 9, _null("c_kl"), _abi.ERR_INVALID_ARGUMENT, "c_kl"),
    "abi": ("hmm-multinom", 4, 9, _poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    model, K, L, change, status, word = BAD[case]
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _gibbs.prepare(model, data, draws, synth.ffbs_uniforms(4, 5), "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_draw_stats(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_draw_stats_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_host_entry_rejects_symbols_outside_the_data_block(engine, bad):
    data, draws = make("hmm-multinom-semisup", 2, 2, 5, 4, 9)
    u = synth.ffbs_uniforms(4, 5)
    data["x"][1, 3] = bad
    pr, res, _out = _gibbs.prepare("hmm-multinom-semisup", data, draws, u)
    assert engine.hhmm_draw_stats(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "x[1, 4]" in engine.hhmm_last_error().decode()
    data["x"][1, 3] = 1
    data["g"][0, 2] = 4                                                            # g outside 1..G
    pr, res, _out = _gibbs.prepare("hmm-multinom-semisup", data, draws, u)
    assert engine.hhmm_draw_stats(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT
    assert "g[0, 3]" in engine.hhmm_last_error().decode()


# the largest accepted tables: L * (4 * ceil(K / 2) + K) + K * K = 640
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 8, 24), ("hmm-multinom-semisup", 5, 36),
                                       ("hhmm-tayal2009", 4, 52)])
def test_good_request_passes_the_argument_checks(engine, model, K, L):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK."""
    data, draws = make(model, 2, 2, 5, K, L)
    pr, res, _out = _gibbs.prepare(model, data, draws, synth.ffbs_uniforms(4, 5))
    st = engine.hhmm_draw_stats(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws, es = C.c_size_t(0), C.c_size_t(1)
    assert engine.hhmm_draw_stats_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-5 // fb_chunk(K)) * K * 4 * 8                            # the checkpoints
    if model == "hmm-multinom" and L == 9:
        assert engine.hhmm_estep_workspace_size(C.byref(pr.req), C.byref(es)) == 0 and es.value == ws.value


def _expand(model, d):
    if model == "hhmm-tayal2009":
        return dsr.tayal_expand(float(d["p_11"]), d["A_row"])
    return d["p_1k"], d["A_ij"]


@pytest.mark.parametrize("model", MODELS)
def test_reference_counts_reproduce_the_weight_of_the_oracles_path(oracle, model):
    """n1 . log p + xi . log A + c . log phi == the path's coded log-weight: pins the masked definitions."""
    N, S, T, K, L = 3, 4, 23, 4, 5
    data, draws = make(model, N, S, T, K, L, seed=5)
    data["T"] = np.array([T, 9, 1], dtype=np.int32)
    u = synth.ffbs_uniforms(N * S, T, seed=6)
    out = oracle.gqs(model, data, draws, pars=["z_ffbs", "loglik"], uniforms=u)
    z = out["z_ffbs"]
    st = dsr.counts_pairs(model, data, z, out["loglik"], "grid", S)
    aux = data.get("g", data.get("sign"))
    seen = 0
    for p in range(N * S):
        n, s = p // S, p % S
        Tn = int(data["T"][n])
        if np.isnan(st["n_1k"][p]).any():
            continue
        seen += 1
        d = {k: np.asarray(v)[s] for k, v in draws.items()}
        pv, A = _expand(model, d)
        direct = dsr.log_weight(model, z[p, :Tn], data["x"][n, :Tn], None if aux is None else aux[n, :Tn], pv, A,
                                d["phi_k"])
        via = 0.0
        for cnt, par in ((st["n_1k"][p], np.asarray(pv)), (st["xi_ij"][p], np.asarray(A)), (st["c_kl"][p], d["phi_k"])):
            used = cnt > 0
            via += float((cnt[used] * np.log(par[used])).sum())
        assert np.isfinite(direct) and abs(via - direct) <= 1e-12 * max(1.0, abs(direct)), (p, via, direct)
        assert st["c_kl"][p].sum() == Tn and st["xi_ij"][p].sum() <= Tn - 1 and st["n_1k"][p].sum() <= 1
        if model == "hmm-multinom":
            assert st["xi_ij"][p].sum() == Tn - 1 and st["n_1k"][p].sum() == 1
        # the vectorised form the samplers below use
        v = dsr.counts_chains(model, K, L, z[p:p + 1, :Tn], data["x"][n, :Tn], None if aux is None else aux[n, :Tn])
        assert all(np.array_equal(a[0], st[k][p]) for a, k in zip(v, COUNTS))
    assert seen >= N * S // 2


# ---- the exact posterior of a T = 6 series, and the samplers against it

CHAINS, SWEEPS = 4096, 40
X6 = np.array([1, 3, 2, 2, 1, 3], dtype=np.int32)
# hmm-multinom and semisup: phi row k ~ Dir(1 + 4 e_k) -- under the flat prior every mean is 1/2 (1/K) by
# label symmetry and the comparison shows nothing; Tayal's structure breaks the symmetry by itself
EXACT = {
    "hmm-multinom": dict(K=2, L=3, aux=None, prior={"phi_k": 1.0 + 4.0 * np.eye(2, 3)}),
    "hmm-multinom-semisup": dict(K=4, L=3, aux=np.array([1, 2, 3, 1, 2, 2], dtype=np.int32),
                                 prior={"phi_k": 1.0 + 4.0 * np.eye(4, 3)}),
    "hhmm-tayal2009": dict(K=4, L=3, aux=np.array([1, 2, 1, 1, 2, 1], dtype=np.int32), prior=None),
}


@functools.lru_cache(maxsize=None)
def exact_means(model):
    """Computed once, shared by the CPU and the GPU sampler tests."""
    e = EXACT[model]
    means = dsr.posterior_means(model, e["K"], e["L"], X6, e["aux"], e["prior"])
    for v in means.values():
        v.setflags(write=False)
    return means


def exact_data(model):
    e = EXACT[model]
    data = {"K": e["K"], "L": e["L"], "x": X6.reshape(1, -1)}
    if model == "hmm-multinom-semisup":
        data.update(g=e["aux"].reshape(1, -1), G=3)
    if model == "hhmm-tayal2009":
        data["sign"] = e["aux"].reshape(1, -1)
    return data


def prior_draw(model, seed):
    """CHAINS starts from the prior (conditional_draw on empty statistics)."""
    import torch
    e = EXACT[model]
    zero = {"n_1k": np.zeros((CHAINS, e["K"])), "xi_ij": np.zeros((CHAINS, e["K"], e["K"])),
            "c_kl": np.zeros((CHAINS, e["K"], e["L"]))}
    gen = torch.Generator().manual_seed(seed)
    return {k: v.numpy() for k, v in hhmm_amd.conditional_draw(model, zero, e["prior"], gen).items()}, gen


def worst_z(model, final):
    """max |z-score| of the across-chain mean of the final draw against the exact posterior mean; final draws
    of independent chains are iid, so the standard error is the sample sd over chains / sqrt(chains)."""
    worst = 0.0
    for name, want in exact_means(model).items():
        v = np.asarray(final[name], dtype=float)
        assert v.shape == (CHAINS,) + want.shape, (name, v.shape)
        se = v.std(axis=0, ddof=1) / np.sqrt(CHAINS)
        z = np.abs(v.mean(axis=0) - want) / se
        print(model, name, "max |z| =", float(z.max()))
        worst = max(worst, float(z.max()))
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_cpu_sampler_matches_the_exact_posterior(oracle, model):
    e, data = EXACT[model], exact_data(model)
    params, gen = prior_draw(model, seed=41)
    ug = np.random.Generator(np.random.Philox(key=43))
    for _ in range(SWEEPS):
        u = 1.0 - ug.random((CHAINS, X6.size))
        z = oracle.gqs(model, data, params, pars=["z_ffbs"], pairing="block", uniforms=u, nthreads=8)["z_ffbs"]
        assert z.min() >= 1
        n1, xi, c = dsr.counts_chains(model, e["K"], e["L"], z, X6, e["aux"])
        new = hhmm_amd.conditional_draw(model, {"n_1k": n1, "xi_ij": xi, "c_kl": c}, e["prior"], gen)
        params = {k: v.numpy() for k, v in new.items()}
    w = worst_z(model, params)
    assert w < ZCAP, (model, w)


# ---------------------------------------------------------------- GPU

def compare(got, want, ref_loglik, tag):
    for name in COUNTS:
        assert got[name].shape == want[name].shape, (tag, name)
        assert np.array_equal(got[name], want[name], equal_nan=True), (tag, name)
    ll = got["loglik"]
    fin = np.isfinite(ref_loglik)
    assert np.array_equal(np.isnan(ll), np.isnan(ref_loglik)), tag
    assert np.array_equal(ll[~fin & ~np.isnan(ref_loglik)], ref_loglik[~fin & ~np.isnan(ref_loglik)]), tag
    if fin.any():
        w = float(np.max(np.abs(ll[fin] - ref_loglik[fin]) / np.maximum(1.0, np.abs(ref_loglik[fin]))))
        assert w <= TOL, (tag, w)


def check(engine, model, data, draws, u, pairing="grid"):
    """Host and device entries against the reference counts of the engine's own z_ffbs (the bit-exact path)."""
    from stats_devrun import DeviceDrawStats
    ref = hhmm_amd.gqs(model, data, draws, pars=["z_ffbs", "loglik"], pairing=pairing, uniforms=u, lib=engine)
    want = dsr.counts_pairs(model, data, ref["z_ffbs"], ref["loglik"], pairing, draws["phi_k"].shape[0])
    host = hhmm_amd.draw_stats(model, data, draws, u, pairing, lib=engine, return_status=True)
    assert host["status"] == 0 and not host["pair_status"].any()
    compare(host, want, ref["loglik"], (model, pairing, "host"))
    dv = DeviceDrawStats(engine, model, data, draws, u, pairing)
    assert dv.run() == 0
    dev = dv.stats()
    assert not dev["pair_status"].any()
    compare(dev, want, ref["loglik"], (model, pairing, "device"))
    return host, ref


KL = [(m, K, L) for m in MODELS[:2] for K in (1, 2, 3, 4, 5, 8) for L in (1, 2, 9, 16)] + \
     [("hhmm-tayal2009", 4, L) for L in (1, 2, 9, 16)] + \
     [("hmm-multinom", 8, 24), ("hmm-multinom-semisup", 7, 25), ("hmm-multinom", 1, 127), ("hhmm-tayal2009", 4, 52)]


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", KL)
def test_gpu_counts_every_K_and_L(engine, model, K, L):
    data, draws = make(model, 3, 5, 2 * fb_chunk(K) + 1, K, L, seed=K * 100 + L)
    check(engine, model, data, draws, synth.ffbs_uniforms(15, 2 * fb_chunk(K) + 1, seed=L))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom", 5, 3), ("hmm-multinom-semisup", 4, 9),
                                       ("hmm-multinom-semisup", 6, 2), ("hhmm-tayal2009", 4, 9)])
@pytest.mark.parametrize("Tsel", ["1", "2", "C-1", "C", "C+1", "2C+1"])
def test_gpu_chunk_edges_in_T(engine, model, K, L, Tsel):
    c = fb_chunk(K)
    T = {"1": 1, "2": 2, "C-1": c - 1, "C": c, "C+1": c + 1, "2C+1": 2 * c + 1}[Tsel]
    data, draws = make(model, 2, 3, T, K, L, seed=T)
    got, _ref = check(engine, model, data, draws, synth.ffbs_uniforms(6, T, seed=T))
    ok = ~np.isnan(got["n_1k"]).any(axis=1)
    assert ok.any() and (got["c_kl"][ok].sum(axis=(1, 2)) == T).all()
    if T == 1:
        assert not got["xi_ij"][ok].any()


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom-semisup", 6, 4), ("hhmm-tayal2009", 4, 5)])
def test_gpu_ragged_lengths_inside_one_wave(engine, model, K, L):
    c = fb_chunk(K)
    Tmax = 2 * c + 1
    lens = np.array([1, Tmax, 2, c, c + 1, Tmax, 1, c - 1] * 3, dtype=np.int32)
    N = lens.size
    data, draws = make(model, N, 2, Tmax, K, L, seed=7)
    for n in range(N):  # padding rows must not matter: garbage symbols
        data["x"][n, lens[n]:] = L + 5
    data["T"] = lens
    check(engine, model, data, draws, synth.ffbs_uniforms(2 * N, Tmax, seed=8))


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 4, 9), ("hmm-multinom-semisup", 5, 3), ("hhmm-tayal2009", 4, 9)])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 300])
def test_gpu_partial_last_wave(engine, model, K, L, P):
    data, draws = make(model, P, P, 11, K, L, seed=P)
    check(engine, model, data, draws, synth.ffbs_uniforms(P, 11, seed=P), "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("model,K,L", [("hmm-multinom", 3, 5), ("hmm-multinom-semisup", 4, 3), ("hhmm-tayal2009", 4, 4)])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, model, K, L, pairing, N, S):
    data, draws = make(model, N, S, 13, K, L, seed=N * S)
    check(engine, model, data, draws, synth.ffbs_uniforms(npairs(data, draws, pairing), 13, seed=S), pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["all1", "all2", "alt1", "alt2", "mixed"])
def test_gpu_tayal_sign_patterns(engine, pattern):
    """One sign per step over the whole wave (tayal_dispatch's sign-class path) and a mixed wave (the masks
    per lane); sign_1 both ways."""
    N, S, T = 2, 70, 19
    data, draws = make("hhmm-tayal2009", N, S, T, 4, 5, seed=31)
    t = np.arange(T)
    if pattern != "mixed":
        row = {"all1": np.ones(T), "all2": np.full(T, 2), "alt1": 1 + t % 2, "alt2": 2 - t % 2}[pattern]
        data["sign"] = np.tile(row.astype(np.int32), (N, 1))
        check(engine, "hhmm-tayal2009", data, draws, synth.ffbs_uniforms(N * S, T, seed=32))
    else:
        data, draws = make("hhmm-tayal2009", 140, 140, T, 4, 5, seed=33)
        data["sign"][::2, 0] = 1
        data["sign"][1::2, 0] = 2
        check(engine, "hhmm-tayal2009", data, draws, synth.ffbs_uniforms(140, T, seed=34), "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1, 2, 3, "mixed"])
@pytest.mark.parametrize("K", [4, 5])
def test_gpu_semisup_groups(engine, g, K):
    data, draws = make("hmm-multinom-semisup", 3, 30, 19, K, 4, seed=37)
    if g != "mixed":
        data["g"][:] = g
    got, _ref = check(engine, "hmm-multinom-semisup", data, draws, synth.ffbs_uniforms(90, 19, seed=38))
    if g == 3:  # no transition is ever applied
        assert not got["xi_ij"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_uniforms_at_the_ends_of_their_range(engine, model):
    N, S, T = 2, 40, 21
    data, draws = make(model, N, S, T, 4, 6, seed=41)
    g = np.random.Generator(np.random.Philox(key=42))
    u = synth.ffbs_uniforms(N * S, T, seed=43)
    pick = g.integers(0, 6, size=u.shape)
    for k in (1, 2, 3):
        u[pick == k] = k * 2.0 ** -1074
    u[pick == 4] = 1.0
    check(engine, model, data, draws, u)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_zero_emission_on_an_observed_symbol(engine, model):
    N, S, T, L = 3, 20, 17, 5
    data, draws = make(model, N, S, T, 4, L, seed=45)
    data["x"][:, 3] = 2
    draws["phi_k"][:, 1, 1] = 0.0                      # state 2 never emits symbol 2 ...
    draws["phi_k"] /= draws["phi_k"].sum(axis=2, keepdims=True)
    got, _ref = check(engine, model, data, draws, synth.ffbs_uniforms(N * S, T, seed=46))
    ok = ~np.isnan(got["n_1k"]).any(axis=1)
    assert ok.any() and not got["c_kl"][ok][:, 1, 1].any()   # ... so no path passes through it there


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS[:2])
def test_gpu_impossible_series_is_nan_for_that_pair_only(engine, model):
    N, S, L = 3, 5, 9
    data, draws = make(model, N, S, 17, 4, L, seed=11)
    x = data["x"]
    x[x == L] = 1
    x[1, 9] = L                              # only series 1 shows symbol L ...
    draws["phi_k"][2, :, L - 1] = 0.0        # ... which no state of draw 2 emits
    draws["phi_k"][2] /= draws["phi_k"][2].sum(axis=1, keepdims=True)
    got, _ref = check(engine, model, data, draws, synth.ffbs_uniforms(N * S, 17, seed=12))
    p = 2 + S * 1
    assert got["loglik"][p] == -np.inf
    for name in COUNTS:
        assert np.isnan(got[name][p]).all()
        assert np.isfinite(np.delete(got[name], p, axis=0)).all()
    assert np.isfinite(np.delete(got["loglik"], p)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_nan_draw_is_nan_for_its_pairs_only(engine, model):
    N, S = 3, 5
    data, draws = make(model, N, S, 20, 4, 9, seed=13)
    data["x"][:] = np.random.Generator(np.random.Philox(key=14)).integers(1, 10, size=(N, 20))
    if model == "hhmm-tayal2009":
        data["sign"][:] = 2                  # every series possible: columns 1 and 4 take A, 2 and 3 the total
        draws["p_11"][1] = np.nan
    else:
        draws["A_ij"][1, 0, 1] = np.nan
    got, _ref = check(engine, model, data, draws, synth.ffbs_uniforms(N * S, 20, seed=15))
    hit = np.arange(N * S) % S == 1
    for name in COUNTS + ("loglik",):
        assert np.isnan(got[name][hit]).all() and np.isfinite(got[name][~hit]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [10, 0, INT32_MIN])
def test_gpu_device_entry_flags_invalid_data(engine, bad):
    from stats_devrun import DeviceDrawStats
    N, S, L = 4, 20, 9
    data, draws = make("hmm-multinom-semisup", N, S, 15, 4, L, seed=19)
    u = synth.ffbs_uniforms(N * S, 15, seed=20)
    clean = DeviceDrawStats(engine, "hmm-multinom-semisup", data, draws, u)
    assert clean.run() == 0
    want = clean.stats()
    data["x"][2, 6] = bad
    dv = DeviceDrawStats(engine, "hmm-multinom-semisup", data, draws, u)
    assert dv.run() == 0
    got = dv.stats()
    hit = np.arange(N * S) // S == 2
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in COUNTS + ("loglik",):
        assert np.array_equal(got[name][~hit], want[name][~hit], equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_gibbs_matches_the_exact_posterior(engine, model):
    init, _gen = prior_draw(model, seed=51)
    draws, trace = hhmm_amd.gibbs(model, exact_data(model), init, SWEEPS, burn=SWEEPS - 1, prior=EXACT[model]["prior"],
                                  seed=53, pairing="block", lib=engine)
    assert trace.shape == (SWEEPS, CHAINS) and np.isfinite(trace).all()
    final = {k: v[0] for k, v in draws.items()}
    assert all(v.shape[0] == 1 for v in draws.values())
    w = worst_z(model, final)
    assert w < ZCAP, (model, w)


@pytest.mark.gpu
def test_gpu_gibbs_is_reproducible(engine):
    data, init = make("hmm-multinom-semisup", 5, 5, 11, 4, 3, seed=61)
    a, ta = hhmm_amd.gibbs("hmm-multinom-semisup", data, init, 6, burn=1, thin=2, seed=7, lib=engine)
    b, tb = hhmm_amd.gibbs("hmm-multinom-semisup", data, init, 6, burn=1, thin=2, seed=7, lib=engine)
    c, _tc = hhmm_amd.gibbs("hmm-multinom-semisup", data, init, 6, burn=1, thin=2, seed=8, lib=engine)
    assert np.array_equal(ta, tb) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(a[k].shape[:2] == (3, 5) for k in a)                               # sweeps 1, 3, 5
    assert not np.array_equal(a["phi_k"], c["phi_k"])
    # the first sweep starts from init
    ll = hhmm_amd.gqs("hmm-multinom-semisup", data, init, pars=["loglik"], pairing="zip", lib=engine)["loglik"]
    assert np.max(np.abs(ta[0] - ll) / np.maximum(1.0, np.abs(ll))) <= TOL


@pytest.mark.gpu
def test_gpu_gibbs_to_gqs_end_to_end(engine):
    """gibbs on two short series -> stack_chains -> gqs(block): shapes agree, no pair carries a status."""
    N, B, T = 2, 8, 14
    data, init = make("hhmm-tayal2009", N, N * B, T, 4, 5, seed=71)
    data["sign"] = np.tile(1 + np.arange(T) % 2, (N, 1)).astype(np.int32)
    data["T"] = np.array([T, 9], dtype=np.int32)
    draws, trace = hhmm_amd.gibbs("hhmm-tayal2009", data, init, 6, burn=2, thin=2, seed=3, pairing="block", lib=engine)
    assert trace.shape == (6, N * B) and draws["phi_k"].shape == (2, N * B, 4, 5)
    stacked = hhmm_amd.stack_chains(draws, N)
    S = 2 * B
    assert stacked["p_11"].shape == (N * S,) and stacked["A_row"].shape == (N * S, 2, 2)
    out = hhmm_amd.gqs("hhmm-tayal2009", data, stacked, pars=["loglik", "gamma_tk", "zstar_t"], pairing="block",
                       lib=engine, return_status=True)
    assert out["status"] == 0 and not out["pair_status"].any()
    assert out["loglik"].shape == (N * S,) and out["gamma_tk"].shape == (N * S, T, 4)
    assert np.isfinite(out["loglik"]).all()
    summ = hhmm_amd.gqs_summary("hhmm-tayal2009", data, stacked, pars=["gamma_tk"], pairing="block", lib=engine)
    assert summ["gamma_tk"].shape == (N, T, 4, 3) and not summ["pair_status"].any()
