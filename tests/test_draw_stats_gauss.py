"""Gaussian draw statistics and the blocked Gibbs sampler of hmm.stan
(include/hhmm_gibbs_gauss.h, hhmm_amd/gibbs_gauss.py).

CPU: symbols, the header as C, Python shape checks, the argument checks (they
come before the device check), the reference statistics against the oracle's
FFBS path (they must reproduce the path's coded weight through the closed form),
conditional_draw_gauss against the Normal-Inverse-Gamma moments, relabel_ordered,
and the sampler built from the oracle's FFBS + reference statistics +
conditional_draw_gauss against the exact posterior of a T = 6 series (all K^T
paths enumerated, tests/draw_stats_gauss_ref.py).

gpu: the kernel against the reference statistics of the path
hhmm_amd.gqs("hmm", ..., pars=["z_ffbs"]) returns for the same uniforms: n_1k,
xi_ij and w_k with ==, loglik to 1e-9 relative to max(1, |v|), s1_k within
T 2^-52 sum|x_t| and s2_k within T 2^-52 sum x_t^2 -- the first-order bound of
T sequential fp64 additions in any order, doubled (it covers an FMA or a
product-then-add for x^2).  Then hhmm_amd.gibbs_gauss against the same
enumeration under the cap |z| < 5 of tests/test_draw_stats.py and test_ffbs.py.

Shapes: C = fb_chunk(K) is 8 at K <= 4 and 4 above; T covers the chunk edges and
the grouped forward loop, P the partial last wave, K every template instance.
"""
import ctypes as C
import functools
import math
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import draw_stats_gauss_ref as ref
import estep_ref
import hhmm_amd
from hhmm_amd import _abi, synth

REPO = pathlib.Path(__file__).resolve().parent.parent
_gg = sys.modules["hhmm_amd.gibbs_gauss"]
COUNTS = ("n_1k", "xi_ij", "w_k")
TOL = 1e-9
ZCAP = 5.0
K_FWD_GROUP = 4


def fb_chunk(K):
    return 8 if K <= 4 else 4


def make(N, S, T, K, seed=0):
    """Random parameters and series: overlapping states, so the paths vary with the uniforms."""
    g = np.random.Generator(np.random.Philox(key=3000 + seed))
    mu = 1.5 * np.arange(K) - 0.75 * (K - 1)
    zs = g.integers(0, K, size=(N, T))
    data = {"K": K, "x": mu[zs] + g.normal(0.0, 1.0, size=(N, T))}
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K)),
             "mu_k": mu[None, :] + g.normal(0.0, 0.3, size=(S, K)), "sigma_k": g.uniform(0.6, 1.6, size=(S, K))}
    return data, draws


def npairs(data, draws, pairing):
    N, S = np.atleast_2d(data["x"]).shape[0], draws["mu_k"].shape[0]
    return N * S if pairing == "grid" else (N if pairing == "zip" else S)


# ---------------------------------------------------------------- CPU

def test_symbols_load(engine):
    for name in ("hhmm_draw_stats_gauss", "hhmm_draw_stats_gauss_device", "hhmm_draw_stats_gauss_workspace_size"):
        assert getattr(engine, name).restype is C.c_int
    for name in ("draw_stats_gauss", "conditional_draw_gauss", "gibbs_gauss", "relabel_ordered"):
        assert callable(getattr(hhmm_amd, name))
    assert _gg.stack_chains is hhmm_amd.stack_chains


def test_header_compiles_as_c(tmp_path):
    c = tmp_path / "use.c"
    c.write_text('#include "hhmm_gibbs_gauss.h"\n'
                 "int main(void){ hhmm_request r; hhmm_estep_result o; size_t b = 0; (void)r; (void)o;\n"
                 "  hhmm_status (*f)(const hhmm_request *, hhmm_estep_result *) = hhmm_draw_stats_gauss;\n"
                 "  hhmm_status (*g)(const hhmm_request *, size_t *) = hhmm_draw_stats_gauss_workspace_size;\n"
                 "  hhmm_status (*h)(const hhmm_request *, hhmm_estep_result *, void *, size_t, void *) = "
                 "hhmm_draw_stats_gauss_device;\n"
                 "  return (f && g && h && HHMM_ABI_VERSION == 2) ? (int)b : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(REPO / "include"), "-c", str(c),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_python_shape_checks():
    data, draws = make(3, 5, 6, 4)
    u = synth.ffbs_uniforms(15, 6)
    pr, _res, out = _gg.prepare(data, draws, u, "grid")
    assert pr.P == 15 and pr.req.ffbs_u and pr.req.model == 1
    assert {k: v.shape for k, v in out.items()} == {"loglik": (15,), "n_1k": (15, 4), "xi_ij": (15, 4, 4),
                                                     "w_k": (15, 4), "s1_k": (15, 4), "s2_k": (15, 4)}
    with pytest.raises(ValueError):
        _gg.prepare(data, draws, u[:5], "zip")                                     # N != S
    with pytest.raises(ValueError):
        _gg.prepare(data, draws, u[:5], "block")                                   # S % N
    with pytest.raises(ValueError):
        _gg.prepare(data, dict(draws, mu_k=draws["mu_k"][:, :3]), u)
    with pytest.raises(ValueError):
        _gg.prepare(data, {k: v for k, v in draws.items() if k != "sigma_k"}, u)
    with pytest.raises(ValueError):
        _gg.prepare(data, draws, None)
    with pytest.raises(ValueError):
        _gg.prepare(data, draws, u[:, :5])
    prior = {"mu_sigma": (0.0, 1.0, 3.0, 2.0)}
    with pytest.raises(ValueError):
        hhmm_amd.gibbs_gauss(data, draws, 1, prior=prior, pairing="grid")
    with pytest.raises(ValueError):
        hhmm_amd.gibbs_gauss(data, draws, 0, prior=prior, pairing="block")


def test_existing_entries_still_refuse_the_gaussian_hmm(engine):
    data, draws = make(2, 2, 5, 3)
    with pytest.raises(ValueError):
        sys.modules["hhmm_amd.gibbs"].prepare("hmm", data, draws, synth.ffbs_uniforms(4, 5))
    assert "hmm" not in sys.modules["hhmm_amd.gibbs"].MODELS


def _poke(field, value):
    def f(pr, res):
        obj, name = (pr.req, field) if "." not in field else (getattr(pr.req, field.split(".")[0]), field.split(".")[1])
        setattr(obj, name, value)
    return f


def _null(field):
    def f(pr, res):
        setattr(res, field, None)
    return f


# name -> (change to the prepared request, expected status, word of the message)
BAD = {f"model_{m}": (_poke("model", m), _abi.ERR_UNSUPPORTED, "model") for m in range(2, 10)}
BAD.update({
    "K9": (_poke("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": (_poke("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
    "no_uniforms": (_poke("ffbs_u", None), _abi.ERR_INVALID_ARGUMENT, "ffbs_u"),
    "abi": (_poke("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
})
BAD.update({f"null_{f}": (_null(f), _abi.ERR_INVALID_ARGUMENT, f)
            for f in ("loglik", "n_1k", "xi_ij", "w_k", "s1_k", "s2_k")})


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    change, status, word = BAD[case]
    data, draws = make(2, 2, 5, 4)
    pr, res, _out = _gg.prepare(data, draws, synth.ffbs_uniforms(4, 5), "grid")
    change(pr, res)
    if entry == "host":
        st = engine.hhmm_draw_stats_gauss(C.byref(pr.req), C.byref(res))
    else:  # rejected before any pointer is used
        st = engine.hhmm_draw_stats_gauss_device(C.byref(pr.req), C.byref(res), None, 0, None)
    msg = engine.hhmm_last_error().decode()
    assert st == status and word in msg, (case, entry, st, msg)


@pytest.mark.parametrize("K", [1, 4, 8])
def test_good_request_passes_the_argument_checks(engine, K):
    """No GPU: NO_DEVICE (there is no CPU path); with one: OK.  c_kl is ignored, pair_status optional."""
    data, draws = make(2, 2, 5, K)
    pr, res, _out = _gg.prepare(data, draws, synth.ffbs_uniforms(4, 5))
    res.c_kl = None
    res.pair_status = None
    st = engine.hhmm_draw_stats_gauss(C.byref(pr.req), C.byref(res))
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), engine.hhmm_last_error().decode()
    ws, es = C.c_size_t(0), C.c_size_t(1)
    assert engine.hhmm_draw_stats_gauss_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
    assert ws.value == -(-5 // fb_chunk(K)) * K * 4 * 8                            # the checkpoints
    assert engine.hhmm_estep_workspace_size(C.byref(pr.req), C.byref(es)) == 0 and es.value == ws.value


def test_draw_stats_still_refuses_model_1_and_names_the_model(engine):
    data, draws = make(2, 2, 5, 4)
    pr, res, _out = _gg.prepare(data, draws, synth.ffbs_uniforms(4, 5))
    assert engine.hhmm_draw_stats(C.byref(pr.req), C.byref(res)) == _abi.ERR_UNSUPPORTED
    assert "model" in engine.hhmm_last_error().decode()


def test_reference_statistics_reproduce_the_weight_of_the_oracles_path(oracle):
    """The closed form in (n1, xi, w, s1, s2) == the path's coded log-weight, step by step: pins Q2."""
    N, S, T, K = 3, 4, 23, 3
    data, draws = synth.hmm_gauss(N=N, S=S, T=T, K=K, seed=5)
    data["T"] = np.array([T, 9, 1], dtype=np.int32)
    u = synth.ffbs_uniforms(N * S, T, seed=6)
    out = oracle.gqs("hmm", data, draws, pars=["z_ffbs", "loglik"], uniforms=u)
    z = out["z_ffbs"]
    st = ref.stats_pairs(data, z, out["loglik"], "grid", S)
    seen = 0
    for p in range(N * S):
        n, s = p // S, p % S
        Tn = int(data["T"][n])
        if np.isnan(st["n_1k"][p]).any():
            continue
        seen += 1
        d = {k: np.asarray(v)[s] for k, v in draws.items()}
        direct = ref.log_weight(z[p, :Tn], data["x"][n, :Tn], d["p_1k"], d["A_ij"], d["mu_k"], d["sigma_k"])
        via = ref.log_weight_stats(*(st[k][p] for k in ref.NAMES), d["p_1k"], d["A_ij"], d["mu_k"], d["sigma_k"])
        assert np.isfinite(direct) and abs(via - direct) <= 1e-12 * max(1.0, abs(direct)), (p, via, direct)
        assert st["w_k"][p].sum() == K + Tn - 1 and st["xi_ij"][p].sum() == Tn - 1 and st["n_1k"][p].sum() == 1
        v = ref.stats_chains(z[p:p + 1, :Tn], data["x"][n, :Tn], K)
        for a, k in zip(v, ref.NAMES):
            assert np.allclose(a[0], st[k][p], rtol=1e-14, atol=0), k
    assert seen == N * S


# ---- conditional_draw_gauss

PRIOR = {"mu_sigma": (0.5, 2.0, 3.0, 1.5)}


def _stats_rows(P, K=2):
    return {"n_1k": np.tile([1.0, 0.0], (P, 1)), "xi_ij": np.tile([[2.0, 1.0], [1.0, 3.0]], (P, 1, 1)),
            "w_k": np.tile([4.0, 5.0], (P, 1)), "s1_k": np.tile([-2.0, 6.0], (P, 1)),
            "s2_k": np.tile([3.5, 9.0], (P, 1))}


def test_conditional_draw_gauss_keeps_nan_and_checks_the_prior():
    import torch
    gen = torch.Generator().manual_seed(3)
    stats = _stats_rows(5)
    for v in stats.values():
        v[2] = np.nan
    new = hhmm_amd.conditional_draw_gauss(stats, PRIOR, gen)
    assert set(new) == {"p_1k", "A_ij", "mu_k", "sigma_k"}
    for name, t in new.items():
        t = t.numpy()
        assert t.shape == _gg.param_shapes(5, 2)[name], name
        assert np.isnan(t[2]).all() and np.isfinite(np.delete(t, 2, axis=0)).all(), name
    assert (np.delete(new["sigma_k"].numpy(), 2, axis=0) > 0).all()
    assert np.allclose(np.delete(new["A_ij"].numpy(), 2, axis=0).sum(axis=-1), 1.0, rtol=0, atol=1e-12)
    for bad in [(0.0, 0.0, 3.0, 1.5), (0.0, 1.0, 0.0, 1.5), (0.0, 1.0, 3.0, 0.0), (0.0, -1.0, 3.0, 1.5),
                (0.0, 1.0, -1.0, 1.5), (0.0, 1.0, 3.0, -2.0), (0.0, (1.0, 0.0), 3.0, 1.0),
                (0.0, 1.0, float("nan"), 1.0)]:
        with pytest.raises(ValueError):
            hhmm_amd.conditional_draw_gauss(stats, {"mu_sigma": bad}, gen)
    for missing in (None, {}, {"p_1k": 1.0}):
        with pytest.raises(ValueError):
            hhmm_amd.conditional_draw_gauss(stats, missing, gen)
    a = hhmm_amd.conditional_draw_gauss(stats, PRIOR, torch.Generator().manual_seed(9))
    b = hhmm_amd.conditional_draw_gauss(stats, PRIOR, torch.Generator().manual_seed(9))
    c = hhmm_amd.conditional_draw_gauss(stats, PRIOR, torch.Generator().manual_seed(10))
    assert all(np.array_equal(a[k].numpy(), b[k].numpy(), equal_nan=True) for k in a)
    assert not np.array_equal(a["mu_k"].numpy(), c["mu_k"].numpy(), equal_nan=True)


def test_conditional_draw_gauss_moments():
    """20,000 draws at one statistics row: the means of mu, sigma^2 and sigma against mn, bn / (an - 1) and
    sqrt(bn) Gamma(an - 1/2) / Gamma(an), |z| < 5 with the sample standard error."""
    import torch
    n = 20000
    stats = _stats_rows(n)
    new = hhmm_amd.conditional_draw_gauss(stats, PRIOR, torch.Generator().manual_seed(17))
    mu, sg = new["mu_k"].numpy(), new["sigma_k"].numpy()
    m0, k0, a0, b0 = PRIOR["mu_sigma"]
    for k in range(2):
        _kn, mn, an, bn = ref.nig_posterior(stats["w_k"][0, k], stats["s1_k"][0, k], stats["s2_k"][0, k], m0, k0, a0,
                                            b0)
        want = {"mu": (mu[:, k], mn), "sigma2": (sg[:, k] ** 2, bn / (an - 1.0)),
                "sigma": (sg[:, k], math.sqrt(bn) * math.exp(math.lgamma(an - 0.5) - math.lgamma(an)))}
        for name, (v, exact) in want.items():
            z = (v.mean() - exact) / (v.std(ddof=1) / math.sqrt(n))
            print(name, k, "z =", z)
            assert abs(z) < ZCAP, (name, k, z)


# ---- relabel_ordered

def test_relabel_ordered_is_one_consistent_permutation():
    g = np.random.Generator(np.random.Philox(key=77))
    n_keep, P, K, T = 3, 5, 4, 12
    draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=(n_keep, P)),
             "A_ij": g.dirichlet(np.full(K, 2.0), size=(n_keep, P, K)),
             "mu_k": g.normal(0.0, 2.0, size=(n_keep, P, K)), "sigma_k": g.uniform(0.5, 2.0, size=(n_keep, P, K))}
    x = g.normal(0.0, 2.0, size=T)
    out = hhmm_amd.relabel_ordered(draws)
    assert all(out[k].shape == draws[k].shape for k in draws)
    assert (np.diff(out["mu_k"], axis=-1) >= 0).all()
    for i in range(n_keep):
        for p in range(P):
            perm = np.argsort(draws["mu_k"][i, p])
            assert np.array_equal(out["mu_k"][i, p], draws["mu_k"][i, p][perm])
            assert np.array_equal(out["sigma_k"][i, p], draws["sigma_k"][i, p][perm])
            assert np.array_equal(out["p_1k"][i, p], draws["p_1k"][i, p][perm])
            assert np.array_equal(out["A_ij"][i, p], draws["A_ij"][i, p][np.ix_(perm, perm)])
            la = estep_ref.forward_backward("hmm", x, {k: v[i, p] for k, v in draws.items()})[0]
            lb = estep_ref.forward_backward("hmm", x, {k: v[i, p] for k, v in out.items()})[0]
            assert abs(la - lb) <= 1e-12 * max(1.0, abs(la)), (i, p, la, lb)


def test_relabel_needs_a_label_symmetric_prior():
    data, init = make(4, 4, 6, 2)
    for prior in [{"mu_sigma": ((-1.0, 1.0), 1.0, 3.0, 2.0)}, {"mu_sigma": (0.0, 1.0, 3.0, (2.0, 1.0))},
                  {"mu_sigma": (0.0, 1.0, 3.0, 2.0), "p_1k": (1.0, 2.0)},
                  {"mu_sigma": (0.0, 1.0, 3.0, 2.0), "A_ij": ((1.0, 2.0), (3.0, 1.0))}]:
        with pytest.raises(ValueError, match="relabel"):
            hhmm_amd.gibbs_gauss(data, init, 2, prior=prior, relabel=True)
    assert _gg._label_symmetric({"mu_sigma": (0.0, 1.0, 3.0, 2.0), "A_ij": 1.0 + 4.0 * np.eye(2)}, 4, 2)
    assert _gg._label_symmetric({"mu_sigma": (0.0, 1.0, 3.0, 2.0), "p_1k": 2.0, "A_ij": 0.5}, 4, 2)
    with pytest.raises(ValueError, match="mu_sigma"):
        hhmm_amd.gibbs_gauss(data, init, 2, prior=None)


# ---- the exact posterior of a T = 6 series, and the samplers against it

CHAINS, SWEEPS = 4096, 40
X6 = np.array([-1.2, 0.9, 1.4, -0.7, 1.1, -1.6])
# m0 per state: the labels are identified without relabelling
PRIOR6 = {"mu_sigma": ((-1.0, 1.0), 1.0, 3.0, 2.0)}
# the figures of the issue, from its own enumeration
PINNED = {"mu_k": [-0.9385, 0.3720], "sigma2_k": [0.8262, 1.1699], "A_ij": [[0.3903, 0.6097], [0.4572, 0.5428]]}


@functools.lru_cache(maxsize=None)
def exact_means():
    """Computed once, shared by the CPU and the GPU sampler tests."""
    means = ref.posterior_means(X6, PRIOR6, 2)
    for v in means.values():
        v.setflags(write=False)
    return means


def test_exact_means_are_the_pinned_ones():
    m = exact_means()
    for name, want in PINNED.items():
        assert np.abs(m[name] - np.array(want)).max() < 5e-5, (name, m[name])
    assert np.allclose(m["p_1k"].sum(), 1.0) and np.allclose(m["A_ij"].sum(axis=1), 1.0)


def init6():
    return {"p_1k": np.full((CHAINS, 2), 0.5), "A_ij": np.full((CHAINS, 2, 2), 0.5),
            "mu_k": np.tile([-1.0, 1.0], (CHAINS, 1)), "sigma_k": np.ones((CHAINS, 2))}


def worst_z(final):
    """max |z-score| of the across-chain mean of the final draw against the exact posterior mean; final draws
    of independent chains are iid, so the standard error is the sample sd over chains / sqrt(chains)."""
    final = dict(final, sigma2_k=np.asarray(final["sigma_k"]) ** 2)
    worst = 0.0
    for name, want in exact_means().items():
        v = np.asarray(final[name], dtype=float)
        assert v.shape == (CHAINS,) + want.shape, (name, v.shape)
        se = v.std(axis=0, ddof=1) / np.sqrt(CHAINS)
        z = np.abs(v.mean(axis=0) - want) / se
        print(name, "max |z| =", float(z.max()))
        worst = max(worst, float(z.max()))
    return worst


def test_cpu_sampler_matches_the_exact_posterior(oracle):
    import torch
    data = {"K": 2, "x": X6.reshape(1, -1)}
    params = init6()
    gen = torch.Generator().manual_seed(41)
    ug = np.random.Generator(np.random.Philox(key=43))
    for _ in range(SWEEPS):
        u = 1.0 - ug.random((CHAINS, X6.size))
        z = oracle.gqs("hmm", data, params, pars=["z_ffbs"], pairing="block", uniforms=u, nthreads=8)["z_ffbs"]
        assert z.min() >= 1
        st = dict(zip(ref.NAMES, ref.stats_chains(z, X6, 2)))
        params = {k: v.numpy() for k, v in hhmm_amd.conditional_draw_gauss(st, PRIOR6, gen).items()}
    w = worst_z(params)
    assert w < ZCAP, w


# ---------------------------------------------------------------- GPU

def bounds(data, pairing, S, P):
    """Per pair (T 2^-52 sum |x_t|, T 2^-52 sum x_t^2) over the pair's own steps."""
    x = np.atleast_2d(np.asarray(data["x"], dtype=np.float64))
    N, Tm = x.shape
    Ts = np.asarray(data["T"]).reshape(N) if "T" in data else np.full(N, Tm)
    ser = ref.pair_series(pairing, P, S, N)
    b1, b2 = np.zeros(P), np.zeros(P)
    for p in range(P):
        n = int(ser[p])
        T = int(min(max(Ts[n], 1), Tm))
        xs = np.nan_to_num(x[n, :T])
        b1[p] = T * 2.0 ** -52 * math.fsum(np.abs(xs))
        b2[p] = T * 2.0 ** -52 * math.fsum(xs * xs)
    return b1, b2


def compare(got, want, ref_loglik, b1, b2, tag):
    for name in COUNTS:
        assert got[name].shape == want[name].shape, (tag, name)
        assert np.array_equal(got[name], want[name], equal_nan=True), (tag, name)
    for name, b in (("s1_k", b1), ("s2_k", b2)):
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), (tag, name)
        err = np.abs(got[name] - want[name])
        ok = ~np.isnan(want[name])
        print(tag, name, "max err / bound =", float(np.max((err / b[:, None])[ok], initial=0.0)))
        assert (err[ok] <= np.broadcast_to(b[:, None], err.shape)[ok]).all(), (tag, name)
    ll = got["loglik"]
    fin = np.isfinite(ref_loglik)
    assert np.array_equal(np.isnan(ll), np.isnan(ref_loglik)), tag
    assert np.array_equal(ll[~fin & ~np.isnan(ref_loglik)], ref_loglik[~fin & ~np.isnan(ref_loglik)]), tag
    if fin.any():
        w = float(np.max(np.abs(ll[fin] - ref_loglik[fin]) / np.maximum(1.0, np.abs(ref_loglik[fin]))))
        assert w <= TOL, (tag, w)


def check(engine, data, draws, u, pairing="grid"):
    """Host and device entries against the reference statistics of the engine's own z_ffbs (the bit-exact path)."""
    from stats_devrun import DeviceDrawStatsGauss
    S = draws["mu_k"].shape[0]
    r = hhmm_amd.gqs("hmm", data, draws, pars=["z_ffbs", "loglik"], pairing=pairing, uniforms=u, lib=engine)
    want = ref.stats_pairs(data, r["z_ffbs"], r["loglik"], pairing, S)
    b1, b2 = bounds(data, pairing, S, r["loglik"].shape[0])
    host = hhmm_amd.draw_stats_gauss(data, draws, u, pairing, lib=engine, return_status=True)
    assert host["status"] == 0 and not host["pair_status"].any()
    compare(host, want, r["loglik"], b1, b2, (pairing, "host"))
    dv = DeviceDrawStatsGauss(engine, data, draws, u, pairing)
    assert dv.run() == 0
    dev = dv.stats()
    assert not dev["pair_status"].any()
    compare(dev, want, r["loglik"], b1, b2, (pairing, "device"))
    # the two entries run the same kernel on the same values
    for name in ref.NAMES + ("loglik",):
        assert np.array_equal(host[name], dev[name], equal_nan=True), name
    return host, r


@pytest.mark.gpu
@pytest.mark.parametrize("K", range(1, 9))
def test_gpu_stats_every_K(engine, K):
    T = 2 * fb_chunk(K) + 1
    data, draws = make(7, 10, T, K, seed=K)
    got, _r = check(engine, data, draws, synth.ffbs_uniforms(70, T, seed=K))
    ok = ~np.isnan(got["n_1k"]).any(axis=1)
    assert ok.all() and (got["w_k"].sum(axis=1) == K + T - 1).all() and (got["xi_ij"].sum(axis=(1, 2)) == T - 1).all()
    if K > 1:
        assert len({tuple(r) for r in got["w_k"]}) > 1                              # the paths do differ


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 8])
@pytest.mark.parametrize("Tsel", ["1", "2", "C-1", "C", "C+1", "2C", "4C+3", "2GC+3"])
def test_gpu_chunk_edges_in_T(engine, K, Tsel):
    c = fb_chunk(K)
    T = {"1": 1, "2": 2, "C-1": c - 1, "C": c, "C+1": c + 1, "2C": 2 * c, "4C+3": 4 * c + 3,
         "2GC+3": K_FWD_GROUP * c * 2 + 3}[Tsel]
    data, draws = make(2, 3, T, K, seed=T)
    got, _r = check(engine, data, draws, synth.ffbs_uniforms(6, T, seed=T))
    assert (got["w_k"].sum(axis=1) == K + T - 1).all()
    if T == 1:  # x_1 alone: every state holds it once
        assert not got["xi_ij"].any() and (got["w_k"] == 1).all()
        assert np.array_equal(got["s1_k"], np.repeat(data["x"][:, :1], 3, axis=0) * np.ones((1, K)))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 6])
def test_gpu_ragged_lengths_inside_one_wave(engine, K):
    c = fb_chunk(K)
    Tmax = 2 * c + 1
    lens = np.array([1, Tmax, 2, c, c + 1, Tmax, 1, c - 1] * 3, dtype=np.int32)
    N = lens.size
    data, draws = make(N, 2, Tmax, K, seed=7)
    for n in range(N):  # padding must not matter: garbage observations
        data["x"][n, lens[n]:] = 1e300
    data["T"] = lens
    check(engine, data, draws, synth.ffbs_uniforms(2 * N, Tmax, seed=8))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("P", [1, 63, 65, 130])
def test_gpu_partial_last_wave(engine, K, P):
    data, draws = make(P, P, 11, K, seed=P)
    check(engine, data, draws, synth.ffbs_uniforms(P, 11, seed=P), "zip")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("pairing,N,S", [("grid", 3, 5), ("zip", 7, 7), ("block", 3, 6)])
def test_gpu_pairings(engine, K, pairing, N, S):
    data, draws = make(N, S, 13, K, seed=N * S)
    check(engine, data, draws, synth.ffbs_uniforms(npairs(data, draws, pairing), 13, seed=S), pairing)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 4, 8])
def test_gpu_uniforms_at_the_ends_of_their_range(engine, K):
    N, S, T = 2, 40, 21
    data, draws = make(N, S, T, K, seed=41)
    g = np.random.Generator(np.random.Philox(key=42))
    u = synth.ffbs_uniforms(N * S, T, seed=43)
    pick = g.integers(0, 6, size=u.shape)
    for k in (1, 2, 3):
        u[pick == k] = k * 2.0 ** -1074
    u[pick == 4] = 1.0
    check(engine, data, draws, u)


@pytest.mark.gpu
def test_gpu_nan_parameter_and_nan_observation_are_nan_for_their_pairs_only(engine):
    N, S, T = 3, 5, 20
    data, draws = make(N, S, T, 4, seed=13)
    draws["mu_k"][1, 2] = np.nan
    data["x"][2, 7] = np.nan
    got, _r = check(engine, data, draws, synth.ffbs_uniforms(N * S, T, seed=15))
    p = np.arange(N * S)
    hit = (p % S == 1) | (p // S == 2)
    for name in ref.NAMES + ("loglik",):
        assert np.isnan(got[name][hit]).all() and np.isfinite(got[name][~hit]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [0, 16, -3])
def test_gpu_device_entry_flags_only_the_pair_with_T_out_of_range(engine, bad):
    from stats_devrun import DeviceDrawStatsGauss
    N, S, T = 4, 20, 15
    data, draws = make(N, S, T, 4, seed=19)
    data["T"] = np.array([T, 9, T, 4], dtype=np.int32)
    u = synth.ffbs_uniforms(N * S, T, seed=20)
    clean = DeviceDrawStatsGauss(engine, data, draws, u)
    assert clean.run() == 0
    want = clean.stats()
    assert not want["pair_status"].any()
    data["T"] = np.array([T, 9, bad, 4], dtype=np.int32)
    dv = DeviceDrawStatsGauss(engine, data, draws, u)
    assert dv.run() == 0
    got = dv.stats()
    hit = np.arange(N * S) // S == 2
    assert (got["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not got["pair_status"][~hit].any()
    for name in ref.NAMES + ("loglik",):
        assert np.array_equal(got[name][~hit], want[name][~hit], equal_nan=True), name
    # the host entry validates the data block as hhmm_run does
    pr, res, _out = _gg.prepare(data, draws, u)
    assert engine.hhmm_draw_stats_gauss(C.byref(pr.req), C.byref(res)) == _abi.ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_gpu_gibbs_gauss_matches_the_exact_posterior(engine):
    data = {"K": 2, "x": X6.reshape(1, -1)}
    draws, trace = hhmm_amd.gibbs_gauss(data, init6(), SWEEPS, burn=SWEEPS - 1, prior=PRIOR6, seed=53,
                                        pairing="block", lib=engine)
    assert trace.shape == (SWEEPS, CHAINS) and np.isfinite(trace).all()
    assert all(v.shape[0] == 1 for v in draws.values())
    w = worst_z({k: v[0] for k, v in draws.items()})
    assert w < ZCAP, w


@pytest.mark.gpu
def test_gpu_gibbs_gauss_is_reproducible(engine):
    data, init = make(5, 5, 11, 3, seed=61)
    prior = {"mu_sigma": (0.0, 0.5, 2.0, 1.0)}
    a, ta = hhmm_amd.gibbs_gauss(data, init, 6, burn=1, thin=2, prior=prior, seed=7, lib=engine)
    b, tb = hhmm_amd.gibbs_gauss(data, init, 6, burn=1, thin=2, prior=prior, seed=7, lib=engine)
    c, _tc = hhmm_amd.gibbs_gauss(data, init, 6, burn=1, thin=2, prior=prior, seed=8, lib=engine)
    assert np.array_equal(ta, tb) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(a[k].shape[:2] == (3, 5) for k in a)                               # sweeps 1, 3, 5
    assert not np.array_equal(a["mu_k"], c["mu_k"])
    # the first sweep starts from init
    ll = hhmm_amd.gqs("hmm", data, init, pars=["loglik"], pairing="zip", lib=engine)["loglik"]
    assert np.max(np.abs(ta[0] - ll) / np.maximum(1.0, np.abs(ll))) <= TOL


@pytest.mark.gpu
def test_gpu_gibbs_gauss_to_gqs_end_to_end(engine):
    """gibbs_gauss(relabel=True) on two short series -> stack_chains -> gqs(block): shapes agree, no pair
    carries a status, every kept mu_k row is ascending."""
    N, B, T, K = 2, 8, 14, 3
    data, init = make(N, N * B, T, K, seed=71)
    data["T"] = np.array([T, 9], dtype=np.int32)
    prior = {"mu_sigma": (0.0, 0.25, 2.0, 1.0), "A_ij": 1.0 + 2.0 * np.eye(K)}
    draws, trace = hhmm_amd.gibbs_gauss(data, init, 6, burn=2, thin=2, prior=prior, seed=3, pairing="block",
                                        relabel=True, lib=engine)
    assert trace.shape == (6, N * B) and draws["A_ij"].shape == (2, N * B, K, K)
    assert np.isfinite(draws["mu_k"]).all() and (np.diff(draws["mu_k"], axis=-1) >= 0).all()
    stacked = hhmm_amd.stack_chains(draws, N)
    S = 2 * B
    assert stacked["mu_k"].shape == (N * S, K) and stacked["A_ij"].shape == (N * S, K, K)
    out = hhmm_amd.gqs("hmm", data, stacked, pars=["loglik", "gamma_tk", "zstar_t"], pairing="block", lib=engine,
                       return_status=True)
    assert out["status"] == 0 and not out["pair_status"].any()
    assert out["loglik"].shape == (N * S,) and out["gamma_tk"].shape == (N * S, T, K)
    assert np.isfinite(out["loglik"]).all()
