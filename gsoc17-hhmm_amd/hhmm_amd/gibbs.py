"""Blocked Gibbs sampling on the GPU (include/hhmm_gibbs.h).

The state half of the sampler is FFBS (the reference's technical
review introduces it for this purpose, techreview/Rmd/hmm.Rmd:193-221):
`draw_stats()` draws one path per (series, draw) pair and returns only its
sufficient statistics -- z_1, the transition counts and the (state, symbol)
counts -- so nothing per step leaves the chip.  The parameter half is
conjugate: the weight of a path under the CODED likelihood of the Stan program
is prod p^n_1k prod A^xi_ij prod phi^c_kl, and the three discrete programs put
(implicit) uniform priors on every simplex and on p_11, so theta | z is a
product of Dirichlet / Beta distributions (`conditional_draw()`).  `gibbs()`
alternates the two on the device for many independent chains at once, and
`stack_chains()` lays the kept draws out for gqs(..., pairing="block").

The counts follow the model's forward masks (hmm-multinom-semisup.stan:42,
hhmm-tayal2009.stan:51 and :62): a transition or an initial state is counted
only where the program multiplies its probability in.  hmm-multinom,
hmm-multinom-semisup and hhmm-tayal2009 at K <= 8.
"""
import numpy as np

from . import _stats
from .api import load_library

MODELS = ("hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009")


def param_shapes(model, S, K, L):
    """{name: shape} of the draw arrays `model` takes."""
    if model == "hhmm-tayal2009":
        return {"p_11": (S,), "A_row": (S, 2, 2), "phi_k": (S, K, L)}
    return {"p_1k": (S, K), "A_ij": (S, K, K), "phi_k": (S, K, L)}


def stat_shapes(P, K, L):
    """{name: shape} of the statistics draw_stats() returns."""
    return {"loglik": (P,), "n_1k": (P, K), "xi_ij": (P, K, K), "c_kl": (P, K, L)}


def _request(model, data, draws, pairing, device):
    """(PreparedRequest, EstepResult, {name: array}) with the shape checks; no uniforms yet."""
    if model not in MODELS:
        raise ValueError(f"the draw statistics cover {MODELS}, not {model!r}")
    return _stats.request(model, data, draws, pairing, device, lambda S, K, L: param_shapes(model, S, K, L),
                          stat_shapes)


def prepare(model, data, draws, uniforms, pairing="grid", device=-1):
    """_request() plus the uniforms of the draw, shape (P, T_max)."""
    pr, res, out = _request(model, data, draws, pairing, device)
    _stats.add_uniforms(pr, uniforms)
    return pr, res, out


def draw_stats(model, data, draws, uniforms, pairing="grid", device=-1, lib=None, return_status=False):
    """Sufficient statistics of one FFBS path per (series, draw) pair.

    The path is the z_ffbs that gqs() returns for the same uniforms, shape
    (P, T_max), values in (0, 1].  Returns {name: array}: loglik (P,), n_1k
    (P, K), xi_ij (P, K, K), c_kl (P, K, L) -- exact counts as float64.  A pair
    whose log-likelihood is not finite, or whose draw is undefined at some step,
    has NaN statistics."""
    lib = lib or load_library()
    return _stats.call(lib, "draw_stats", *prepare(model, data, draws, uniforms, pairing, device), return_status)


def _dirichlet(torch, conc, generator):
    """Dirichlet rows (last axis) as normalised standard gammas; a row with a NaN
    concentration is NaN."""
    bad = torch.isnan(conc).any(dim=-1, keepdim=True)
    g = torch._standard_gamma(torch.where(bad, torch.ones_like(conc), conc), generator=generator)
    return torch.where(bad, torch.full_like(g, float("nan")), g / g.sum(dim=-1, keepdim=True))


def conditional_draw(model, stats, prior=None, generator=None):
    """theta | z: one draw of the parameters of every pair from its statistics.

    stats: {n_1k (P, K), xi_ij (P, K, K), c_kl (P, K, L)} as torch tensors (any
    device; numpy arrays are taken as CPU tensors).  prior: {name:
    concentration} broadcastable to each parameter array (hhmm-tayal2009's p_11:
    the Beta's (a, b), broadcastable to (P, 2)); the default is 1 everywhere,
    the Stan programs' implicit uniform priors.  Returns {name: (P, ...)}
    tensors.  hmm-multinom and semisup: p_1k ~ Dir(a + n_1k), every row of A_ij
    ~ Dir(a + xi[i, :]), phi_k[k] ~ Dir(a + c[k, :]).  hhmm-tayal2009: p_11 ~
    Beta(a + n1[0], b + n1[2]), A_row[0] ~ Dir(a + (xi[0,1], xi[0,2])),
    A_row[1] ~ Dir(a + (xi[2,0], xi[2,3])), phi_k as above.  A pair with NaN
    statistics gets NaN parameters."""
    import torch
    if model not in MODELS:
        raise ValueError(f"the draw statistics cover {MODELS}, not {model!r}")
    n1, xi, c = (torch.as_tensor(stats[k]) for k in ("n_1k", "xi_ij", "c_kl"))
    prior = prior or {}

    def conc(name, counts):
        a = torch.as_tensor(prior.get(name, 1.0), dtype=counts.dtype, device=counts.device)
        return counts + a

    if model == "hhmm-tayal2009":
        p = _dirichlet(torch, conc("p_11", torch.stack([n1[:, 0], n1[:, 2]], dim=-1)), generator)
        rows = torch.stack([torch.stack([xi[:, 0, 1], xi[:, 0, 2]], dim=-1),
                            torch.stack([xi[:, 2, 0], xi[:, 2, 3]], dim=-1)], dim=1)
        return {"p_11": p[:, 0], "A_row": _dirichlet(torch, conc("A_row", rows), generator),
                "phi_k": _dirichlet(torch, conc("phi_k", c), generator)}
    return {"p_1k": _dirichlet(torch, conc("p_1k", n1), generator),
            "A_ij": _dirichlet(torch, conc("A_ij", xi), generator),
            "phi_k": _dirichlet(torch, conc("phi_k", c), generator)}


def _fortran_flat(t):
    """The elements of t in first-index-fastest order (the ABI's layout)."""
    return t.permute(*reversed(range(t.dim()))).reshape(-1)


def gibbs(model, data, init, n_iter, burn=0, thin=1, prior=None, seed=0, pairing="zip", lib=None):
    """n_iter sweeps of the blocked Gibbs sampler for every pair, on the device.

    Every pair is a chain with its own parameters, so pairing is "zip" (one
    chain per series) or "block" (S / N chains for each series); init: {name:
    (P, ...)} draw arrays as draw_stats() takes them.  The data goes to the
    device once and the parameters stay there.  One sweep draws the uniforms
    u = 1 - torch.rand(P * T_max), takes the statistics of the path they select
    under the current parameters (hhmm_draw_stats_device on torch's current
    stream) and redraws the parameters from them (conditional_draw).  The
    uniforms must lie in (0, 1]: torch.rand can return 0, and at u = 0 the
    categorical draw picks state 1 even when its weight is 0 -- a path of
    probability zero; 1 - rand lies in (0, 1].

    Returns (draws, trace): the kept draws {name: (n_keep, P, ...)} -- sweeps
    burn, burn + thin, ... -- and the (n_iter, P) log-likelihoods of the
    parameters each sweep started from.  Only those come to the host.  The same
    seed gives the same draws.  A pair whose statistics are NaN keeps NaN
    parameters from then on."""
    import torch
    if pairing not in ("zip", "block"):
        raise ValueError("gibbs: every pair carries its own parameters, pairing is 'zip' or 'block'")
    n_iter, burn, thin = int(n_iter), int(burn), int(thin)
    if n_iter < 1 or burn < 0 or thin < 1:
        raise ValueError("gibbs: n_iter >= 1, burn >= 0 and thin >= 1")
    lib = lib or load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    pr, res, _out = _request(model, data, init, pairing, -1)
    P, K, Tmax, L = pr.P, pr.K, pr.Tmax, int(data.get("L", 0))
    # the request's arrays on the device (the parameters: updated in place every sweep)
    ubuf = torch.empty(P * Tmax, dtype=torch.float64, device=dev)
    pr.req.ffbs_u = ubuf.data_ptr()
    run = _stats.DeviceStats(lib, "draw_stats", pr, res, stat_shapes(P, K, L))
    names = list(param_shapes(model, P, K, L))
    pbuf, sbuf = run.arrays, run.out
    views = {"n_1k": sbuf["n_1k"].view(K, P).t(), "xi_ij": sbuf["xi_ij"].view(K, K, P).permute(2, 1, 0),
             "c_kl": sbuf["c_kl"].view(L, K, P).permute(2, 1, 0)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    trace = torch.empty((n_iter, P), dtype=torch.float64, device=dev)
    kept = {name: [] for name in names}
    for it in range(n_iter):
        torch.rand(P * Tmax, dtype=torch.float64, device=dev, generator=gen, out=ubuf)
        ubuf.neg_().add_(1.0)
        run.run()
        trace[it] = sbuf["loglik"]
        new = conditional_draw(model, views, prior, gen)
        for name in names:
            pbuf[name].copy_(_fortran_flat(new[name]))
            if it >= burn and (it - burn) % thin == 0:
                kept[name].append(new[name])
    shapes = param_shapes(model, P, K, L)
    draws = {name: (torch.stack(v).cpu().numpy() if v else np.empty((0,) + shapes[name])) for name, v in kept.items()}
    return draws, trace.cpu().numpy()


def stack_chains(draws, N):
    """Kept draws of B chains per series -> one block of S = B * n_keep draws per series.

    draws: {name: (n_keep, P, ...)} from gibbs() with P = B * N chains, chain b
    of series n at p = b + B * n ("block" pairing; "zip": B = 1).  Returns
    {name: (S * N, ...)}, series-major: the layout walkforward.assemble produces
    and gqs(..., pairing="block") takes."""
    out = {}
    for name, v in draws.items():
        v = np.asarray(v)
        n_keep, P = v.shape[:2]
        if P % N:
            raise ValueError(f"{name}: {P} chains are not a multiple of {N} series")
        B = P // N
        w = v.reshape((n_keep, N, B) + v.shape[2:])
        out[name] = np.ascontiguousarray(np.moveaxis(w, 1, 0)).reshape((N * n_keep * B,) + v.shape[2:])
    return out
