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
hmm-multinom-semisup and hhmm-tayal2009 at K <= 8 (hhmm_draw_stats, a lane per
pair); hmm-multinom also at 8 < K <= 32 (hhmm_draw_stats_large, a group of 16
or 32 lanes per pair) -- the flattened hierarchical HMMs, whose sparse A_ij the
`support` argument of conditional_draw() and gibbs() keeps sparse.
"""
import numpy as np

from . import _stats
from .api import load_library

MODELS = ("hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009")
MAX_K_LANE = 8  # hhmm_draw_stats: the lane-per-pair kernel (csrc kMaxK)


def entry_name(model, K):
    """The library entry draw_stats() and gibbs() call: "draw_stats" up to
    MAX_K_LANE states, "draw_stats_large" above for hmm-multinom (the masked
    programs are K <= 8 programs: they and K > 32 reach the library, which
    rejects them)."""
    return "draw_stats_large" if model == "hmm-multinom" and int(K) > MAX_K_LANE else "draw_stats"


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
    has NaN statistics.  K <= 32 for hmm-multinom; hhmm_draw_stats_large above 8."""
    lib = lib or load_library()
    pr, res, out = prepare(model, data, draws, uniforms, pairing, device)
    return _stats.call(lib, entry_name(model, pr.K), pr, res, out, return_status)


def _dirichlet(torch, conc, generator, support=None, counts=None):
    """Dirichlet rows (last axis) as normalised standard gammas; a row with a NaN
    concentration is NaN.

    support (a boolean mask broadcastable to conc) restricts every row to its
    supported entries: the gammas outside are replaced by exact zeros before the
    row is normalised, so the row is a Dirichlet draw over the support.  A row
    whose `counts` are positive somewhere outside its support is NaN (the
    statistics contradict the structure), and so is a row with no supported
    entry.  None is the unrestricted draw, with the same generator consumption
    as before the argument existed."""
    bad = torch.isnan(conc).any(dim=-1, keepdim=True)
    if support is None:
        g = torch._standard_gamma(torch.where(bad, torch.ones_like(conc), conc), generator=generator)
        return torch.where(bad, torch.full_like(g, float("nan")), g / g.sum(dim=-1, keepdim=True))
    m = torch.as_tensor(support, dtype=torch.bool, device=conc.device).expand(conc.shape)
    bad = bad | ((counts > 0) & ~m).any(dim=-1, keepdim=True)
    g = torch._standard_gamma(torch.where(bad | ~m, torch.ones_like(conc), conc), generator=generator)
    g = torch.where(m, g, torch.zeros_like(g))
    return torch.where(bad, torch.full_like(g, float("nan")), g / g.sum(dim=-1, keepdim=True))


def _check_support(support, names):
    """support or {}, its keys checked against the model's parameter names."""
    support = support or {}
    for name in support:
        if name not in names:
            raise ValueError(f"support names {name!r}; the parameters are {tuple(names)}")
    return support


def conditional_draw(model, stats, prior=None, generator=None, support=None):
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
    statistics gets NaN parameters.

    support: {name: boolean mask broadcastable to the parameter (p_11: to its
    Beta pair, (P, 2))} -- the structural zeros of a sparse model, e.g. the
    transition matrix of a flattened hierarchical HMM.  Outside its support a
    drawn parameter is an exact 0 and every Dirichlet row is drawn over its
    supported entries only (a zero prior concentration does not do this: the
    gamma sampler returns the smallest normal number for it, not 0).  FFBS never
    draws a transition of weight zero for u in (0, 1], so with parameters that
    respect the support the counts outside it are 0; a row whose statistics hold
    a positive count outside its support is NaN.  The default None is the
    unrestricted draw, bit for bit."""
    import torch
    if model not in MODELS:
        raise ValueError(f"the draw statistics cover {MODELS}, not {model!r}")
    n1, xi, c = (torch.as_tensor(stats[k]) for k in ("n_1k", "xi_ij", "c_kl"))
    prior = prior or {}
    support = _check_support(support, param_shapes(model, 1, 1, 1))

    def draw(name, counts):
        a = torch.as_tensor(prior.get(name, 1.0), dtype=counts.dtype, device=counts.device)
        return _dirichlet(torch, counts + a, generator, support.get(name), counts)

    if model == "hhmm-tayal2009":
        p = draw("p_11", torch.stack([n1[:, 0], n1[:, 2]], dim=-1))
        rows = torch.stack([torch.stack([xi[:, 0, 1], xi[:, 0, 2]], dim=-1),
                            torch.stack([xi[:, 2, 0], xi[:, 2, 3]], dim=-1)], dim=1)
        return {"p_11": p[:, 0], "A_row": draw("A_row", rows), "phi_k": draw("phi_k", c)}
    return {"p_1k": draw("p_1k", n1), "A_ij": draw("A_ij", xi), "phi_k": draw("phi_k", c)}


def _fortran_flat(t):
    """The elements of t in first-index-fastest order (the ABI's layout)."""
    return t.permute(*reversed(range(t.dim()))).reshape(-1)


def gibbs(model, data, init, n_iter, burn=0, thin=1, prior=None, seed=0, pairing="zip", lib=None, support=None):
    """n_iter sweeps of the blocked Gibbs sampler for every pair, on the device.

    Every pair is a chain with its own parameters, so pairing is "zip" (one
    chain per series) or "block" (S / N chains for each series); init: {name:
    (P, ...)} draw arrays as draw_stats() takes them.  The data goes to the
    device once and the parameters stay there.  One sweep draws the uniforms
    u = 1 - torch.rand(P * T_max), takes the statistics of the path they select
    under the current parameters (hhmm_draw_stats_device on torch's current
    stream; hhmm_draw_stats_large_device for hmm-multinom at 8 < K <= 32) and
    redraws the parameters from them (conditional_draw; `support` is its
    argument: with an init that respects it, every kept draw does).  The
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
    run = _stats.DeviceStats(lib, entry_name(model, K), pr, res, stat_shapes(P, K, L))
    names = list(param_shapes(model, P, K, L))
    support = {name: torch.as_tensor(np.asarray(m, dtype=bool), device=dev)
               for name, m in _check_support(support, names).items()} or None
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
        new = conditional_draw(model, views, prior, gen, support)
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
