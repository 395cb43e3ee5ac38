"""Blocked Gibbs sampling of the Gaussian hmm on the GPU (include/hhmm_gibbs_gauss.h).

hmm/stan/hmm.stan adds normal_lpdf(x_1 | mu_k, sigma_k) for every state at
t = 1 (quirk Q2), so the coded weight of a path z is

    p_1(z_1) prod_k N(x_1 | mu_k, sigma_k) prod_{t>=2} A(z_{t-1}, z_t) N(x_t | mu_{z_t}, sigma_{z_t})
  = prod p^n_1k prod A^xi_ij prod_k (2 pi)^(-w_k/2) sigma_k^(-w_k)
        exp(-(s2_k - 2 mu_k s1_k + mu_k^2 w_k) / (2 sigma_k^2))

with w_k = 1 + #{t >= 2: z_t = k}, s1_k = x_1 + sum x_t, s2_k = x_1^2 + sum x_t^2
over the steps t >= 2 the state owns.  `draw_stats_gauss()` draws one FFBS path
per (series, draw) pair and returns those statistics; nothing per step leaves
the chip.

The parameter half needs a decision the discrete programs do not: under
hmm.stan's flat priors a state that owns no step beyond x_1 has an improper
sigma conditional.  `conditional_draw_gauss()` therefore REQUIRES a proper
Normal-Inverse-Gamma prior, sigma_k^2 ~ InvGamma(a0, b0), mu_k | sigma_k^2 ~
N(m0, sigma_k^2 / kappa0), and has no default: Stan's flat prior is the improper
limit kappa0 -> 0, a0 -> -1, b0 -> 0, and any proper default would silently
change the target.  With it

    kn = kappa0 + w          mn = (kappa0 m0 + s1) / kn
    an = a0 + w / 2          bn = max(b0, b0 + (s2 + kappa0 m0^2 - kn mn^2) / 2)
    sigma^2 = bn / Gamma(an, 1)     mu = mn + sqrt(sigma^2 / kn) N(0, 1)

s2 - kn mn^2 cancels in fp64: the relative error it leaves in bn is about
2^-53 s2 / bn, so a series whose mean dwarfs its spread should be centred
first.  The bound sigma_k >= 0.0001 of hmm.stan:21 is not applied.

ordered[K] mu_k: the chain runs unconstrained.  When every state shares the
same (m0, kappa0, a0, b0) and the Dirichlet concentrations are symmetric under
relabelling, the unconstrained posterior is invariant under label permutations
and sorting each kept draw by mu (`relabel_ordered`) is an exact draw from the
ordered posterior.
"""
import numpy as np

from . import _stats
from .api import load_library
from .gibbs import _check_support, _dirichlet, _fortran_flat, stack_chains  # noqa: F401  (stack_chains: reused as is)

MODEL = "hmm"
PARAMS = ("p_1k", "A_ij", "mu_k", "sigma_k")
SUPPORTED = ("p_1k", "A_ij")  # the parameters `support` can restrict: the two simplexes
MAX_K_LANE = 8  # hhmm_draw_stats_gauss: the lane-per-pair kernel (csrc kMaxK)


def entry_name(K):
    """The library entry draw_stats_gauss() and gibbs_gauss() call at K states:
    "draw_stats_gauss" up to MAX_K_LANE, "draw_stats_large" above (K > 32
    reaches the library, which rejects it)."""
    return "draw_stats_gauss" if int(K) <= MAX_K_LANE else "draw_stats_large"


def param_shapes(S, K):
    """{name: shape} of the draw arrays hmm takes."""
    return {"p_1k": (S, K), "A_ij": (S, K, K), "mu_k": (S, K), "sigma_k": (S, K)}


def stat_shapes(P, K):
    """{name: shape} of the statistics draw_stats_gauss() returns."""
    return {"loglik": (P,), "n_1k": (P, K), "xi_ij": (P, K, K), "w_k": (P, K), "s1_k": (P, K), "s2_k": (P, K)}


def _request(data, draws, pairing, device):
    """(PreparedRequest, EstepResult, {name: array}) with the shape checks; no uniforms yet."""
    return _stats.request(MODEL, data, draws, pairing, device, lambda S, K, L: param_shapes(S, K),
                          lambda P, K, L: stat_shapes(P, K))


def prepare(data, draws, uniforms, pairing="grid", device=-1):
    """_request() plus the uniforms of the draw, shape (P, T_max)."""
    pr, res, out = _request(data, draws, pairing, device)
    _stats.add_uniforms(pr, uniforms)
    return pr, res, out


def draw_stats_gauss(data, draws, uniforms, pairing="grid", device=-1, lib=None, return_status=False):
    """Sufficient statistics of one FFBS path of hmm.stan per (series, draw) pair.

    The path is the z_ffbs that gqs("hmm", ...) returns for the same uniforms,
    shape (P, T_max), values in (0, 1].  Returns {name: array}: loglik (P,), n_1k
    (P, K), xi_ij (P, K, K), w_k, s1_k, s2_k (P, K) as float64; x_1 counts once
    for every state.  A pair whose log-likelihood is not finite, or whose draw is
    undefined at some step, has NaN statistics.  K <= 32; hhmm_draw_stats_large
    above 8."""
    lib = lib or load_library()
    pr, res, out = prepare(data, draws, uniforms, pairing, device)
    return _stats.call(lib, entry_name(pr.K), pr, res, out, return_status)


def _nig_prior(prior):
    """(m0, kappa0, a0, b0) of prior["mu_sigma"] as float64 numpy arrays, checked to be proper."""
    if not prior or "mu_sigma" not in prior:
        raise ValueError("the Gaussian hmm needs prior['mu_sigma'] = (m0, kappa0, a0, b0): hmm.stan's flat prior "
                         "gives an empty state an improper sigma conditional, and there is no default")
    ms = prior["mu_sigma"]
    if len(ms) != 4:
        raise ValueError("prior['mu_sigma'] is (m0, kappa0, a0, b0)")
    m0, k0, a0, b0 = (c.detach().cpu().numpy() if hasattr(c, "detach") else np.asarray(c, dtype=np.float64)
                      for c in ms)
    for name, v in (("kappa0", k0), ("a0", a0), ("b0", b0)):
        if not np.all(v > 0):  # NaN fails too
            raise ValueError(f"prior['mu_sigma']: {name} must be positive (a proper Normal-Inverse-Gamma prior)")
    if not np.all(np.isfinite(m0)):
        raise ValueError("prior['mu_sigma']: m0 must be finite")
    return m0, k0, a0, b0


def _prior_tensors(torch, prior, dtype, device):
    """The checked prior as tensors: (m0, kappa0, a0, b0, concentration of p_1k, of A_ij)."""
    nig = _nig_prior(prior)
    return tuple(torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=dtype, device=device)
                 for v in nig + (prior.get("p_1k", 1.0), prior.get("A_ij", 1.0)))


def _conditional(torch, stats, pt, generator, support=None):
    m0, k0, a0, b0, cp, cA = pt
    n1, xi, w, s1, s2 = (stats[k] for k in ("n_1k", "xi_ij", "w_k", "s1_k", "s2_k"))
    kn = k0 + w
    mn = (k0 * m0 + s1) / kn
    an = a0 + 0.5 * w
    bn = torch.maximum(b0 + torch.zeros_like(w), b0 + 0.5 * (s2 + k0 * m0 * m0 - kn * mn * mn))
    bad = torch.isnan(an) | torch.isnan(bn) | torch.isnan(mn)
    g = torch._standard_gamma(torch.where(bad, torch.ones_like(an), an), generator=generator)
    sig2 = torch.where(bad, torch.full_like(bn, float("nan")), bn / g)
    eps = torch.randn(sig2.shape, dtype=sig2.dtype, device=sig2.device, generator=generator)
    mu = mn + torch.sqrt(sig2 / kn) * eps
    support = support or {}
    return {"p_1k": _dirichlet(torch, n1 + cp, generator, support.get("p_1k"), n1),
            "A_ij": _dirichlet(torch, xi + cA, generator, support.get("A_ij"), xi),
            "mu_k": mu, "sigma_k": torch.sqrt(sig2)}


def conditional_draw_gauss(stats, prior, generator=None, support=None):
    """theta | z for hmm.stan: one draw of the parameters of every pair from its statistics.

    stats: {n_1k (P, K), xi_ij (P, K, K), w_k, s1_k, s2_k (P, K)} as torch
    tensors (any device; numpy arrays are taken as CPU tensors).  prior:
    {"mu_sigma": (m0, kappa0, a0, b0), "p_1k": ..., "A_ij": ...}; mu_sigma is
    required, its components broadcast to (P, K), and kappa0, a0, b0 must be
    positive (ValueError otherwise); the Dirichlet concentrations default to 1,
    the program's implicit uniform.  Returns {p_1k, A_ij, mu_k, sigma_k} as
    (P, ...) tensors: p_1k ~ Dir(a + n_1k), every row of A_ij ~ Dir(a + xi[i, :]),
    sigma_k^2 ~ InvGamma(an, bn), mu_k ~ N(mn, sigma_k^2 / kn) (the module
    docstring has an, bn, kn, mn).  A pair with NaN statistics gets NaN
    parameters.  support: {"p_1k": mask, "A_ij": mask}, the structural zeros of
    the two simplexes as gibbs.conditional_draw takes them (exact zeros outside,
    rows drawn over their support, NaN for a count outside it); None is the
    unrestricted draw, bit for bit."""
    import torch
    st = {k: torch.as_tensor(stats[k]) for k in ("n_1k", "xi_ij", "w_k", "s1_k", "s2_k")}
    pt = _prior_tensors(torch, prior, st["w_k"].dtype, st["w_k"].device)
    return _conditional(torch, st, pt, generator, _check_support(support, SUPPORTED))


def _label_symmetric(prior, P, K):
    """Is the prior invariant under a relabelling of the states?"""
    for v in _nig_prior(prior) + (np.asarray(prior.get("p_1k", 1.0), dtype=np.float64),):
        b = np.broadcast_to(v, (P, K))
        if not np.array_equal(b, np.broadcast_to(b[:, :1], (P, K))):
            return False
    A = np.broadcast_to(np.asarray(prior.get("A_ij", 1.0), dtype=np.float64), (P, K, K))
    eye = np.eye(K, dtype=bool)
    diag, off = A[:, eye], A[:, ~eye]
    return bool(np.array_equal(diag, np.broadcast_to(diag[:, :1], diag.shape)) and
                (K == 1 or np.array_equal(off, np.broadcast_to(off[:, :1], off.shape))))


def relabel_ordered(draws):
    """Sorts every draw by mu_k: one permutation applied to mu_k, sigma_k, p_1k and both axes of A_ij.

    draws: {p_1k (..., K), A_ij (..., K, K), mu_k (..., K), sigma_k (..., K)} numpy
    arrays.  Under a label-symmetric prior this maps a draw of the unconstrained
    posterior to a draw of hmm.stan's ordered[K] mu_k posterior.  Returns new
    arrays; a NaN mu sorts last."""
    mu = np.asarray(draws["mu_k"], dtype=np.float64)
    perm = np.argsort(mu, axis=-1, kind="stable")
    out = {"mu_k": np.take_along_axis(mu, perm, axis=-1),
           "sigma_k": np.take_along_axis(np.asarray(draws["sigma_k"], dtype=np.float64), perm, axis=-1),
           "p_1k": np.take_along_axis(np.asarray(draws["p_1k"], dtype=np.float64), perm, axis=-1)}
    A = np.asarray(draws["A_ij"], dtype=np.float64)
    A = np.take_along_axis(A, perm[..., :, None], axis=-2)
    out["A_ij"] = np.take_along_axis(A, perm[..., None, :], axis=-1)
    return out


def gibbs_gauss(data, init, n_iter, burn=0, thin=1, prior=None, seed=0, pairing="zip", relabel=False, lib=None,
                support=None):
    """n_iter sweeps of the blocked Gibbs sampler of hmm.stan for every pair, on the device.

    The structure of gibbs(): every pair is a chain with its own parameters, so
    pairing is "zip" or "block"; init: {p_1k, A_ij, mu_k, sigma_k} with P rows.
    The data goes to the device once and the parameters stay there.  One sweep
    draws the uniforms u = 1 - torch.rand(P * T_max) (in (0, 1]), takes the
    statistics of the path they select (hhmm_draw_stats_gauss_device on torch's
    current stream; hhmm_draw_stats_large_device at 8 < K <= 32) and redraws the
    parameters (conditional_draw_gauss's update; `support` is its argument).
    prior["mu_sigma"] is required.  relabel=True sorts the kept draws
    by mu_k (relabel_ordered) and needs a label-symmetric prior: the same
    (m0, kappa0, a0, b0) for every state, a scalar p_1k concentration and a
    scalar or diagonal / off-diagonal A_ij concentration (ValueError otherwise).

    Returns (draws, trace): the kept draws {name: (n_keep, P, ...)} -- sweeps
    burn, burn + thin, ... -- and the (n_iter, P) log-likelihoods of the
    parameters each sweep started from.  Only those come to the host.  The same
    seed gives the same draws."""
    if pairing not in ("zip", "block"):
        raise ValueError("gibbs_gauss: every pair carries its own parameters, pairing is 'zip' or 'block'")
    n_iter, burn, thin = int(n_iter), int(burn), int(thin)
    if n_iter < 1 or burn < 0 or thin < 1:
        raise ValueError("gibbs_gauss: n_iter >= 1, burn >= 0 and thin >= 1")
    pr, res, _out = _request(data, init, pairing, -1)
    P, K, Tmax = pr.P, pr.K, pr.Tmax
    _nig_prior(prior)
    if relabel and not _label_symmetric(prior, P, K):
        raise ValueError("gibbs_gauss: relabel=True needs a prior that is the same for every state (sorting by mu_k "
                         "is exact only when the posterior is invariant under label permutations)")
    if relabel and _check_support(support, SUPPORTED):
        raise ValueError("gibbs_gauss: relabel=True cannot be combined with support (a mask ties the parameters to "
                         "the labels, so the posterior is not invariant under label permutations)")
    import torch
    lib = lib or load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    # the request's arrays on the device (the parameters: updated in place every sweep)
    ubuf = torch.empty(P * Tmax, dtype=torch.float64, device=dev)
    pr.req.ffbs_u = ubuf.data_ptr()
    run = _stats.DeviceStats(lib, entry_name(K), pr, res, stat_shapes(P, K))
    support = {name: torch.as_tensor(np.asarray(m, dtype=bool), device=dev)
               for name, m in _check_support(support, SUPPORTED).items()}
    pbuf, sbuf = run.arrays, run.out
    views = {"n_1k": sbuf["n_1k"].view(K, P).t(), "xi_ij": sbuf["xi_ij"].view(K, K, P).permute(2, 1, 0)}
    for name in ("w_k", "s1_k", "s2_k"):
        views[name] = sbuf[name].view(K, P).t()
    pt = _prior_tensors(torch, prior, torch.float64, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    trace = torch.empty((n_iter, P), dtype=torch.float64, device=dev)
    kept = {name: [] for name in PARAMS}
    for it in range(n_iter):
        torch.rand(P * Tmax, dtype=torch.float64, device=dev, generator=gen, out=ubuf)
        ubuf.neg_().add_(1.0)
        run.run()
        trace[it] = sbuf["loglik"]
        new = _conditional(torch, views, pt, gen, support)
        for name in PARAMS:
            pbuf[name].copy_(_fortran_flat(new[name]))
            if it >= burn and (it - burn) % thin == 0:
                kept[name].append(new[name])
    shapes = param_shapes(P, K)
    draws = {name: (torch.stack(v).cpu().numpy() if v else np.empty((0,) + shapes[name])) for name, v in kept.items()}
    if relabel:
        draws = relabel_ordered(draws)
    return draws, trace.cpu().numpy()
