"""Batched E-step on the GPU (include/hhmm_estep.h) and what follows from it.

`estep()` returns, per (series, draw) pair, the expected sufficient statistics
of the HMM summed over the steps: gamma_1, the pairwise posterior sum xi_ij and
the emission sums.  Nothing [P, T, K]-sized leaves the device.  Two things the
reference's drivers lack are plain arithmetic on these [P, K..] arrays:

  score()   the gradient of the model-block log-likelihood with respect to
            every constrained parameter (Fisher's identity) -- what Stan's
            autodiff recomputes inside NUTS on every leapfrog step;
  m_step()  one Baum-Welch update (hhmm_amd.em.baum_welch iterates it).

The statistics follow the CODED likelihood of each Stan program: hmm.stan:30
adds sum_k normal_lpdf(x_1 | mu_k, sigma_k) to every state at t = 1 (quirk Q2),
so x_1 enters w_k / s1_k / s2_k with weight 1 for every state.  hmm and
hmm-multinom at K <= 32: hhmm_estep up to K = 8 (a lane per pair),
hhmm_estep_large above (a group of 16 or 32 lanes per pair).  One or a few long
series (an EM fit of one long series from a handful of starts) leave a
lane-per-pair kernel one lane each for T dependent steps: `schedule="scan"`
runs the same E-step in parallel over T (hhmm_estep_scan, K <= 8), and
`schedule="auto"`, the default, takes it where the library's plan does.

score() and m_step() also take the statistics hhmm_amd.expected_stats returns
for the two masked programs (FIT_MODELS): hmm-multinom-semisup with the
hmm-multinom formulas, hhmm-tayal2009 in the parameters the program has --
p_11, the two rows of A_row and phi_k.
"""
import numpy as np

from . import _abi, _stats
from .api import load_library

MODELS = ("hmm", "hmm-multinom")
FIT_MODELS = MODELS + ("hmm-multinom-semisup", "hhmm-tayal2009")  # score / m_step / baum_welch
_TINY = 1e-300
MAX_K_LANE = 8  # hhmm_estep: the lane-per-pair kernel (csrc kMaxK)
SCHEDULES = ("auto", "lanes", "scan")
SCAN_MAX_P = 4096  # schedule="auto": the scan only under this many pairs ... (csrc kEstepScanMaxP)
SCAN_MIN_T = 8192  # ... and from this T_max on (csrc kEstepScanMinT)


def entry_name(K, schedule="lanes"):
    """The library entry estep() calls at K states: "estep" up to MAX_K_LANE,
    "estep_large" above (K > 32 reaches the library, which rejects it); under
    the resolved schedule "scan" (K <= MAX_K_LANE only), "estep_scan"."""
    if schedule == "scan":
        return "estep_scan"
    return "estep" if int(K) <= MAX_K_LANE else "estep_large"


def resolve_schedule(pr, schedule="auto", lib=None):
    """"lanes" or "scan": the schedule estep() and expected_stats() run a prepared request on.

    "lanes" is the kernel that walks every series step by step.  "scan" is the
    parallel scan over T: K <= MAX_K_LANE, else a ValueError that names
    estep_large.  "auto" takes the scan only when K <= MAX_K_LANE, P <
    SCAN_MAX_P and T_max >= SCAN_MIN_T (or pr's flags force it) and the
    library's plan (hhmm_estep_scan_plan, no device needed) chooses it; a
    request outside that gate is "lanes" without a call into the library."""
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES}, not {schedule!r}")
    if schedule == "lanes":
        return "lanes"
    if schedule == "scan":
        if pr.K > MAX_K_LANE:
            raise ValueError(f"schedule='scan' covers K <= {MAX_K_LANE}; K = {pr.K} goes to estep_large "
                             "(schedule='lanes' or 'auto')")
        return "scan"
    forced = bool(int(pr.req.flags) & _abi.FLAG_SCAN_FORCE)
    if pr.K > MAX_K_LANE or not (forced or (pr.P < SCAN_MAX_P and pr.Tmax >= SCAN_MIN_T)):
        return "lanes"
    import ctypes as C
    cl, nc = C.c_int32(0), C.c_int32(0)
    if (lib or load_library()).hhmm_estep_scan_plan(C.byref(pr.req), C.byref(cl), C.byref(nc)) < 0:
        return "lanes"
    return "scan" if cl.value > 0 else "lanes"


def stat_shapes(model, P, K, L):
    """{name: shape} of the statistics estep() returns for `model`."""
    shapes = {"loglik": (P,), "n_1k": (P, K), "xi_ij": (P, K, K)}
    if model == "hmm-multinom":
        shapes["c_kl"] = (P, K, L)
    else:
        shapes.update({"w_k": (P, K), "s1_k": (P, K), "s2_k": (P, K)})
    return shapes


def prepare(model, data, draws, pairing="grid", device=-1):
    """(PreparedRequest, EstepResult, {name: array}) with the shape checks."""
    if model not in MODELS:
        raise ValueError(f"the E-step covers {MODELS}, not {model!r}")

    def param_shapes(S, K, L):
        if model == "hmm-multinom":
            return {"p_1k": (S, K), "A_ij": (S, K, K), "phi_k": (S, K, L)}
        return {"p_1k": (S, K), "A_ij": (S, K, K), "mu_k": (S, K), "sigma_k": (S, K)}

    return _stats.request(model, data, draws, pairing, device, param_shapes,
                          lambda P, K, L: stat_shapes(model, P, K, L))


def estep(model, data, draws, pairing="grid", device=-1, lib=None, return_status=False, schedule="auto", flags=0):
    """Expected sufficient statistics of every (series, draw) pair.

    schedule: "lanes" (a lane, or a group of lanes above K = 8, walks each
    series step by step), "scan" (the parallel scan over T, K <= 8: few pairs,
    long series) or "auto" (resolve_schedule).  flags: HHMM_FLAG_SCAN_* for the
    scan's chunk length (_abi.flag_scan_chunk_log2).

    Returns {name: array}: loglik (P,), n_1k (P, K), xi_ij (P, K, K) and c_kl
    (P, K, L) for hmm-multinom or w_k, s1_k, s2_k (P, K) for hmm.  A pair whose
    log-likelihood is -inf or NaN has NaN statistics.  K <= 32; hhmm_estep_large
    above 8."""
    lib = lib or load_library()
    pr, res, out = prepare(model, data, draws, pairing, device)
    pr.req.flags = int(flags)
    return _stats.call(lib, entry_name(pr.K, resolve_schedule(pr, schedule, lib)), pr, res, out, return_status)


def pair_draw(pairing, P, S, N):
    """The draw index of every pair (include/hhmm.h, "Pairing")."""
    p = np.arange(P)
    return p % S if pairing == "grid" else p


def _ratio(count, par):
    """count / par with 0 / 0 -> 0 (a structural zero has no count and no score)."""
    count, par = np.broadcast_arrays(np.asarray(count, dtype=np.float64), np.asarray(par, dtype=np.float64))
    out = np.zeros(count.shape)
    both0 = (count == 0) & (par == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.divide(count, par, out=out, where=~both0)
    return out


def score(model, draws, stats, pairing, S, N):
    """Gradient of loglik with respect to the constrained parameters, per pair.

    {name: (P, ...)} for p_1k, A_ij and phi_k (hmm-multinom, semisup) or mu_k,
    sigma_k (hmm), by Fisher's identity from the statistics of estep() (K <= 32;
    hhmm_estep_large above 8) or expected_stats().  hhmm-tayal2009: p_11 (P,), n1[0] / p_11 - n1[2] / (1 -
    p_11); A_row (P, 2, 2), (xi[0,1], xi[0,2]) / A_row[0] and (xi[2,0], xi[2,3])
    / A_row[1]; phi_k.  The simplex parameters are treated as free coordinates:
    a directional derivative along a tangent of the simplex is the matching
    difference of entries."""
    if model not in FIT_MODELS:
        raise ValueError(f"score covers {FIT_MODELS}, not {model!r}")
    P = stats["loglik"].shape[0]
    d = pair_draw(pairing, P, S, N)
    if model == "hhmm-tayal2009":
        n1, p11 = stats["n_1k"], np.asarray(draws["p_11"], dtype=np.float64)[d]
        return {"p_11": _ratio(n1[:, 0], p11) - _ratio(n1[:, 2], 1.0 - p11),
                "A_row": _ratio(tayal_rows(stats["xi_ij"]), np.asarray(draws["A_row"])[d]),
                "phi_k": _ratio(stats["c_kl"], np.asarray(draws["phi_k"])[d])}
    g = {"p_1k": _ratio(stats["n_1k"], np.asarray(draws["p_1k"])[d]),
         "A_ij": _ratio(stats["xi_ij"], np.asarray(draws["A_ij"])[d])}
    if model != "hmm":
        g["phi_k"] = _ratio(stats["c_kl"], np.asarray(draws["phi_k"])[d])
    else:
        mu, sg = np.asarray(draws["mu_k"])[d], np.asarray(draws["sigma_k"])[d]
        w, s1, s2 = stats["w_k"], stats["s1_k"], stats["s2_k"]
        g["mu_k"] = (s1 - mu * w) / sg ** 2
        g["sigma_k"] = -w / sg + (s2 - 2 * mu * s1 + mu ** 2 * w) / sg ** 3
    return g


def tayal_rows(xi):
    """(P, 2, 2): the counts of A_row's entries inside xi_ij (hhmm-tayal2009.stan:36-44)."""
    return np.stack([np.stack([xi[:, 0, 1], xi[:, 0, 2]], axis=-1),
                     np.stack([xi[:, 2, 0], xi[:, 2, 3]], axis=-1)], axis=1)


def _rows(counts, prev):
    """Counts over their row sums (last axis); a row whose sum is 0 keeps prev."""
    tot = counts.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        new = counts / tot
    return np.where(tot > 0, new, prev)


def m_step(model, stats, prev=None):
    """One Baum-Welch update from the statistics of estep() (K <= 32;
    hhmm_estep_large above 8): per-pair parameters.

    p_1k = n_1k; rows of A and phi are counts over their row sums (a row whose
    sum is 0 keeps its value in `prev`, {name: (P, ...)}); mu = s1 / w;
    sigma = sqrt(max(s2 / w - mu^2, tiny)).  hhmm-tayal2009 (tied parameters):
    p_11 = n1[0] / (n1[0] + n1[2]), the rows of A_row are (xi[0,1], xi[0,2]) and
    (xi[2,0], xi[2,3]) over their sums, phi_k as above; a zero total keeps
    `prev`."""
    if model not in FIT_MODELS:
        raise ValueError(f"m_step covers {FIT_MODELS}, not {model!r}")
    xi = stats["xi_ij"]
    if model == "hhmm-tayal2009":
        n1, c, rows = stats["n_1k"], stats["c_kl"], tayal_rows(xi)
        tot = n1[:, 0] + n1[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            p11 = np.where(tot == 0, prev["p_11"] if prev is not None else np.nan, n1[:, 0] / tot)
        return {"p_11": p11, "A_row": _rows(rows, prev["A_row"] if prev is not None else np.full(rows.shape, np.nan)),
                "phi_k": _rows(c, prev["phi_k"] if prev is not None else np.full(c.shape, np.nan))}
    pa = prev["A_ij"] if prev is not None else np.full(xi.shape, np.nan)
    new = {"p_1k": np.array(stats["n_1k"]), "A_ij": _rows(xi, pa)}
    if model != "hmm":
        c = stats["c_kl"]
        new["phi_k"] = _rows(c, prev["phi_k"] if prev is not None else np.full(c.shape, np.nan))
    else:
        w = stats["w_k"]
        mu = stats["s1_k"] / w
        new["mu_k"] = mu
        new["sigma_k"] = np.sqrt(np.maximum(stats["s2_k"] / w - mu ** 2, _TINY))
    return new
