"""Reference side of the Gaussian draw statistics (include/hhmm_gibbs_gauss.h).  TEST INFRASTRUCTURE ONLY.

Plain Python / numpy, sharing no code with the engine:

  stats()            the statistics of a GIVEN path from the table in the header;
                     hmm.stan:30 (Q2) makes x_1 count once for EVERY state.
                     Sums are math.fsum (correctly rounded).
  stats_pairs()      the same for the (P, T) paths of a request.
  log_weight()       the coded log-weight of a path, step by step.
  log_weight_stats() the same through the closed form in the statistics.
  posterior_means()  the exact posterior means of a short series by enumerating
                     all K^T paths: with Dirichlet priors on p_1k and the rows of
                     A_ij and a Normal-Inverse-Gamma prior on (mu_k, sigma_k^2)
                     the parameters integrate out of the coded weight state by
                     state.
"""
import itertools
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)


def stats(z, x, K):
    """(n1 [K], xi [K, K], w [K], s1 [K], s2 [K]) of the 1-based path z over the series x."""
    n1, xi = np.zeros(K), np.zeros((K, K))
    own = [[] for _ in range(K)]
    n1[int(z[0]) - 1] = 1.0
    for t in range(1, len(z)):
        xi[int(z[t - 1]) - 1, int(z[t]) - 1] += 1.0
        own[int(z[t]) - 1].append(float(x[t]))
    x1 = float(x[0])
    w = np.array([1.0 + len(o) for o in own])
    s1 = np.array([math.fsum([x1] + o) for o in own])
    s2 = np.array([math.fsum([x1 * x1] + [v * v for v in o]) for o in own])
    return n1, xi, w, s1, s2


def pair_series(pairing, P, S, N):
    """The series index of every pair (include/hhmm.h, "Pairing")."""
    p = np.arange(P)
    return p // S if pairing == "grid" else (p if pairing == "zip" else p // (S // N))


NAMES = ("n_1k", "xi_ij", "w_k", "s1_k", "s2_k")


def stats_pairs(data, z, loglik, pairing, S):
    """Reference statistics of a request from its (P, T_max) paths z (0 = undefined) and loglik; all NaN for a
    pair whose loglik is not finite or whose path has an undefined step."""
    K = int(data["K"])
    x = np.atleast_2d(np.asarray(data["x"], dtype=np.float64))
    N, Tm = x.shape
    Ts = np.asarray(data["T"]).reshape(N) if "T" in data else np.full(N, Tm)
    P = z.shape[0]
    ser = pair_series(pairing, P, S, N)
    out = {"n_1k": np.zeros((P, K)), "xi_ij": np.zeros((P, K, K)), "w_k": np.zeros((P, K)),
           "s1_k": np.zeros((P, K)), "s2_k": np.zeros((P, K))}
    for p in range(P):
        n, T = int(ser[p]), int(Ts[ser[p]])
        zp = z[p, :T]
        if not np.isfinite(loglik[p]) or (zp < 1).any():
            for v in out.values():
                v[p] = np.nan
            continue
        for name, v in zip(NAMES, stats(zp, x[n, :T], K)):
            out[name][p] = v
    return out


def stats_chains(Z, x, K):
    """stats() for many paths Z (P, T) of ONE series, vectorised over the paths (plain fp64 additions in the
    order of t, not fsum: for the samplers): (n1 [P, K], xi [P, K, K], w, s1, s2 [P, K])."""
    Z = np.asarray(Z)
    P, T = Z.shape
    rows = np.arange(P)
    n1, xi = np.zeros((P, K)), np.zeros((P, K, K))
    x1 = float(x[0])
    w, s1, s2 = np.ones((P, K)), np.full((P, K), x1), np.full((P, K), x1 * x1)
    n1[rows, Z[:, 0] - 1] = 1.0
    for t in range(1, T):
        xt = float(x[t])
        np.add.at(xi, (rows, Z[:, t - 1] - 1, Z[:, t] - 1), 1.0)
        np.add.at(w, (rows, Z[:, t] - 1), 1.0)
        np.add.at(s1, (rows, Z[:, t] - 1), xt)
        np.add.at(s2, (rows, Z[:, t] - 1), xt * xt)
    return n1, xi, w, s1, s2


def _normal_lpdf(x, mu, sigma):
    zz = (x - mu) / sigma
    return -0.5 * LOG_2PI - math.log(sigma) - 0.5 * zz * zz


def log_weight(z, x, p, A, mu, sigma):
    """Coded log-weight of the 1-based path z, factor by factor as hmm.stan's forward pass applies them."""
    K = len(mu)
    j = int(z[0]) - 1
    lw = math.log(p[j])
    for k in range(K):  # Q2: every state takes x_1
        lw += _normal_lpdf(float(x[0]), mu[k], sigma[k])
    for t in range(1, len(z)):
        i, j = int(z[t - 1]) - 1, int(z[t]) - 1
        lw += math.log(A[i][j]) + _normal_lpdf(float(x[t]), mu[j], sigma[j])
    return lw


def log_weight_stats(n1, xi, w, s1, s2, p, A, mu, sigma):
    """The closed form: n1 . log p + xi . log A
    + sum_k -(w/2) log 2 pi - w log sigma - (s2 - 2 mu s1 + mu^2 w) / (2 sigma^2)."""
    p, A = np.asarray(p, dtype=float), np.asarray(A, dtype=float)
    lw = float((n1[n1 > 0] * np.log(p[n1 > 0])).sum()) + float((xi[xi > 0] * np.log(A[xi > 0])).sum())
    for k in range(len(mu)):
        q = s2[k] - 2.0 * mu[k] * s1[k] + mu[k] * mu[k] * w[k]
        lw += -0.5 * w[k] * LOG_2PI - w[k] * math.log(sigma[k]) - q / (2.0 * sigma[k] * sigma[k])
    return lw


def _lbeta(a):
    return sum(math.lgamma(v) for v in a) - math.lgamma(sum(a))


def nig_posterior(w, s1, s2, m0, k0, a0, b0):
    """(kn, mn, an, bn) of one state."""
    kn = k0 + w
    mn = (k0 * m0 + s1) / kn
    an = a0 + 0.5 * w
    bn = max(b0, b0 + 0.5 * (s2 + k0 * m0 * m0 - kn * mn * mn))
    return kn, mn, an, bn


def posterior_means(x, prior, K):
    """Exact posterior means {p_1k, A_ij, mu_k, sigma2_k, sigma_k} of the series x under the coded weight.

    prior: {"mu_sigma": (m0, kappa0, a0, b0) each broadcastable to (K,), "p_1k", "A_ij": concentrations
    (default 1)}.  Per path the marginal weight is the Dirichlet-multinomial term of p_1k and of every row of
    A_ij times, per state, (2 pi)^(-w/2) sqrt(kappa0 / kn) Gamma(an) / Gamma(a0) b0^a0 / bn^an."""
    m0, k0, a0, b0 = (np.broadcast_to(np.asarray(v, dtype=float), (K,)) for v in prior["mu_sigma"])
    cp = np.broadcast_to(np.asarray(prior.get("p_1k", 1.0), dtype=float), (K,))
    cA = np.broadcast_to(np.asarray(prior.get("A_ij", 1.0), dtype=float), (K, K))
    base = _lbeta(cp) + sum(_lbeta(cA[i]) for i in range(K))
    acc = {"p_1k": np.zeros(K), "A_ij": np.zeros((K, K)), "mu_k": np.zeros(K), "sigma2_k": np.zeros(K),
           "sigma_k": np.zeros(K)}
    logs, terms = [], []
    for z in itertools.product(range(1, K + 1), repeat=len(x)):
        n1, xi, w, s1, s2 = stats(z, x, K)
        lw = _lbeta(cp + n1) + sum(_lbeta(cA[i] + xi[i]) for i in range(K)) - base
        t = {"p_1k": (cp + n1) / (cp + n1).sum(), "A_ij": (cA + xi) / (cA + xi).sum(axis=1, keepdims=True),
             "mu_k": np.zeros(K), "sigma2_k": np.zeros(K), "sigma_k": np.zeros(K)}
        for k in range(K):
            kn, mn, an, bn = nig_posterior(w[k], s1[k], s2[k], m0[k], k0[k], a0[k], b0[k])
            lw += (-0.5 * w[k] * LOG_2PI + 0.5 * math.log(k0[k] / kn) + math.lgamma(an) - math.lgamma(a0[k]) +
                   a0[k] * math.log(b0[k]) - an * math.log(bn))
            t["mu_k"][k] = mn
            t["sigma2_k"][k] = bn / (an - 1.0)
            t["sigma_k"][k] = math.sqrt(bn) * math.exp(math.lgamma(an - 0.5) - math.lgamma(an))
        logs.append(lw)
        terms.append(t)
    top = max(logs)
    tot = 0.0
    for lw, t in zip(logs, terms):
        wgt = math.exp(lw - top)
        tot += wgt
        for name in acc:
            acc[name] += wgt * t[name]
    return {name: v / tot for name, v in acc.items()}
