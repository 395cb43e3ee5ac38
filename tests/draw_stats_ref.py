"""Reference side of the draw statistics (include/hhmm_gibbs.h).  TEST INFRASTRUCTURE ONLY.

Two things, both plain Python / numpy and sharing no code with the engine:

  counts()      the statistics of a GIVEN path, from the table in the header:
                n_1k, xi_ij and c_kl with the model's forward masks
                (hmm-multinom-semisup.stan:42, hhmm-tayal2009.stan:51 / :62);
                counts_pairs() does it for the (P, T) paths of a request.
  log_weight()  the coded log-weight of a path evaluated directly, step by
                step -- what the counts must reproduce as
                n1 . log p + xi . log A + c . log phi.
  posterior_means()  the exact posterior mean of every free parameter of a
                short series by enumerating all K^T paths: with Dirichlet /
                Beta priors the parameters integrate out of prod p^n1 prod A^xi
                prod phi^c group by group, so a path's marginal weight is a
                product of Dirichlet-multinomial terms; a path through a
                structural zero of the Tayal matrix where the mask is on has
                weight 0.
"""
import itertools
import math

import numpy as np

# hhmm-tayal2009.stan:36-44 -- 0: structural zero, 1: one, (r, c): A_row[r][c]
TAYAL_A = {(0, 1): (0, 0), (0, 2): (0, 1), (1, 0): 1, (2, 0): (1, 0), (2, 3): (1, 1), (3, 2): 1}


def trans_on(model, aux_t, j1):
    """The forward pass multiplies A(i, j) in at a step with aux value aux_t, new state j1 (1-based)."""
    if model == "hmm-multinom-semisup":
        return (aux_t == 1 and j1 in (1, 4)) or (aux_t == 2 and j1 in (2, 3))
    if model == "hhmm-tayal2009":
        return (aux_t == 1 and j1 in (2, 3)) or (aux_t == 2 and j1 in (1, 4))
    return True


def init_on(model, aux_1, j1):
    """The forward pass multiplies p_1k[j] in at t = 1."""
    if model == "hhmm-tayal2009":
        return (aux_1 == 1 and j1 == 3) or (aux_1 == 2 and j1 == 1)
    return True


def counts(model, K, L, z, x, aux=None):
    """(n1 [K], xi [K, K], c [K, L]) of the 1-based path z over the symbols x."""
    n1, xi, c = np.zeros(K), np.zeros((K, K)), np.zeros((K, L))
    T = len(z)
    if init_on(model, None if aux is None else int(aux[0]), int(z[0])):
        n1[int(z[0]) - 1] = 1.0
    for t in range(T):
        c[int(z[t]) - 1, int(x[t]) - 1] += 1.0
        if t >= 1 and trans_on(model, None if aux is None else int(aux[t]), int(z[t])):
            xi[int(z[t - 1]) - 1, int(z[t]) - 1] += 1.0
    return n1, xi, c


def log_weight(model, z, x, aux, p, A, phi):
    """Coded log-weight of the path, factor by factor as the forward pass applies them."""
    lw = 0.0
    with np.errstate(divide="ignore"):
        for t in range(len(z)):
            j = int(z[t]) - 1
            lw += math.log(phi[j][int(x[t]) - 1]) if phi[j][int(x[t]) - 1] > 0 else -math.inf
            a = None if aux is None else int(aux[t])
            if t == 0:
                if init_on(model, a, j + 1):
                    lw += math.log(p[j]) if p[j] > 0 else -math.inf
            elif trans_on(model, a, j + 1):
                v = A[int(z[t - 1]) - 1][j]
                lw += math.log(v) if v > 0 else -math.inf
    return lw


def counts_chains(model, K, L, Z, x, aux=None):
    """counts() for many paths Z (P, T) of ONE series, vectorised over the paths:
    (n1 [P, K], xi [P, K, K], c [P, K, L])."""
    Z = np.asarray(Z)
    P, T = Z.shape
    rows = np.arange(P)
    n1, xi, c = np.zeros((P, K)), np.zeros((P, K, K)), np.zeros((P, K, L))
    on = np.array([init_on(model, None if aux is None else int(aux[0]), j) for j in range(1, K + 1)])[Z[:, 0] - 1]
    n1[rows[on], Z[on, 0] - 1] = 1.0
    for t in range(T):
        np.add.at(c, (rows, Z[:, t] - 1, int(x[t]) - 1), 1.0)
        if t >= 1:
            on = np.array([trans_on(model, None if aux is None else int(aux[t]), j)
                           for j in range(1, K + 1)])[Z[:, t] - 1]
            np.add.at(xi, (rows[on], Z[on, t - 1] - 1, Z[on, t] - 1), 1.0)
    return n1, xi, c


def pair_series(pairing, P, S, N):
    """The series index of every pair (include/hhmm.h, "Pairing")."""
    p = np.arange(P)
    return p // S if pairing == "grid" else (p if pairing == "zip" else p // (S // N))


def counts_pairs(model, data, z, loglik, pairing, S):
    """Reference statistics of a request from its (P, T_max) paths z (0 = undefined)
    and loglik: {n_1k (P, K), xi_ij (P, K, K), c_kl (P, K, L)}; all NaN for a pair
    whose loglik is not finite or whose path has an undefined step."""
    K, L = int(data["K"]), int(data["L"])
    x = np.atleast_2d(np.asarray(data["x"]))
    N, Tm = x.shape
    aux = np.atleast_2d(np.asarray(data["g"] if model == "hmm-multinom-semisup" else data["sign"])) \
        if model != "hmm-multinom" else None
    Ts = np.asarray(data["T"]).reshape(N) if "T" in data else np.full(N, Tm)
    P = z.shape[0]
    ser = pair_series(pairing, P, S, N)
    out = {"n_1k": np.zeros((P, K)), "xi_ij": np.zeros((P, K, K)), "c_kl": np.zeros((P, K, L))}
    for p in range(P):
        n, T = int(ser[p]), int(Ts[ser[p]])
        zp = z[p, :T]
        if not np.isfinite(loglik[p]) or (zp < 1).any():
            for v in out.values():
                v[p] = np.nan
            continue
        out["n_1k"][p], out["xi_ij"][p], out["c_kl"][p] = counts(model, K, L, zp, x[n, :T],
                                                                  None if aux is None else aux[n, :T])
    return out


def tayal_expand(p11, A_row):
    """(p_1k, A_ij) of the flattened Tayal HHMM."""
    A = np.zeros((4, 4))
    for (i, j), code in TAYAL_A.items():
        A[i, j] = 1.0 if code == 1 else A_row[code[0]][code[1]]
    return np.array([p11, 0.0, 1.0 - p11, 0.0]), A


def _lbeta(a):
    return sum(math.lgamma(v) for v in a) - math.lgamma(sum(a))


def groups(model, K, L, n1, xi, c, prior):
    """The free parameter groups with their posterior concentrations:
    [(name, index, concentration vector)], or None for a path of weight 0."""
    def a(name, shape):
        return np.broadcast_to(np.asarray(prior.get(name, 1.0), dtype=float), shape)
    out = []
    if model == "hhmm-tayal2009":
        for i in range(4):
            for j in range(4):
                if xi[i, j] > 0 and (i, j) not in TAYAL_A:
                    return None
        out.append(("p_11", (), a("p_11", (2,)) + np.array([n1[0], n1[2]])))
        ar = a("A_row", (2, 2))
        out.append(("A_row", (0,), ar[0] + np.array([xi[0, 1], xi[0, 2]])))
        out.append(("A_row", (1,), ar[1] + np.array([xi[2, 0], xi[2, 3]])))
    else:
        out.append(("p_1k", (), a("p_1k", (K,)) + n1))
        aA = a("A_ij", (K, K))
        for i in range(K):
            out.append(("A_ij", (i,), aA[i] + xi[i]))
    ap = a("phi_k", (K, L))
    for k in range(K):
        out.append(("phi_k", (k,), ap[k] + c[k]))
    return out


def posterior_means(model, K, L, x, aux=None, prior=None):
    """Exact posterior mean of every free parameter: {name: array} (p_11 a scalar array)."""
    prior = prior or {}
    zero = groups(model, K, L, np.zeros(K), np.zeros((K, K)), np.zeros((K, L)), prior)
    base = sum(_lbeta(g[2]) for g in zero)
    shapes = {"p_11": (), "A_row": (2, 2), "p_1k": (K,), "A_ij": (K, K), "phi_k": (K, L)}
    acc = {name: np.zeros(shapes[name]) for name in {g[0] for g in zero}}
    tot = 0.0
    for z in itertools.product(range(1, K + 1), repeat=len(x)):
        gs = groups(model, K, L, *counts(model, K, L, z, x, aux), prior)
        if gs is None:
            continue
        w = math.exp(sum(_lbeta(g[2]) for g in gs) - base)
        tot += w
        for name, idx, conc in gs:
            m = conc / conc.sum()
            if name == "p_11":
                acc[name] += w * m[0]
            else:
                acc[name][idx] += w * m
    return {name: v / tot for name, v in acc.items()}
