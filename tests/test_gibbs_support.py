"""Structural zeros in the conjugate updates: the `support` argument of conditional_draw / gibbs and of
conditional_draw_gauss / gibbs_gauss (hhmm_amd/gibbs.py, hhmm_amd/gibbs_gauss.py).

A flattened hierarchical HMM has a sparse transition matrix.  A zero prior concentration does not keep it
sparse: torch's gamma sampler returns the smallest normal number for it, not 0.  With support={name: mask} the
drawn parameter is an exact 0 outside the mask, every Dirichlet row is drawn over its supported entries, and a
row whose statistics hold a positive count outside its support is NaN.  The default None is the draw as it
was before the argument existed, bit for bit: the old formula is restated here.

gpu: gibbs(..., support=band) at K = 12 keeps every kept A_ij exactly 0 outside the band.
"""
import numpy as np
import pytest

import hhmm_amd

K, L, P = 12, 5, 7
BAND = np.abs(np.subtract.outer(np.arange(K), np.arange(K))) <= 2


def old_dirichlet(torch, conc, generator):
    """_dirichlet as it was before `support`."""
    bad = torch.isnan(conc).any(dim=-1, keepdim=True)
    g = torch._standard_gamma(torch.where(bad, torch.ones_like(conc), conc), generator=generator)
    return torch.where(bad, torch.full_like(g, float("nan")), g / g.sum(dim=-1, keepdim=True))


def counts(seed=0, gauss=False):
    """Statistics whose transitions stay inside the band."""
    g = np.random.Generator(np.random.Philox(key=500 + seed))
    st = {"n_1k": np.eye(K)[g.integers(0, K, size=P)], "xi_ij": g.integers(0, 6, size=(P, K, K)) * BAND * 1.0}
    if gauss:
        w = 1.0 + st["xi_ij"].sum(axis=1)
        st.update(w_k=w, s1_k=g.normal(0.0, 1.0, size=(P, K)) * w, s2_k=(1.0 + g.uniform(0, 1, size=(P, K))) * w * 4.0)
    else:
        st["c_kl"] = g.integers(0, 6, size=(P, K, L)) * 1.0
    return st


GPRIOR = {"mu_sigma": (0.0, 1.0, 3.0, 2.0)}


def test_default_is_the_old_draw_bit_for_bit():
    import torch
    st = counts()
    st["c_kl"][3] = np.nan
    prior = {"A_ij": 0.5, "phi_k": np.linspace(0.5, 2.0, L)}
    for kw in ({}, {"support": None}):
        used = torch.Generator().manual_seed(5)
        new = hhmm_amd.conditional_draw("hmm-multinom", st, prior, used, **kw)
        gen = torch.Generator().manual_seed(5)
        want = {"p_1k": old_dirichlet(torch, torch.as_tensor(st["n_1k"]) + 1.0, gen),
                "A_ij": old_dirichlet(torch, torch.as_tensor(st["xi_ij"]) + 0.5, gen),
                "phi_k": old_dirichlet(torch, torch.as_tensor(st["c_kl"]) + torch.as_tensor(prior["phi_k"]), gen)}
        for name, v in want.items():
            assert np.array_equal(new[name].numpy(), v.numpy(), equal_nan=True), name
        # the generator has been consumed alike: the next draw agrees too
        assert torch.equal(torch.rand(4, generator=used), torch.rand(4, generator=gen))


def test_default_is_the_old_gaussian_draw_bit_for_bit():
    import torch
    st = counts(gauss=True)
    a = hhmm_amd.conditional_draw_gauss(st, GPRIOR, torch.Generator().manual_seed(5))
    b = hhmm_amd.conditional_draw_gauss(st, GPRIOR, torch.Generator().manual_seed(5), support=None)
    # an all-true mask masks nothing: the same gammas, the same bits
    c = hhmm_amd.conditional_draw_gauss(st, GPRIOR, torch.Generator().manual_seed(5),
                                        support={"A_ij": np.ones((K, K), dtype=bool), "p_1k": np.ones(K, dtype=bool)})
    for name in a:
        assert np.array_equal(a[name].numpy(), b[name].numpy()) and np.array_equal(a[name].numpy(), c[name].numpy())
    # p_1k and A_ij are drawn last (after the gamma and the normal of mu, sigma): restated from the same state
    gen = torch.Generator().manual_seed(5)
    torch._standard_gamma(torch.as_tensor(3.0 + 0.5 * st["w_k"]), generator=gen)
    torch.randn((P, K), dtype=torch.float64, generator=gen)
    assert np.array_equal(a["p_1k"].numpy(), old_dirichlet(torch, torch.as_tensor(st["n_1k"]) + 1.0, gen).numpy())
    assert np.array_equal(a["A_ij"].numpy(), old_dirichlet(torch, torch.as_tensor(st["xi_ij"]) + 1.0, gen).numpy())


def test_zero_concentration_alone_does_not_keep_a_zero():
    """What `support` is for: Dir with concentration 0 outside the band comes back positive there."""
    import torch
    st = counts()
    new = hhmm_amd.conditional_draw("hmm-multinom", st, {"A_ij": BAND * 1.0}, torch.Generator().manual_seed(1))
    assert (new["A_ij"].numpy()[:, ~BAND] > 0.0).all()


@pytest.mark.parametrize("family", ["multinom", "gauss"])
def test_band_mask_gives_exact_zeros_and_rows_over_the_support(family):
    import torch
    gauss = family == "gauss"
    st = counts(1, gauss)
    first = np.arange(K) < 4                                              # z_1 is one of the first four states
    st["n_1k"] = np.eye(K)[np.arange(P) % 4]
    support = {"A_ij": BAND, "p_1k": first}
    gen = torch.Generator().manual_seed(2)
    if gauss:
        new = hhmm_amd.conditional_draw_gauss(st, GPRIOR, gen, support=support)
    else:
        new = hhmm_amd.conditional_draw("hmm-multinom", st, None, gen, support=support)
    A, p1 = new["A_ij"].numpy(), new["p_1k"].numpy()
    assert (A[:, ~BAND] == 0.0).all() and (A[:, BAND] > 0.0).all()
    assert (p1[:, ~first] == 0.0).all() and (p1[:, first] > 0.0).all()
    assert np.abs(np.where(BAND, A, 0.0).sum(axis=-1) - 1.0).max() <= 1e-12
    assert np.abs(p1[:, first].sum(axis=-1) - 1.0).max() <= 1e-12
    other = "mu_k" if gauss else "phi_k"
    assert np.isfinite(new[other].numpy()).all() and (gauss or (new[other].numpy() > 0.0).all())
    # the supported entries are the Dirichlet over the support: a strong prior pins them
    m = BAND / BAND.sum(axis=1, keepdims=True)
    zero = {k: np.zeros_like(v) for k, v in st.items()}
    if gauss:
        zero["w_k"] += 1.0
        pinned = hhmm_amd.conditional_draw_gauss(zero, dict(GPRIOR, A_ij=1e8 * m + ~BAND), gen, support=support)
    else:
        pinned = hhmm_amd.conditional_draw("hmm-multinom", zero, {"A_ij": 1e8 * m + ~BAND}, gen, support=support)
    assert np.abs(pinned["A_ij"].numpy() - m).max() < 1e-3


@pytest.mark.parametrize("family", ["multinom", "gauss"])
def test_a_count_outside_the_support_and_nan_statistics_are_nan(family):
    import torch
    gauss = family == "gauss"
    st = counts(2, gauss)
    st["xi_ij"][1, 0, 7] = 1.0                                   # planted outside the band: row 0 of pair 1
    for v in st.values():
        v[4] = np.nan
    gen = torch.Generator().manual_seed(3)
    support = {"A_ij": BAND}
    if gauss:
        new = hhmm_amd.conditional_draw_gauss(st, GPRIOR, gen, support=support)
    else:
        new = hhmm_amd.conditional_draw("hmm-multinom", st, None, gen, support=support)
    A = new["A_ij"].numpy()
    assert np.isnan(A[1, 0]).all() and np.isfinite(A[1, 1:]).all()
    assert all(np.isnan(v.numpy()[4]).all() for v in new.values())
    keep = np.ones(P, dtype=bool)
    keep[[1, 4]] = False
    assert np.isfinite(A[keep]).all() and (A[keep][:, ~BAND] == 0.0).all()
    assert all(np.isfinite(v.numpy()[keep]).all() for v in new.values())


def test_unknown_support_names_are_rejected():
    import torch
    gen = torch.Generator().manual_seed(3)
    with pytest.raises(ValueError, match="support"):
        hhmm_amd.conditional_draw("hmm-multinom", counts(), None, gen, support={"A": BAND})
    with pytest.raises(ValueError, match="support"):
        hhmm_amd.conditional_draw_gauss(counts(gauss=True), GPRIOR, gen, support={"mu_k": np.ones(K, dtype=bool)})
    # a mask ties the parameters to the labels: sorting the kept draws by mu_k is not exact any more
    data, init = banded_init(True, 3, 0)
    with pytest.raises(ValueError, match="relabel"):
        hhmm_amd.gibbs_gauss(data, init, 2, prior=GPRIOR, relabel=True, support={"A_ij": BAND})


# ---------------------------------------------------------------- GPU

def banded_init(gauss, chains, seed):
    g = np.random.Generator(np.random.Philox(key=600 + seed))
    A = g.dirichlet(np.full(K, 2.0), size=(chains, K)) * BAND
    init = {"p_1k": g.dirichlet(np.full(K, 2.0), size=chains), "A_ij": A / A.sum(axis=2, keepdims=True)}
    if gauss:
        init["mu_k"] = np.tile(np.linspace(-3.0, 3.0, K), (chains, 1))
        init["sigma_k"] = np.ones((chains, K))
        return {"K": K, "x": g.normal(0.0, 2.0, size=(chains, 30))}, init
    init["phi_k"] = g.dirichlet(np.full(L, 2.0), size=(chains, K))
    return {"K": K, "L": L, "x": g.integers(1, L + 1, size=(chains, 30)).astype(np.int32)}, init


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["multinom", "gauss"])
def test_gpu_gibbs_keeps_a_banded_matrix_banded(engine, family):
    gauss = family == "gauss"
    data, init = banded_init(gauss, 6, 1)
    if gauss:
        draws, trace = hhmm_amd.gibbs_gauss(data, init, 5, prior=GPRIOR, seed=4, support={"A_ij": BAND}, lib=engine)
    else:
        draws, trace = hhmm_amd.gibbs("hmm-multinom", data, init, 5, seed=4, support={"A_ij": BAND}, lib=engine)
    assert trace.shape == (5, 6) and np.isfinite(trace).all()
    assert draws["A_ij"].shape == (5, 6, K, K)
    assert (draws["A_ij"][..., ~BAND] == 0.0).all() and (draws["A_ij"][..., BAND] > 0.0).all()
    assert all(np.isfinite(v).all() for v in draws.values())
    # without the argument the matrix fills in after one sweep
    if gauss:
        dense, _t = hhmm_amd.gibbs_gauss(data, init, 1, prior=GPRIOR, seed=4, lib=engine)
    else:
        dense, _t = hhmm_amd.gibbs("hmm-multinom", data, init, 1, seed=4, lib=engine)
    assert (dense["A_ij"][..., ~BAND] > 0.0).all()
