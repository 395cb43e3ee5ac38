"""CPU: the numpy restatement of the PSIS contract (tests/psis_ref.py) pinned
independently of the kernel -- the quantile function against scipy's
generalised Pareto, the fit on Pareto samples of known shape, the integer
rules of the tail, a cell worked by hand in scalar arithmetic, and the LFO
cell of the last step being the LOO cell."""
import math

import numpy as np
import pytest
import scipy.stats

import psis_ref


@pytest.mark.parametrize("k", [-0.3, 0.2, 0.7])
@pytest.mark.parametrize("M", [5, 20, 384])
def test_quantiles_are_scipys_generalised_pareto(k, M):
    sigma = 1.7
    p = (np.arange(1, M + 1) - 0.5) / M
    want = scipy.stats.genpareto.ppf(p, c=k, scale=sigma)
    got = psis_ref.gpd_quantiles(k, sigma, M)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-12
    assert np.allclose(psis_ref.gpd_quantiles(0.0, sigma, M), scipy.stats.expon.ppf(p, scale=sigma), rtol=1e-12, atol=0)


def test_fit_recovers_the_shape_of_pareto_exceedances():
    """4000 exceedances from a GPD with k = 0.5 (the prior's own mean, 5 / 10: no
    shrinkage bias), 20 seeds.  The spread measured over these 20 seeds is a
    standard deviation of 0.0169 (the asymptotic (1 + k) / sqrt(4000) = 0.0237
    bounds it), mean 0.4991, largest deviation 0.0251.  Margins: 4 standard
    deviations, 0.068, for every seed; 3 standard errors of the mean,
    3 * 0.0169 / sqrt(20) = 0.0113, for the mean."""
    ks, sig = [], []
    for seed in range(20):
        g = np.random.Generator(np.random.Philox(key=seed))
        x = np.sort(scipy.stats.genpareto.rvs(0.5, scale=2.0, size=4000, random_state=g))
        k, sigma = psis_ref.gpd_fit(x)
        ks.append(k)
        sig.append(sigma)
    ks = np.array(ks)
    print("k: mean", ks.mean(), "sd", ks.std(ddof=1), "worst", np.abs(ks - 0.5).max(), "sigma: mean", np.mean(sig))
    assert np.abs(ks - 0.5).max() < 0.068
    assert abs(ks.mean() - 0.5) < 0.0113
    assert abs(np.mean(sig) - 2.0) < 0.1


def test_integer_rules_of_the_tail():
    # D: (M, c, m, the 1-based rank of x*)
    want = {24: (4, 15), 25: (5, 15), 26: (5, 16), 100: (20, 30), 4096: (192, 192), 16384: (384, 384)}
    for D, (M, c) in want.items():
        assert psis_ref.tail_length(D) == M, D
        assert c * c >= 9 * D > (c - 1) * (c - 1), D   # c in integers: 9 * 25 = 225 = 15^2 exactly
    assert [psis_ref.xstar_rank(M) for M in (5, 6, 7, 20, 192, 384)] == [1, 2, 2, 5, 48, 96]
    assert [psis_ref.fit_points(M) for M in (5, 8, 9, 20, 384)] == [32, 32, 33, 34, 49]
    # D = 24 leaves no tail to fit; D = 25 is the first that is smoothed
    g = np.random.Generator(np.random.Philox(key=77))
    for D in (24, 25, 26, 100):
        r, l = 2.0 * g.standard_normal(D), g.standard_normal(D) - 3.0
        _elpd, khat, _neff = psis_ref.cell(r, l)
        assert (khat == np.inf) == (D < 25), D
    # x* is the exceedance of that rank: scaling only the others' spacing moves the fit less than moving x* does
    x = np.sort(g.exponential(size=20))
    base = psis_ref.gpd_fit(x)[0]
    moved = x.copy()
    moved[4] = 0.5 * (x[3] + x[4])          # rank 5 of 20
    other = x.copy()
    other[5] = 0.5 * (x[5] + x[6])          # rank 6: enters the sums, not the grid of theta
    th = lambda y: 1.0 / y[-1] + (1.0 - math.sqrt(34 / 0.5)) / (3.0 * y[4])   # noqa: E731  theta_1
    assert th(moved) != th(x) and th(other) == th(x)
    assert psis_ref.gpd_fit(moved)[0] != base


def _cell_by_hand(r, l):
    """D = 25 in scalar arithmetic with the constants written out: M = 5, m = 32, x* = x_1."""
    D = 25
    assert len(r) == D
    top = max(r)
    r = [v - top for v in r]
    order = sorted(range(D), key=lambda d: (r[d], d))
    cut = r[order[19]]
    tail = [r[d] for d in order[20:]]
    x = [math.exp(v) - math.exp(cut) for v in tail]
    theta, L = [], []
    for j in range(1, 33):
        th = 1.0 / x[4] + (1.0 - math.sqrt(32 / (j - 0.5))) / (3.0 * x[0])
        kj = sum(math.log1p(-th * xi) for xi in x) / 5
        theta.append(th)
        L.append(5 * (math.log(-th / kj) - kj - 1.0))
    th = sum(theta[j] / sum(math.exp(L[i] - L[j]) for i in range(32)) for j in range(32))
    k = sum(math.log1p(-th * xi) for xi in x) / 5
    sigma = -k / th
    k = (k * 5 + 5.0) / 15.0
    w = list(r)
    for i in range(1, 6):
        p = (i - 0.5) / 5
        q = sigma * math.expm1(-k * math.log1p(-p)) / k
        w[order[19 + i]] = min(math.log(math.exp(cut) + q), 0.0)
    a, b = max(wi + li for wi, li in zip(w, l)), max(w)
    num = sum(math.exp(wi + li - a) for wi, li in zip(w, l))
    den = sum(math.exp(wi - b) for wi in w)
    return (a + math.log(num)) - (b + math.log(den)), k, den ** 2 / sum(math.exp(2.0 * (wi - b)) for wi in w)


def test_hand_worked_cell_of_25_draws():
    g = np.random.Generator(np.random.Philox(key=25))
    r, l = 1.5 * g.standard_normal(25), g.standard_normal(25) - 2.0
    r[7] = r[3]                                        # a tie below the cut
    want = _cell_by_hand(list(r), list(l))
    got = psis_ref.cell(r, l)
    assert np.isfinite(got).all() and 0.0 < got[2] <= 25.0
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12), (got, want)
    # unsmoothed weights give the plain importance-sampling estimate: the smoothing changed it
    w = r - r.max()
    plain = np.log(np.sum(np.exp(w + l))) - np.log(np.sum(np.exp(w)))
    assert abs(plain - got[0]) > 1e-6


def test_ties_break_by_the_draw_index():
    """Two members with the same r straddle the cut: the smaller index stays below it."""
    g = np.random.Generator(np.random.Philox(key=31))
    D, M = 30, 6
    r = np.sort(g.standard_normal(D))
    r[D - M] = r[D - M - 1]                            # ranks D - M - 1 and D - M are equal
    l = np.zeros(D)
    l[D - M - 1], l[D - M] = -5.0, 5.0
    perm = np.arange(D)
    a = psis_ref.cell(r[perm], l[perm])
    perm[[D - M - 1, D - M]] = perm[[D - M, D - M - 1]]  # the other member first
    b = psis_ref.cell(r[perm], l[perm])
    assert a[1] == b[1] and a[0] != b[0]


def test_special_cells():
    D = 40
    l = np.linspace(-3.0, -1.0, D)
    elpd, khat, neff = psis_ref.cell(np.full(D, 0.3), l)
    assert khat == np.inf and neff == D and np.isclose(elpd, np.log(np.mean(np.exp(l))), rtol=1e-14)
    for bad in (np.nan, np.inf, -np.inf):
        for into in ("r", "l"):
            r, ll = np.linspace(0.0, 1.0, D), l.copy()
            (r if into == "r" else ll)[5] = bad
            assert np.isnan(psis_ref.cell(r, ll)).all()
    assert psis_ref.cell([0.7], [-1.25]) == (-1.25, np.inf, 1.0)


def test_lfo_cell_of_the_last_step_is_the_loo_cell():
    g = np.random.Generator(np.random.Philox(key=9))
    N, D, T = 2, 40, 6
    lp = g.standard_normal((N * D, T)) - 2.0
    Tn = np.array([T, 4])
    lp[D:, 4:] = np.nan
    loo, lfo = psis_ref.from_lp(lp, N, "loo", Tn), psis_ref.from_lp(lp, N, "lfo", Tn)
    for name in loo:
        for n in range(N):
            assert loo[name][n, Tn[n] - 1] == lfo[name][n, Tn[n] - 1], name
            assert np.isnan(lfo[name][n, Tn[n]:]).all() and np.isfinite(lfo[name][n, :Tn[n]]).all()
        assert not np.array_equal(loo[name][:, 0], lfo[name][:, 0]), name
    r = psis_ref.log_ratios(lp, N, "lfo", Tn)
    assert np.array_equal(r[:D, T - 1], -lp[:D, T - 1]) and np.array_equal(r[:D, T - 2], -(lp[:D, T - 1] + lp[:D, T - 2]))
    assert np.isnan(r[D:, 4:]).all()
