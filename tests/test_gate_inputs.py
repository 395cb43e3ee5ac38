"""CPU: the inputs of tests/test_gpu_renorm_gate.py are what that file says.

* b (gate_inputs.gate_b: phi_min * min(min_i rowmax_i(A), min_i colmax_i(A)))
  is sqrt(2) above the gate's bound 2^-39 at every `inside` pair and sqrt(2)
  below it at every `outside` pair; `mixed` alternates the two over its first
  64 draws and is inside from there on.  Every row of phi_k and A_ij is a
  simplex to within 4 ulp.
* On these inputs the oracle's outputs are all finite, pair_status is 0, and
  no gamma entry is below 1e-240: the 1e-250 floor of tests/tolerances.py
  excuses nothing in the GPU comparison.  The smallest gamma is still far
  below 1 where the builder makes the components diverge (one_likely_state,
  rare_state), so a renormalisation that lost low components would show.
* The oracle itself is pinned on them: its libm build is bit-equal to the
  independent transcription (tests/oracle_numpy.py) on a two-pair sub-batch
  of the rare_symbol inside case, and at the (K, L) the hot-sweep cases of
  tests/test_gpu_hot_sweeps.py use."""
import numpy as np
import pytest

import gate_inputs
import oracle_numpy as onp
from gate_inputs import BOUND, BUILDERS, SIDES, gate_b, simplex_error_ulps
from hhmm_amd import synth
from test_oracle import _compare_exact

MODEL = "hmm-multinom"
PARS = synth.PARS[MODEL]
KS = [2, 3, 4, 8, 12, 23]


def test_gate_b_is_the_kernels_formula():
    """A hand-checked matrix: row maxima (0.7, 0.6), column maxima (0.7, 0.6): tmin = 0.6; phi_min = 0.05."""
    draws = {"A_ij": np.array([[[0.7, 0.3], [0.4, 0.6]]]), "phi_k": np.array([[[0.05, 0.95], [0.5, 0.5]]])}
    assert gate_b(draws)[0] == 0.05 * 0.6
    # a column whose largest entry is small bounds the backward step
    draws["A_ij"] = np.array([[[0.9, 0.1], [0.8, 0.2]]])
    assert gate_b(draws)[0] == 0.05 * 0.2


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_b_sits_where_the_side_says(builder, side, K):
    for pairing in ("zip", "grid"):
        data, draws = BUILDERS[builder](side, K=K, pairing=pairing)
        b = gate_b(draws)
        S = b.size
        assert S == (130 if pairing == "zip" else 65)
        want_in = np.ones(S, dtype=bool)
        if side == "outside":
            want_in[:] = False
        elif side == "mixed":
            want_in[1:64:2] = False
            assert want_in[:64].sum() == 32 and want_in[64:].all() and S > 64
        inside, outside = b[want_in], b[~want_in]
        assert ((inside > 2.0 ** -39) & (inside <= 2.0 ** -37)).all()
        assert ((outside >= 2.0 ** -41) & (outside < 2.0 ** -39)).all()
        # sqrt(2) of margin on either side, at every pair
        assert np.allclose(inside / BOUND, 2.0 ** 0.5, rtol=1e-12) and np.allclose(outside / BOUND, 2.0 ** -0.5,
                                                                                    rtol=1e-12)
        assert simplex_error_ulps(draws["phi_k"]) <= 4 and simplex_error_ulps(draws["A_ij"]) <= 4
        assert (draws["phi_k"] > 0).all() and (draws["A_ij"] > 0).all()
        x = np.asarray(data["x"])
        assert x.min() >= 1 and x.max() <= 9
        if builder != "rare_state":
            assert (x[:, gate_inputs.RUN] == 9).all() and gate_inputs.RUN.stop - gate_inputs.RUN.start == 40


# smallest gamma of the K = 4 inside batch, as the oracle gives it: the components the sparse cadence must keep
DIVERGED = {"one_likely_state": (1e-20, 1e-12), "rare_state": (1e-18, 1e-10)}


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_oracle_outputs_stay_clear_of_the_floor(oracle, builder, side, K):
    data, draws = BUILDERS[builder](side, K=K)
    ref = oracle.gqs(MODEL, data, draws, pars=PARS, pairing="zip", return_status=True, nthreads=8)
    assert all(np.isfinite(ref[k]).all() for k in PARS if k != "zstar_t")
    assert not ref["pair_status"].any() and ref["status"] == 0
    g = ref["gamma_tk"]
    print(f"{builder} {side} K={K}: smallest gamma {g.min():.2e}, alpha {ref['alpha_tk'].min():.2e}, "
          f"beta {ref['beta_tk'].min():.2e}")
    assert float((g < 1e-240).mean()) == 0.0
    assert g.min() > 1e-240 and ref["alpha_tk"].min() > 1e-240 and ref["beta_tk"].min() > 1e-240
    if K == 4 and side == "inside" and builder in DIVERGED:
        lo, hi = DIVERGED[builder]
        assert lo < g.min() < hi


def _sub(data, draws, idx):
    d = dict(data, x=np.asarray(data["x"])[idx])
    return d, {k: np.asarray(v)[idx] for k, v in draws.items()}


def test_oracle_is_the_transcription_at_the_gate(oracle):
    """Two pairs of the rare_symbol inside batch (zip): libm build == tests/oracle_numpy.py, bit for bit."""
    data, draws = _sub(*BUILDERS["rare_symbol"]("inside"), [0, 77])
    ref = oracle.gqs(MODEL, data, draws, pars=PARS, pairing="zip", variant="libm", return_status=True)
    _compare_exact(MODEL, ref, onp.run(MODEL, data, draws, pairing="zip"), PARS)


@pytest.mark.parametrize("builder", ["one_likely_state", "rare_state"])
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_oracle_is_the_transcription_on_the_other_builders(oracle, builder, side):
    data, draws = _sub(*BUILDERS[builder](side), [1, 64])
    ref = oracle.gqs(MODEL, data, draws, pars=PARS, pairing="zip", variant="libm", return_status=True)
    _compare_exact(MODEL, ref, onp.run(MODEL, data, draws, pairing="zip"), PARS)


@pytest.mark.parametrize("K,L", [(4, 16), (4, 17), (4, 1), (1, 1), (2, 16), (3, 15), (5, 16), (8, 2)])
def test_oracle_is_the_transcription_at_the_hot_sweep_shapes(oracle, K, L):
    data, draws = synth.hmm_multinom(N=2, S=2, T=33, K=K, L=L)
    data["T"] = np.array([33, 17], dtype=np.int32)
    ref = oracle.gqs(MODEL, data, draws, pars=PARS, variant="libm", return_status=True)
    _compare_exact(MODEL, ref, onp.run(MODEL, data, draws), PARS)
