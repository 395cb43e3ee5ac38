"""GPU: a NaN draw parameter against the oracle, on every decoder and
forward-backward schedule.

A sampler can hand over a NaN draw.  The reference computes such a draw like
any other: in log space a NaN poisons the sums it enters (loglik and the
posteriors of that draw become NaN), while the Viterbi's strict `logp > delta`
from -inf never lets a NaN candidate win, so zstar_t and logp_zstar stay
finite wherever a finite candidate exists (hmm/stan/hmm.stan:103-117).  The
oracle restates that, and the device must place every NaN and decode every
path exactly as it does: one draw of 64 is spoiled, two series, T = 60, GRID.

Kinds: A_ij[s, 0, j] for each column j (candidate 0 of column j is NaN at every
step: the running max must not start from it), A_ij[s, K-1, 0], one emission
parameter of state 2 (phi_k[s, 1, l]; mu_k[s, 1] for hmm.stan), p_1k[s, 0], and
w_km[s, 0, 0] for iohmm-reg.  FFBS and the fitted draws are not covered, nor
infinite parameters (the two arithmetics part there, tests/test_gpu_table4.py)."""
import functools

import numpy as np
import pytest

from hhmm_amd import _abi, synth
from hot_plan import SCHEDULE_PLAN, assert_plan
from tolerances import compare_all

pytestmark = pytest.mark.gpu

PARS = ["loglik", "gamma_tk", "zstar_t", "logp_zstar"]
N, S, T, SPOILED = 2, 64, 60, 5

MULTINOM4 = ("hmm-multinom", (("K", 4), ("L", 9)))
_LANES = _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF | _abi.FLAG_VIT_LANES
def _plan(schedule="separate", fb="linear", fb_mode="GAMMA", vit="lanes", **more):
    return dict(schedule=schedule, fb=fb, fb_mode=fb_mode, vit=vit, **more)


_BIG = "GAMMA|PACK|BIG"
_NONE = dict(schedule="none")    # not an HMM-family request at K <= 8: no plan (hhmm_large.h, hhmm_iohmm.h)
PATHS = [
    # (id, (model, sizes), flags, the plan words the request must give: asserted before the run)
    # At K <= 4 a batch this small decodes state-parallel (use_vit_states: P < 131072): these five rows
    # share viterbi_sp_kernel and differ in the forward-backward half (fb_kernel on its own or beside the
    # decoder, its forward launch alone, the T-scan).
    ("multinom-states-default", MULTINOM4, 0, _plan(fb_mode=_BIG, vit="states")),
    ("multinom-states-vfb-off", MULTINOM4, _abi.FLAG_VFB_OFF, _plan(fb_mode=_BIG, vit="states")),
    ("multinom-states-fb-split", MULTINOM4, _abi.FLAG_FB_SPLIT, _plan(fb_mode=_BIG, vit="states")),
    ("multinom-states-forced", MULTINOM4, _abi.FLAG_VIT_STATES, _plan(fb_mode=_BIG, vit="states")),
    ("multinom-states-tscan", MULTINOM4, _abi.FLAG_SCAN_FORCE, _plan(fb="scan", vit="states", scan_nc="1")),
    ("hmm-K3", ("hmm", (("K", 3),)), 0, _plan(vit="states")),
    ("multinom-K12", ("hmm-multinom", (("K", 12), ("L", 9))), 0, _NONE),
    ("iohmm-reg-K3", ("iohmm-reg", (("K", 3),)), 0, _NONE),
    # The rows above never reach the lane-per-pair recursions that the large batches run (vit_step: the
    # phased sweep, viterbi_kernel, the split and the fused sweeps).  FLAG_VIT_LANES puts this batch on
    # them; K = 6 takes them by default.
    ("multinom-lanes-phased", MULTINOM4, _LANES, SCHEDULE_PLAN["phased"]),
    ("multinom-lanes-two-kernels", MULTINOM4, _LANES | _abi.FLAG_VFB_OFF, SCHEDULE_PLAN["two-kernels"]),
    ("multinom-lanes-fb-split", MULTINOM4, _LANES | _abi.FLAG_FB_SPLIT, SCHEDULE_PLAN["split"]),
    ("multinom-lanes-fused", MULTINOM4, _LANES | _abi.FLAG_FUSED, SCHEDULE_PLAN["fused"]),
    ("hmm-K3-lanes", ("hmm", (("K", 3),)), _LANES, _plan()),
    ("multinom-K6", ("hmm-multinom", (("K", 6), ("L", 9))), 0, _plan(fb_mode="GAMMA|PACK")),
    ("iohmm-reg-K3-lanes", ("iohmm-reg", (("K", 3),)), _LANES, _NONE),
    ("tayal-lanes", ("hhmm-tayal2009", (("K", 4),)), _LANES, _plan()),
    # the T-parallel exact decoder (hhmm_vscan.h: chosen by itself for few long series), forced below its
    # automatic range.  Its chunk 0 runs the step decoder and T = 60 is one chunk of 512 steps, so the
    # T = 1100 rows add the chunk products, the tie grid and the chunk-parallel back-trace (3 chunks);
    # at T = 1100 >= 256 the forward-backward beside it is the T-scan.
    ("multinom-vit-scan", MULTINOM4, _abi.FLAG_VIT_SCAN, _plan(fb_mode=_BIG, vit="vscan", vs_nc="1")),
    ("hmm-K4-vit-scan", ("hmm", (("K", 4),)), _abi.FLAG_VIT_SCAN, _plan(vit="vscan", vs_nc="1")),
    ("tayal-vit-scan", ("hhmm-tayal2009", (("K", 4),)), _abi.FLAG_VIT_SCAN, _plan(vit="vscan", vs_nc="1")),
    ("multinom-vit-scan-T1100", ("hmm-multinom", (("K", 4), ("L", 9), ("T", 1100))), _abi.FLAG_VIT_SCAN,
     _plan(fb="scan", vit="vscan", vs_nc="3")),
    ("hmm-K4-vit-scan-T1100", ("hmm", (("K", 4), ("T", 1100))), _abi.FLAG_VIT_SCAN,
     _plan(fb="scan", vit="vscan", vs_nc="3")),
]

# Seeds at which the oracle's path of the spoiled draw enters column j from
# state 2 (a back-pointer of 1: the first candidate after the NaN one) at least
# once, found by running the oracle over seeds 9000...  (model, K[, T]) -> {j: seed}.
# hmm-multinom K = 4, j = 1 and 3: state 2 of hmm/main-multinom-semisup.R's A
# moves to state 1 only, no seed of 400 takes that step, so these columns (and
# K = 12, j = 10) run the comparison without the assertion.
BP1_SEEDS = {
    ("hmm-multinom", 4): {0: 9000, 2: 9001},
    ("hmm-multinom", 4, 1100): {0: 9000, 2: 9000},
    ("hmm", 4, 1100): {0: 9000, 1: 9000, 2: 9000, 3: 9000},
    ("hmm", 3): {0: 9000, 1: 9000, 2: 9000},
    ("hmm", 4): {0: 9000, 1: 9000, 2: 9000, 3: 9000},
    ("hmm-multinom", 6): {0: 9033, 1: 9000, 2: 9003, 3: 9000, 4: 9000, 5: 9005},
    ("hmm-multinom", 12): {0: 9057, 1: 9000, 2: 9007, 3: 9011, 4: 9011, 5: 9003, 6: 9000, 7: 9001, 8: 9002,
                           9: 9016, 11: 9004},
}


def _seed_key(mk):
    kw = dict(mk[1])
    return (mk[0], kw["K"]) + ((kw["T"],) if "T" in kw else ())


def _kinds(model, K):
    if model == "iohmm-reg":
        return ["p1", "w"]
    if model == "hhmm-tayal2009":    # p_11, A_row and phi_k: the draws of tests/test_gpu_table4.py
        return ["p11", "A-row", "emission"]
    return [f"A-0-{j}" for j in range(K)] + ["A-last-0", "emission", "p1"]


CASES = [(pid, mk, flags, kind) for pid, mk, flags, _ in PATHS for kind in _kinds(mk[0], dict(mk[1])["K"])]
PLANS = {pid: plan for pid, _, _, plan in PATHS}


@functools.lru_cache(maxsize=None)
def _request(mk, kind):
    """The spoiled request and the oracle's outputs: computed once per (model, kind), shared by every
    schedule and only read."""
    import pyoracle
    model, kw = mk[0], dict(mk[1])
    K = kw["K"]
    seed = synth.SEED
    if kind.startswith("A-0-"):
        seed = BP1_SEEDS.get(_seed_key(mk), {}).get(int(kind[4:]), synth.SEED)
    if model == "hhmm-tayal2009":
        kw.pop("K")                              # a K = 4 model
    data, draws = synth.GENERATORS[model](N=N, S=S, seed=seed, **{"T": T, **kw})
    s = SPOILED
    if kind.startswith("A-0-"):
        draws["A_ij"][s, 0, int(kind[4:])] = np.nan
    elif kind == "A-last-0":
        draws["A_ij"][s, K - 1, 0] = np.nan
    elif kind == "emission":
        if model == "hmm":
            draws["mu_k"][s, 1] = np.nan
        else:
            draws["phi_k"][s, 1, 1] = np.nan     # symbol 2, the one state 2 favours
    elif kind == "p1":
        draws["p_1k"][s, 0] = np.nan
    elif kind == "p11":
        draws["p_11"][s] = np.nan
    elif kind == "A-row":
        draws["A_row"][s, 1, 0] = np.nan
    elif kind == "w":
        draws["w_km"][s, 0, 0] = np.nan
    ref = pyoracle.gqs(model, data, draws, pars=PARS, return_status=True)
    return data, draws, ref


@pytest.mark.parametrize("pid,mk,flags,kind", CASES, ids=[f"{c[0]}-{c[3]}" for c in CASES])
def test_nan_draw_matches_oracle(engine, oracle, pid, mk, flags, kind):
    import hhmm_amd
    model, K = mk[0], dict(mk[1])["K"]
    data, draws, ref = _request(mk, kind)
    spoiled = SPOILED + S * np.arange(N)     # grid pairing: p = s + S n
    if kind.startswith("A-0-") and int(kind[4:]) in BP1_SEEDS.get(_seed_key(mk), {}):
        j = int(kind[4:])
        z = ref["zstar_t"][spoiled]
        assert np.any((z[:, :-1] == 2) & (z[:, 1:] == j + 1)), "the oracle's path never takes back-pointer 1"
    # the NaN stays in its draw: every other pair is an ordinary one
    others = np.setdiff1d(np.arange(N * S), spoiled)
    assert np.isfinite(ref["loglik"][others]).all() and np.isnan(ref["loglik"][spoiled]).all()
    assert_plan(engine, model, data, draws, PARS, flags, "grid", PLANS[pid])
    got =hhmm_amd.gqs(model, data, draws, pars=PARS, lib=engine, return_status=True, flags=flags)
    # Tayal's gamma has a comparison of its own (Q6: tests/test_gpu_configs.py compare_tayal_gamma)
    names = [n for n in PARS if not (model == "hhmm-tayal2009" and n == "gamma_tk")]
    compare_all(got, ref, names + ["pair_status"])
    if model == "hhmm-tayal2009":
        from test_gpu_configs import compare_tayal_gamma
        compare_tayal_gamma(got, ref, max_forgiven=0)
    assert got["status"] == ref["status"]
