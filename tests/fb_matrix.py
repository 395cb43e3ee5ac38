"""The case table of tests/test_gpu_fb_matrix.py: every forward-backward and
Viterbi kernel of the HMM family at K <= 8 that a request of a small shape can
reach, each case pinned to its launch plan (tests/hot_plan.py).

Every (MODEL, K, mode) of launch_fb, launch_fb_scan and launch_viterbi
(csrc/hhmm_hmm.h) is a kernel compiled on its own, and the forward-backward
and the decoder of one request run side by side (side_stream), so a case is a
pair (forward-backward row, decoder) of one (model, K): the rows of FB_ROWS,
BRANCH_ROWS and SCAN_ROWS crossed with the decoders the plan gives at that K
(decoders()), and every combination of Tayal-lite's three launches.  The
universe the table must cover is enumerated from hmm_plan itself by the ledger
of tests/test_fb_matrix_plan.py, on the CPU.

Inputs.  One ragged batch per (model, K): zip pairing, P = 200 pairs = three
full waves and one of 8 lanes, T_max = 130 < 256 (no automatic T-scan).  With
C = fb_chunk(K) (8 steps at K <= 4, else 4) and D = kFwdGroup = 4 chunks:
  wave 0  lengths cycle through WAVE0(C): Tw_min = 1, nfull = 0
  wave 1  2DC everywhere, one lane of 2DC + 1: nfull = 2D (the grouped
          prefetch loop runs twice), one lane needs one chunk more
  wave 2  DC and DC + 1 alternate, one lane of length 1
  wave 3  8 lanes of 130 steps; the lanes past P redo pair P - 1
Tayal-lite's T_oos follows the same pattern.  The lane decoder's chunks are
vit_chunk(K) = 32, 16, 10, 8, 8, 8, 8, 8 steps for K = 1..8 (csrc/hhmm_plan.h),
the state-parallel decoder's twice that: 130 steps is several chunks and a
partial one of each.  At K = 3 and 6 (Tayal: 4) a grid batch (3 series x 70
draws, waves straddle series) and a block batch (3 series x 50 draws) follow.

Discrete models run at L = 9.  hmm-multinom's gamma profile packs its symbols
at L <= 16 (the PACK modes): its unpacked GAMMA rows run at L = 17, and the
packed modes tests/test_gpu_hot_sweeps.py does not pin are added at L = 9.

A series of one step at odd K >= 3 cannot be backtracked by the reference
itself (q3_flagged): those six pairs of a ragged batch are flagged on both
sides whenever a path is asked for, and compared like every other pair.
"""
import collections
import functools

import numpy as np

from hhmm_amd import _abi, synth
from hot_plan import LANES

Case = collections.namedtuple("Case", "id model key pars flags pairing plan")

D = 4                                            # kFwdGroup (csrc/hhmm_fbchunk.h)
T_MAX = 130
MULTINOM, SEMISUP, GAUSS, TAYAL, LITE = ("hmm-multinom", "hmm-multinom-semisup", "hmm", "hhmm-tayal2009",
                                         "hhmm-tayal2009-lite")
MODEL_K = ([(m, K) for m in (GAUSS, MULTINOM, SEMISUP) for K in range(1, 9)] + [(TAYAL, 4), (LITE, 4)])
EXTRA_K = {GAUSS: (3, 6), MULTINOM: (3, 6), SEMISUP: (3, 6), TAYAL: (4,), LITE: (4,)}   # grid and block batches

# the flag sets of the table (and of the ledger): lane-per-pair sweeps; the forced T-scan in chunks of 2^n steps
# beside the lane decoder; the state-parallel decoder; the T-parallel decoder
STATES = _abi.FLAG_VIT_STATES | _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF
VSCAN = _abi.FLAG_VIT_SCAN | _abi.FLAG_SCAN_OFF


def scan_forced(log2):
    return _abi.FLAG_VIT_LANES | _abi.FLAG_VIT_SCAN_OFF | _abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(log2)


# Batches whose default seed (synth.SEED) fails a non-vacuity check of tests/test_fb_matrix_plan.py: key -> seed.
RESEEDED = {}


def fb_chunk(K):
    return 8 if K <= 4 else 4


def wave0(C):
    return [1, 2, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, D * C - 1, D * C, D * C + 1, 2 * D * C - 1,
            2 * D * C, 2 * D * C + 1, T_MAX]


def ragged_lengths(C):
    """The 200 lengths of the ragged batch (module docstring)."""
    T = np.empty(200, dtype=np.int32)
    w0 = wave0(C)
    T[:64] = [w0[i % len(w0)] for i in range(64)]
    T[64:128] = 2 * D * C
    T[100] = 2 * D * C + 1
    T[128:192] = [D * C + (i & 1) for i in range(64)]
    T[150] = 1
    T[192:] = T_MAX
    return T


def pairs_of(kind):
    return {"ragged": 200, "grid": 210, "block": 150}[kind]


def pairing_of(kind):
    return {"ragged": "zip", "grid": "grid", "block": "block"}[kind]


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(data, draws, uniforms) of a batch key (kind, model, K, L); built once and only read."""
    kind, model, K, L = key
    C = fb_chunk(K)
    kw = dict(seed=RESEEDED.get(key, synth.SEED))
    if model in (GAUSS, MULTINOM, SEMISUP):
        kw["K"] = K
    if model != GAUSS:
        kw["L"] = L
    if model == LITE:
        kw["T_oos"] = T_MAX
    if kind == "ragged":
        N, S, T = 200, 200, ragged_lengths(C)
    elif kind == "grid":
        N, S, T = 3, 70, np.array([T_MAX, 2 * D * C + 1, D * C], dtype=np.int32)
    elif kind == "block":
        N, S, T = 3, 150, np.array([2 * D * C + 1, C + 1, T_MAX], dtype=np.int32)
    else:
        raise KeyError(kind)
    data, draws = synth.GENERATORS[model](N=N, S=S, T=T_MAX, **kw)
    data["T"] = T
    if model == LITE:
        data["T_oos"] = T.copy()
    return data, draws, synth.ffbs_uniforms(pairs_of(kind), T_MAX, seed=K + L)


FB7 = ["loglik", "alpha_tk", "beta_tk", "unalpha_tk", "unbeta_tk", "ungamma_tk", "gamma_tk"]
VIT = ["zstar_t", "logp_zstar"]
ALL_PARS = {m: FB7 + ["z_ffbs"] + VIT for m in (GAUSS, MULTINOM, SEMISUP, TAYAL)}
ALL_PARS[LITE] = ["loglik", "alpha_tk", "unalpha_tk", "alpha_tk_oos", "unalpha_tk_oos"] + VIT


@functools.lru_cache(maxsize=4)
def reference_all(key):
    """Every output the oracle has of a batch.  The oracle computes all of a pair's outputs whatever the request
    names and copies out those it names (oracle/hhmm_oracle.c run_pair, scatter), so one call per batch serves
    every case of it; the cases of one batch are adjacent in CASES, which keeps a small cache enough."""
    import pyoracle
    kind, model = key[:2]
    data, draws, uu = inputs(key)
    return pyoracle.gqs(model, data, draws, pars=ALL_PARS[model], pairing=pairing_of(kind), return_status=True,
                        nthreads=8, uniforms=None if model == LITE else uu)


def q3_flagged(key):
    """The pairs whose Viterbi the reference itself cannot backtrack: a series of one step at odd K >= 3.  Q3
    writes delta[1, K] alone, so delta_T = delta_1 holds NaN, and Stan's max over it (Eigen's packet reduction,
    oracle/hhmm_oracle.c stan_max_vec) is NaN when K is odd: PAIR_INVALID_BACKPOINTER, the path zeroed, on both
    sides.  The length-1 lanes are part of the batch on purpose, so these pairs stay, and every decoder is held
    to the flag as well."""
    kind, model, K, _ = key
    data = inputs(key)[0]
    T = np.asarray(data["T_oos" if model == LITE else "T"])
    if kind != "ragged":                         # no series of one step in the grid and block batches
        assert T.min() > 1
        return np.zeros(pairs_of(kind), dtype=bool)
    return (T == 1) & (K >= 3 and K % 2 == 1)


def reference(key, pars):
    """The oracle's outputs of a case: computed once per batch, shared by its cases, never written.  pair_status
    is the Viterbi backtrack's: zero for a request that decodes no path (include/hhmm.h)."""
    ref = reference_all(key)
    out = {k: ref[k] for k in pars}
    vit = bool(set(pars) & set(VIT))
    out["pair_status"] = ref["pair_status"] if vit else np.zeros_like(ref["pair_status"])
    out["status"] = int(out["pair_status"].any())
    return out


# ---- the rows: (id, outputs, fb, fb_mode, needs the checkpoints) ----
FULL = ["loglik", "alpha_tk", "beta_tk", "ungamma_tk", "gamma_tk"]
LG = ["loglik", "gamma_tk"]
GZ = ["gamma_tk", "z_ffbs"]
FB_ROWS = [
    ("fwd-loglik", ["loglik"], "linear", "FWD", False),
    ("fwd-alpha", ["alpha_tk"], "linear", "FWD", False),
    ("gamma", LG, "linear", "GAMMA", True),
    ("gamma-ffbs", GZ, "linear", "GAMMA|FFBS", True),
    ("full", FULL, "linear", "FULL", True),
    ("full-ffbs", FULL + ["z_ffbs"], "linear", "FULL|FFBS", True),
    ("log-fwd", ["unalpha_tk"], "log", "FWD", False),
    ("log-both", FB7, "log", "BOTH", True),
    # the second launch is the unpacked GAMMA|FFBS fb_kernel, for hmm-multinom at L <= 16 too
    ("log-both-ffbs", FB7 + ["z_ffbs"], "log", "BOTH+FFBS", True),
]
# FB_FULL branches on every output pointer: each of these alone, the others' pointers null (K = 3 and 6)
BRANCH_ROWS = [
    ("full-beta", ["beta_tk"], "linear", "FULL", True),
    ("full-ungamma", ["ungamma_tk"], "linear", "FULL", True),
    ("full-alpha-gamma", ["alpha_tk", "gamma_tk"], "linear", "FULL", True),
]
SCAN_ROWS = [
    ("scan-fwd", ["loglik", "alpha_tk"], "scan", "FWD", True),
    ("scan-gamma", LG, "scan", "GAMMA", True),
    ("scan-full", FULL, "scan", "FULL", True),
]
UNPACKED_AT_L17 = {"gamma", "gamma-ffbs"}        # hmm-multinom: these rows pack their symbols at L <= 16
EXTRA_ROWS = [("full-ffbs", "lanes"), ("log-both", "none"), ("scan-gamma", "lanes"), ("gamma-ffbs", "states"),
              ("vit", "lanes")]                  # what the grid and block batches run (states: K <= 4)


def decoders(K):
    """(suffix, flags, vit, vs_nc) of the decoders a (model, K) has; `none`: no path asked for."""
    out = [("none", LANES, "none", "0"), ("lanes", LANES, "lanes", "0")]
    if 2 <= K <= 4:
        out.append(("states", STATES, "states", "0"))
    if K in (2, 4):
        out.append(("vscan", VSCAN, "vscan", "1"))           # ceil(130 / kVsChunk) = 1 chunk
    return out


def _plan(schedule, fb, fb_mode, oos_fb, vit, vs_nc, ckpt=False, packed=False, scan_cl="0"):
    regions = (["ckpt", "ckpt_ls"] if ckpt else []) + (["xpk", "rnw"] if packed else [])
    regions += (["bp"] if vit != "none" else []) + (["scan"] if fb == "scan" else [])
    regions += ["vscan"] if vit == "vscan" else []
    side = schedule == "separate" and vit != "none" and fb != "none"
    return dict(schedule=schedule, fb=fb, fb_mode=fb_mode, oos_fb=oos_fb, vit=vit, scan_cl=scan_cl, vs_nc=vs_nc,
                regions=",".join(regions) or "-", side_stream=str(int(side)))


def _model_cases(model, K):
    out = []
    L = 0 if model == GAUSS else 9

    def add(kind, Lc, rid, pars, fb, mode, ckpt, dec, flags=None, packed=False, scan_cl="0"):
        sfx, dflags, vit, vs_nc = dec
        tag = f"{model}-K{K}" + (f"-L{Lc}" if Lc not in (0, 9) else "") + ("" if kind == "ragged" else f"-{kind}")
        out.append(Case(f"{tag}-{rid}" + ("" if sfx == "none" else f"+{sfx}"), model, (kind, model, K, Lc),
                        list(pars) + (VIT if vit != "none" else []), dflags if flags is None else flags,
                        pairing_of(kind), _plan("separate", fb, mode, "none", vit, vs_nc, ckpt, packed, scan_cl)))

    def rows_of(kind, want=None):
        decs = {d[0]: d for d in decoders(K)}
        rows = FB_ROWS + (BRANCH_ROWS if K in (3, 6) else [])
        for rid, pars, fb, mode, ckpt in rows:
            Lc = 17 if model == MULTINOM and rid in UNPACKED_AT_L17 else L
            for sfx, dec in decs.items():
                if want is None or (rid, sfx) in want:
                    add(kind, Lc, rid, pars, fb, mode, ckpt, dec)
        for sfx, dec in decs.items():
            if sfx != "none" and (want is None or ("vit", sfx) in want):
                add(kind, L, "vit", [], "none", "-", False, dec)
        for rid, pars, fb, mode, ckpt in SCAN_ROWS:           # 17 chunks of 8 steps; at K > 4 also 33 of 4
            for sfx in ("none", "lanes"):
                if want is None or (rid, sfx) in want:
                    add(kind, L, rid, pars, fb, mode, ckpt, decs[sfx], flags=scan_forced(3), scan_cl="8")
            if K > 4 and want is None:
                add(kind, L, rid + "-cl4", pars, fb, mode, ckpt, decs["none"], flags=scan_forced(2), scan_cl="4")
        if model == MULTINOM and want is None:
            # the packed keys tests/test_gpu_hot_sweeps.py does not pin: GAMMA|FFBS|PACK off K = 4, 6 and beside
            # every decoder; the packed gamma profile beside the state-parallel and T-parallel decoders
            big = "GAMMA|PACK|BIG" if K <= 4 else "GAMMA|PACK"
            for sfx, dec in decs.items():
                if not (sfx == "none" and K in (4, 6)):
                    add(kind, 9, "gamma-ffbs-pack", GZ, "linear", "GAMMA|FFBS|PACK", True, dec, packed=True)
                if sfx in ("states", "vscan"):
                    add(kind, 9, "gamma-pack", LG, "linear", big, True, dec, packed=True)

    rows_of("ragged")
    if K in EXTRA_K[model]:
        rows_of("grid", set(EXTRA_ROWS))
        rows_of("block", set(EXTRA_ROWS))
    return out


LITE_IN = [("", [], "none", "-"), ("loglik", ["loglik"], "linear", "FWD"), ("alpha", ["alpha_tk"], "linear", "FWD"),
           ("unalpha", ["unalpha_tk"], "log", "FWD")]
LITE_OOS = [("", [], "none"), ("alpha_oos", ["alpha_tk_oos"], "linear"), ("unalpha_oos", ["unalpha_tk_oos"], "log")]
LITE_EXTRA = {("loglik", "alpha_oos", "lanes"), ("unalpha", "unalpha_oos", "states"), ("alpha", "", "none")}


def _lite_cases():
    """Tayal-lite: the in-sample forward, the OOS forward and the OOS decoder are launched one after the other
    (SCHED_LITE); every combination of the three, the decoder over T_oos."""
    out = []
    for kind in ("ragged", "grid", "block"):
        for iid, ipars, fb, mode in LITE_IN:
            for oid, opars, oos in LITE_OOS:
                for sfx, flags, vit, vs_nc in decoders(4):
                    if not (ipars or opars or vit != "none"):
                        continue
                    if kind != "ragged" and (iid, oid, sfx) not in LITE_EXTRA:
                        continue
                    rid = "+".join(w for w in (iid, oid, "" if sfx == "none" else sfx) if w)
                    tag = f"{LITE}-K4" + ("" if kind == "ragged" else f"-{kind}")
                    out.append(Case(f"{tag}-{rid}", LITE, (kind, LITE, 4, 9),
                                    ipars + opars + (VIT if vit != "none" else []), flags, pairing_of(kind),
                                    _plan("lite", fb, mode, oos, vit, vs_nc)))
    return out


def _cases():
    out = []
    for model, K in MODEL_K:
        out += _lite_cases() if model == LITE else _model_cases(model, K)
    return sorted(out, key=lambda c: (MODEL_K.index((c.model, c.key[2])), c.key))   # a batch's cases adjacent


CASES = _cases()


def key_of(model, K, plan):
    """What the ledger counts: (model, K, schedule, fb, fb_mode, oos_fb, vit) of a plan's words."""
    return (model, K, plan["schedule"], plan.get("fb", "none"), plan.get("fb_mode", "-"),
            plan.get("oos_fb", "none"), plan.get("vit", "none"))


def symbol_L_occurs(key):
    """Symbol L is among the steps the kernels read (the discrete models)."""
    data = inputs(key)[0]
    hits = []
    for x, T in (("x", "T"), ("x_oos", "T_oos")):
        if x in data:
            a = np.asarray(data[x])
            hits.append(bool((a[np.arange(a.shape[1])[None, :] < np.asarray(data[T])[:, None]] == key[3]).any()))
    return all(hits)
