"""GPU: the packed gamma profile of hmm-multinom off its benchmark shape,
every case pinned to its launch plan (tests/hot_plan.py) and compared with
the CPU oracle at tests/tolerances.py.

The benchmark request (K = 4, L = 9, loglik + gamma_tk + zstar_t +
logp_zstar over a million pairs of T = 1000) runs the phased sweep; the
fused sweep, the split launches and fb_kernel beside viterbi_kernel are its
other schedules.  Below 131072 pairs these run only with HHMM_FLAG_VIT_LANES
and either T < 256 or HHMM_FLAG_SCAN_OFF (hot_plan.LANES), so every case
here sets those flags and asserts the plan before it runs.

Shapes: 4 steps per back-pointer word at K = 4, 8-step chunks, kBigChunk =
16, kVitGroup = 2 chunks after chunk 0, kFwdGroup = 4 chunks and the 8-word
(64-step) prefetch group of vfb_forward give the edge set EDGES; a wave is
64 lanes, so P = 70 is two waves, the last with 6 lanes.  Symbols pack 4
bits each at L <= 16 (nibble L - 1), and L = 17 is the first unpacked size.

CASES is a table: tests/test_hot_plan.py walks it without a device and
asserts every case's plan."""
import collections
import functools

import numpy as np
import pytest

from hhmm_amd import _abi, synth
from hot_plan import C2, LANES, PACKED, SCHEDULES, run_planned

pytestmark = pytest.mark.gpu

MODEL = "hmm-multinom"
EDGES = [3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
OTHER_K_T = [1, 3, 4, 5, 15, 16, 17, 33, 130]
LG = ["loglik", "gamma_tk"]

# id, key of inputs(), outputs, flags, pairing, the plan words pinned
Case = collections.namedtuple("Case", "id key pars flags pairing plan")


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(data, draws, uniforms) of a case key; built once and only read."""
    kind, K, L = key[:3]
    if kind == "uniform":                        # zip, P pairs of one length
        P, T = key[3:]
        data, draws = synth.hmm_multinom(N=P, S=P, T=T, K=K, L=L)
    elif kind == "ragged":                       # zip, three waves of section B.2
        data, draws = synth.hmm_multinom(N=192, S=192, T=257, K=K, L=L)
        edges = [t for t in EDGES if t <= 257]
        Tn = np.empty(192, dtype=np.int32)
        Tn[:64] = [edges[i % len(edges)] for i in range(64)]          # Tw_min = 3
        Tn[64:128] = 64
        Tn[100] = 65
        Tn[128:] = [16 + (i & 1) for i in range(64)]
        Tn[150] = 1
        data["T"] = Tn
    elif kind == "cycle":                        # zip, P pairs whose lengths cycle through key[4]
        P, Ts = key[3:]
        data, draws = synth.hmm_multinom(N=P, S=P, T=max(Ts), K=K, L=L)
        data["T"] = np.array([Ts[i % len(Ts)] for i in range(P)], dtype=np.int32)
    elif kind == "grid":                         # 3 series x 70 draws: waves straddle series
        data, draws = synth.hmm_multinom(N=3, S=70, T=257, K=K, L=L)
        data["T"] = np.array([130, 257, 65], dtype=np.int32)
    elif kind == "block":                        # 3 series, 50 draws each
        data, draws = synth.hmm_multinom(N=3, S=150, T=257, K=K, L=L)
        data["T"] = np.array([257, 9, 130], dtype=np.int32)
    else:
        raise KeyError(kind)
    P = {"grid": 210, "block": 150}.get(kind, np.asarray(data["x"]).shape[0])
    return data, draws, synth.ffbs_uniforms(P, np.asarray(data["x"]).shape[1], seed=K + L)


@functools.lru_cache(maxsize=None)
def reference(key, pars, pairing):
    """The oracle's outputs of a case's inputs: computed once per (inputs, outputs), shared by the schedules."""
    import pyoracle
    data, draws, uu = inputs(key)
    return pyoracle.gqs(MODEL, data, draws, pars=list(pars), pairing=pairing, return_status=True, nthreads=8,
                        uniforms=uu if "z_ffbs" in pars else None)


def _cases():
    out = []
    sep = dict(schedule="separate", fb="linear", scan_cl="0", vs_nc="0")
    big, pack = dict(sep, fb_mode="GAMMA|PACK|BIG"), dict(sep, fb_mode="GAMMA|PACK")
    for sid, flags, plan in SCHEDULES:
        # 1. uniform T at every loop edge
        for T in EDGES:
            out.append(Case(f"edge-T{T}-{sid}", ("uniform", 4, 9, 70, T), C2, flags, "zip", plan))
        # 2. ragged inside a wave
        out.append(Case(f"ragged-{sid}", ("ragged", 4, 9), C2, flags, "zip", plan))
        # 3. L on both sides of the 4-bit boundary
        for L in (1, 2, 15, 16):
            out.append(Case(f"L{L}-{sid}", ("uniform", 4, L, 70, 130), C2, flags, "zip",
                            dict(plan, regions=PACKED + ",bp")))
        out.append(Case(f"L17-{sid}", ("uniform", 4, 17, 70, 130), C2, flags, "zip",
                        dict(sep, fb_mode="GAMMA", vit="lanes", regions="ckpt,ckpt_ls,bp")))
        # 4. pairings
        out.append(Case(f"grid-{sid}", ("grid", 4, 9), C2, flags, "grid", plan))
        out.append(Case(f"block-{sid}", ("block", 4, 9), C2, flags, "block", plan))
        out.append(Case(f"P1-{sid}", ("uniform", 4, 9, 1, 130), C2, flags, "zip", plan))
        out.append(Case(f"P257-{sid}", ("uniform", 4, 9, 257, 130), C2, flags, "zip", plan))
    # 5. output subsets (null pointers for the outputs left out)
    sub = ("uniform", 4, 9, 70, 130)
    phased = SCHEDULES[0][2]
    out += [
        Case("subset-gamma-zstar", sub, ["gamma_tk", "zstar_t"], LANES, "zip", phased),
        Case("subset-gamma-zstar-logp", sub, ["gamma_tk", "zstar_t", "logp_zstar"], LANES, "zip", phased),
        # the phased sweep needs zstar_t
        Case("subset-no-zstar", sub, ["loglik", "gamma_tk", "logp_zstar"], LANES, "zip", dict(big, vit="lanes")),
        Case("subset-no-zstar-fused", sub, ["loglik", "gamma_tk", "logp_zstar"], LANES | _abi.FLAG_FUSED, "zip",
             SCHEDULES[1][2]),
        Case("subset-no-zstar-split", sub, ["loglik", "gamma_tk", "logp_zstar"], LANES | _abi.FLAG_FB_SPLIT, "zip",
             SCHEDULES[2][2]),
        Case("subset-gamma", sub, ["gamma_tk"], LANES, "zip", dict(big, vit="none", regions=PACKED)),
        Case("subset-loglik-gamma", sub, LG, LANES, "zip", dict(big, vit="none", regions=PACKED)),
    ]
    # 6. other K: FB_BIG below K = 4, 4-step chunks (one packed word per chunk) above; one ragged batch of 200
    # pairs each (four waves: two workgroups where a 64 KB table leaves two waves per workgroup, K = 7, 8 at L = 16)
    for K in (1, 2, 3, 5, 6, 7, 8):
        for L in (2, 9, 16):
            mode = big if K <= 3 else pack
            key = ("cycle", K, L, 200, tuple(OTHER_K_T))
            out.append(Case(f"K{K}-L{L}-gamma", key, LG, LANES, "zip", dict(mode, vit="none", regions=PACKED)))
            out.append(Case(f"K{K}-L{L}-c2", key, C2, LANES, "zip", dict(mode, vit="lanes", regions=PACKED + ",bp")))
    # 7. the third packed instantiation: gamma + FFBS draws
    for K in (4, 6):
        for L in (9, 16):
            out.append(Case(f"ffbs-K{K}-L{L}", ("cycle", K, L, 70, (1, 9, 130)), ["gamma_tk", "z_ffbs"], LANES, "zip",
                            dict(sep, fb_mode="GAMMA|FFBS|PACK", vit="none", regions=PACKED)))
    return out


CASES = _cases()    # the library refuses none of these shapes: the largest table, K = 7, 8 at L = 16, is 64 KB a wave


def symbol_L_occurs(case):
    """Symbol L (nibble L - 1 of the packed record) is among the steps the kernels read."""
    data = inputs(case.key)[0]
    x = np.asarray(data["x"])
    T = np.asarray(data["T"]) if "T" in data else np.full(x.shape[0], x.shape[1])
    return bool((x[np.arange(x.shape[1])[None, :] < T[:, None]] == case.key[2]).any())


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_hot_sweep(engine, oracle, case):
    data, draws, uu = inputs(case.key)
    assert symbol_L_occurs(case)
    got, _ = run_planned(engine, oracle, MODEL, data, draws, case.pars, case.flags, case.pairing, case.plan,
                         uniforms=uu if "z_ffbs" in case.pars else None, tag=case.id,
                         ref=reference(case.key, tuple(case.pars), case.pairing))
    assert set(got) == set(case.pars) | {"pair_status", "status"}
