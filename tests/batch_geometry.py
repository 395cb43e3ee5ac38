"""Large batches of the five "statistics per (series, draw) pair" entries built from a few base pairs
(test helper of tests/test_stats_geometry.py; a plain module).

The entries' kernels (csrc/hhmm_estep.hip for the E-step and the expected statistics, hhmm_draw_stats.hip for
both draw statistics entries, hhmm_estep_io.hip) give one lane to one pair, carve a per-wave LDS slab at
`wave * elems` and address a pair by `gwave = blockIdx.x * nw + wave`.  A numpy reference of a 577-pair
batch would be slow, so the batch is made of B <= 32 BASE pairs (a zip request with N = S = B, referenced
once) and an index vector:

    make_base(entry, shape)   the base pairs, their lengths and roles, the uniforms of the two draw entries
    reference(base, ...)      their reference statistics, from the existing reference modules
    gather(req, idx)          the zip request whose pair p is base pair idx[p]
    layout(P, classes)        idx, wave by wave: wave j takes its 64 pairs from class j % 3

Lengths.  C = fb_chunk(K) steps per forward chunk; the forward sweep takes the full chunks D at a time
(kFwdGroup = 4 in csrc/hhmm_fbchunk.h; the Gaussian draw statistics take D = 2 at K = 8) while
c + D <= nfull = (shortest lane of the wave) / C, then a guarded tail up to ceil(longest lane / C).
    long    D C, D C + 1, (D + 1) C - 1, (D + 1) C + 1, 2 D C + C + 3 = T_max
    short   1, 2, C, C + 1
D C, D C + 1 and (D + 1) C - 1 all have length / C = D, and a wave that holds one of them has nfull = D, a
multiple of D.  (D + 1) C + 1 is there so that a ragged wave with nfull = D + 1 exists: the group loop
hands over to the tail inside the full chunks.

Classes of a wave (layout):
    0  long and ragged.  Class-0 waves alternate between every long length (nfull = D: one group, then
       D + 2 tail chunks, the shorter lanes reading checkpoint rows past their own last chunk) and the
       lengths >= (D + 1) C + 1 alone (nfull = D + 1, not a multiple of D).
    1  everything: every base pair, the length-1 lane and the abnormal pairs included.
    2  uniform: one base pair 64 times (broadcast loads; one sign per step for the whole wave, the Tayal
       sign-class arm).
The IOHMM E-step has no chunks; it takes the same lengths so that its waves mix short and long lanes.

Abnormal base pairs (class-1 waves only): one with a NaN draw parameter; for the discrete models one
impossible series (its draw emits the symbol L nowhere and the series shows it); and `flag`, a clean pair
whose copy in the device request (device_request) carries a symbol outside 1..L -- a length outside
1..T_max for the Gaussian hmm and the IOHMM programs, which read no symbols -- so that only the device
entries, which flag a pair, see it: the host entries refuse such a request as a whole.
"""
import numpy as np

import draw_stats_gauss_ref
import draw_stats_ref
import estep_io_ref
import estep_ref
import expect_ref

K_FWD_GROUP = 4          # csrc/hhmm_fbchunk.h kFwdGroup
LDS_LIMIT = 160 * 1024   # csrc/hhmm_internal.h kLdsLimit
BLOCK_WAVES = 4          # kBlock / 64
EXP2_TAB_BYTES = 128 * 16  # kExp2TabBytes: 128 entries of two doubles
P_BATCH = 577
ENTRIES = ("estep", "expected_stats", "draw_stats", "draw_stats_gauss", "estep_io")
DISCRETE = ("hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009")


def fb_chunk(K):
    return 8 if K <= 4 else 4


def fwd_group(entry, K):
    """Chunks per group of the entry's forward loop: draw_stats_gauss at K = 8 uses D = 2 (its kernel's
    `constexpr int D = K >= 8 ? 2 : kFwdGroup`), everything else kFwdGroup."""
    return 2 if entry == "draw_stats_gauss" and K >= 8 else K_FWD_GROUP


# ---------------------------------------------------------------- waves per workgroup, restated

def _waves_that_fit(per_wave):
    """csrc/hhmm_stats.h waves_that_fit."""
    w = BLOCK_WAVES
    while w > 0 and per_wave * w > LDS_LIMIT:
        w -= 1
    return w


def waves_per_workgroup(entry, model, K, L=0, M=0):
    """The entry's launch geometry as its sizing function computes it (estep_waves, expect's the same,
    draw_stats_wave_lds, draw_stats_gauss_waves, eio_wave_bytes); 0: rejected for LDS."""
    KP = (K + 1) // 2
    if entry in ("estep", "expected_stats"):
        if model == "hmm":
            return BLOCK_WAVES
        return _waves_that_fit(2 * L * KP * 64 * 16)
    if entry == "draw_stats":
        return _waves_that_fit(L * KP * 64 * 16 + (L * K + K * K) * 64 * 4)
    if entry == "draw_stats_gauss":  # of 4, 2, 1 the size that lets a CU hold the most waves; the larger on a tie
        per_wave = 2 * K * 64 * 8 + (K + K * K) * 64 * 4
        best, most = 1, 0
        for w in (4, 2, 1):
            cu = LDS_LIMIT // (EXP2_TAB_BYTES + per_wave * w) * w
            if cu > most:
                best, most = w, cu
        return best
    assert entry == "estep_io"
    mmax = 4 if M <= 4 else 8
    gw = 0 if K * mmax <= 32 else K * (mmax // 2)
    if model == "iohmm-reg":
        elems = K * (mmax * (mmax + 1) // 2 // 2 + mmax // 2 + 1) + gw
    else:
        elems = K * L * 4 + gw
    return _waves_that_fit(elems * 64 * 16)


def gw_in_slab(K, M):
    """hhmm_estep_io.hip eio_gw_regs, negated."""
    return K * (4 if M <= 4 else 8) > 32


# ---------------------------------------------------------------- lengths, classes, layout

def long_lengths(C, D):
    return [D * C, D * C + 1, (D + 1) * C - 1, (D + 1) * C + 1, 2 * D * C + C + 3]


def short_lengths(C):
    return [1, 2, C, C + 1]


def base_lengths(C, D):
    """(lengths [B], roles): two base pairs per long length, one per short length, then the NaN draw, the
    impossible series and the pair the device request flags, all three at T_max (an impossible series must
    be long enough to show the symbol; the NaN parameter is read from step 2 on)."""
    lens = [t for t in long_lengths(C, D) for _ in range(2)] + short_lengths(C)
    tmax = long_lengths(C, D)[-1]
    roles = {"nan": len(lens), "impossible": len(lens) + 1, "flag": len(lens) + 2}
    return np.array(lens + [tmax] * 3, dtype=np.int32), roles


def classes_of(lengths, C, D, abnormal):
    """{0: (every long pair, the pairs of length >= (D + 1) C + 1), 1: all, 2: the uniform waves' pairs}
    as lists of base indices; `abnormal` indices stay out of classes 0 and 2."""
    lengths = np.asarray(lengths)
    normal = [i for i in range(lengths.size) if i not in set(abnormal)]
    longs = [i for i in normal if lengths[i] in long_lengths(C, D)]
    tail = [i for i in longs if lengths[i] >= (D + 1) * C + 1]
    first = {int(lengths[i]): i for i in reversed(normal)}
    uniform = [first[2 * D * C + C + 3], first[D * C + 1], first[C + 1]]
    return {0: (longs, tail), 1: list(range(lengths.size)), 2: uniform}


def layout(P, classes):
    """idx [P]: wave j (pairs 64 j .. 64 j + 63) takes its base pairs from class j % 3.  Class 0 alternates
    between its two lists from one class-0 wave to the next; inside a wave the list is walked from an offset
    that moves with the wave, so the same base pair meets different lanes.  Class 2 repeats one base pair."""
    idx = np.empty(P, dtype=np.int64)
    for j in range((P + 63) // 64):
        lo, hi = 64 * j, min(64 * j + 64, P)
        lane = np.arange(hi - lo)
        r = j // 3
        if j % 3 == 2:
            idx[lo:hi] = classes[2][r % len(classes[2])]
            continue
        pool = np.asarray(classes[0][r % 2] if j % 3 == 0 else classes[1])
        idx[lo:hi] = pool[(lane + 5 * r) % pool.size]
    return idx


# ---------------------------------------------------------------- base pairs

def _generator(entry):
    import test_draw_stats
    import test_draw_stats_gauss
    import test_estep
    import test_estep_io
    import test_expected_stats
    return {"estep": test_estep.make, "expected_stats": test_expected_stats.make, "draw_stats": test_draw_stats.make,
            "draw_stats_gauss": test_draw_stats_gauss.make, "estep_io": test_estep_io.make}[entry]


def _aux_key(model):
    return {"hmm-multinom-semisup": "g", "hhmm-tayal2009": "sign"}.get(model)


def make_base(entry, shape, seed=0, garbage=True):
    """The base pairs of one case.  shape: {"model", "K"} and "L" / "M" where the model has them.

    Returns a dict: entry, model, K, L, M, C, D, B, data, draws (a zip request, N = S = B), u (the [B, T_max]
    uniforms of the two draw entries, else None), T (the lengths), roles ({"nan", "impossible", "flag"} ->
    base index; "impossible" only for the discrete models) and abnormal (their indices).  With `garbage` the
    padding past a pair's length holds values that must not matter."""
    from hhmm_amd import synth
    model, K = shape["model"], int(shape["K"])
    L, M = int(shape.get("L", 0)), int(shape.get("M", 0))
    C, D = fb_chunk(K), fwd_group(entry, K)
    lens, roles = base_lengths(C, D)
    if model not in DISCRETE:
        roles.pop("impossible")
        lens = np.delete(lens, -2)
        roles["flag"] -= 1
    B, tmax = lens.size, int(lens.max())
    assert B <= 32 and tmax == 2 * D * C + C + 3
    make = _generator(entry)
    if entry == "draw_stats_gauss":
        data, draws = make(B, B, tmax, K, seed=seed)
    elif entry == "estep_io":
        data, draws = make(model, B, B, tmax, K, M, L, seed=seed)
    else:
        data, draws = make(model, B, B, tmax, K, L, seed=seed)
    data["T"] = lens.copy()
    aux = _aux_key(model)
    # --- the abnormal pairs
    i = roles["nan"]
    if entry == "estep_io":
        draws["w_km"][i, 0, 1] = np.nan
    elif entry == "draw_stats_gauss":
        draws["mu_k"][i, K - 1] = np.nan
    elif model == "hhmm-tayal2009":
        draws["p_11"][i] = np.nan
        data["sign"][i, 0] = 2               # sign_1 = 2: p_11 is read
    else:
        draws["A_ij"][i, 0, min(1, K - 1)] = np.nan
        if model == "hmm-multinom-semisup":
            data["g"][i, 1] = 2              # column 2 takes A at step 2: A(1, 2) is read
    if "impossible" in roles:
        i = roles["impossible"]
        data["x"][i, 9] = L                  # the series shows symbol L ...
        draws["phi_k"][i, :, L - 1] = 0.0    # ... which no state of its draw emits
        draws["phi_k"][i] /= draws["phi_k"][i].sum(axis=1, keepdims=True)
    if garbage:
        for n in range(B):
            if model in DISCRETE:
                data["x"][n, lens[n]:] = L + 5
                if aux:
                    data[aux][n, lens[n]:] = [77, -5, 0, -2 ** 31][n % 4]
            elif entry == "estep_io":
                data["x_t"][n, lens[n]:] = 1e300
                data["u_tm"][n, lens[n]:] = np.nan
            else:
                data["x"][n, lens[n]:] = 1e300
    u = synth.ffbs_uniforms(B, tmax, seed=seed + 1) if entry in ("draw_stats", "draw_stats_gauss") else None
    return {"entry": entry, "model": model, "K": K, "L": L, "M": M, "C": C, "D": D, "B": B, "data": data,
            "draws": draws, "u": u, "T": lens, "roles": roles, "abnormal": sorted(roles.values())}


def base_classes(base):
    return classes_of(base["T"], base["C"], base["D"], base["abnormal"])


def gather(req, idx):
    """The zip request with N = S = P = len(idx) whose series row p, draw row p, T[p] and (where the entry
    reads them) uniforms row p are row idx[p] of `req` (a base, or anything with its keys)."""
    idx = np.asarray(idx, dtype=np.int64)
    B = req["B"]

    def rows(v):
        return np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v

    out = dict(req)
    out["data"] = {k: rows(v) for k, v in req["data"].items()}
    out["draws"] = {k: rows(np.asarray(v)) for k, v in req["draws"].items()}
    out["u"] = None if req["u"] is None else np.ascontiguousarray(req["u"][idx])
    out["T"] = req["T"][idx]
    out["B"] = idx.size
    return out


def device_request(req, idx):
    """gather(req, idx) with the copies of the `flag` pair made invalid: a symbol L + 1 inside the series, or
    (no symbols) the length T_max + 1.  Returns (request, hit [P] bool)."""
    out = gather(req, idx)
    hit = np.asarray(idx) == req["roles"]["flag"]
    if req["model"] in DISCRETE:
        out["data"]["x"][hit, 6] = req["L"] + 1
    else:
        out["data"]["T"][hit] = int(req["T"].max()) + 1
    return out, hit


# ---------------------------------------------------------------- the reference

def reference(req, gqs=None):
    """Reference statistics of a request, pair-major, from the existing reference modules.  The two draw
    entries count the path `gqs(model, data, draws, pars=["z_ffbs", "loglik"], pairing="zip", uniforms=u)`
    returns (the oracle's on the CPU, the engine's own on the GPU: the FFBS contract) and return its loglik
    under "loglik"."""
    entry, model, data, draws = req["entry"], req["model"], req["data"], req["draws"]
    if entry == "estep":
        return estep_ref.estep(model, data, draws, "zip")
    if entry == "expected_stats":
        return expect_ref.expected_stats(model, data, draws, "zip")
    if entry == "estep_io":
        return estep_io_ref.estep(model, data, draws, "zip")
    r = gqs(model, data, draws, pars=["z_ffbs", "loglik"], pairing="zip", uniforms=req["u"])
    if entry == "draw_stats":
        out = draw_stats_ref.counts_pairs(model, data, r["z_ffbs"], r["loglik"], "zip", req["B"])
    else:
        out = draw_stats_gauss_ref.stats_pairs(data, r["z_ffbs"], r["loglik"], "zip", req["B"])
    out["loglik"] = np.asarray(r["loglik"])
    return out


def same_bits(a, b):
    """Bit for bit: fp64 compared as 64-bit words, so a NaN equals only the same NaN and -0.0 is not 0.0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))
