/*
 * hhmm_plan.cpp -- the pure host decisions of hhmm_plan.h: the T-scan and
 * V-scan plans and the launch plan of an HMM-family request.  No HIP, no
 * device: tests/test_plan.py pins these through hhmm_selftest_plan.
 */
#include "hhmm_plan.h"

#include <stdio.h>

#include <algorithm>

namespace hhmm {

/* Parallel scan over T for the HMM-family forward-backward:
 * used when a batch has too few pairs to fill the chip with one lane per
 * pair.  The T-chunk length targets ~512k (pair, chunk) lanes. */
ScanPlan scan_plan(int model, int K, int Tmax, int64_t P, uint32_t outputs, uint32_t flags)
{
    ScanPlan sp{0, 0};
    /* the log-scale outputs run the sequential log-space recursion (hhmm_fblog.h) */
    if (!hmm_has_backward(model) || (flags & HHMM_FLAG_SCAN_OFF) || (outputs & (HHMM_OUT_FFBS | kOutLog)) ||
        !(outputs & kOutFb))
        return sp;
    const int log2cl = (int)((flags >> 8) & 0xffu);
    if (K > kMaxK) {
        /* large K (hhmm_lkscan.h): hmm-multinom and hmm; chunks a multiple of the
         * 32-step observation blocks; automatic when the batch is under 4096
         * pairs (2048 waves of two groups: two per SIMD) and long, with about
         * 128k (pair, chunk) groups for the chunks' sweeps.  At N2 (250 pairs x
         * T = 10^6) that is 2048-step chunks: 223.4 ms against 228.2 for 4096
         * and 226.0 for 1024, and lk_fb_kernel writes 55.7 GB against 68.1
         * (1024: 53.6) for 46 GB of gamma + 5.75 GB of checkpoints: a 128-byte
         * line of a gamma row is written by several waves, whose stores meet in
         * L2 less often the longer the chunks (profiles/r04r_n2_chunks.txt) */
        if ((model != HHMM_MODEL_HMM_MULTINOM && model != HHMM_MODEL_HMM_GAUSS) || K > kMaxKLarge)
            return sp;
        if (!(flags & HHMM_FLAG_SCAN_FORCE) && !(P < 4096 && Tmax >= 8192))
            return sp;
        int cl = 256;
        if (log2cl > 0) {
            cl = std::max(32, 1 << log2cl);
        } else {
            while ((int64_t)P * ((Tmax + cl - 1) / cl) > 131072 && cl < (1 << 20))
                cl *= 2;
        }
        cl = (cl + 31) & ~31;
        sp.cl = cl;
        sp.nc = (Tmax + cl - 1) / cl;
        return sp;
    }
    const int C = fb_chunk(K);
    /* a batch of under 16384 pairs (256 waves: a quarter of the chip's SIMDs)
     * is latency-bound on its T sequential steps already at T of a few hundred:
     * chunks of 4 C steps (C1, 1000 pairs x T = 500: 0.32 -> 0.10 ms), grown
     * until about 512k (pair, chunk) lanes.  At C5 (250 pairs x T = 10^6, the
     * V-scan on the high-priority side stream) that is 512-step chunks: once
     * the V-scan's tie chunks left its grid pass (round 6) the forward-backward
     * chain was the longer one, and 512 measured 6.85 / 7.50 ms against 7.96 /
     * 7.94 for 128, 7.19 for 256, 8.18 for 1024 (two boxes,
     * profiles/r06w_ab_c5_fb_chunks*.log).  Before it, 128 had been best
     * (9.80 ms against 10.22 for 256, profiles/r04l_ab_c5_rn4_chunks.log). */
    const bool small = P < 16384 && Tmax >= 256;
    int cl;
    if (log2cl > 0) {
        cl = 1 << log2cl;
    } else if (small) {
        cl = 4 * C;
        while ((int64_t)P * ((Tmax + cl - 1) / cl) > 524288 && cl < 65536)
            cl *= 2;
    } else {
        const int64_t want = (int64_t)Tmax * P / 524288;
        cl = 8 * C;
        while (cl < want && cl < 65536)
            cl *= 2;
    }
    if (cl < C)
        cl = C;
    cl -= cl % C;
    const int nc = (Tmax + cl - 1) / cl;
    if (!(flags & HHMM_FLAG_SCAN_FORCE) && !small && (P >= 131072 || Tmax < 16384 || nc < 4))
        return sp;
    if (!(flags & HHMM_FLAG_SCAN_FORCE) && nc < 4)
        return sp;
    if (scan_lanes_per_chunk(P) * nc >= (int64_t(1) << 29)) /* checkpoint columns are 32-bit byte offsets */
        return sp;
    sp.cl = cl;
    sp.nc = nc;
    return sp;
}

ScanPlan estep_scan_plan(int model, int K, int, int Tmax, int64_t P, uint32_t flags)
{
    ScanPlan sp{0, 0};
    if (!hmm_has_backward(model) || K < 1 || K > kMaxK || (model == HHMM_MODEL_TAYAL && K != 4) || Tmax < 1 || P < 1 ||
        (flags & HHMM_FLAG_SCAN_OFF))
        return sp;
    /* the gate of scan_plan at large K, borrowed: under 4096 pairs the lane
     * kernel leaves SIMDs idle, and from 8192 steps on a series is long enough
     * to pay for phases 1-2 */
    if (!(flags & HHMM_FLAG_SCAN_FORCE) && !(P < kEstepScanMaxP && Tmax >= kEstepScanMinT))
        return sp;
    const int C = fb_chunk(K);
    const int log2cl = (int)((flags >> 8) & 0xffu);
    int cl;
    if (log2cl > 0) {
        cl = 1 << std::min(log2cl, 30);
    } else {
        cl = 4 * C;
        while (P * (((int64_t)Tmax + cl - 1) / cl) > kEstepScanLanes && cl < (1 << 20))
            cl *= 2;
    }
    cl = std::max(C, cl - cl % C);
    const int64_t nc = ((int64_t)Tmax + cl - 1) / cl;
    if (P * scan_lanes_per_chunk(nc) >= (int64_t(1) << 29)) /* checkpoint columns are 32-bit byte offsets */
        return sp;
    sp.cl = cl;
    sp.nc = (int)nc;
    return sp;
}

EstepScanLayout estep_scan_layout(int model, int K, int L, int Tmax, int64_t P, uint32_t flags)
{
    EstepScanLayout w{};
    w.sp = estep_scan_plan(model, K, L, Tmax, P, flags);
    if (w.sp.cl == 0)
        return w;
    const size_t d = sizeof(double), nc = (size_t)w.sp.nc, k = (size_t)K, p = (size_t)P;
    w.ncw = scan_lanes_per_chunk(w.sp.nc);
    w.nwp = w.ncw / 64;
    w.G = P * w.ncw;
    w.ns = K + K * K + (model == HHMM_MODEL_HMM_GAUSS ? 3 * K : K * L);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    w.mf = take(nc * k * k * p * d);
    w.mx = take(nc * 3 * p * d);
    w.st = take(nc * k * p * d);
    w.sl = take(nc * p * d);
    w.be = take(nc * k * p * d);
    w.bl = take(nc * p * d);
    w.ckpt = take((size_t)(w.sp.cl / fb_chunk(K)) * k * (size_t)w.G * d);
    w.part = take(p * (size_t)w.nwp * (size_t)(w.ns + kEstepScanTail) * d);
    w.pa = take(p * k * k * d);
    w.total = off;
    return w;
}

int lkm_plan(int model, int K, int64_t N, int pairing, uint32_t outputs, uint32_t flags, int scan_cl)
{
    if (model != HHMM_MODEL_HMM_MULTINOM || K <= kMaxK || K > kMaxKLarge || pairing != HHMM_PAIR_GRID || N < 16 ||
        scan_cl > 0 || !(flags & HHMM_FLAG_LKM_MFMA) || !(outputs & kOutFb) ||
        (outputs & kOutFb & ~(HHMM_OUT_LOGLIK | HHMM_OUT_GAMMA)))
        return 0;
    return K <= 16 ? 4 : (K <= 24 ? 6 : 8);
}

int vscan_chunks(int model, int K, int Tv, int64_t P, uint32_t outputs, uint32_t flags)
{
    if (!is_hmm_family(model) || !(K == 2 || K == 4) || !(outputs & kOutVit) ||
        (flags & (HHMM_FLAG_VIT_SCAN_OFF | HHMM_FLAG_VIT_LANES | HHMM_FLAG_VIT_STATES)))
        return 0;
    if (!(flags & HHMM_FLAG_VIT_SCAN) && (P >= 2048 || Tv < 16384))
        return 0;
    const int64_t nc = (Tv + kVsChunk - 1) / kVsChunk;
    if (nc * P * K * K >= (int64_t(1) << 31)) /* 32-bit element offsets of the chunk products */
        return 0;
    return (int)nc;
}

/* State-parallel decoding for batches too small to hide the per-step
 * latency with other waves (lane-per-pair below ~2 waves per SIMD), or when
 * the caller forces it; K = 2..4 (one lane quad per pair). */
static bool use_vit_states(int K, int64_t P, uint32_t flags)
{
    if (K < 2 || K > 4 || (flags & HHMM_FLAG_VIT_LANES))
        return false;
    return (flags & HHMM_FLAG_VIT_STATES) || P < 131072;
}

/* The sequential forward(-backward) of `out` (launch_fb).  packed: the gamma
 * profile of hmm-multinom at L <= 16, whose forward sweep packs the symbols.
 * Every fb_kernel sweeps x forward over whole series and checks it inline
 * where x is all the data there is (hmm-multinom); fb_log_kernel does not. */
static void plan_fb(HmmPlan &p, int model, int K, uint32_t out, bool fwd_only, bool packed)
{
    const bool ffbs = (out & HHMM_OUT_FFBS) != 0;
    if (out & kOutLog) { /* FFBS draws (if any) from the linear filter of the contract in a second launch */
        p.fb = FBK_LOG;
        p.fb_mode = fwd_only ? FB_FWD : 0;
        p.fb_ffbs2 = ffbs;
    } else {
        p.fb = FBK_LINEAR;
        if (fwd_only)
            p.fb_mode = FB_FWD;
        else if (packed)
            p.fb_mode = FB_GAMMA | FB_PACK | (ffbs ? FB_FFBS : fb_big_ok(model, K) ? FB_BIG : 0);
        else
            p.fb_mode = ((out & kOutExtra) ? FB_FULL : FB_GAMMA) | (ffbs ? FB_FFBS : 0);
    }
    p.checked_inline |= model == HHMM_MODEL_HMM_MULTINOM && (p.fb == FBK_LINEAR || ffbs);
}

/* The Viterbi as a kernel of its own (launch_viterbi); the lane-per-pair
 * decoder reads x itself and checks it inline (hmm-multinom). */
static void plan_vit(HmmPlan &p, int model, int K, int64_t P, uint32_t flags)
{
    p.vit = p.vs_nc > 0 ? VITK_VSCAN : use_vit_states(K, P, flags) ? VITK_STATES : VITK_LANES;
    p.checked_inline |= p.vit == VITK_LANES && model == HHMM_MODEL_HMM_MULTINOM;
}

HmmPlan hmm_plan(int model, int K, int L, int Tmax, int Toos, int64_t P, int64_t, int, uint32_t out, uint32_t flags,
                 int seg_phase)
{
    HmmPlan p;
    if (!is_hmm_family(model) || K < 1 || K > kMaxK)
        return p;
    const bool lite = model == HHMM_MODEL_TAYAL_LITE;
    const bool vit = (out & kOutVit) != 0, any_fwd = (out & (kOutFb | HHMM_OUT_FFBS)) != 0;
    const bool bwd = needs_backward(model, out);
    p.sp = scan_plan(model, K, Tmax, P, out, flags);
    const bool scan = p.sp.cl > 0;
    /* hot profile of hmm-multinom: symbols repacked 4 bits each for the backward sweep */
    const bool packed = !scan && bwd && model == HHMM_MODEL_HMM_MULTINOM && L <= 16 && !(out & kOutExtra);
    if (scan)
        p.regions |= WS_CKPT | WS_CKPT_LS | WS_SCAN;
    else if (bwd)
        p.regions |= WS_CKPT | WS_CKPT_LS | (packed ? WS_XPK | WS_RNW : 0);
    if (vit) {
        p.vs_nc = vscan_chunks(model, K, lite ? Toos : Tmax, P, out, flags);
        p.regions |= WS_BP | (p.vs_nc > 0 ? WS_VSCAN : 0);
    }
    if (lite) {
        /* in-sample forward (hhmm-tayal2009-lite.stan:50-92), then the forward
         * and the Viterbi on (x_oos, sign_oos) (:94-158) */
        p.schedule = SCHED_LITE;
        HmmPlan oos;
        if (out & (HHMM_OUT_ALPHA_OOS | HHMM_OUT_UNALPHA_OOS))
            plan_fb(oos, model, K, (out & HHMM_OUT_UNALPHA_OOS) ? HHMM_OUT_UNALPHA : HHMM_OUT_ALPHA, true, false);
        p.oos_fb = oos.fb;
        if (out & (HHMM_OUT_LOGLIK | HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA))
            plan_fb(p, model, K, out, true, false);
        if (vit)
            plan_vit(p, model, K, P, flags);
        return p;
    }
    /* gamma (+ loglik) and the path in one request at hmm-multinom K = 4: one
     * of the sweeps that share x between the two (hhmm_fbv.h, launch_split) */
    const bool both = fbv_ok(model, K) && vit && (out & HHMM_OUT_GAMMA) && !(out & HHMM_OUT_FFBS) && packed &&
                      !use_vit_states(K, P, flags);
    const bool vfb_on = (flags & HHMM_FLAG_VFB) ||
                        (HHMM_VFB_DEFAULT && !(flags & (HHMM_FLAG_VFB_OFF | HHMM_FLAG_FUSED | HHMM_FLAG_FB_SPLIT |
                                                        HHMM_FLAG_NO_FUSE)));
    if (both && (flags & HHMM_FLAG_FUSED))
        p.schedule = SCHED_FUSED;
    else if (both && (out & HHMM_OUT_ZSTAR) && p.vs_nc == 0 && vfb_on)
        p.schedule = SCHED_PHASED;
    else if (both && p.vs_nc == 0 && (flags & HHMM_FLAG_FB_SPLIT) && !(flags & HHMM_FLAG_NO_FUSE))
        p.schedule = SCHED_SPLIT;
    else
        p.schedule = SCHED_SEPARATE;
    if (p.schedule != SCHED_SEPARATE) {
        p.fb = FBK_LINEAR;
        p.fb_mode = FB_GAMMA | FB_PACK | FB_BIG;
        p.vit = p.schedule == SCHED_SPLIT ? VITK_PACKED : VITK_SWEEP;
        p.side_stream = p.schedule == SCHED_SPLIT;
        /* phase 1 of the phased sweep and the split schedule's forward launch check x; the fused sweep does not */
        p.checked_inline = p.schedule != SCHED_FUSED;
    } else {
        /* the Viterbi is independent of the forward-backward: on the side stream beside it */
        p.side_stream = vit && any_fwd && !(flags & HHMM_FLAG_NO_FUSE);
        if (any_fwd && scan) {
            p.fb = FBK_SCAN;
            p.fb_mode = !bwd ? FB_FWD : (out & kOutExtra) ? FB_FULL : FB_GAMMA;
        } else if (any_fwd) {
            plan_fb(p, model, K, out, !bwd, packed);
        }
        if (vit)
            plan_vit(p, model, K, P, flags);
    }
    if (seg_phase) { /* launch_segment: the T-scan split at its exchange point; no Viterbi, no inline check */
        p.schedule = SCHED_SEGMENT;
        p.vit = VITK_NONE;
        p.side_stream = p.checked_inline = false;
    }
    return p;
}

void plan_line(const HmmPlan &p, uint32_t bound, char *buf, size_t n)
{
    static const char *const sched[] = {"none", "segment", "lite", "fused", "phased", "split", "separate"};
    static const char *const fbk[] = {"none", "log", "linear", "scan"};
    static const char *const vitk[] = {"none", "sweep", "vscan", "states", "lanes", "packed"};
    static const char *const base[] = {"GAMMA", "FULL", "FWD", "?"};
    static const char *const reg[] = {"ckpt", "ckpt_ls", "xpk", "rnw", "bp", "scan", "vscan"};
    auto regions = [&](uint32_t mask, char *out, size_t len) {
        size_t o = 0;
        out[0] = '\0';
        for (int i = 0; i < 7; ++i)
            if ((mask >> i) & 1u)
                o += (size_t)snprintf(out + o, len - o, "%s%s", o ? "," : "", reg[i]);
        if (!o)
            snprintf(out, len, "-");
    };
    char want[64], got[64], mode[48];
    regions(p.regions, want, sizeof(want));
    regions(bound, got, sizeof(got));
    if (p.fb == FBK_NONE)
        snprintf(mode, sizeof(mode), "-");
    else if (p.fb == FBK_LOG)
        snprintf(mode, sizeof(mode), "%s%s", p.fb_mode == FB_FWD ? "FWD" : "BOTH", p.fb_ffbs2 ? "+FFBS" : "");
    else
        snprintf(mode, sizeof(mode), "%s%s%s%s", base[p.fb_mode & 3], (p.fb_mode & FB_FFBS) ? "|FFBS" : "",
                 (p.fb_mode & FB_PACK) ? "|PACK" : "", (p.fb_mode & FB_BIG) ? "|BIG" : "");
    snprintf(buf, n,
             "schedule=%s fb=%s fb_mode=%s oos_fb=%s vit=%s scan_cl=%d scan_nc=%d vs_nc=%d regions=%s bound=%s "
             "checked_inline=%d side_stream=%d",
             sched[p.schedule], fbk[p.fb], mode, fbk[p.oos_fb], vitk[p.vit], p.sp.cl, p.sp.nc, p.vs_nc, want, got,
             (int)p.checked_inline, (int)p.side_stream);
}

} // namespace hhmm
