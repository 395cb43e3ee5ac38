/*
 * hhmm_hmm.h -- the HMM family (hmm, hmm-multinom, semisup, Tayal full /
 * lite) as templates; each hhmm_m_*.hip includes this header and instantiates
 * one model (one translation unit per model so the library builds in
 * parallel).  The kernels are in the headers included below:
 *   hhmm_step.h     per-step primitives: masks, observation loads, per-pair
 *                   parameters, LDS emission tables, one recursion step; the
 *                   HBM / LDS layout and the latency rules
 *   hhmm_fbchunk.h  one checkpoint chunk of the forward and backward sweeps
 *                   (what the statistics kernels share with fb_kernel)
 *   hhmm_fb.h       fb_sweep, fb_kernel, fb_dense_kernel
 *   hhmm_viterbi.h  viterbi_kernel, viterbi_sp_kernel
 *   hhmm_fbv.h      the fused (fbv) and phased (vfb) sweeps
 *   hhmm_vscan.h    T-parallel exact Viterbi
 *   hhmm_fblog.h    fb_log_kernel
 *   hhmm_scan.h     the parallel scan over T, fb_scan_kernel
 * This file holds the host side: the launch templates and run_model_k /
 * run_model_range, which launch what the request's plan (hmm_plan,
 * hhmm_plan.h) names; no launcher decides anything from the request itself.
 * Build with -ffp-contract=off: the Viterbi sums must round exactly as written.
 */
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "hhmm_fb.h"
#include "hhmm_viterbi.h"
#include "hhmm_fbv.h"
#include "hhmm_vscan.h"
#include "hhmm_fblog.h"
#include "hhmm_scan.h"

namespace hhmm {

/* ------------------------------------------------------------------ */
/* Launch templates (instantiated per model in hhmm_m_*.hip)            */
/* ------------------------------------------------------------------ */
struct LaunchShape {
    dim3 grid, block;
    size_t lds;
};

/* Probe knob (tools/ab_bench.py --env): a minimum LDS request per workgroup
 * in KiB from the environment variable `name`, which caps how many of the
 * kernel's workgroups share a CU (and so leaves room for the other kernel's). */
static size_t lds_floor(const char *name)
{
    const char *v = probe_env(name);
    return v ? (size_t)atoi(v) * 1024 : 0;
}

/* One lane per pair, a wave's emission table in LDS; an error when one wave's does not fit. */
static hhmm_status shape_for(const DevArgs &a, bool discrete, LaunchShape &s, const char *probe = nullptr)
{
    const int KP = (a.K + 1) / 2;
    int waves = 4;
    if (probe && probe_env(probe)) /* probe knob (tools/ab_bench.py --env): waves per workgroup, 1..4 */
        waves = std::min(std::max(atoi(probe_env(probe)), 1), 4);
    waves = waves_that_fit(discrete ? (size_t)a.L * KP * 64 * sizeof(double2) : 0, &s.lds, waves);
    if (waves == 0)
        return lds_fit_error(a.K, a.L);
    const int threads = 64 * waves;
    s.block = dim3(threads);
    s.grid = dim3((unsigned)((a.P + threads - 1) / threads));
    return HHMM_OK;
}

/* A plan names a kernel this (MODEL, K) does not instantiate, or a workspace
 * region bind_workspace left unbound: never a launch. */
static hhmm_status plan_error(const DevArgs &a, const char *what)
{
    set_error("launch plan of model %d at K = %d: %s", a.model, a.K, what);
    return HHMM_ERR_INVALID_ARGUMENT;
}

/* The sequential forward(-backward): the plan's kind and FbMode bits to the instantiation. */
template <int MODEL, int K>
static hhmm_status launch_fb(const DevArgs &a, FbKind kind, int mode, bool ffbs2, hipStream_t st)
{
    LaunchShape s;
    const hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_FB_WAVES");
    if (r != HHMM_OK)
        return r;
    s.lds = std::max(s.lds, std::min(lds_floor("HHMM_PROBE_FB_LDS_KB"), kLdsLimit));
    if (ModelTraits<MODEL>::kGauss && (ffbs2 || (mode & FB_FFBS))) /* fb_exp2_lds's table copy */
        s.lds = std::max(s.lds, kExp2TabBytes);
    auto fb = [&](auto m, const DevArgs &b) {
        hipLaunchKernelGGL((fb_kernel<MODEL, K, decltype(m)::value>), s.grid, s.block, s.lds, st, b);
    };
    constexpr int BIG = fb_big_ok<MODEL, K>() ? FB_GAMMA | FB_PACK | FB_BIG : FB_GAMMA;
    if (kind == FBK_LOG) {
        /* log-scale outputs: the log-space recursion; FFBS draws (if any)
         * from the linear filter of the contract in a second launch */
        DevArgs b = a;
        b.outputs &= ~HHMM_OUT_FFBS;
        if (mode == FB_FWD)
            hipLaunchKernelGGL((fb_log_kernel<MODEL, K, true>), s.grid, s.block, s.lds, st, b);
        else
            hipLaunchKernelGGL((fb_log_kernel<MODEL, K, false>), s.grid, s.block, s.lds, st, b);
        if (ffbs2) {
            DevArgs f = a;
            f.outputs = HHMM_OUT_FFBS;
            f.gamma = nullptr;
            f.loglik = nullptr;
            fb(std::integral_constant<int, FB_GAMMA | FB_FFBS>{}, f);
        }
    } else {
        switch (mode) {
        case FB_FWD: fb(std::integral_constant<int, FB_FWD>{}, a); break;
        case FB_GAMMA | FB_FFBS | FB_PACK: fb(std::integral_constant<int, FB_GAMMA | FB_FFBS | FB_PACK>{}, a); break;
        case FB_GAMMA | FB_PACK | FB_BIG:
            if (!fb_big(BIG))
                return plan_error(a, "no FB_BIG kernel");
            if constexpr (fb_big(BIG))
                (void)hipMemsetAsync(a.rnw, 0, sizeof(int32_t), st); /* the dense-wave list's count */
            fb(std::integral_constant<int, BIG>{}, a);
            if constexpr (fb_big(BIG)) /* the waves it listed (renorm_sparse_safe) */
                hipLaunchKernelGGL((fb_dense_kernel<MODEL, K, BIG>), dim3(kDenseBlocks), dim3(64),
                                   s.lds / (s.block.x / 64), st, a);
            break;
        case FB_GAMMA | FB_PACK: fb(std::integral_constant<int, FB_GAMMA | FB_PACK>{}, a); break;
        case FB_FULL | FB_FFBS: fb(std::integral_constant<int, FB_FULL | FB_FFBS>{}, a); break;
        case FB_FULL: fb(std::integral_constant<int, FB_FULL>{}, a); break;
        case FB_GAMMA | FB_FFBS: fb(std::integral_constant<int, FB_GAMMA | FB_FFBS>{}, a); break;
        case FB_GAMMA: fb(std::integral_constant<int, FB_GAMMA>{}, a); break;
        default: return plan_error(a, "no fb_kernel of that mode");
        }
    }
    return launch_status("fb_kernel");
}

/* The forward-backward as a parallel scan over T (phases 1-3 above). */
template <int MODEL, int K>
static hhmm_status launch_fb_scan(const DevArgs &a, int mode, hipStream_t st)
{
    LaunchShape s;
    const hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s);
    if (r != HHMM_OK)
        return r;
    const int64_t G = a.P * (int64_t)a.scan_nc;                        /* phase 1 lanes */
    const int64_t G3 = scan_lanes_per_chunk(a.P) * (int64_t)a.scan_nc; /* phase 3 lanes */
    const dim3 gridG((unsigned)((G + s.block.x - 1) / s.block.x));
    const dim3 gridG3((unsigned)((G3 + s.block.x - 1) / s.block.x));
    if (mode == FB_FWD) {
        hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, false>), gridG, s.block, s.lds, st, a);
        hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, false>), dim3((unsigned)a.P), dim3(64 * kBoundWaves), 0,
                           st, a);
        hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FWD>), gridG3, s.block, s.lds, st, a);
    } else {
        hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, true>), gridG, s.block, s.lds, st, a);
        hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, true>), dim3((unsigned)a.P, 2), dim3(64 * kBoundWaves), 0, st,
                           a);
        if (mode == FB_FULL)
            hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FULL>), gridG3, s.block, s.lds, st, a);
        else
            hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_GAMMA>), gridG3, s.block, s.lds, st, a);
    }
    return launch_status("scan");
}

/* The Viterbi as a kernel of its own: the plan's kind to the decoder. */
template <int MODEL, int K>
static hhmm_status launch_viterbi(const DevArgs &a, VitKind kind, hipStream_t st)
{
    if (kind == VITK_VSCAN) {
        if constexpr (K == 2 || K == 4)
            return launch_vscan<MODEL, K>(a, st);
        return plan_error(a, "no V-scan");
    }
    if (kind == VITK_STATES) {
        if constexpr (K >= 2 && K <= 4) {
            const size_t lds = ((ModelTraits<MODEL>::kDiscrete ? (size_t)a.L : 0) +
                                (ModelTraits<MODEL>::kTayal ? (size_t)3 * K : 0)) * 64 * sizeof(double);
            if (lds > kLdsLimit) {
                set_error("emission column L = %d does not fit in LDS", a.L);
                return HHMM_ERR_UNSUPPORTED;
            }
            const int64_t lanes = 4 * a.P;
            hipLaunchKernelGGL((viterbi_sp_kernel<MODEL, K>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), lds,
                               st, a);
            return launch_status("viterbi_sp_kernel");
        }
        return plan_error(a, "no state-parallel decoder");
    }
    LaunchShape s;
    const hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_VIT_WAVES");
    if (r != HHMM_OK)
        return r;
    s.lds = std::max(s.lds, std::min(lds_floor("HHMM_PROBE_VIT_LDS_KB"), kLdsLimit));
    if (kind == VITK_PACKED && fbv_ok<MODEL, K>()) /* the packed record of the split schedule's forward launch */
        hipLaunchKernelGGL((viterbi_kernel<MODEL, K, fbv_ok<MODEL, K>()>), s.grid, s.block, s.lds, st, a);
    else if (kind == VITK_LANES)
        hipLaunchKernelGGL((viterbi_kernel<MODEL, K>), s.grid, s.block, s.lds, st, a);
    else
        return plan_error(a, "no such Viterbi kernel");
    return launch_status("viterbi_kernel");
}

/* The fused forward-backward + Viterbi sweep: both emission tables per wave. */
template <int MODEL, int K>
static hhmm_status launch_fbv(const DevArgs &a, hipStream_t st)
{
    size_t lds;
    const int waves = waves_that_fit(2 * (size_t)a.L * ((K + 1) / 2) * 64 * sizeof(double2), &lds);
    if (waves == 0) {
        set_error("emission tables 2*K*L = 2*%d*%d do not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int threads = 64 * waves;
    hipLaunchKernelGGL((fbv_kernel<MODEL, K>), dim3((unsigned)((a.P + threads - 1) / threads)), dim3(threads), lds,
                       st, a);
    return launch_status("fbv_kernel");
}

/* The phased sweep (HHMM_FLAG_VFB): vfb_kernel, then vfb_dense_kernel over the
 * waves it listed. */
template <int MODEL, int K>
static hhmm_status launch_vfb(const DevArgs &a, hipStream_t st)
{
    LaunchShape s;
    const hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_FB_WAVES");
    if (r != HHMM_OK)
        return r;
    const hipError_t e = hipMemsetAsync(a.rnw, 0, sizeof(int32_t), st); /* the dense-wave list's count */
    if (e != hipSuccess) {
        set_error("vfb_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    hipLaunchKernelGGL((vfb_kernel<MODEL, K>), s.grid, s.block, s.lds, st, a);
    hipLaunchKernelGGL((vfb_dense_kernel<MODEL, K>), dim3(kDenseBlocks), dim3(64), s.lds / (s.block.x / 64), st, a);
    return launch_status("vfb_kernel");
}

/* The split schedule (HHMM_FLAG_FB_SPLIT, C2's profile): the forward sweep
 * alone (x read once: loglik, checkpoints, packed symbols), then the
 * HBM-bound backward sweep on the caller's stream beside the VALU-bound
 * Viterbi on the side stream, which decodes the packed symbols. */
template <int MODEL, int K>
static hhmm_status launch_split(const DevArgs &a, hipStream_t st)
{
    constexpr int MODE = FB_GAMMA | FB_PACK | FB_BIG;
    LaunchShape s;
    hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s);
    if (r != HHMM_OK)
        return r;
    hipLaunchKernelGGL((fb_kernel<MODEL, K, MODE, FB_PH_FWD>), s.grid, s.block, s.lds, st, a);
    if ((r = launch_status("fb_kernel (forward)")) != HHMM_OK)
        return r;
    hipStream_t vs = st;
    if ((r = fork_stream(st, &vs)) != HHMM_OK)
        return r;
    if ((r = launch_viterbi<MODEL, K>(a, VITK_PACKED, vs)) == HHMM_OK) {
        hipLaunchKernelGGL((fb_kernel<MODEL, K, MODE, FB_PH_BWD>), s.grid, s.block, s.lds, st, a);
        r = launch_status("fb_kernel (backward)");
    }
    const hhmm_status j = join_stream(st, vs); /* the caller's stream orders the decoder also after an error */
    return r != HHMM_OK ? r : j;
}

/* The two calls of a segment window (hhmm_segment; the T-scan of
 * launch_fb_scan split at its exchange point). */
template <int MODEL, int K>
static hhmm_status launch_segment(const DevArgs &a, hipStream_t st)
{
    LaunchShape s;
    const hhmm_status r = shape_for(a, ModelTraits<MODEL>::kDiscrete, s);
    if (r != HHMM_OK)
        return r;
    const bool bwd = needs_backward(MODEL, a.outputs);
    if (a.seg_phase == 1) {
        const int64_t G = a.P * (int64_t)a.scan_nc;
        const dim3 gridG((unsigned)((G + s.block.x - 1) / s.block.x));
        const dim3 gridP((unsigned)((a.P + kBlock - 1) / kBlock));
        if (bwd) {
            hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, true>), gridG, s.block, s.lds, st, a);
            hipLaunchKernelGGL((seg_summary_kernel<MODEL, K, true>), gridP, dim3(kBlock), 0, st, a);
        } else {
            hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, false>), gridG, s.block, s.lds, st, a);
            hipLaunchKernelGGL((seg_summary_kernel<MODEL, K, false>), gridP, dim3(kBlock), 0, st, a);
        }
    } else {
        const int64_t G3 = scan_lanes_per_chunk(a.P) * (int64_t)a.scan_nc;
        const dim3 gridG3((unsigned)((G3 + s.block.x - 1) / s.block.x));
        if (bwd) {
            hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, true>), dim3((unsigned)a.P, 2), dim3(64 * kBoundWaves), 0,
                               st, a);
            if (a.outputs & kOutExtra)
                hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FULL>), gridG3, s.block, s.lds, st, a);
            else
                hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_GAMMA>), gridG3, s.block, s.lds, st, a);
        } else {
            hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, false>), dim3((unsigned)a.P), dim3(64 * kBoundWaves), 0,
                               st, a);
            if (a.outputs & (HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA))
                hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FWD>), gridG3, s.block, s.lds, st, a);
        }
    }
    return launch_status("segment");
}

/* Forward-backward and Viterbi as kernels of their own.  The Viterbi pass is
 * independent of the forward-backward: with p.side_stream it runs on a side
 * stream forked from (and joined back into) the caller's stream, so the
 * VALU-bound decoder's workgroups fill in beside the HBM-bound
 * forward-backward's instead of strictly after them. */
template <int MODEL, int K>
static hhmm_status launch_separate(const DevArgs &a, const HmmPlan &p, hipStream_t st)
{
    hhmm_status s = HHMM_OK;
    hipStream_t vs = st;
    if (p.side_stream) {
        if ((s = fork_stream(st, &vs)) != HHMM_OK)
            return s;
        if ((s = launch_viterbi<MODEL, K>(a, p.vit, vs)) != HHMM_OK) {
            join_stream(st, vs);
            return s;
        }
    }
    if (p.fb == FBK_SCAN)
        s = launch_fb_scan<MODEL, K>(a, p.fb_mode, st);
    else if (p.fb != FBK_NONE)
        s = launch_fb<MODEL, K>(a, p.fb, p.fb_mode, p.fb_ffbs2, st);
    if (p.side_stream) { /* after an error too: the caller's stream still orders the running decoder */
        const hhmm_status j = join_stream(st, vs);
        return s != HHMM_OK ? s : j;
    }
    if (s == HHMM_OK && p.vit != VITK_NONE)
        s = launch_viterbi<MODEL, K>(a, p.vit, st);
    return s;
}

template <int MODEL, int K>
static hhmm_status run_model_k(const DevArgs &a, const HmmPlan &p, const hhmm_request *req, const hhmm_result *res,
                               hipStream_t st)
{
    if (p.regions & ~bound_regions(a))
        return plan_error(a, "a workspace region of a planned kernel is not bound");
    if (p.schedule == SCHED_PHASED && !a.zstar)
        return plan_error(a, "the phased sweep writes zstar_t, which is NULL");
    /* The forward-backward's launch shape is checked before any kernel is
     * enqueued, so an unsupported shape never leaves a kernel running on the
     * side stream while the caller reclaims its buffers. */
    if (p.schedule >= SCHED_FUSED && p.fb != FBK_NONE) {
        LaunchShape chk;
        const hhmm_status s = shape_for(a, ModelTraits<MODEL>::kDiscrete, chk);
        if (s != HHMM_OK)
            return s;
    }
    switch (p.schedule) {
    case SCHED_SEGMENT:
        if constexpr (MODEL == HHMM_MODEL_TAYAL_LITE) {
            set_error("segment windows: tayal-lite has no backward pass to split (use hhmm-tayal2009)");
            return HHMM_ERR_UNSUPPORTED;
        } else {
            return launch_segment<MODEL, K>(a, st);
        }
    case SCHED_LITE: {
        hhmm_status s = HHMM_OK;
        /* in-sample forward: alpha_tk / unalpha_tk / loglik (hhmm-tayal2009-lite.stan:50-92) */
        if (p.fb != FBK_NONE && (s = launch_fb<MODEL, K>(a, p.fb, p.fb_mode, false, st)) != HHMM_OK)
            return s;
        /* out-of-sample forward and Viterbi on (x_oos, sign_oos) (:94-158) */
        DevArgs o = a;
        o.Tmax = req->data.T_oos_max;
        o.Tout = req->data.T_oos_max;
        o.T = req->data.T_oos;
        o.x = req->data.x_oos;
        o.sign = req->data.sign_oos;
        o.loglik = nullptr;
        o.alpha = res->alpha_tk_oos;
        o.unalpha = res->unalpha_tk_oos;
        o.outputs = a.outputs & kOutVit;
        if (a.outputs & HHMM_OUT_ALPHA_OOS)
            o.outputs |= HHMM_OUT_ALPHA;
        if (a.outputs & HHMM_OUT_UNALPHA_OOS)
            o.outputs |= HHMM_OUT_UNALPHA;
        if (p.oos_fb != FBK_NONE && (s = launch_fb<MODEL, K>(o, p.oos_fb, FB_FWD, false, st)) != HHMM_OK)
            return s;
        if (p.vit != VITK_NONE)
            s = launch_viterbi<MODEL, K>(o, p.vit, st);
        return s;
    }
    case SCHED_FUSED:
    case SCHED_PHASED:
    case SCHED_SPLIT:
        if constexpr (fbv_ok<MODEL, K>()) {
            return p.schedule == SCHED_FUSED    ? launch_fbv<MODEL, K>(a, st)
                   : p.schedule == SCHED_PHASED ? launch_vfb<MODEL, K>(a, st)
                                                : launch_split<MODEL, K>(a, st);
        }
        break;
    case SCHED_SEPARATE: return launch_separate<MODEL, K>(a, p, st);
    default: break;
    }
    return plan_error(a, "no such schedule");
}

/* Dispatch on K for the K values [KK, KHI] this translation unit instantiates. */
template <int MODEL, int KK, int KHI>
static hhmm_status run_model_range(const DevArgs &a, const HmmPlan &p, const hhmm_request *req,
                                   const hhmm_result *res, hipStream_t st)
{
    if constexpr (KK > KHI) {
        set_error("K = %d not supported by this build of model %d", a.K, MODEL);
        return HHMM_ERR_UNSUPPORTED;
    } else {
        if (a.K == KK)
            return run_model_k<MODEL, KK>(a, p, req, res, st);
        return run_model_range<MODEL, KK + 1, KHI>(a, p, req, res, st);
    }
}

} // namespace hhmm
