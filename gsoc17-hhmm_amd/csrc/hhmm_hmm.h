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
 * run_model_range, which pick the kernels of one request.
 * Build with -ffp-contract=off: the Viterbi sums must round exactly as written.
 */
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "hhmm_fb.h"
#include "hhmm_viterbi.h"
#include "hhmm_fbv.h"
#include "hhmm_vscan.h"
#include "hhmm_fblog.h"
#include "hhmm_scan.h"

namespace hhmm {

static inline bool model_has_backward(int model)
{
    return model == HHMM_MODEL_HMM_GAUSS || model == HHMM_MODEL_HMM_MULTINOM ||
           model == HHMM_MODEL_HMM_MULTINOM_SEMISUP || model == HHMM_MODEL_TAYAL;
}

static inline bool needs_backward(int model, uint32_t out)
{
    return model_has_backward(model) &&
           (out & (HHMM_OUT_UNBETA | HHMM_OUT_BETA | HHMM_OUT_UNGAMMA | HHMM_OUT_GAMMA | HHMM_OUT_FFBS)) != 0;
}

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

static bool shape_for(const DevArgs &a, bool discrete, LaunchShape &s, const char *probe = nullptr)
{
    const int KP = (a.K + 1) / 2;
    size_t per_wave = discrete ? (size_t)a.L * KP * 64 * sizeof(double2) : 0;
    int waves = 4;
    if (probe && probe_env(probe)) /* probe knob (tools/ab_bench.py --env): waves per workgroup, 1..4 */
        waves = std::min(std::max(atoi(probe_env(probe)), 1), 4);
    if (per_wave > 0) {
        while (waves > 0 && per_wave * waves > kLdsLimit)
            --waves;
        if (waves == 0)
            return false;
    }
    const int threads = 64 * waves;
    s.block = dim3(threads);
    s.grid = dim3((unsigned)((a.P + threads - 1) / threads));
    s.lds = per_wave * waves;
    return true;
}

template <int MODEL, int K>
static hhmm_status launch_fb(const DevArgs &a, bool fwd_only, hipStream_t st)
{
    LaunchShape s;
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_FB_WAVES")) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    s.lds = std::max(s.lds, std::min(lds_floor("HHMM_PROBE_FB_LDS_KB"), kLdsLimit));
    const uint32_t extra = HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA | HHMM_OUT_BETA | HHMM_OUT_UNBETA | HHMM_OUT_UNGAMMA;
    const bool ffbs = (a.outputs & HHMM_OUT_FFBS) != 0;
    if (ModelTraits<MODEL>::kGauss && ffbs) /* fb_exp2_lds's table copy */
        s.lds = std::max(s.lds, kExp2TabBytes);
    constexpr bool xchk = !ModelTraits<MODEL>::kAux && ModelTraits<MODEL>::kDiscrete;
    /* every fb_kernel below sweeps x forward over whole series (fb_sweep's inline check) */
    t_data_checked_inline |= xchk && (ffbs || !(a.outputs & (HHMM_OUT_UNALPHA | HHMM_OUT_UNBETA)));
    if (a.outputs & (HHMM_OUT_UNALPHA | HHMM_OUT_UNBETA)) {
        /* log-scale outputs: the log-space recursion; FFBS draws (if any)
         * from the linear filter of the contract in a second launch */
        DevArgs b = a;
        b.outputs &= ~HHMM_OUT_FFBS;
        if (fwd_only)
            hipLaunchKernelGGL((fb_log_kernel<MODEL, K, true>), s.grid, s.block, s.lds, st, b);
        else
            hipLaunchKernelGGL((fb_log_kernel<MODEL, K, false>), s.grid, s.block, s.lds, st, b);
        if (ffbs) {
            DevArgs f = a;
            f.outputs = HHMM_OUT_FFBS;
            f.gamma = nullptr;
            f.loglik = nullptr;
            hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_GAMMA | FB_FFBS>), s.grid, s.block, s.lds, st, f);
        }
    } else if (fwd_only)
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_FWD>), s.grid, s.block, s.lds, st, a);
    else if (MODEL == HHMM_MODEL_HMM_MULTINOM && a.xpk && !(a.outputs & extra) && ffbs)
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_GAMMA | FB_FFBS | FB_PACK>), s.grid, s.block, s.lds, st, a);
    else if (fb_big_ok<MODEL, K>() && a.xpk && !(a.outputs & extra)) {
        constexpr int BIG = fb_big_ok<MODEL, K>() ? FB_GAMMA | FB_PACK | FB_BIG : FB_GAMMA;
        if constexpr (fb_big(BIG))
            (void)hipMemsetAsync(a.rnw, 0, sizeof(int32_t), st); /* the dense-wave list's count */
        hipLaunchKernelGGL((fb_kernel<MODEL, K, BIG>), s.grid, s.block, s.lds, st, a);
        if constexpr (fb_big(BIG)) /* the waves it listed (renorm_sparse_safe) */
            hipLaunchKernelGGL((fb_dense_kernel<MODEL, K, BIG>), dim3(kDenseBlocks), dim3(64),
                               s.lds / (s.block.x / 64), st, a);
    }
    else if (MODEL == HHMM_MODEL_HMM_MULTINOM && a.xpk && !(a.outputs & extra))
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_GAMMA | FB_PACK>), s.grid, s.block, s.lds, st, a);
    else if ((a.outputs & extra) && ffbs)
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_FULL | FB_FFBS>), s.grid, s.block, s.lds, st, a);
    else if (a.outputs & extra)
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_FULL>), s.grid, s.block, s.lds, st, a);
    else if (ffbs)
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_GAMMA | FB_FFBS>), s.grid, s.block, s.lds, st, a);
    else
        hipLaunchKernelGGL((fb_kernel<MODEL, K, FB_GAMMA>), s.grid, s.block, s.lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("fb_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

/* The forward-backward as a parallel scan over T (phases 1-3 above). */
template <int MODEL, int K>
static hhmm_status launch_fb_scan(const DevArgs &a, bool fwd_only, hipStream_t st)
{
    LaunchShape s;
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s)) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int64_t G = a.P * (int64_t)a.scan_nc;                        /* phase 1 lanes */
    const int64_t G3 = scan_lanes_per_chunk(a.P) * (int64_t)a.scan_nc; /* phase 3 lanes */
    const dim3 gridG((unsigned)((G + s.block.x - 1) / s.block.x));
    const dim3 gridG3((unsigned)((G3 + s.block.x - 1) / s.block.x));
    const uint32_t extra = HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA | HHMM_OUT_BETA | HHMM_OUT_UNBETA | HHMM_OUT_UNGAMMA;
    if (fwd_only) {
        hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, false>), gridG, s.block, s.lds, st, a);
        hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, false>), dim3((unsigned)a.P), dim3(64 * kBoundWaves), 0,
                           st, a);
        hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FWD>), gridG3, s.block, s.lds, st, a);
    } else {
        hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, true>), gridG, s.block, s.lds, st, a);
        hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, true>), dim3((unsigned)a.P, 2), dim3(64 * kBoundWaves), 0, st,
                           a);
        if (a.outputs & extra)
            hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_FULL>), gridG3, s.block, s.lds, st, a);
        else
            hipLaunchKernelGGL((fb_scan_kernel<MODEL, K, FB_GAMMA>), gridG3, s.block, s.lds, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("scan launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

/* State-parallel decoding for batches too small to hide the per-step
 * latency with other waves (lane-per-pair below ~2 waves per SIMD), or when
 * the caller forces it; K = 2..4 (one lane quad per pair). */
static inline bool use_vit_states(const DevArgs &a)
{
    if (a.K < 2 || a.K > 4 || (a.flags & HHMM_FLAG_VIT_LANES))
        return false;
    return (a.flags & HHMM_FLAG_VIT_STATES) || a.P < 131072;
}

template <int MODEL, int K>
static hhmm_status launch_viterbi(const DevArgs &a, hipStream_t st, bool packed = false)
{
    if constexpr (K == 2 || K == 4) {
        if (a.vs_nc > 0)
            return launch_vscan<MODEL, K>(a, st);
    }
    if constexpr (K >= 2 && K <= 4) {
        if (use_vit_states(a)) {
            const size_t lds = ((ModelTraits<MODEL>::kDiscrete ? (size_t)a.L : 0) +
                                (ModelTraits<MODEL>::kTayal ? (size_t)3 * K : 0)) * 64 * sizeof(double);
            if (lds > kLdsLimit) {
                set_error("emission column L = %d does not fit in LDS", a.L);
                return HHMM_ERR_UNSUPPORTED;
            }
            const int64_t lanes = 4 * a.P;
            hipLaunchKernelGGL((viterbi_sp_kernel<MODEL, K>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), lds,
                               st, a);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) {
                set_error("viterbi_sp_kernel launch: %s", hipGetErrorString(e));
                return HHMM_ERR_HIP;
            }
            return HHMM_OK;
        }
    }
    LaunchShape s;
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_VIT_WAVES")) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    s.lds = std::max(s.lds, std::min(lds_floor("HHMM_PROBE_VIT_LDS_KB"), kLdsLimit));
    if (packed && fbv_ok<MODEL, K>()) {
        hipLaunchKernelGGL((viterbi_kernel<MODEL, K, fbv_ok<MODEL, K>()>), s.grid, s.block, s.lds, st, a);
    } else {
        /* decodes x itself: viterbi_block's inline check */
        t_data_checked_inline |= !ModelTraits<MODEL>::kAux && ModelTraits<MODEL>::kDiscrete;
        hipLaunchKernelGGL((viterbi_kernel<MODEL, K>), s.grid, s.block, s.lds, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("viterbi_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

/* The fused forward-backward + Viterbi sweep: both emission tables per wave. */
template <int MODEL, int K>
static hhmm_status launch_fbv(const DevArgs &a, hipStream_t st)
{
    const size_t per_wave = 2 * (size_t)a.L * ((K + 1) / 2) * 64 * sizeof(double2);
    int waves = 4;
    while (waves > 0 && per_wave * waves > kLdsLimit)
        --waves;
    if (waves == 0) {
        set_error("emission tables 2*K*L = 2*%d*%d do not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int threads = 64 * waves;
    hipLaunchKernelGGL((fbv_kernel<MODEL, K>), dim3((unsigned)((a.P + threads - 1) / threads)), dim3(threads),
                       per_wave * waves, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("fbv_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

/* The phased sweep (HHMM_FLAG_VFB): vfb_kernel, then vfb_dense_kernel over the
 * waves it listed. */
template <int MODEL, int K>
static hhmm_status launch_vfb(const DevArgs &a, hipStream_t st)
{
    LaunchShape s;
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s, "HHMM_PROBE_FB_WAVES")) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    hipError_t e = hipMemsetAsync(a.rnw, 0, sizeof(int32_t), st); /* the dense-wave list's count */
    if (e == hipSuccess) {
        t_data_checked_inline |= !ModelTraits<MODEL>::kAux; /* x (and T) checked in phase 1 */
        hipLaunchKernelGGL((vfb_kernel<MODEL, K>), s.grid, s.block, s.lds, st, a);
        hipLaunchKernelGGL((vfb_dense_kernel<MODEL, K>), dim3(kDenseBlocks), dim3(64), s.lds / (s.block.x / 64), st,
                           a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        set_error("vfb_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
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
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s)) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    /* the forward launch sweeps x over whole series (fb_sweep's inline check) */
    t_data_checked_inline |= !ModelTraits<MODEL>::kAux && ModelTraits<MODEL>::kDiscrete;
    hipLaunchKernelGGL((fb_kernel<MODEL, K, MODE, FB_PH_FWD>), s.grid, s.block, s.lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("fb_kernel (forward) launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    hipStream_t vs = st;
    hhmm_status r = fork_stream(st, &vs);
    if (r != HHMM_OK)
        return r;
    r = launch_viterbi<MODEL, K>(a, vs, true);
    if (r != HHMM_OK) {
        join_stream(st, vs);
        return r;
    }
    hipLaunchKernelGGL((fb_kernel<MODEL, K, MODE, FB_PH_BWD>), s.grid, s.block, s.lds, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) {
        join_stream(st, vs);
        set_error("fb_kernel (backward) launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return join_stream(st, vs);
}

/* The two calls of a segment window (hhmm_segment; the T-scan of
 * launch_fb_scan split at its exchange point). */
template <int MODEL, int K>
static hhmm_status launch_segment(const DevArgs &a, hipStream_t st)
{
    LaunchShape s;
    if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, s)) {
        set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
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
        const uint32_t extra = HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA | HHMM_OUT_BETA | HHMM_OUT_UNBETA | HHMM_OUT_UNGAMMA;
        if (bwd) {
            hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, true>), dim3((unsigned)a.P, 2), dim3(64 * kBoundWaves), 0,
                               st, a);
            if (a.outputs & extra)
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("segment launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

template <int MODEL, int K>
static hhmm_status run_model_k(const DevArgs &a, const hhmm_request *req, const hhmm_result *res,
                               hipStream_t st)
{
    hhmm_status s = HHMM_OK;
    const uint32_t out = a.outputs;
    if (a.seg_phase) {
        if constexpr (MODEL == HHMM_MODEL_TAYAL_LITE) {
            set_error("segment windows: tayal-lite has no backward pass to split (use hhmm-tayal2009)");
            return HHMM_ERR_UNSUPPORTED;
        } else {
            return launch_segment<MODEL, K>(a, st);
        }
    }
    if (MODEL == HHMM_MODEL_TAYAL_LITE) {
        /* in-sample forward: alpha_tk / unalpha_tk / loglik (hhmm-tayal2009-lite.stan:50-92) */
        if (out & (HHMM_OUT_LOGLIK | HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA)) {
            s = launch_fb<MODEL, K>(a, true, st);
            if (s != HHMM_OK)
                return s;
        }
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
        o.outputs = out & (HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR);
        if (out & HHMM_OUT_ALPHA_OOS)
            o.outputs |= HHMM_OUT_ALPHA;
        if (out & HHMM_OUT_UNALPHA_OOS)
            o.outputs |= HHMM_OUT_UNALPHA;
        if (o.outputs & (HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA)) {
            s = launch_fb<MODEL, K>(o, true, st);
            if (s != HHMM_OK)
                return s;
        }
        if (o.outputs & (HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR))
            s = launch_viterbi<MODEL, K>(o, st);
        return s;
    }
    const bool any_fwd = (out & (HHMM_OUT_LOGLIK | HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA | HHMM_OUT_BETA |
                                 HHMM_OUT_UNBETA | HHMM_OUT_GAMMA | HHMM_OUT_UNGAMMA | HHMM_OUT_FFBS)) != 0;
    /* The Viterbi pass is independent of the forward-backward: it runs on a
     * side stream forked from (and joined back into) the caller's stream, so
     * the VALU-bound decoder's workgroups fill in beside the HBM-bound
     * forward-backward's instead of strictly after them. */
    const bool vit = (out & (HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR)) != 0;
    /* Both launch shapes are checked before either kernel is enqueued, so an
     * unsupported shape never leaves a kernel running on the side stream
     * while the caller reclaims its buffers. */
    if (any_fwd) {
        LaunchShape chk;
        if (!shape_for(a, ModelTraits<MODEL>::kDiscrete, chk)) {
            set_error("emission table K*L = %d*%d does not fit in LDS", a.K, a.L);
            return HHMM_ERR_UNSUPPORTED;
        }
    }
    if constexpr (fbv_ok<MODEL, K>()) {
        /* gamma (+ loglik) and the path in one request, on request: the fused sweep */
        const uint32_t extra = HHMM_OUT_ALPHA | HHMM_OUT_UNALPHA | HHMM_OUT_BETA | HHMM_OUT_UNBETA |
                               HHMM_OUT_UNGAMMA | HHMM_OUT_FFBS;
        if (vit && (out & HHMM_OUT_GAMMA) && !(out & extra) && a.xpk && a.scan_cl == 0 &&
            (a.flags & HHMM_FLAG_FUSED) && !use_vit_states(a))
            return launch_fbv<MODEL, K>(a, st);
        const bool vfb_on = (a.flags & HHMM_FLAG_VFB) ||
                            (HHMM_VFB_DEFAULT && !(a.flags & (HHMM_FLAG_VFB_OFF | HHMM_FLAG_FUSED | HHMM_FLAG_FB_SPLIT |
                                                              HHMM_FLAG_NO_FUSE)));
        if (vit && (out & HHMM_OUT_GAMMA) && (out & HHMM_OUT_ZSTAR) && a.zstar && !(out & extra) && a.xpk &&
            a.rnw && a.scan_cl == 0 && a.vs_nc == 0 && vfb_on && !use_vit_states(a))
            return launch_vfb<MODEL, K>(a, st);
        if (vit && (out & HHMM_OUT_GAMMA) && !(out & extra) && a.xpk && a.scan_cl == 0 && a.vs_nc == 0 &&
            (a.flags & HHMM_FLAG_FB_SPLIT) && !(a.flags & HHMM_FLAG_NO_FUSE) && !use_vit_states(a))
            return launch_split<MODEL, K>(a, st);
    }
    hipStream_t vs = st;
    if (vit && any_fwd && !(a.flags & HHMM_FLAG_NO_FUSE)) {
        s = fork_stream(st, &vs);
        if (s != HHMM_OK)
            return s;
        s = launch_viterbi<MODEL, K>(a, vs);
        if (s != HHMM_OK) {
            join_stream(st, vs);
            return s;
        }
    }
    if (any_fwd) {
        if (a.scan_cl > 0 && !(out & HHMM_OUT_FFBS))
            s = launch_fb_scan<MODEL, K>(a, !needs_backward(MODEL, out), st);
        else
            s = launch_fb<MODEL, K>(a, !needs_backward(MODEL, out), st);
        if (s != HHMM_OK) {
            if (vs != st)
                join_stream(st, vs); /* the caller's stream still orders the running decoder */
            return s;
        }
    }
    if (vs != st)
        return join_stream(st, vs);
    if (vit)
        s = launch_viterbi<MODEL, K>(a, st);
    return s;
}

/* Dispatch on K for the K values [KK, KHI] this translation unit instantiates. */
template <int MODEL, int KK, int KHI>
static hhmm_status run_model_range(const DevArgs &a, const hhmm_request *req, const hhmm_result *res,
                                   hipStream_t st)
{
    if constexpr (KK > KHI) {
        set_error("K = %d not supported by this build of model %d", a.K, MODEL);
        return HHMM_ERR_UNSUPPORTED;
    } else {
        if (a.K == KK)
            return run_model_k<MODEL, KK>(a, req, res, st);
        return run_model_range<MODEL, KK + 1, KHI>(a, req, res, st);
    }
}

} // namespace hhmm
