/*
 * hhmm_plan.h -- everything the host decides about a request before a kernel
 * runs, in one place: the output classes and model predicates, the chunk
 * geometry shared by host and kernels, and the launch plan of an HMM-family
 * request (hmm_plan, hhmm_plan.cpp).  Workspace sizing (ws_layout,
 * hhmm_kernels.hip) and dispatch (run_model_k, hhmm_hmm.h) both read the plan,
 * so a region a kernel writes is a region that was sized.  Host-only: no HIP
 * header, no device, no pointers.  Not part of the public ABI.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hhmm.h"

namespace hhmm {

/* ---- output classes ---- */
constexpr uint32_t kOutLog = HHMM_OUT_UNALPHA | HHMM_OUT_UNBETA; /* log scale: the log-space recursion (hhmm_fblog.h) */
/* the outputs that take a request off the gamma profile (FB_FULL) */
constexpr uint32_t kOutExtra = HHMM_OUT_ALPHA | HHMM_OUT_BETA | HHMM_OUT_UNGAMMA | kOutLog;
/* the outputs that need the backward sweep (and so the forward checkpoints) */
constexpr uint32_t kOutBack = HHMM_OUT_UNBETA | HHMM_OUT_BETA | HHMM_OUT_UNGAMMA | HHMM_OUT_GAMMA | HHMM_OUT_FFBS;
/* the forward-backward set: what the filter and smoother produce (FFBS aside) */
constexpr uint32_t kOutFb = HHMM_OUT_LOGLIK | HHMM_OUT_GAMMA | kOutExtra;
constexpr uint32_t kOutVit = HHMM_OUT_ZSTAR | HHMM_OUT_LOGP_ZSTAR;
/* The outputs the IOHMM linear-space filter produces; a pair whose filter
 * drops below kIoWeak is listed in a.io_redo and re-run in log space by
 * launch_iohmm_log (hhmm_iolog.hip). */
constexpr uint32_t kIoFilt = kOutFb | HHMM_OUT_OBLIK_T;
constexpr uint32_t kIoBack = kOutBack & ~HHMM_OUT_FFBS;

/* ---- model predicates ---- */
constexpr bool is_tayal(int m) { return m == HHMM_MODEL_TAYAL || m == HHMM_MODEL_TAYAL_LITE; }
/* the HMM family with a backward pass (tayal-lite is forward + Viterbi only) */
constexpr bool hmm_has_backward(int m)
{
    return m == HHMM_MODEL_HMM_GAUSS || m == HHMM_MODEL_HMM_MULTINOM || m == HHMM_MODEL_HMM_MULTINOM_SEMISUP ||
           m == HHMM_MODEL_TAYAL;
}
constexpr bool is_hmm_family(int m) { return hmm_has_backward(m) || m == HHMM_MODEL_TAYAL_LITE; }
constexpr bool is_discrete(int m) { return is_hmm_family(m) && m != HHMM_MODEL_HMM_GAUSS; }
constexpr bool is_iohmm(int m) { return m >= HHMM_MODEL_IOHMM_REG && m <= HHMM_MODEL_IOHMM_HMIX_LITE; }
constexpr bool needs_backward(int m, uint32_t out) { return hmm_has_backward(m) && (out & kOutBack) != 0; }

/* ---- chunk geometry (host and kernels) ---- */
constexpr int kMaxK = 8;       /* lane-per-pair kernels (hhmm_hmm.h, hhmm_iohmm.h) */
constexpr int kMaxKLarge = 32; /* state-parallel HMM-family kernels (hhmm_large.h) */

/* Time steps between forward checkpoints kept for the backward sweep. */
constexpr int fb_chunk(int K) { return K <= 4 ? 8 : 4; }

/* Viterbi back-pointer packing: bits per state, bits per step, steps per word. */
constexpr int bp_bits(int K) { return K <= 2 ? 1 : (K <= 4 ? 2 : (K <= 8 ? 3 : 4)); }
constexpr int bp_steps_per_word(int K) { return 32 / (K * bp_bits(K)); }

/* Viterbi chunk length: a multiple of the back-pointer steps per word so
 * that every word boundary falls on a static unrolled slot. */
constexpr int vit_chunk(int K)
{
    return bp_steps_per_word(K) >= 8 ? bp_steps_per_word(K)
                                      : (8 % bp_steps_per_word(K) == 0 ? 8 : 2 * bp_steps_per_word(K));
}

/* Phase-3 lanes of the T-scan per T-chunk: P rounded up to whole waves. */
constexpr int64_t scan_lanes_per_chunk(int64_t P) { return (P + 63) & ~(int64_t)63; }

/* Parallel-scan plan of one request: T-chunk length and count (cl = 0: off). */
struct ScanPlan {
    int cl;
    int nc;
};
ScanPlan scan_plan(int model, int K, int Tmax, int64_t P, uint32_t outputs, uint32_t flags);

/* The E-step and the expected statistics as a parallel scan over T
 * (hhmm_estep_scan.hip), hmm, hmm-multinom, hmm-multinom-semisup and
 * hhmm-tayal2009 at K <= kMaxK: T-chunk length and count (cl = 0: the
 * sequential lane kernel).  HHMM_FLAG_SCAN_CHUNK_LOG2(n) gives the length
 * (rounded down to a multiple of fb_chunk(K), at least one), HHMM_FLAG_SCAN_FORCE
 * passes the gate, HHMM_FLAG_SCAN_OFF closes it.  Left alone the scan runs
 * where P < kEstepScanMaxP and Tmax >= kEstepScanMinT, with chunks of
 * 4 fb_chunk(K) steps doubled until P * nc <= kEstepScanLanes: that bounds the
 * phase-3 lanes (one per (pair, chunk), a pair's chunks padded to whole waves:
 * at most kEstepScanLanes + 63 P while chunks stay under 2^20 steps, where the
 * doubling stops) and with them the partials, one record per wave.  Off where the padded lanes reach 2^29 (checkpoint columns are 32-bit
 * byte offsets), whatever the flags. */
constexpr int64_t kEstepScanMaxP = 4096;
constexpr int kEstepScanMinT = 8192;
constexpr int64_t kEstepScanLanes = 262144;
ScanPlan estep_scan_plan(int model, int K, int L, int Tmax, int64_t P, uint32_t flags);

/* Workspace of a T-scan E-step, in this order, every region at a 256-byte
 * boundary, all fp64 (include/hhmm_estep.h documents it): the scan regions of
 * DevArgs (sc_mf [P][nc][K][K], sc_mx [P][nc][3], sc_st [nc][K][P], sc_sl
 * [nc][P], sc_be [nc][K][P], sc_bl [nc][P]; no sc_qb), the in-chunk checkpoints
 * [cl / fb_chunk(K)][K][G] over G = P * ncw phase-3 lanes (ncw: nc rounded up
 * to whole waves), the partials [P][nwp][ns + kEstepScanTail] (nwp = ncw / 64
 * waves per pair; ns = K + K^2 + K L statistics, 3 K in place of K L for the
 * Gaussian hmm) and each pair's A, [P][K][K].  total = 0: no scan (estep_scan_plan). */
constexpr int kEstepScanTail = 5; /* bad, max x - 1, max aux - 1, aux_1, x_1 */
struct EstepScanLayout {
    ScanPlan sp;
    int64_t ncw, nwp, G;
    int ns;
    size_t mf, mx, st, sl, be, bl, ckpt, part, pa, total;
};
EstepScanLayout estep_scan_layout(int model, int K, int L, int Tmax, int64_t P, uint32_t flags);

/* T-parallel exact Viterbi (hhmm_vscan.h): V-chunks of kVsChunk steps (a whole
 * number of back-pointer words at K = 2 and 4); returns the chunk count per
 * pair of a Viterbi over Tv steps, 0 when the sequential decoders run. */
#ifndef HHMM_VS_CHUNK
#define HHMM_VS_CHUNK 512 /* build knob: steps per V-chunk */
#endif
constexpr int kVsChunk = HHMM_VS_CHUNK;
int vscan_chunks(int model, int K, int Tv, int64_t P, uint32_t outputs, uint32_t flags);

/* Large K under GRID pairing (hhmm_lkscan.h lkm_fb_kernel): the k-steps of
 * its state capacity when it runs the forward-backward, else 0. */
int lkm_plan(int model, int K, int64_t N, int pairing, uint32_t outputs, uint32_t flags, int scan_cl);

/* ---- forward-backward kernel profiles ---- */
/* Output profile of the forward-backward kernel (compile time). */
enum FbMode {
    FB_GAMMA = 0, /* loglik + gamma_tk: the hot path, no per-output branches */
    FB_FULL = 1,  /* any mix of alpha/beta/unalpha/unbeta/ungamma/gamma (+ per-step log scale) */
    FB_FWD = 2,   /* forward only: loglik / alpha / unalpha (tayal-lite, no backward output) */
    FB_FFBS = 4,  /* flag: FFBS draws in the backward sweep */
    FB_PACK = 8,  /* flag: the forward sweep packs each chunk's symbols (4 bits, L <= 16)
                   * into the checkpoint record; the backward sweep reads those
                   * instead of re-reading x (hmm-multinom: 4 B -> 1 B per step) */
    FB_BIG = 16,  /* flag (gamma profile): checkpoints every kBigChunk steps, and a
                   * two-level recompute in the backward sweep (every kGroup-th
                   * state kept, each group recomputed before it is consumed):
                   * checkpoint traffic 8 -> 4 B per step for ~1.44 forward
                   * recomputes per step instead of 1 */
    FB_RN1 = 32   /* flag (with FB_BIG): renormalise every step -- the waves whose
                   * pairs' parameters do not bound the kBigRenorm-step shrink
                   * (renorm_sparse_safe) */
};
/* FB_BIG applies to hmm-multinom's packed gamma profile with 8-step chunks. */
constexpr bool fb_big_ok(int model, int K) { return model == HHMM_MODEL_HMM_MULTINOM && fb_chunk(K) == 8; }
/* The fused and phased sweeps (hhmm_fbv.h) walk forward and Viterbi chunks together. */
constexpr bool fbv_ok(int model, int K) { return fb_big_ok(model, K) && vit_chunk(K) == fb_chunk(K); }
#ifndef HHMM_VFB_DEFAULT
#define HHMM_VFB_DEFAULT 1 /* the phased sweep for the C2 request without flags */
#endif

/* ---- the launch plan of one HMM-family request at K <= kMaxK ---- */
enum Schedule {
    SCHED_NONE,     /* not an HMM-family request at K <= kMaxK */
    SCHED_SEGMENT,  /* one window of a series split along T (launch_segment) */
    SCHED_LITE,     /* tayal-lite: in-sample forward, OOS forward, OOS Viterbi */
    SCHED_FUSED,    /* fbv_kernel */
    SCHED_PHASED,   /* vfb_kernel + vfb_dense_kernel */
    SCHED_SPLIT,    /* forward launch, then backward launch beside the packed Viterbi */
    SCHED_SEPARATE, /* forward-backward and Viterbi as kernels of their own */
};
enum FbKind { FBK_NONE, FBK_LOG, FBK_LINEAR, FBK_SCAN };
enum VitKind {
    VITK_NONE,
    VITK_SWEEP,  /* inside the fused / phased sweep */
    VITK_VSCAN,  /* T-parallel (launch_vscan) */
    VITK_STATES, /* viterbi_sp_kernel: a lane quad per pair */
    VITK_LANES,  /* viterbi_kernel decoding x */
    VITK_PACKED, /* viterbi_kernel decoding the packed record */
};
enum WsRegion : uint32_t {
    WS_CKPT = 1, WS_CKPT_LS = 2, WS_XPK = 4, WS_RNW = 8, WS_BP = 16, WS_SCAN = 32, WS_VSCAN = 64,
};

struct HmmPlan {
    Schedule schedule = SCHED_NONE;
    bool side_stream = false; /* the Viterbi kernel runs on the side stream */
    FbKind fb = FBK_NONE;     /* in-sample forward(-backward) */
    int fb_mode = 0;          /* FBK_LINEAR / FBK_SCAN: FbMode bits; FBK_LOG: FB_FWD or 0 (both sweeps) */
    bool fb_ffbs2 = false;    /* FBK_LOG: a second, linear launch draws FFBS */
    FbKind oos_fb = FBK_NONE; /* SCHED_LITE: the OOS forward launch (FBK_LOG or FBK_LINEAR, forward only) */
    VitKind vit = VITK_NONE;
    ScanPlan sp{0, 0};
    int vs_nc = 0;
    uint32_t regions = 0;        /* WsRegion bits the planned kernels read or write */
    bool checked_inline = false; /* one of the sweeps checks x against 1..L as it reads it */
};

/* seg_phase: 0 a whole series, 1 / 2 the calls of a segment window. */
HmmPlan hmm_plan(int model, int K, int L, int Tmax, int Toos, int64_t P, int64_t N, int pairing, uint32_t outputs,
                 uint32_t flags, int seg_phase = 0);

/* The plan as one line of key=value words (hhmm_selftest_plan); `bound`: the
 * WsRegion bits bind_workspace gave a non-NULL pointer. */
void plan_line(const HmmPlan &p, uint32_t bound, char *buf, size_t n);

} // namespace hhmm
