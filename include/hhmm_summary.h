/*
 * hhmm_summary.h -- C ABI of the reduction over draws (quantiles and hard
 * states), part of libhhmm.so.
 *
 * Every consumer in the reference reduces the [S, T, K] arrays extract()
 * returns over the draws straight away and drops the draws:
 *     apply(apply(alpha_tk, c(2, 3), median), 1, which.max)
 *         (tayal2009/main.R:131-132, tayal2009/R/wf-trade.R:119-120,
 *          tayal2009/main-sim.R:102, hmm/main-multinom.R:136,
 *          hmm/main-multinom-semisup.R:115, iohmm-reg/main.R:81-85)
 *     apply(alpha, c(2, 3), quantile(x, c(0.1, 0.5, 0.9)))   (common/R/plots.R:261-271)
 *     apply(zstar, 2, median)      (plots.R:328,448; tayal2009/main.R:134)
 *     apply(xhat, 2, median)       (plots.R:396)
 * Here that reduction runs on the device, on the engine's pair-major outputs:
 * N series with S draws each, pair p = s + S*n (GRID pairing, or BLOCK pairing
 * with S = n_draws / N), so the S values of one cell (n, t, k) are the S
 * contiguous elements at  values + S*n + P*(t + T_max*k),  P = N*S.
 *
 * Cell quantile at probability p in [0, 1] -- R's default (type 7):
 *     if any x is NaN: q = NaN
 *     y = x sorted ascending by <
 *     h = (S - 1) * p;  lo = floor(h);  hi = ceil(h);  q = y[lo]
 *     if (h > lo and y[hi] != y[lo]):  g = h - lo;  q = (1 - g) * y[lo] + g * y[hi]
 * evaluated in fp64 exactly as written (no contraction); +-inf are ordinary
 * values; the order statistics are exact (a selection, not a sketch).  int32
 * inputs (zstar_t, z_ffbs, hatz_t, hatl_t) are converted to double first, so
 * an even S can give x.5 as R's median() does.  With p = 0.5 the result equals
 * R's median() except where a middle value is subnormal: median() takes
 * mean(sort(x)[half + 0:1]) = (a + b) / 2, the formula above 0.5 * a + 0.5 * b,
 * and halving a subnormal before the sum can round where the sum first cannot.
 *
 * Argmax (optional): argmax[n, t] is the 1-based first k maximising the
 * quantile at argmax_prob (R's which.max); NaN quantiles are skipped, and the
 * result is 0 when all K are NaN.
 *
 * Layouts (R column-major, first index fastest, as in hhmm.h):
 *     values     [P, T_max, K]  ([P, T_max] when K = 1)
 *     quantiles  [N, T_max, K, Q]   quantiles[n + N*(t + T_max*(k + K*j))]
 *     argmax     [N, T_max]
 * Steps t >= T[n] of a ragged series are neither read nor written.  Failed
 * pairs (hhmm_result.pair_status != 0; e.g. zstar_t = 0 after an unset Viterbi
 * back-pointer) are summarised as they are: the caller holds pair_status.
 */
#ifndef HHMM_SUMMARY_H
#define HHMM_SUMMARY_H

#include "hhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HHMM_SUMMARY_MAX_PROBS 16
/* S doubles of one cell are sorted in one workgroup's LDS (128 KiB of 160). */
#define HHMM_SUMMARY_MAX_DRAWS 16384

typedef struct hhmm_summary_request {
    int64_t n_series;          /* N */
    int64_t n_draws;           /* S draws per series, 1 .. HHMM_SUMMARY_MAX_DRAWS; P = N * S */
    int32_t T_max;             /* padded time extent */
    int32_t K;                 /* trailing extent (1 for a [P, T_max] array) */
    const int32_t *T;          /* [N] lengths; NULL: every series has T_max */
    int32_t n_probs;           /* Q, 1 .. 16 */
    int32_t reserved;          /* 0 */
    double probs[HHMM_SUMMARY_MAX_PROBS]; /* each in [0, 1] */
    double argmax_prob;        /* in [0, 1], or -1: no argmax */
    const double *values_f64;  /* exactly one of the two */
    const int32_t *values_i32;
} hhmm_summary_request;

/* Device pointers on the current device (values, T, quantiles, argmax),
 * enqueued on `stream`; does not synchronise.  argmax may be NULL when
 * argmax_prob is -1. */
hhmm_status hhmm_summary_device(const hhmm_summary_request *req, double *quantiles, int32_t *argmax, void *stream);

/* Host pointers: uploads, runs on `device` (-1 = current), downloads. */
hhmm_status hhmm_summary(const hhmm_summary_request *req, double *quantiles, int32_t *argmax, int device);

/* ---- fused: hhmm_run, then the reduction, without the per-draw arrays ever
 * reaching the host ------------------------------------------------------- */
typedef struct hhmm_summary_spec {
    int32_t n_probs;           /* Q, 1 .. 16 */
    uint32_t summarise;        /* HHMM_OUT_* bits of per-step outputs to reduce */
    uint32_t argmax;           /* subset of `summarise` with a K axis: also the hard state */
    int32_t reserved;          /* 0 */
    double probs[HHMM_SUMMARY_MAX_PROBS];
    double argmax_prob;        /* needed (in [0, 1]) when argmax != 0 */
} hhmm_summary_spec;

/* Caller-allocated, indexed by the bit NUMBER of HHMM_OUT_* (alpha_tk: 2):
 * quantiles[b] is [N, T, K, Q] ([N, T, Q] without a K axis), argmax[b] is
 * [N, T]; T is T_max, or T_oos_max for the tayal-lite zstar_t and *_oos. */
typedef struct hhmm_summary_result {
    double *quantiles[32];
    int32_t *argmax[32];
} hhmm_summary_result;

/* Host arrays in, summaries out.  The request is split into ranges of series
 * (all draws of a series stay together) sized so that a range's per-draw
 * outputs and workspace fit a device budget (HHMM_FLAG_HOST_CHUNKS(n) forces
 * the count); per range the inputs are uploaded, hhmm_run_device's kernels
 * fill pooled device buffers, the summary kernel reduces them there, and only
 * the summaries, the [P] outputs (loglik, logp_zstar: in `pairs`) and
 * pair_status come back.  Every per-step bit of req->outputs must be in
 * spec->summarise (the bits of spec->summarise are computed whether or not
 * req->outputs names them); HHMM_PAIR_ZIP is rejected (nothing to reduce).
 * Results do not depend on the number of ranges (more than one pins SCAN_OFF |
 * VIT_SCAN_OFF, as hhmm_run's pipeline does; a request that runs a parallel
 * scan over T is one range).  req->device == HHMM_DEVICE_SET splits the series
 * over min(N, set size) devices, one host thread each, never the draws.
 * pair_status and HHMM_WARN_PAIR_FAILURES behave as in hhmm_run. */
hhmm_status hhmm_run_summary(const hhmm_request *req, const hhmm_summary_spec *spec, hhmm_result *pairs,
                             hhmm_summary_result *out);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_SUMMARY_H */
