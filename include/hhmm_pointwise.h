/*
 * hhmm_pointwise.h -- pointwise predictive densities of libhhmm.so: the
 * one-step-ahead predictive log density of every step of every (series, draw)
 * pair, reduced over the draws of each series on the device.
 *
 *   l_t(n, d) = log p(x_t | x_{1:t-1}, theta_d),    sum_t l_t = loglik
 *
 * is the ingredient of WAIC, leave-future-out cross-validation and PSIS.  The
 * outputs of include/hhmm.h carry it only inside unalpha_tk ([P, T, K]); here
 * one forward sweep per pair forms it, and three [N, T_max] arrays leave the
 * device.
 *
 * D is the number of draws per series: S under HHMM_PAIR_GRID, S / N under
 * HHMM_PAIR_BLOCK, 1 under HHMM_PAIR_ZIP.  Under every pairing the pairs of
 * series n are the consecutive p = n*D .. n*D + D - 1.
 *
 * l_t follows the CODED likelihood of the Stan program, as every other entry:
 *   l_1 = log sum_k p_1k e_1(k);  hmm.stan:30 (quirk Q2 of SURVEY.md App. A)
 *         gives l_1 = sum_j normal_lpdf(x_1 | mu_j, sigma_j) + log sum_k p_1k
 *   l_t = log(sum_j alpha_t(j) / sum_i alpha_{t-1}(i))  for t >= 2
 *
 *   loglik [P]            as hhmm_estep
 *   lpd_t  [N, T_max]     at n + N*t: log((1 / D) sum_d exp l_t(n, d)), shifted by
 *                         the largest member
 *   mean_t [N, T_max]     (1 / D) sum_d l_t(n, d)
 *   var_t  [N, T_max]     sum_d (l_t(n, d) - mean_t)^2 / (D - 1)
 *   lp_t   [P, T_max]     at p + P*t, optional (NULL: not written): l_t(n, d)
 *                         itself, for PSIS / leave-future-out
 *
 * All outputs are fp64, tolerance 1e-9 relative to max(1, |value|).  A step
 * t >= T[n] of any of the four per-step arrays is left untouched.
 *
 * Non-finite values are IEEE arithmetic on the formulas above.  An impossible
 * observation gives l_t = -inf at that step and NaN after it (0 / 0); loglik
 * is -inf.  A cell (n, t) with a NaN member is NaN in lpd_t, mean_t and var_t.
 * A cell whose members are finite or -inf has lpd_t finite (-inf when every
 * member is -inf), never NaN; with a -inf member mean_t = -inf and var_t =
 * NaN.  D = 1 gives var_t = NaN.  pair_status stays HHMM_PAIR_OK in all of
 * these.
 *
 * The reduction uses no floating-point atomics and a fixed order: the same
 * request gives the same bits on every run, with and without lp_t.
 *
 * Scope: hmm and hmm-multinom at 1 <= K <= 8 (9 <= K <= 32: the
 * hhmm_pointwise_large entries at the end), every pairing, ragged T.  The
 * semisup, Tayal and IOHMM programs answer HHMM_ERR_UNSUPPORTED (their coded
 * step weights are masked or factorised: the ratio of consecutive forward sums
 * is not a predictive density), as do K > 8, HHMM_DEVICE_SET and an emission
 * table with L * ceil(K / 2) > 154 (the table of one wave does not fit a CU's
 * LDS beside the reduction buffers).  The request is the hhmm_request of
 * hhmm.h; outputs, ffbs_u, hat_rand and the scan flags are ignored.
 */
#ifndef HHMM_POINTWISE_H
#define HHMM_POINTWISE_H

#include "hhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-allocated outputs; lp_t and pair_status are optional. */
typedef struct hhmm_pointwise_result {
    double  *loglik;           /* [P] */
    double  *lpd_t;            /* [N, T_max] */
    double  *mean_t;           /* [N, T_max] */
    double  *var_t;            /* [N, T_max] */
    double  *lp_t;             /* [P, T_max] optional */
    int32_t *pair_status;      /* [P] optional */
} hhmm_pointwise_result;

/* Bytes of device workspace hhmm_pointwise_device needs.  One workgroup
 * reduces 64 w draws of one series, w = the most waves (at most 4) whose
 * tables of L * ceil(K / 2) + 6 KiB each fit 160 KiB of LDS (hmm: w = 4).  A
 * series with D <= 64 w draws needs none: 0.  Otherwise ceil(D / (64 w)) tiles
 * per series each leave five partial sums per cell: tiles * 5 * N * T_max * 8
 * bytes. */
hhmm_status hhmm_pointwise_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series breaks a data-block bound (x outside 1..L, T[n] outside
 * 1..T_max) is flagged HHMM_PAIR_INVALID_DATA when pair_status is given (its
 * values and its series' cells are unspecified; the table is never indexed with
 * the bad symbol); every other series is unaffected. */
hhmm_status hhmm_pointwise_device(const hhmm_request *req, hhmm_pointwise_result *res, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does (a violation
 * rejects the request), uploads, runs on req->device (-1 = current), downloads
 * and synchronises.  The per-step arrays make the round trip whole (uploaded,
 * then downloaded), so a step t >= T[n] keeps what the caller put there. */
hhmm_status hhmm_pointwise(const hhmm_request *req, hhmm_pointwise_result *res);

/* The same three at 9 <= K <= 32 (the state-parallel kernels: a group of 16
 * lanes per pair up to K = 16, of 32 above), hmm and hmm-multinom, the same
 * hhmm_pointwise_result with every field as above -- the layouts, the steps
 * t >= T[n] left untouched, the IEEE rules, the coded likelihood, the same bits
 * on every run with and without lp_t and through either entry.  K <= 8 answers
 * HHMM_ERR_UNSUPPORTED here (hhmm_pointwise takes it), as do K > 32, the other
 * programs, HHMM_DEVICE_SET and an emission table whose group does not fit a
 * CU's LDS: two exchange slots and the [L][G] table, (2 + L) * G * 8 bytes
 * against 160 KiB, i.e. L > 1278 at K <= 16 (G = 16) and L > 638 above (G = 32).
 *
 * Workspace: l_t itself, P * T_max * 8 bytes, which a second kernel reduces
 * over the draws of each cell.  The size is a function of the request alone,
 * so it is reported (and required by the device entry) whatever the result
 * struct holds; when lp_t is given l_t goes there and the workspace is not
 * touched. */
hhmm_status hhmm_pointwise_large_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_pointwise_large_device(const hhmm_request *req, hhmm_pointwise_result *res, void *workspace,
                                        size_t workspace_bytes, void *stream);
hhmm_status hhmm_pointwise_large(const hhmm_request *req, hhmm_pointwise_result *res);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_POINTWISE_H */
