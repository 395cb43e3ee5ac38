/*
 * hhmm_psis.h -- Pareto-smoothed importance sampling over the draws, on the
 * device: PSIS-LOO and the "backward" approximate leave-future-out
 * cross-validation of Buerkner, Gabry and Vehtari on top of the pointwise
 * predictive densities of hhmm_pointwise.h, and the same per-cell operation on
 * caller-supplied log ratios.
 *
 * D (the draws per series), the pairings, the layouts (n + N*t for [N, T_max],
 * p + P*t for [P, T_max], the pairs of series n consecutive) and ragged T are
 * those of hhmm_pointwise.h; t is 1-based below as there.
 *
 * A cell (n, t) has D members (r_d, l_d): log importance ratios and targets.
 *   LOO   r_d = -l_t(n, d)
 *   LFO   r_d = -(l_{T_n} + l_{T_n - 1} + ... + l_t)(n, d), accumulated in that
 *         order from +0.0, one addition per step: the draws conditioned on all
 *         of x_{1:T} are re-weighted towards the posterior given x_{1:t-1}.  At
 *         t = T_n it is -l_{T_n} exactly: the LFO and LOO cells of the last step
 *         have the same bits.  The cell at t = 1 re-weights to the prior.
 * In both kinds l_d = l_t(n, d).
 *
 * One cell:
 *   1  If any r_d or l_d is NaN or +-inf: elpd = khat = neff = NaN (no IEEE
 *      propagation as in lpd_t: a draw of zero likelihood makes the weights
 *      meaningless).
 *   2  r_d <- r_d - max_d r_d.
 *   3  M = min(floor(D / 5), c), c the smallest integer with c^2 >= 9 D.
 *   4  The draws are ranked ascending by (r_d, d).  The tail is the ranks
 *      D - M .. D - 1; cut is the value at rank D - M - 1.
 *   5  M < 5 (D < 25): the cell is not smoothed, w_d = r_d, khat = +inf.
 *   6  x_i = exp(tail_i) - exp(cut), ascending, i = 1..M.  x_1 == x_M: not
 *      smoothed, khat = +inf.
 *   7  The generalised Pareto fit of Zhang and Stephens with the weakly
 *      informative prior of PSIS: m = 30 + floor(sqrt(M)), x* = x_{(M + 2) div 4},
 *        theta_j = 1 / x_M + (1 - sqrt(m / (j - 0.5))) / (3 x*)        j = 1..m
 *        k_j = mean_i log1p(-theta_j x_i)
 *        L_j = M (log(-theta_j / k_j) - k_j - 1)
 *        omega_j = 1 / sum_i exp(L_i - L_j)
 *        theta = sum_j theta_j omega_j,  k = mean_i log1p(-theta x_i),
 *        sigma = -k / theta,  k <- (k M + 5) / (M + 10).
 *      k or sigma not finite: not smoothed, khat = +inf.
 *   8  p_i = (i - 0.5) / M, q_i = sigma expm1(-k log1p(-p_i)) / k (k == 0:
 *      -sigma log1p(-p_i)); the draw of rank D - M - 1 + i gets
 *      w = min(log(exp(cut) + q_i), 0), every other draw keeps w_d = r_d;
 *      khat = k.
 *   9  elpd = log sum_d exp(w_d + l_d) - log sum_d exp(w_d), each log shifted by
 *      its largest term; neff = (sum_d exp w_d)^2 / sum_d exp(2 w_d), the
 *      weights shifted by the largest w_d.
 *
 *   elpd_t [N, T_max]   at n + N*t: the PSIS estimate of log p(x_t | the rest)
 *                       (LOO) or of log p(x_t | x_{1:t-1}) (LFO)
 *   khat_t [N, T_max]   the Pareto shape: above 0.7 the estimate of the step
 *                       is unreliable (LFO: a refit is due)
 *   neff_t [N, T_max]   the effective number of draws of the cell
 *
 * All fp64, tolerance 1e-9 relative to max(1, |value|).  A step t >= T[n] of
 * any output is left untouched.  Every reduction has a fixed order and there
 * are no floating-point atomics: the same request gives the same bits on every
 * run, through either entry, with and without lp_t.
 *
 * D is at most HHMM_PSIS_MAX_DRAWS = 16384, the cap of hhmm_summary.h, for the
 * same reason: one cell is ordered in one workgroup's LDS.  A larger D answers
 * HHMM_ERR_UNSUPPORTED.
 */
#ifndef HHMM_PSIS_H
#define HHMM_PSIS_H

#include "hhmm_pointwise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HHMM_PSIS_MAX_DRAWS 16384

/* Caller-allocated outputs.  `pw` keeps the hhmm_pointwise.h contract field by
 * field and is filled as hhmm_pointwise fills it (lp_t and pair_status stay
 * optional); elpd_t, khat_t and neff_t are required. */
typedef struct hhmm_psis_result {
    hhmm_pointwise_result pw;
    double *elpd_t;            /* [N, T_max] */
    double *khat_t;            /* [N, T_max] */
    double *neff_t;            /* [N, T_max] */
} hhmm_psis_result;

/* PSIS-LOO and PSIS-LFO of an hhmm_request (hhmm.h; outputs, ffbs_u, hat_rand
 * and the scan flags are ignored).  Scope: hmm and hmm-multinom at
 * 1 <= K <= 32; the entry takes the kernels of hhmm_pointwise up to K = 8 and
 * of hhmm_pointwise_large above, and the other programs, K > 32,
 * HHMM_DEVICE_SET and an emission table that does not fit LDS are rejected as
 * there, with the same statuses, before the device is touched.
 *
 * Workspace, a function of the request alone (W_pw and W_pwl: the sizes
 * hhmm_pointwise_workspace_size and hhmm_pointwise_large_workspace_size
 * report):
 *     K <= 8:  W_pw + P * T_max * 8     the tiles' partials, then l_t
 *     K >  8:  W_pwl                    l_t itself
 *     LFO:     + P * T_max * 8          the suffix sums
 * The cell kernel needs none.  When lp_t is given l_t goes there and its part
 * of the workspace is not touched.
 *
 * Device entries: every pointer is a device pointer on the current HIP device;
 * the work is enqueued on `stream` without synchronising.  A pair flagged
 * HHMM_PAIR_INVALID_DATA leaves its series' cells unspecified, as in
 * hhmm_pointwise_device; every other series is unaffected.  Host entries:
 * validate the data block as hhmm_run does, upload, run on req->device (-1 =
 * current), download and synchronise; the per-step arrays make the round trip
 * whole, so a step t >= T[n] keeps what the caller put there. */
hhmm_status hhmm_psis_loo_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_psis_loo_device(const hhmm_request *req, hhmm_psis_result *res, void *workspace,
                                 size_t workspace_bytes, void *stream);
hhmm_status hhmm_psis_loo(const hhmm_request *req, hhmm_psis_result *res);

hhmm_status hhmm_psis_lfo_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_psis_lfo_device(const hhmm_request *req, hhmm_psis_result *res, void *workspace,
                                 size_t workspace_bytes, void *stream);
hhmm_status hhmm_psis_lfo(const hhmm_request *req, hhmm_psis_result *res);

/* The cell operation alone, on caller-supplied members: the building block of
 * M-step-ahead LFO or of any other importance ratios.  lr and lp are
 * [N * D, T_max] in the lp_t layout (the member d of cell (n, t) at
 * n*D + d + N*D*t); T is optional (NULL: every series has T_max steps), a
 * T[n] outside 1..T_max is rejected by the host entry and clamped to
 * 0..T_max by the device entry. */
typedef struct hhmm_psis_cells_request {
    int64_t n_series;          /* N */
    int64_t n_draws;           /* D, per series */
    int32_t T_max;
    int32_t reserved;          /* 0 */
    const int32_t *T;          /* [N] optional */
    const double *lr;          /* [N * D, T_max] log ratios r_d */
    const double *lp;          /* [N * D, T_max] targets l_d */
} hhmm_psis_cells_request;

/* 0 bytes today; asked for like every other workspace so that it may grow. */
hhmm_status hhmm_psis_cells_workspace_size(const hhmm_psis_cells_request *req, size_t *bytes);
hhmm_status hhmm_psis_cells_device(const hhmm_psis_cells_request *req, double *elpd_t, double *khat_t, double *neff_t,
                                   void *workspace, size_t workspace_bytes, void *stream);
hhmm_status hhmm_psis_cells(const hhmm_psis_cells_request *req, double *elpd_t, double *khat_t, double *neff_t,
                            int device);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_PSIS_H */
