/*
 * hhmm_estep_io.h -- batched E-step of libhhmm.so for the input-output HMM
 * programs (iohmm-reg, iohmm-mix, iohmm-hmix, iohmm-hmix-lite; models 4..7):
 * the expected sufficient statistics of every (series, draw) pair, summed over
 * the steps, and the transition-weight gradient that no per-step output of
 * include/hhmm.h carries.
 *
 * The coded "transition" A_t = softmax(u_t' w_k) is a K-vector indexed by the
 * previous state only (iohmm-reg.stan:70), so the coded path weight factorises
 * over the steps:
 *   W(z) = [p_1k(z_1) e_1(z_1) A_2(z_1)] [e_2(z_2) A_3(z_2)] ... [e_T(z_T)]
 * with e_t(k) the program's emission density (iohmm-reg.stan:54,
 * iohmm-mix.stan:53-65).  With lw_t(k) = oblik_t(k) + log A_{t+1}(k) -- plus
 * log p_1k(k) at t = 1, without the log A term at t = T --
 *   c_t = LSE_k lw_t(k),   l = sum_t c_t,   q_t = softmax_k lw_t.
 * q_t is the posterior of z_t under the coded weight (the adjoint of the coded
 * forward pass), NOT the program's gamma_tk, which equals alpha_tk because the
 * coded beta is 1/K.  With r_t(k,l) = q_t(k) lambda_kl N(x_t | mu_kl, s_kl) /
 * e_t(k):
 *
 *   every model
 *   loglik [P]          l, the model-block log-likelihood (HHMM_OUT_LOGLIK)
 *   n_1k   [P, K]       q_1(k)
 *   gw_km  [P, K, M]    sum_{t=2..T} (q_{t-1}(k) - A_t(k)) u_t: dl/dw_km itself;
 *                       all zero at T = 1
 *   iohmm-reg
 *   n_k    [P, K]       sum_t q_t(k)
 *   uu_kmm [P, K, M, M] sum_t q_t(k) u_t u_t' (full matrix, bitwise symmetric)
 *   ux_km  [P, K, M]    sum_t q_t(k) u_t x_t
 *   xx_k   [P, K]       sum_t q_t(k) x_t^2
 *   iohmm-mix, iohmm-hmix, iohmm-hmix-lite (one likelihood)
 *   n_kl   [P, K, L]    sum_t r_t(k,l)
 *   sx_kl  [P, K, L]    sum_t r_t(k,l) x_t
 *   sxx_kl [P, K, L]    sum_t r_t(k,l) x_t^2
 *
 * The score of l (Fisher's identity):
 *   dl/dp_1k[k] = n_1k / p_1k          dl/dw_km = gw_km
 *   reg: dl/db_k = (ux_k - uu_k b_k) / s_k^2
 *        dl/ds_k = -n_k / s_k + (xx_k - 2 b_k' ux_k + b_k' uu_k b_k) / s_k^3
 *   mix: dl/dlambda_kl = n_kl / lambda_kl   dl/dmu_kl = (sx - mu n) / s^2
 *        dl/ds_kl = -n / s + (sxx - 2 mu sx + mu^2 n) / s^3
 * The priors of the model blocks are not part of l.
 *
 * All outputs are fp64, pair-fastest ([P, a, b] at p + P*(a + A*b)), tolerance
 * 1e-9 relative to max(1, |value|).  When l is -inf or NaN (a NaN draw, s <= 0)
 * every statistic of the pair is NaN and pair_status stays HHMM_PAIR_OK.
 * p_1k[k] = 0 makes q_1(k) an exact 0.  Padding past T[n] is never read into a
 * result.  Steps carry no running scale: an outlier whose every density
 * underflows in linear space still gives a finite l and the right q.
 *
 * Scope: models 4..7 at 1 <= K <= 8, 1 <= M <= 8, mixtures of L <= 8
 * components, every pairing, ragged T.  Other models, K > 8, HHMM_DEVICE_SET
 * and a shape whose accumulators of one wave do not fit a CU's LDS answer
 * HHMM_ERR_UNSUPPORTED.  What fits: iohmm-reg at M <= 4 for every K, at M > 4
 * for K <= 5; the mixtures at K * L <= 40, and at M > 4 with K >= 5 (gw joins the
 * accumulators in LDS) at K * (L + 1) <= 40.  The request is the hhmm_request
 * of hhmm.h (x_real, u as [N, T_max, M], M, L; p_1k, w_km, then b_km, s_k or
 * lambda_kl, mu_kl, s_kl); outputs, ffbs_u, hat_rand and flags are ignored.
 */
#ifndef HHMM_ESTEP_IO_H
#define HHMM_ESTEP_IO_H

#include "hhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-allocated outputs.  The pointers of the other family may be NULL
 * (n_kl, sx_kl, sxx_kl for iohmm-reg; n_k, uu_kmm, ux_km, xx_k for the mixture
 * programs); pair_status is optional. */
typedef struct hhmm_estep_io_result {
    double  *loglik;           /* [P] */
    double  *n_1k;             /* [P, K] */
    double  *gw_km;            /* [P, K, M] */
    double  *n_k;              /* [P, K]        iohmm-reg */
    double  *uu_kmm;           /* [P, K, M, M]  iohmm-reg */
    double  *ux_km;            /* [P, K, M]     iohmm-reg */
    double  *xx_k;             /* [P, K]        iohmm-reg */
    double  *n_kl;             /* [P, K, L]     mixture programs */
    double  *sx_kl;            /* [P, K, L]     mixture programs */
    double  *sxx_kl;           /* [P, K, L]     mixture programs */
    int32_t *pair_status;      /* [P] optional */
} hhmm_estep_io_result;

/* Bytes of device workspace hhmm_estep_io_device needs: 0 (one forward sweep,
 * no checkpoints). */
hhmm_status hhmm_estep_io_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series has T[n] outside 1..T_max is flagged
 * HHMM_PAIR_INVALID_DATA when pair_status is given (its statistics are
 * unspecified); every other pair is unaffected.  workspace may be NULL. */
hhmm_status hhmm_estep_io_device(const hhmm_request *req, hhmm_estep_io_result *res, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does (a violation
 * rejects the request), uploads, runs on req->device (-1 = current), downloads
 * and synchronises. */
hhmm_status hhmm_estep_io(const hhmm_request *req, hhmm_estep_io_result *res);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_ESTEP_IO_H */
