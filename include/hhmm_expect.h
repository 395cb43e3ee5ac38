/*
 * hhmm_expect.h -- expected draw statistics of libhhmm.so: the E-step of the
 * programs whose forward pass is masked.  For every (series, draw) pair the
 * posterior expectation, under the CODED path weight, of each statistic that
 * hhmm_gibbs.h tabulates for one drawn path:
 *
 *   weight(z) = prod_k p_1k^n_1k(z) * prod_ij A_ij^xi_ij(z) * prod_kl phi_kl^c_kl(z)
 *
 * with the counts of hhmm_gibbs.h, which follow the forward masks
 * (hmm-multinom-semisup.stan:42 on g_t, hhmm-tayal2009.stan:62 on sign_t, the
 * init predicate hhmm-tayal2009.stan:51).  hhmm_estep.h refuses these programs
 * because their own backward passes are not the adjoint of their forward
 * (semisup's is unmasked, Tayal's masks on the previous state, quirk Q6), so
 * gamma_tk of hhmm_run is not the posterior of that weight.  Here:
 *
 *   M_t(i, j)   = A(i, j) where the forward mask applies the factor at (t, j), else 1
 *   alpha_1(k)  = e_1(k) p_1k[k] where the init factor applies, else e_1(k)
 *   alpha_t(j)  = e_t(j) sum_i alpha_{t-1}(i) M_t(i, j)          (the forward of hhmm_run)
 *   beta_T      = 1,  beta_{t-1}(i) = sum_j M_t(i, j) e_t(j) beta_t(j)   (its adjoint)
 *   Z           = sum_k alpha_t(k) beta_t(k)                      (the same at every t)
 *
 *   loglik [P]        the model-block log-likelihood (HHMM_OUT_LOGLIK)
 *   n_1k   [P, K]     gamma_1(k) where the init factor applies at (aux_1, k), else 0
 *   xi_ij  [P, K, K]  sum over t >= 2 with the mask on at (t, j) of
 *                     alpha_{t-1}(i) A(i, j) e_t(j) beta_t(j) / Z, at p + P*(i + K*j)
 *   c_kl   [P, K, L]  sum_t gamma_t(k) [x_t = l],  gamma_t = alpha_t .* beta_t / Z
 *
 * These are the exact score of loglik (Fisher's identity) for all three programs:
 *   dl/dp_1k[k] = n_1k / p_1k    dl/dA_ij = xi_ij / A_ij    dl/dphi_kl = c_kl / phi_kl
 * and the mean of hhmm_draw_stats over its uniforms (Rao-Blackwell).
 *
 * The result is hhmm_estep_result: fp64, pair-fastest, tolerance 1e-9 relative to
 * max(1, |value|).  w_k, s1_k and s2_k are ignored and may be NULL.  A structural
 * zero of A gives an exact zero.  A pair whose loglik is not finite, or whose Z
 * at some step is not positive and finite, has all-NaN statistics and
 * HHMM_PAIR_OK.  outputs, ffbs_u, hat_rand and the scan flags are ignored.
 *
 * Scope: hmm-multinom, hmm-multinom-semisup and hhmm-tayal2009 at 1 <= K <= 8,
 * every pairing, ragged T, one device.  hmm-multinom has no mask: the entry runs
 * the E-step's kernel and its outputs are those of hhmm_estep, bit for bit.
 * hmm (Gaussian), tayal-lite, the IOHMMs, K > 8, HHMM_DEVICE_SET and an emission
 * table with L * ceil(K / 2) > 80 (the table and its count table of one wave do
 * not fit a CU's LDS) answer HHMM_ERR_UNSUPPORTED.
 */
#ifndef HHMM_EXPECT_H
#define HHMM_EXPECT_H

#include "hhmm.h"
#include "hhmm_estep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace hhmm_expected_stats_device needs (the forward
 * checkpoints: the E-step's size). */
hhmm_status hhmm_expected_stats_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series breaks a data-block bound (x outside 1..L, g outside
 * 1..G, sign outside 1..2, T[n] outside 1..T_max) is flagged
 * HHMM_PAIR_INVALID_DATA when pair_status is given (its statistics are
 * unspecified; no table is indexed with the bad symbol); every other pair is
 * unaffected. */
hhmm_status hhmm_expected_stats_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does (a violation
 * rejects the request), uploads, runs on req->device (-1 = current), downloads
 * and synchronises. */
hhmm_status hhmm_expected_stats(const hhmm_request *req, hhmm_estep_result *res);

/* The expected statistics as a parallel scan over T (few pairs, long series):
 * the schedule, flags, workspace, accuracy and bit rules of hhmm_estep_scan
 * (hhmm_estep.h) with the scope, definitions, NaN rule and invalid-data rule of
 * hhmm_expected_stats.  The backward boundary vectors of the scan come from the
 * forward chunk products applied as column maps: the adjoint needs no products
 * of its own.  K > 8 answers HHMM_ERR_UNSUPPORTED with "K = <value>" in the
 * message, which names hhmm_estep_large (hmm and hmm-multinom only). */
hhmm_status hhmm_expected_stats_scan_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_expected_stats_scan_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                            size_t workspace_bytes, void *stream);
hhmm_status hhmm_expected_stats_scan(const hhmm_request *req, hhmm_estep_result *res);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_EXPECT_H */
