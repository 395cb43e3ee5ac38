/*
 * hhmm_gibbs_gauss.h -- draw statistics of libhhmm.so for the Gaussian hmm
 * (hmm/stan/hmm.stan): the state half of a blocked Gibbs sampler whose
 * parameter half is a Normal-Inverse-Gamma update.  For every (series, draw)
 * pair one FFBS path z is drawn from the caller's uniforms and reduced, on the
 * chip, to its sufficient statistics.  Nothing per step is written.
 *
 * z is the path hhmm_run returns as z_ffbs (HHMM_OUT_FFBS) for the same
 * request and uniforms: the FFBS contract of DESIGN.md §5, bit for bit.  The
 * result is the E-step's (hhmm_estep.h: fp64, pair-fastest) with the posterior
 * replaced by this one draw:
 *
 *   loglik [P]        the model-block log-likelihood (HHMM_OUT_LOGLIK)
 *   n_1k   [P, K]     one-hot of z_1
 *   xi_ij  [P, K, K]  #{t >= 2 : z_{t-1} = i, z_t = j} at p + P*(i + K*j)
 *   w_k    [P, K]     1 + #{t >= 2 : z_t = k}
 *   s1_k   [P, K]     x_1 + sum_{t >= 2, z_t = k} x_t
 *   s2_k   [P, K]     x_1^2 + sum_{t >= 2, z_t = k} x_t^2
 *
 * hmm.stan:30 adds normal_lpdf(x_1 | mu_k, sigma_k) for EVERY state k (Q2), so
 * the first observation counts once for each state whatever z_1 is.  The
 * weight of z under the CODED likelihood is then exactly
 *   prod_k p_1k^n_1k * prod_ij A_ij^xi_ij *
 *   prod_k (2 pi)^(-w_k/2) sigma_k^(-w_k)
 *          exp(-(s2_k - 2 mu_k s1_k + mu_k^2 w_k) / (2 sigma_k^2)),
 * so a Dirichlet update of p_1k and of the rows of A_ij and a
 * Normal-Inverse-Gamma update of (mu_k, sigma_k^2) from these statistics are
 * the exact conditionals.  The prior on (mu_k, sigma_k^2) must be proper:
 * under hmm.stan's flat priors a state that owns no step beyond x_1 has an
 * improper sigma conditional.  The lower bound
 * sigma_k >= 0.0001 of hmm.stan:21 is NOT applied by such an update.
 *
 * n_1k, xi_ij and w_k are exact integers stored as doubles.  s1_k and s2_k are
 * fp64 sums in the order of the backward sweep (t = T .. 2, then x_1); s2_k
 * adds the rounded product x_t * x_t.  c_kl is ignored and may be NULL.
 *
 * A pair's statistics are all NaN (pair_status stays HHMM_PAIR_OK) when its
 * loglik is not finite, or when any step's draw is undefined (the weights of a
 * step do not sum to a positive finite number: z_ffbs = 0 there).
 *
 * req->ffbs_u ([P, T_max], pair-fastest: the layout HHMM_OUT_FFBS takes) is
 * required; the uniforms belong in (0, 1].  outputs, hat_rand and the scan
 * flags are ignored.
 *
 * Scope: HHMM_MODEL_HMM_GAUSS at 1 <= K <= 8, every pairing, ragged T, one
 * device.  Every other model, K > 8 and HHMM_DEVICE_SET answer
 * HHMM_ERR_UNSUPPORTED (the discrete programs: hhmm_gibbs.h).
 *
 * 8 < K <= 32: hhmm_draw_stats_large, hhmm_draw_stats_large_device and
 * hhmm_draw_stats_large_workspace_size (declared in hhmm_gibbs.h, one entry
 * for hmm-multinom and for this model) return the statistics above, with the
 * same definitions, order of summation and NaN rule, from the state-parallel
 * kernel.
 */
#ifndef HHMM_GIBBS_GAUSS_H
#define HHMM_GIBBS_GAUSS_H

#include "hhmm.h"
#include "hhmm_estep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace hhmm_draw_stats_gauss_device needs (the forward
 * checkpoints: the E-step's size). */
hhmm_status hhmm_draw_stats_gauss_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series has T[n] outside 1..T_max is flagged
 * HHMM_PAIR_INVALID_DATA when pair_status is given (its statistics are
 * unspecified); every other pair is unaffected. */
hhmm_status hhmm_draw_stats_gauss_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                         size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does for hmm (a
 * violation rejects the request), uploads, runs on req->device (-1 = current),
 * downloads and synchronises. */
hhmm_status hhmm_draw_stats_gauss(const hhmm_request *req, hhmm_estep_result *res);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_GIBBS_GAUSS_H */
