/*
 * hhmm_gibbs.h -- draw statistics of libhhmm.so: the state half of a blocked
 * Gibbs sampler.  For every (series, draw) pair one FFBS path z is drawn from
 * the caller's uniforms and reduced, on the chip, to the sufficient statistics
 * the conjugate parameter updates need.  Nothing per step is written.
 *
 * z is the path hhmm_run returns as z_ffbs (HHMM_OUT_FFBS) for the same
 * request and uniforms: the FFBS contract of DESIGN.md §5, bit for bit.  The
 * result is the E-step's (hhmm_estep.h: fp64, pair-fastest) with the posterior
 * replaced by this one draw:
 *
 *   loglik [P]        the model-block log-likelihood (HHMM_OUT_LOGLIK)
 *   n_1k   [P, K]     one-hot of z_1.  Tayal: only where the init predicate
 *                     (hhmm-tayal2009.stan:51) applies the factor p_1k at
 *                     (sign_1, z_1); otherwise the row is all zeros.
 *   xi_ij  [P, K, K]  #{t >= 2 : z_{t-1} = i, z_t = j} at p + P*(i + K*j), over
 *                     the steps where the model's forward mask applies A(i, j)
 *                     at (t, j): every step for hmm-multinom,
 *                     hmm-multinom-semisup.stan:42 on g_t, hhmm-tayal2009.stan:62
 *                     on sign_t.
 *   c_kl   [P, K, L]  #{t >= 1 : z_t = k, x_t = l}
 *
 * The weight of z under the CODED likelihood is then exactly
 *   prod_k p_1k^n_1k * prod_ij A_ij^xi_ij * prod_kl phi_kl^c_kl,
 * so Dirichlet / Beta updates from these counts are the exact conditionals.
 * The counts are exact integers stored as doubles.  w_k, s1_k and s2_k are
 * ignored and may be NULL.
 *
 * A pair's statistics are all NaN (pair_status stays HHMM_PAIR_OK) when its
 * loglik is not finite, or when any step's draw is undefined (the weights of a
 * step do not sum to a positive finite number: z_ffbs = 0 there).
 *
 * req->ffbs_u ([P, T_max], pair-fastest: the layout HHMM_OUT_FFBS takes) is
 * required; the uniforms belong in (0, 1].  outputs, hat_rand and the scan
 * flags are ignored.
 *
 * Scope: hmm-multinom, hmm-multinom-semisup and hhmm-tayal2009 at 1 <= K <= 8,
 * every pairing, ragged T, one device.  hmm (Gaussian), tayal-lite, the
 * IOHMMs, K > 8, HHMM_DEVICE_SET and tables that do not fit a CU's LDS answer
 * HHMM_ERR_UNSUPPORTED.  One wave keeps its emission table (fp64) and its two
 * count tables (32-bit) in LDS: the bound is
 *   L * (4 * ceil(K / 2) + K) + K * K <= 640      (units of 256 bytes, 160 KiB)
 * i.e. L <= 24 at K = 8, L <= 52 at K = 4.
 *
 * 8 < K <= 32: hhmm_draw_stats_large (below) takes hmm-multinom and the
 * Gaussian hmm (hhmm_gibbs_gauss.h has its statistics) there, on groups of 16
 * or 32 lanes per pair.
 */
#ifndef HHMM_GIBBS_H
#define HHMM_GIBBS_H

#include "hhmm.h"
#include "hhmm_estep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace hhmm_draw_stats_device needs (the forward
 * checkpoints: the E-step's size). */
hhmm_status hhmm_draw_stats_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series breaks a data-block bound (x outside 1..L, T[n] outside
 * 1..T_max) is flagged HHMM_PAIR_INVALID_DATA when pair_status is given (its
 * statistics are unspecified; no table is indexed with the bad symbol); every
 * other pair is unaffected. */
hhmm_status hhmm_draw_stats_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does (a violation
 * rejects the request), uploads, runs on req->device (-1 = current), downloads
 * and synchronises. */
hhmm_status hhmm_draw_stats(const hhmm_request *req, hhmm_estep_result *res);

/*
 * The same statistics at 9 <= K <= 32, for hmm-multinom (loglik, n_1k, xi_ij,
 * c_kl as above) and for the Gaussian hmm (loglik, n_1k, xi_ij, w_k, s1_k, s2_k
 * as hhmm_gibbs_gauss.h defines them; the arrays of the other family are
 * ignored and may be NULL).  A group of G lanes owns a pair, lane j state j:
 * G = 16 up to K = 16, G = 32 above.  z is the path hhmm_run returns as z_ffbs
 * at these K for the same request and uniforms, bit for bit, and loglik comes
 * from that same filter.  NaN statistics, ffbs_u, the pairings, ragged T and
 * HHMM_PAIR_INVALID_DATA on the device entry are as above.
 *
 * Scope: hmm-multinom-semisup and hhmm-tayal2009 are K <= 8 programs and answer
 * HHMM_ERR_UNSUPPORTED here, as do the IOHMMs, K <= 8 (hhmm_draw_stats and
 * hhmm_draw_stats_gauss take those), K > 32 and HHMM_DEVICE_SET.  hmm-multinom:
 * one group keeps two exchange slots and its emission table (fp64), the
 * table's counts and its K rows of xi (32-bit) in LDS, and one group must fit a
 * CU's 160 KiB:
 *   G * (16 + 12 * L + 4 * K) <= 163840 bytes
 * i.e. L <= 848 at K = 12 (G = 16) and L <= 417 at K = 25 (G = 32); a larger L
 * answers HHMM_ERR_UNSUPPORTED, before the device is looked at.
 *
 * The workspace is the forward checkpoints, one every 8 steps:
 *   ceil(T_max / 8) * K * P * 8 bytes.
 */
hhmm_status hhmm_draw_stats_large_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_draw_stats_large_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                         size_t workspace_bytes, void *stream);
hhmm_status hhmm_draw_stats_large(const hhmm_request *req, hhmm_estep_result *res);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_GIBBS_H */
