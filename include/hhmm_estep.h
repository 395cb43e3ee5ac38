/*
 * hhmm_estep.h -- batched E-step of libhhmm.so: the expected sufficient
 * statistics of an HMM, summed over the steps of every (series, draw) pair.
 *
 * Every output of include/hhmm.h is per step ([P, T, K] at the least).  A
 * caller that improves a set of parameters instead of inspecting them needs
 * the sums over t, and the pairwise posterior that no per-step output carries:
 *
 *   loglik [P]        l, the model-block log-likelihood (HHMM_OUT_LOGLIK)
 *   n_1k   [P, K]     gamma_1(k)
 *   xi_ij  [P, K, K]  sum_{t=2..T} P(z_{t-1} = i, z_t = j | x) at p + P*(i + K*j);
 *                     all zero at T = 1
 *   c_kl   [P, K, L]  hmm-multinom: sum_{t=1..T} gamma_t(k) [x_t = l]
 *   w_k, s1_k, s2_k [P, K]  hmm: 1 + sum_{t>=2} gamma_t(k),
 *                     x_1 + sum_{t>=2} gamma_t(k) x_t, x_1^2 + sum_{t>=2} gamma_t(k) x_t^2
 *
 * gamma and xi are the posteriors under the CODED likelihood of the Stan
 * program.  hmm.stan:30 adds sum_k normal_lpdf(x_1 | mu_k, sigma_k) to every
 * state at t = 1 (quirk Q2 of SURVEY.md App. A), so x_1 enters the Gaussian
 * statistics with weight 1 for every state, not gamma_1(k); with that weight
 * the usual formulas are the exact score of l (Fisher's identity):
 *   dl/dmu_k    = (s1 - mu w) / sigma^2
 *   dl/dsigma_k = -w / sigma + (s2 - 2 mu s1 + mu^2 w) / sigma^3
 *   dl/dp_1k[k] = n_1k / p_1k    dl/dA_ij = xi_ij / A_ij    dl/dphi_kl = c_kl / phi_kl
 *
 * All outputs are fp64, pair-fastest ([P, ...] at p + P*(...)), tolerance 1e-9
 * relative to max(1, |value|).  When l is -inf or NaN (an impossible
 * observation, NaN draws) every statistic of the pair is NaN and pair_status
 * stays HHMM_PAIR_OK.
 *
 * Scope: hmm and hmm-multinom at 1 <= K <= 8, every pairing, ragged T.  Other
 * models, K > 8, HHMM_DEVICE_SET and an emission table with L * ceil(K / 2) >
 * 80 (two tables of one wave do not fit a CU's LDS) answer HHMM_ERR_UNSUPPORTED.
 * The request is the hhmm_request of hhmm.h; outputs, ffbs_u, hat_rand and the
 * scan flags are ignored (hhmm_estep is sequential in T per pair; for few, long
 * series the hhmm_estep_scan entries below run the same E-step in parallel over T).
 * hmm and hmm-multinom at 8 < K <= 32 go to the hhmm_estep_large entries below.
 */
#ifndef HHMM_ESTEP_H
#define HHMM_ESTEP_H

#include "hhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-allocated outputs.  The emission pointers of the other model may be
 * NULL (c_kl for hmm; w_k, s1_k, s2_k for hmm-multinom); pair_status is optional. */
typedef struct hhmm_estep_result {
    double  *loglik;           /* [P] */
    double  *n_1k;             /* [P, K] */
    double  *xi_ij;            /* [P, K, K] */
    double  *c_kl;             /* [P, K, L]  hmm-multinom */
    double  *w_k;              /* [P, K]     hmm */
    double  *s1_k;             /* [P, K]     hmm */
    double  *s2_k;             /* [P, K]     hmm */
    int32_t *pair_status;      /* [P] optional */
} hhmm_estep_result;

/* Bytes of device workspace hhmm_estep_device needs (the forward checkpoints). */
hhmm_status hhmm_estep_workspace_size(const hhmm_request *req, size_t *bytes);

/* Device-resident entry: every pointer in req / res is a device pointer on the
 * current HIP device; enqueues on `stream` and returns without synchronising.
 * A pair whose series breaks a data-block bound (x outside 1..L, T[n] outside
 * 1..T_max) is flagged HHMM_PAIR_INVALID_DATA when pair_status is given (its
 * statistics are unspecified; the table is never indexed with the bad symbol);
 * every other pair is unaffected. */
hhmm_status hhmm_estep_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Host-pointer entry: validates the data block as hhmm_run does (a violation
 * rejects the request), uploads, runs on req->device (-1 = current), downloads
 * and synchronises. */
hhmm_status hhmm_estep(const hhmm_request *req, hhmm_estep_result *res);

/* The E-step at 8 < K <= 32 on the state-parallel groups (a group of 16 or 32
 * lanes owns a pair, lane j state j): three entries with the signatures of the
 * three above, filling the same hhmm_estep_result.
 *
 *   Models    hmm and hmm-multinom only.
 *   K         9..32.  K <= 8 answers HHMM_ERR_UNSUPPORTED and names hhmm_estep;
 *             K > 32 answers HHMM_ERR_UNSUPPORTED; both messages contain
 *             "K = <value>".
 *   Outputs   exactly those of hhmm_estep, with the same definitions: loglik,
 *             n_1k = gamma_1, xi_ij = sum_{t>=2} P(z_{t-1} = i, z_t = j | x),
 *             c_kl (hmm-multinom) or w_k, s1_k, s2_k (hmm; x_1 counts with
 *             weight 1 for every state, Q2: w_k = 1 + sum_{t>=2} gamma_t(k)),
 *             all pair-fastest [P, ...].  A zero in A_ij gives an exact zero in
 *             xi_ij.
 *   Request   every pairing, ragged T; sequential in T per pair: outputs,
 *             ffbs_u, hat_rand and the scan flags are ignored.
 *   NaN       a pair with a non-finite loglik, or with a step whose normaliser
 *             is 0 or non-finite, gets NaN statistics; pair_status stays
 *             HHMM_PAIR_OK.
 *   Data      (device entry) a series whose symbols leave 1..L or whose T[n]
 *             leaves 1..T_max sets pair_status = HHMM_PAIR_INVALID_DATA for its
 *             pairs; the check runs on the observations as they are read, and
 *             every emission lookup clamps its symbol.  The host entry rejects
 *             such a request like hhmm_estep.
 *   Device    HHMM_DEVICE_SET is unsupported, as for the other statistics
 *             entries.
 *   LDS       hmm-multinom keeps two [L][G] tables per group; an L whose tables
 *             of one group exceed 160 KiB answers HHMM_ERR_UNSUPPORTED naming L.
 *   Workspace the forward checkpoints, one K-vector per pair every 8 steps in
 *             the [rows][K][P] layout: ceil(T_max / 8) * K * P * 8 bytes.
 *   Bits      no floating-point atomics: both entries and every run give the
 *             same bits. */
hhmm_status hhmm_estep_large_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_estep_large_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                    size_t workspace_bytes, void *stream);
hhmm_status hhmm_estep_large(const hhmm_request *req, hhmm_estep_result *res);

/* The E-step as a parallel scan over T, for one or a few long series (an EM
 * fit of one long series from a handful of starts): three entries with the
 * signatures of the first three, filling the same hhmm_estep_result with the
 * same definitions, NaN rule and invalid-data rule as hhmm_estep.
 *
 *   Schedule  every series is cut into T-chunks of `cl` steps.  Phase 1 forms
 *             each chunk's forward product, phase 2 turns the products into the
 *             filter entering and the beta leaving every chunk (and loglik),
 *             phase 3 gives one lane to one (pair, chunk) for the two sweeps of
 *             hhmm_estep over that chunk, and a reduction adds the chunks'
 *             statistics in chunk order.
 *   Flags     HHMM_FLAG_SCAN_CHUNK_LOG2(n) sets cl = 2^n, rounded down to a
 *             multiple of the checkpoint interval C (8 steps at K <= 4, else 4)
 *             and at least C; left at 0 the library starts from 4 C and doubles
 *             cl until P * ceil(T_max / cl) <= 262144.  These entries always
 *             scan: HHMM_FLAG_SCAN_FORCE is implied, HHMM_FLAG_SCAN_OFF answers
 *             HHMM_ERR_UNSUPPORTED, as does a request whose (pair, chunk) lanes
 *             (a pair's chunks rounded up to a multiple of 64) reach 2^29.
 *   Scope     hmm and hmm-multinom, 1 <= K <= 8, every pairing, ragged T.  K > 8
 *             answers HHMM_ERR_UNSUPPORTED with a message that contains
 *             "K = <value>" and names hhmm_estep_large; other models,
 *             HHMM_DEVICE_SET and L * ceil(K / 2) > 80 as for hhmm_estep.
 *   Accuracy  1e-9 relative to max(1, |value|) like hhmm_estep; not its bits
 *             (the sums over t are associated by chunk).
 *   Bits      no floating-point atomics: both entries and every run give the
 *             same bits.
 *   Workspace with nc = ceil(T_max / cl), ncw = nc rounded up to a multiple of
 *             64 and ns = K + K^2 + K L (hmm: K + K^2 + 3 K) statistics, these
 *             fp64 regions in this order, each rounded up to a multiple of 256
 *             bytes, plus 256 bytes (the regions start at the first 256-byte
 *             boundary of the workspace):
 *               chunk products        nc K^2 P       their exponents    3 nc P
 *               entering filters      nc K P         their log scales   nc P
 *               leaving betas         nc K P         their log scales   nc P
 *               in-chunk checkpoints  (cl / C) K P ncw
 *               partials              P (ncw / 64) (ns + 5)
 *               each pair's A         P K^2
 * hhmm_estep_scan_plan (no device needed) returns the schedule hhmm_amd's
 * schedule="auto" follows for this request: chunk_len = cl and n_chunks = nc of
 * the scan when P < 4096 and T_max >= 8192 (or HHMM_FLAG_SCAN_FORCE is set)
 * and the model and K are in the scope of hhmm_estep_scan or
 * hhmm_expected_stats_scan; 0 and 0 for the sequential entry. */
hhmm_status hhmm_estep_scan_workspace_size(const hhmm_request *req, size_t *bytes);
hhmm_status hhmm_estep_scan_device(const hhmm_request *req, hhmm_estep_result *res, void *workspace,
                                   size_t workspace_bytes, void *stream);
hhmm_status hhmm_estep_scan(const hhmm_request *req, hhmm_estep_result *res);
hhmm_status hhmm_estep_scan_plan(const hhmm_request *req, int32_t *chunk_len, int32_t *n_chunks);

#ifdef __cplusplus
}
#endif

#endif /* HHMM_ESTEP_H */
