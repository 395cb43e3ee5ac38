/*
 * hhmm_stats.h -- host-side pieces shared by the "statistics per (series,
 * draw) pair" entries: the E-step and the expected draw statistics
 * (hhmm_estep.hip), the draw statistics of the discrete programs and of the
 * Gaussian hmm (hhmm_draw_stats.hip), the IOHMM E-step (hhmm_estep_io.hip), the
 * pointwise predictive densities (hhmm_pointwise.hip), the E-step at
 * 8 < K <= 32 (hhmm_estep_large.hip), the draw statistics there
 * (hhmm_draw_stats_large.hip) and the pointwise densities there
 * (hhmm_pointwise_large.hip) and PSIS-LOO / -LFO on top of both
 * (hhmm_psis.hip).  The
 * kernels differ; the argument checks, the DevArgs of a launch, the LDS fit,
 * the dispatch on K and the launch epilogue do not.  stats_check_tail belongs
 * to the eight entries that fill an hhmm_estep_result; the IOHMM E-step and the
 * pointwise densities have a result struct and a tail of their own.  Not part of the public ABI.
 */
#pragma once
#include <type_traits>

#include "hhmm_estep.h"
#include "hhmm_estep_io.h"
#include "hhmm_expect.h"
#include "hhmm_gibbs.h"
#include "hhmm_gibbs_gauss.h"
#include "hhmm_internal.h"
#include "hhmm_pointwise.h"
#include "hhmm_psis.h"

namespace hhmm {

/* Each of the thirteen entries gives the host path of hhmm_stats_api.cpp
 * (StatsEntry, stats_*) a check_* and a launch_*; what those share follows them.
 *
 * Batched E-step (hhmm_estep.hip): argument checks (no device needed), the
 * checkpoint workspace and the launch on `st` (device pointers). */
hhmm_status check_estep(const hhmm_request *r, const hhmm_estep_result *o);
size_t estep_workspace_bytes(int K, int Tmax, int64_t P);
hhmm_status launch_estep(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws, hipStream_t st);

/* Batched E-step at kMaxK < K <= kMaxKLarge (hhmm_estep_large.hip): the same
 * pair; the workspace is lk_ckpt_workspace_bytes. */
hhmm_status check_estep_large(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status launch_estep_large(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                               hipStream_t st);

/* Draw statistics (hhmm_draw_stats.hip): argument checks (no device needed)
 * and the launch on `st` (device pointers); the workspace is the E-step's. */
hhmm_status check_draw_stats(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status launch_draw_stats(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                              hipStream_t st);

/* Gaussian draw statistics (hhmm_draw_stats.hip, the same kernel template):
 * the same pair for hmm.stan; the workspace is the E-step's. */
hhmm_status check_draw_stats_gauss(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status launch_draw_stats_gauss(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                    hipStream_t st);

/* Draw statistics at kMaxK < K <= kMaxKLarge (hhmm_draw_stats_large.hip), hmm
 * and hmm-multinom: the same pair; the workspace is lk_ckpt_workspace_bytes. */
hhmm_status check_draw_stats_large(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status launch_draw_stats_large(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                    hipStream_t st);

/* Expected draw statistics (hhmm_estep.hip, the E-step's kernel template and
 * launch path): argument checks (no device needed) and the launch on `st`
 * (device pointers); the workspace is the E-step's. */
hhmm_status check_expected_stats(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status launch_expected_stats(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                  hipStream_t st);

/* The E-step and the expected statistics as a parallel scan over T
 * (hhmm_estep_scan.hip; the checks sit beside their sequential twins in
 * hhmm_estep.hip and share their scope and LDS fit): argument checks (no device
 * needed), the workspace of EstepScanLayout and the one launch of both entries
 * on `st` (device pointers).  estep_waves: the lane kernels' waves per
 * workgroup and its LDS (two tables per wave for the discrete programs, xi for
 * the Gaussian kernels at K >= 7); 0: one wave's tables do not fit. */
inline constexpr const char *kEstepScanAbove = "hhmm_estep_large takes hmm and hmm-multinom at 8 < K <= 32";
hhmm_status check_estep_scan(const hhmm_request *r, const hhmm_estep_result *o);
hhmm_status check_expected_stats_scan(const hhmm_request *r, const hhmm_estep_result *o);
int estep_waves(int model, int K, int L, size_t *lds);
size_t estep_scan_workspace_bytes(const hhmm_request *r, int64_t P);
hhmm_status launch_estep_scan(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                              hipStream_t st);

/* IOHMM E-step (hhmm_estep_io.hip): argument checks (no device needed) and the
 * launch on `st` (device pointers); its own result struct, no workspace. */
hhmm_status check_estep_io(const hhmm_request *r, const hhmm_estep_io_result *o);
hhmm_status launch_estep_io(const hhmm_request *r, const hhmm_estep_io_result *res, int64_t P, void *ws,
                            hipStream_t st);

/* Pointwise predictive densities (hhmm_pointwise.hip): argument checks (no
 * device needed), the tiles' partials (0 bytes while one workgroup covers a
 * series' draws) and the launch on `st` (device pointers); its own result
 * struct and tail. */
hhmm_status check_pointwise(const hhmm_request *r, const hhmm_pointwise_result *o);
size_t pointwise_workspace_bytes(const hhmm_request *r, int64_t P);
hhmm_status launch_pointwise(const hhmm_request *r, const hhmm_pointwise_result *res, int64_t P, void *ws,
                             hipStream_t st);

/* Pointwise predictive densities at kMaxK < K <= kMaxKLarge
 * (hhmm_pointwise_large.hip): the same three; the workspace holds l_t,
 * [P, T_max], where the caller gives no lp_t (P * T_max * 8 bytes whatever the
 * result holds: the size is a function of the request). */
hhmm_status check_pointwise_large(const hhmm_request *r, const hhmm_pointwise_result *o);
size_t pointwise_large_workspace_bytes(const hhmm_request *r, int64_t P);
hhmm_status launch_pointwise_large(const hhmm_request *r, const hhmm_pointwise_result *res, int64_t P, void *ws,
                                   hipStream_t st);

/* PSIS-LOO and PSIS-LFO (hhmm_psis.hip) at 1 <= K <= kMaxKLarge: one check (it
 * hands the sweep's own scope to check_pointwise or check_pointwise_large by
 * K); the workspace is the chosen sweep's, l_t where that sweep does not keep it
 * (K <= kMaxK) and, for LFO, the suffix sums; the launch is the sweep, the
 * suffix kernel (LFO) and the cell kernel on `st`. */
hhmm_status check_psis(const hhmm_request *r, const hhmm_psis_result *o);
size_t psis_loo_workspace_bytes(const hhmm_request *r, int64_t P);
size_t psis_lfo_workspace_bytes(const hhmm_request *r, int64_t P);
hhmm_status launch_psis_loo(const hhmm_request *r, const hhmm_psis_result *res, int64_t P, void *ws, hipStream_t st);
hhmm_status launch_psis_lfo(const hhmm_request *r, const hhmm_psis_result *res, int64_t P, void *ws, hipStream_t st);

/* Head of an entry's check_*, in this order: NULL request, ABI, model id, the
 * entry's scope (`scope` says which models it takes and where the others go),
 * K, HHMM_DEVICE_SET.  `entry`: the entry's name in messages.  k_lo..k_hi: the
 * K the entry's kernel takes (the lane-per-pair kernels' 1..kMaxK unless given);
 * `below`: the entry a message names for K < k_lo; `above`: where given, what a
 * message says of K > k_hi (the entry that takes it). */
inline hhmm_status stats_check_k(const char *entry, int K, int k_lo, int k_hi, const char *below = "hhmm_estep",
                                 const char *above = nullptr)
{
    if (K > k_hi) {
        if (above)
            set_error("%s: K = %d, the kernel supports K <= %d (%s)", entry, K, k_hi, above);
        else if (k_hi == kMaxK)
            set_error("%s: K = %d, the lane-per-pair kernel supports K <= %d", entry, K, kMaxK);
        else
            set_error("%s: K = %d, the state-parallel kernel supports %d <= K <= %d", entry, K, k_lo, k_hi);
        return HHMM_ERR_UNSUPPORTED;
    }
    if (k_lo > 1 && K < k_lo) {
        set_error("%s: K = %d, the state-parallel kernel supports %d <= K <= %d (%s takes K <= %d)", entry, K, k_lo,
                  k_hi, below, k_lo - 1);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

inline hhmm_status stats_check_head(const char *entry, const hhmm_request *r, bool (*model_ok)(int), const char *scope,
                                    int k_lo = 1, int k_hi = kMaxK, const char *below = "hhmm_estep",
                                    const char *above = nullptr)
{
    if (!r) {
        set_error("%s: request must be non-NULL", entry);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->abi_version != HHMM_ABI_VERSION) {
        set_error("%s: abi_version %u != %u", entry, r->abi_version, HHMM_ABI_VERSION);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->model < 1 || r->model > 9) {
        set_error("%s: unknown model id %d", entry, r->model);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (!model_ok(r->model)) {
        set_error("%s: model %d is not supported (%s)", entry, r->model, scope);
        return HHMM_ERR_UNSUPPORTED;
    }
    if (stats_check_k(entry, r->data.K, k_lo, k_hi, below, above) != HHMM_OK)
        return HHMM_ERR_UNSUPPORTED;
    if (r->device == HHMM_DEVICE_SET) {
        set_error("%s: HHMM_DEVICE_SET is not supported (one device per call)", entry);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

/* Tail of an entry's check_*, after its LDS-fit test: NULL result, the outputs
 * of the model's emission family, and the uniforms where the entry reads them. */
inline hhmm_status stats_check_tail(const char *entry, const hhmm_request *r, const hhmm_estep_result *o, bool reads_u)
{
    if (!o) {
        set_error("%s: result must be non-NULL", entry);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const bool gauss = r->model == HHMM_MODEL_HMM_GAUSS;
    if (!o->loglik || !o->n_1k || !o->xi_ij || (gauss ? !o->w_k || !o->s1_k || !o->s2_k : !o->c_kl)) {
        set_error("%s: loglik, n_1k, xi_ij and %s must be non-NULL", entry, gauss ? "w_k, s1_k and s2_k" : "c_kl");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (reads_u && !r->ffbs_u) {
        set_error("%s: ffbs_u (the [P, T_max] uniforms of the draw) must be non-NULL", entry);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return HHMM_OK;
}

/* The DevArgs fields every entry takes from the request; the data and draw
 * arrays of its own model family are explicit lines at the call site. */
inline DevArgs stats_dev_args(const hhmm_request *r, int64_t P, void *ws)
{
    DevArgs a{};
    a.P = P;
    a.N = r->data.n_series;
    a.S = r->draws.n_draws;
    a.pairing = r->pairing;
    a.model = r->model;
    a.K = r->data.K;
    a.L = r->data.L;
    a.Tmax = r->data.T_max;
    a.Tout = r->data.T_max;
    a.T = r->data.T;
    a.p_1k = r->draws.p_1k;
    a.A_ij = r->draws.A_ij;
    a.ckpt = (double *)ws;
    return a;
}

/* Threads per workgroup of a state-parallel statistics kernel (a group of G
 * lanes per pair, `per` LDS bytes per group beside `fixed` bytes per
 * workgroup), and the workgroup's LDS: kBlock halved down to one group until
 * the LDS fits (0: one group does not).  Whole workgroups share a CU's LDS, so
 * among the sizes of at least one wave the one that lets the most waves (up to
 * two per SIMD) be resident is taken, the larger on a tie: with the large-K
 * E-step's xi rows in LDS 256 threads would hold a CU alone (K = 23, L = 9:
 * 86 KiB, four waves; 64 threads: 21.5 KiB, seven). */
inline int group_threads(size_t per, int G, size_t *lds, size_t fixed = 0)
{
    int threads = kBlock;
    while (threads > G && fixed + (size_t)(threads / G) * per > kLdsLimit)
        threads /= 2;
    size_t best = 0;
    for (int t = threads; t >= 64; t /= 2) {
        const size_t waves = kLdsLimit / (fixed + (size_t)(t / G) * per) * (size_t)(t / 64);
        if ((waves < 8 ? waves : 8) > best) {
            best = waves < 8 ? waves : 8;
            threads = t;
        }
    }
    *lds = fixed + (size_t)(threads / G) * per;
    return *lds > kLdsLimit ? 0 : threads;
}

/* ---- the state-parallel entries: hmm and hmm-multinom at kMaxK < K <=
 * kMaxKLarge, a group of lk_G(K) lanes per pair (hhmm_large.h) ---- */

/* What an entry says of itself, once: check_*, launch_* and its StatsEntry row read it. */
struct LkScope {
    const char *name;   /* in messages */
    bool reads_u;       /* ffbs_u is an input */
    const char *others; /* where the other models go (stats_check_head's `scope`) */
    const char *below;  /* the entry that takes K <= kMaxK */
    int k_lo = kMaxK + 1, k_hi = kMaxKLarge;
};
inline constexpr LkScope kEstepLargeScope = {
    "large-K E-step", false, "hmm and hmm-multinom only; the other programs have no state-parallel E-step",
    "hhmm_estep"};
inline constexpr LkScope kDrawStatsLargeScope = {
    "large-K draw statistics", true,
    "hmm and hmm-multinom only; hmm-multinom-semisup and hhmm-tayal2009 are K <= 8 programs (hhmm_draw_stats)",
    "hhmm_draw_stats / hhmm_draw_stats_gauss"};
inline constexpr LkScope kPointwiseLargeScope = {
    "large-K pointwise", false,
    "hmm and hmm-multinom only; the coded step weights of the semisup, Tayal and IOHMM programs are masked or "
    "factorised, not a predictive density",
    "hhmm_pointwise"};

inline bool lk_stats_model(int m) { return m == HHMM_MODEL_HMM_GAUSS || m == HHMM_MODEL_HMM_MULTINOM; }

/* The forward checkpoints every kLChunk steps, [chunks][K][P] doubles: the
 * workspace of the E-step and of the draw statistics (hhmm_estep_large.hip). */
size_t lk_ckpt_workspace_bytes(const hhmm_request *r, int64_t P);

/* The DevArgs of a launch: stats_dev_args, the data and draw arrays of the two
 * models, the uniforms where the entry reads them; L = 0 for the Gaussian hmm
 * (no tables: lk_setup lays the LDS out by L). */
inline hhmm_status lk_stats_dev_args(const LkScope &sc, const hhmm_request *r, int64_t P, void *ws, DevArgs *a)
{
    *a = stats_dev_args(r, P, ws);
    a->x = r->data.x_int;
    a->xr = r->data.x_real;
    a->phi_k = r->draws.phi_k;
    a->mu_k = r->draws.mu_k;
    a->sigma_k = r->draws.sigma_k;
    if (sc.reads_u)
        a->ffbs_u = r->ffbs_u;
    if (a->model == HHMM_MODEL_HMM_GAUSS)
        a->L = 0;
    if (a->K < sc.k_lo || a->K > sc.k_hi) {
        set_error("%s: K = %d outside %d..%d", sc.name, a->K, sc.k_lo, sc.k_hi);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

/* The outputs of an hhmm_estep_result as a kernel argument (the E-step and the draw statistics). */
struct LkStatsOut {
    double *loglik, *n1, *xi, *c, *w, *s1, *s2;
    int32_t *status;
};
inline LkStatsOut lk_stats_out(const hhmm_estep_result *res)
{
    return {res->loglik, res->n_1k, res->xi_ij, res->c_kl, res->w_k, res->s1_k, res->s2_k, res->pair_status};
}

/* Workgroup, its LDS and the grid over P pairs by group_threads' rule, from the
 * entry's `per` LDS bytes per G-lane group and `fixed` per workgroup.  false:
 * one group does not fit; the entry words the refusal. */
struct LkGeom {
    dim3 grid, block;
    size_t lds;
};
inline bool lk_geometry(size_t per, size_t fixed, int G, int64_t P, LkGeom *g)
{
    const int threads = group_threads(per, G, &g->lds, fixed);
    if (threads < 1)
        return false;
    const int gpb = threads / G;
    g->grid = dim3((unsigned)((P + gpb - 1) / gpb));
    g->block = dim3(threads);
    return true;
}

/* waves_that_fit and launch_status: hhmm_internal.h (the HMM family's launchers use them too).
 *
 * f(std::integral_constant<int, K>{}) for K in 1..kMaxK; false: K outside. */
template <class F>
bool dispatch_k(int K, F &&f)
{
    switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
    }
}

} // namespace hhmm
