/*
 * hhmm_draw_stats_large.hip -- gfx950 kernel of the draw statistics at
 * 8 < K <= 32 (include/hhmm_gibbs.h, hhmm_draw_stats_large): per (series, draw)
 * pair one FFBS path z, reduced to what a conjugate parameter update needs --
 * z_1, the transitions, and the (state, symbol) pairs (hmm-multinom) or per
 * state the count, the sum and the sum of squares of the observations it owns
 * (the Gaussian hmm).  Nothing is written per step.
 *
 * A GROUP of G lanes owns one pair, lane j state j (the layout, the instances
 * and the helpers of lk_ffbs_kernel, hhmm_large.h): lane j keeps column j and
 * row j of A in registers, the group exchanges its vector through its LDS slot.
 *   forward   lk_ffbs_kernel's filter, operation for operation (lkf_emit,
 *             lkf_step, the power-of-two renormalisation by the frexp exponent
 *             of the group max every step; hmm: the Q2 first step, the det exp
 *             on the workgroup's LDS copy of the 2^(j/128) table), a checkpoint
 *             every kLChunk steps in the [rows][K][P] layout: the same bits, so
 *             the same path as hhmm_run's z_ffbs.  Unlike lk_ffbs_kernel it
 *             keeps the exponents (and for hmm the per-step lpdf maxima and the
 *             Q2 term) and returns loglik from this one filter.
 *   backward  chunk by chunk from the end: the filter over the chunk is
 *             recomputed from its checkpoint, z_t drawn by ffbs_cat_rt from
 *             u[p, t], the statistics taken.  The chunk's uniforms and the next
 *             checkpoint are loaded ahead of the recompute.
 * Accumulators (z_t is a run-time index):
 *     n_1k    the lane that is z_1
 *     xi_ij   lane z_{t-1} owns row z_{t-1}: one count at column z_t per step,
 *             in a per-pair LDS block [K][G] of 32-bit counts.  KM
 *             compare-and-add registers instead cost every instance registers
 *             and the two KM = 24 instances their second wave per SIMD
 *             (DESIGN.md §3.12b has the compiler's figures), so all six
 *             instances keep the block
 *     c_kl    lane z_t adds one at [(x_t - 1) * G + z_t] of a per-pair [L][G]
 *             32-bit table beside the phi table
 *     w, s1, s2   three registers on lane k, in the order of the backward sweep
 *             (t = T .. 2), then x_1 once for every state; s2 adds the rounded
 *             product
 * A count is at most T_max < 2^31 and is stored as a double.  No floating-point
 * atomics and no atomics at all: a column of either table belongs to one lane.
 * LDS per group: (2 + L) G doubles and L G words (hmm-multinom), 2 G doubles
 * beside the workgroup's 2 KiB table (hmm), and K G words of xi rows.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_gibbs.h"
#include "hhmm_gibbs_gauss.h"
#include "hhmm_large.h"
#include "hhmm_stats.h"

namespace hhmm {

/* the det exp's 2^(j/128) table, copied to LDS once per workgroup (hmm) */
constexpr size_t kDslTabBytes = 128 * sizeof(hhmm_exp2_entry);

/* lkf_emit (hhmm_large.h) with the group max it subtracts handed back: the same
 * operations on the same values, so the same bits. */
template <int MODEL, int G, int KM>
__device__ __forceinline__ double dsl_emit(const LkLane<MODEL, G, KM> &ln, int x, double xr, double &m)
{
    if constexpr (LkTraits<MODEL>::kGauss) {
        const double lp = ln.on ? lk_lpdf<MODEL, G, KM>(ln, xr) : dev_ninf();
        m = grp_max<G>(lp);
        return ln.on ? hhmm_det_exp_tab(lp - m, ln.etab) : 0.0;
    } else {
        m = 0.0;
        return lkf_emit<MODEL, G, KM>(ln, x, xr);
    }
}

template <int MODEL, int G, int KM>
__global__ void __launch_bounds__(kBlock) draw_stats_large_kernel(const DevArgs a, const LkStatsOut o)
{
    HIP_DYNAMIC_SHARED(double, lds)
    constexpr bool GAUSS = LkTraits<MODEL>::kGauss;
    /* groups past the last pair redo pair P - 1 (identical values, benign
     * duplicate stores): every lane stays in the group reductions */
    const int64_t q = lk_group<G>(a.P);
    LkLane<MODEL, G, KM> ln;
    lk_setup<MODEL, G, KM>(ln, a, lds, false, q);
    const int K = ln.K, L = GAUSS ? 0 : ln.L, Tp = ln.Tp;
    const bool st = ln.on; /* the lane that stores state j's outputs */
    /* LDS after lk_setup's [groups][2][G] slots and [groups][L][G] phi tables:
     * hmm: the det exp's table; then [groups][L][G] symbol counts and
     * [groups][K][G] xi rows, 32-bit.  A lane touches its own column of
     * either only, so it needs no barrier after zeroing it. */
    const int g = threadIdx.x / G, gpb = blockDim.x / G;
    double *const tail = lds + (size_t)gpb * (2 + L) * G;
    uint32_t *words = reinterpret_cast<uint32_t *>(tail);
    if constexpr (GAUSS) {
        hhmm_exp2_entry *t = reinterpret_cast<hhmm_exp2_entry *>(tail);
        for (int i = threadIdx.x; i < 128; i += blockDim.x)
            t[i] = hhmm_exp2_tab[i];
        ln.etab = t;
        words = reinterpret_cast<uint32_t *>(t + 128);
    }
    uint32_t *const cnt = words + (size_t)g * L * G + ln.j;
    uint32_t *const xs = words + (size_t)gpb * L * G + (size_t)g * K * G + ln.j;
    for (int l = 0; l < L; ++l)
        cnt[l * G] = 0u;
    for (int j = 0; j < K; ++j)
        xs[j * G] = 0u;
    if constexpr (GAUSS)
        __syncthreads();

    auto ckpt = [&](int c) -> double & { return a.ckpt[q + a.P * ((int64_t)c * K + (ln.on ? ln.j : 0))]; };
    bool xbad = false; /* the data check rides on the forward sweep's loads */
    auto block = [&](int b) { return lk_block_checked<MODEL, G, KM>(ln, a, b, L, Tp, xbad); };
    double w[KM];
    int slot = 0;

    /* ---- forward: lk_ffbs_kernel's filter, the exponents and shifts kept ---- */
    LkObs<MODEL, G> bcur = block(0), bnxt = block(1);
    double f, lsc = 0.0;
    int ex = 0;
    {
        int x;
        double xr;
        lk_get<MODEL, G>(bcur, 0, x, xr);
        if constexpr (GAUSS) {
            /* log(p_1k) + SUM_k normal_lpdf(x[1] | mu_k, sigma_k): f_1 = p_1k (hmm.stan:30, Q2) */
            const double tk = ln.on ? lk_lpdf<MODEL, G, KM>(ln, xr) : 0.0;
            lsc += grp_sum<G>(tk);
            f = ln.on ? ln.pj : 0.0;
        } else {
            const double e = lkf_emit<MODEL, G, KM>(ln, x, xr);
            f = ln.on ? ln.pj * e : 0.0;
        }
        f = grp_renorm<G>(f, ex);
    }
    if (st)
        ckpt(0) = f;
    for (int t = 1; t < Tp; ++t) {
        const int u = t % G;
        if (u == 0) { /* group-uniform: next block of observations, prefetch the one after */
            bcur = bnxt;
            bnxt = block(t / G + 1);
        }
        int x;
        double xr, m;
        lk_get<MODEL, G>(bcur, u, x, xr);
        const double e = dsl_emit<MODEL, G, KM>(ln, x, xr, m);
        grp_exchange<G, KM>(ln.xch, slot, ln.j, f, w);
        slot ^= 1;
        lsc += m;
        f = grp_renorm<G>(lkf_step<MODEL, G, KM>(ln, w, e), ex);
        if (t % kLChunk == 0 && st)
            ckpt(t / kLChunk) = f;
    }
    const double ll = log(grp_sum<G>(f)) + (lsc + kLn2 * ex); /* the same bits on every lane of the group */

    /* ---- backward sampling, chunk by chunk from the end ---- */
    uint32_t gw = 0u;
    double n1 = 0.0, gs1 = 0.0, gs2 = 0.0, x0 = 0.0;
    bool bad = !__builtin_isfinite(ll);
    constexpr int CPB = G / kLChunk; /* chunks per observation block */
    const int nck = (Tp + kLChunk - 1) / kLChunk;
    int cb = (nck - 1) / CPB;
    LkObs<MODEL, G> ob = lk_block<MODEL, G, KM>(ln, a, cb), obp = lk_block<MODEL, G, KM>(ln, a, cb - 1);
    double ck = ckpt(nck - 1), ckn = ckpt(max(nck - 2, 0));
    int z = -2; /* z_{t+1}, 0-based; -2: not drawn yet (z_T comes from f_T alone), -1: undefined */
    for (int c = nck - 1; c >= 0; --c) {
        if (c / CPB != cb) { /* group-uniform: step back one observation block */
            cb = c / CPB;
            ob = obp;
            obp = lk_block<MODEL, G, KM>(ln, a, cb - 1);
        }
        const int t0 = c * kLChunk, ub = t0 % G;
        /* the chunk's uniforms (one address per group) and observations */
        double uu[kLChunk], xv[kLChunk];
        int sym[kLChunk];
#pragma unroll
        for (int u = 0; u < kLChunk; ++u) {
            uu[u] = a.ffbs_u[ln.p + a.P * (int64_t)min(t0 + u, a.Tmax - 1)];
            lk_get_var<MODEL, G>(ob, ub + u, sym[u], xv[u]);
        }
        /* the filter over the chunk from its checkpoint (the forward's operations: the same bits) */
        double fb[kLChunk];
        fb[0] = ln.on ? ck : 0.0;
        ck = ckn;
        ckn = ckpt(max(c - 2, 0));
#pragma unroll
        for (int u = 1; u < kLChunk; ++u) {
            fb[u] = 0.0;
            if (t0 + u < Tp) { /* group-uniform */
                double m;
                int exb = 0;
                const double e = dsl_emit<MODEL, G, KM>(ln, sym[u], xv[u], m);
                grp_exchange<G, KM>(ln.xch, slot, ln.j, fb[u - 1], w);
                slot ^= 1;
                fb[u] = grp_renorm<G>(lkf_step<MODEL, G, KM>(ln, w, e), exb);
            }
        }
        /* draws of steps t0 + kLChunk - 1 .. t0 */
#pragma unroll
        for (int u = kLChunk - 1; u >= 0; --u) {
            const int t = t0 + u;
            if (t >= Tp) /* group-uniform */
                continue;
            double wt = fb[u];
            if (z >= 0) { /* weight f_t(i) A(i, z_{t+1}): lane i's row, entry z */
                double az = ln.row[0];
#pragma unroll
                for (int k = 1; k < KM; ++k)
                    az = (z == k) ? ln.row[k] : az;
                wt = ln.on ? wt * az : 0.0;
            }
            grp_exchange<G, KM>(ln.xch, slot, ln.j, wt, w);
            slot ^= 1;
            const int zt = (z == -1) ? -1 : ffbs_cat_rt<KM>(w, K, uu[u]);
            bad |= zt < 0;
            const bool mine = ln.j == zt; /* no lane when the draw is undefined */
            if constexpr (GAUSS) {
                if (t == 0) { /* Q2: x_1 counts once for every state */
                    x0 = xv[u];
                } else if (mine) {
                    gw += 1u;
                    gs1 = gs1 + xv[u];
                    gs2 = gs2 + xv[u] * xv[u];
                }
            } else {
                if (mine)
                    cnt[(min(max(sym[u], 1), L) - 1) * G] += 1u;
            }
            if (z >= 0 && mine) /* the transition z_t -> z_{t+1}: row z_t, column z_{t+1} */
                xs[z * G] += 1u;
            if (t == 0)
                n1 = mine ? 1.0 : 0.0;
            z = zt;
        }
    }

    /* ---- the [P, ...] outputs ---- */
    const double nanv = dev_nan();
    const int64_t p = ln.p;
    if (st) {
        o.n1[p + a.P * (int64_t)ln.j] = bad ? nanv : n1;
        for (int j = 0; j < K; ++j)
            o.xi[p + a.P * ((int64_t)ln.j + (int64_t)K * j)] = bad ? nanv : (double)xs[j * G];
        if constexpr (GAUSS) {
            o.w[p + a.P * (int64_t)ln.j] = bad ? nanv : 1.0 + (double)gw;
            o.s1[p + a.P * (int64_t)ln.j] = bad ? nanv : x0 + gs1;
            o.s2[p + a.P * (int64_t)ln.j] = bad ? nanv : x0 * x0 + gs2;
        } else {
            for (int l = 0; l < L; ++l)
                o.c[p + a.P * ((int64_t)ln.j + (int64_t)K * l)] = bad ? nanv : (double)cnt[l * G];
        }
    }
    /* any lane of the group saw a symbol outside 1..L (every lane of the wave takes part) */
    const unsigned long long hit = __ballot(xbad);
    const unsigned long long own = ((1ull << G) - 1) << ((threadIdx.x & 63) & ~(G - 1));
    if (ln.j == 0) {
        o.loglik[p] = ll;
        if (o.status) {
            bool inv = (hit & own) != 0;
            if (a.T)
                inv |= a.T[ln.n] < 1 || a.T[ln.n] > a.Tmax;
            o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
        }
    }
}

/* ---- host side ---- */

/* LDS bytes of one group: two exchange slots and the xi rows (32-bit);
 * hmm-multinom: the phi table (fp64) and its count table (32-bit) too, i.e.
 * G * (16 + 12 L + 4 K). */
static size_t dsl_group_lds(int model, int K, int L)
{
    const size_t G = (size_t)lk_G(K), tabs = model == HHMM_MODEL_HMM_GAUSS ? 0 : (size_t)L;
    return (2 + tabs) * G * sizeof(double) + (tabs + (size_t)K) * G * sizeof(uint32_t);
}

/* lk_geometry (hhmm_stats.h) of the groups' LDS beside the workgroup's det-exp table for hmm */
static bool dsl_geometry(int model, int K, int L, int64_t P, LkGeom *g)
{
    const size_t tab = model == HHMM_MODEL_HMM_GAUSS ? kDslTabBytes : 0;
    return lk_geometry(dsl_group_lds(model, K, L), tab, lk_G(K), P, g);
}

hhmm_status check_draw_stats_large(const hhmm_request *r, const hhmm_estep_result *o)
{
    const LkScope &sc = kDrawStatsLargeScope;
    const hhmm_status s = stats_check_head(sc.name, r, lk_stats_model, sc.others, sc.k_lo, sc.k_hi, sc.below);
    if (s != HHMM_OK)
        return s;
    const int K = r->data.K, L = r->data.L, G = lk_G(K);
    LkGeom g;
    if (r->model == HHMM_MODEL_HMM_MULTINOM && L >= 1 && !dsl_geometry(r->model, K, L, 1, &g)) {
        set_error("%s: L = %d: %d * (16 + 12 * L + 4 * K) = %zu > %zu bytes: the emission table, its count table and "
                  "the xi rows of one %d-lane group do not fit in LDS",
                  sc.name, L, G, dsl_group_lds(r->model, K, L), kLdsLimit, G);
        return HHMM_ERR_UNSUPPORTED;
    }
    return stats_check_tail(sc.name, r, o, sc.reads_u);
}

hhmm_status launch_draw_stats_large(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                    hipStream_t st)
{
    const LkScope &sc = kDrawStatsLargeScope;
    DevArgs a;
    const hhmm_status s = lk_stats_dev_args(sc, r, P, ws, &a);
    if (s != HHMM_OK)
        return s;
    LkGeom g;
    if (!dsl_geometry(a.model, a.K, a.L, P, &g)) {
        set_error("%s: the tables of L = %d do not fit in LDS", sc.name, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const LkStatsOut o = lk_stats_out(res);
    dispatch_lk_model(a.model, a.K, [&](auto M, auto G, auto KM) { /* the instances of lk_ffbs_kernel (run_large) */
        hipLaunchKernelGGL((draw_stats_large_kernel<M, G, KM>), g.grid, g.block, g.lds, st, a, o);
    });
    return launch_status("draw_stats_large_kernel");
}

} // namespace hhmm
