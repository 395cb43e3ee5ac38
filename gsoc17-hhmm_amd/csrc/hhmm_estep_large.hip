/*
 * hhmm_estep_large.hip -- gfx950 kernel of the batched E-step at 8 < K <= 32
 * (include/hhmm_estep.h, hhmm_estep_large): per (series, draw) pair the
 * expected sufficient statistics summed over the steps -- gamma_1, the pairwise
 * posterior sum xi_ij and the emission sums -- for hmm and hmm-multinom.
 * Nothing is written per step.
 *
 * A GROUP of G lanes owns one pair, lane j state j (the layout, the helpers and
 * the arithmetic of lk_fb_kernel, hhmm_large.h): lane j keeps column j and row
 * j of A in registers, the group exchanges its vector through its LDS slot.
 *   forward   lk_fb_kernel's sweep: the scaled linear-space filter, the Q2
 *             first step for hmm, a renormalisation every kLRenorm steps (every
 *             step in a dense wave), a checkpoint every kLChunk steps, loglik.
 *   backward  chunk by chunk from the end: alpha over the chunk is recomputed
 *             from its checkpoint, beta is carried.  The transition into step
 *             t >= 2, with b_t(j) = e_t(j) beta_t(j) on lane j:
 *                 w             = b_t on every lane (one exchange)
 *                 beta_{t-1}(i) = sum_j A(i,j) w[j]          (lane i, row i)
 *                 Z             = group sum of alpha_{t-1}(i) beta_{t-1}(i)
 *                 acc_i[j]     += (alpha_{t-1}(i) / Z) w[j]  (lane i owns row i of xi)
 *             so xi takes KM FMAs on the vector the beta step exchanged and no
 *             exchange of its own; its constant factor A(i,j) is applied once,
 *             at the store (a zero in A stays an exact zero).  Dividing by Z
 *             cancels every power-of-two scale of alpha and beta.  The
 *             transition into the first step of a chunk takes alpha of the
 *             chunk before it, so it is done when that chunk has been
 *             recomputed.  gamma_t(j) = alpha_t(j) beta_t(j) over their group
 *             sum, from the lane's own values (the kGammaDirect rule where the
 *             sum is tiny).  A step whose Z or gamma sum is not in (0, inf), or a
 *             non-finite loglik, makes the pair's statistics NaN.
 * Accumulators: row i of xi in KM registers of lane i, or in a per-pair LDS
 * block [K][G] (estep_large_xi_lds, per instance); the Gaussian sums in three
 * registers per lane; c_kl in a second per-pair LDS table [L][G] beside the phi
 * table -- lane j adds gamma_t(j) at [(x_t - 1) * G + j], its own column, the
 * addresses of a row consecutive.  No floating-point atomics: the same bits on
 * every run.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_estep.h"
#include "hhmm_large.h"
#include "hhmm_stats.h"

namespace hhmm {

/* Where row i of xi lives, per instance: registers where the kernel keeps two
 * waves per SIMD with them (KM = 16) or has one in either form (KM = 32, and
 * hmm at KM = 24); the per-pair LDS block for hmm-multinom at KM = 24, where KM
 * more fp64 registers cost the second wave (235 VGPRs against 282; DESIGN.md
 * §3.11b has the compiler's figures). */
constexpr bool estep_large_xi_lds(bool gauss, int KM) { return !gauss && KM == 24; }

template <int MODEL, int G, int KM>
__global__ void __launch_bounds__(kBlock) estep_large_kernel(const DevArgs a, const LkStatsOut o)
{
    HIP_DYNAMIC_SHARED(double, lds)
    constexpr bool GAUSS = LkTraits<MODEL>::kGauss;
    constexpr bool XL = estep_large_xi_lds(GAUSS, KM);
    /* groups past the last pair redo pair P - 1 (identical values, benign
     * duplicate stores): every lane stays in the group reductions */
    const int64_t q = lk_group<G>(a.P);
    LkLane<MODEL, G, KM> ln;
    lk_setup<MODEL, G, KM>(ln, a, lds, false, q);
    const int K = ln.K, L = GAUSS ? 0 : ln.L, Tp = ln.Tp;
    const bool st = ln.on; /* the lane that stores state j's outputs */
    /* LDS after lk_setup's [groups][2][G] slots and [groups][L][G] phi tables:
     * [groups][L][G] counts, then [groups][K][G] xi rows (XL).  A lane touches
     * its own column of either only, so it needs no barrier after zeroing it. */
    const int g = threadIdx.x / G, gpb = blockDim.x / G;
    double *const cnt = lds + (size_t)gpb * (2 + L) * G + (size_t)g * L * G + ln.j;
    double *const xs = lds + (size_t)gpb * (2 + 2 * L) * G + (size_t)g * K * G + ln.j;
    for (int l = 0; l < L; ++l)
        cnt[l * G] = 0.0;
    if constexpr (XL)
        for (int j = 0; j < K; ++j)
            xs[j * G] = 0.0;

    auto fwd = [&](const double (&wv)[KM], double e) -> double {
        const double d = lk_dot<KM>(wv, ln.col);
        return ln.on ? d * e : 0.0;
    };
    auto xchg = [&](int sl, double v, double (&wv)[KM]) { grp_exchange<G, KM>(ln.xch, sl, ln.j, v, wv); };
    auto ckpt = [&](int c) -> double & { return a.ckpt[q + a.P * ((int64_t)c * K + (ln.on ? ln.j : 0))]; };
    bool xbad = false; /* the data check rides on the forward sweep's loads */
    auto block = [&](int b) { return lk_block_checked<MODEL, G, KM>(ln, a, b, L, Tp, xbad); };
    double w[KM];
    int slot = 0;

    /* ---- forward: lk_fb_kernel's sweep, checkpoints only ---- */
    LkObs<MODEL, G> bcur, bnxt = block(0);
    bcur = bnxt;
    double al = 0.0, lsc = 0.0;
    int ex = 0;
    for (int t = 0; t < Tp; ++t) {
        const int u = t % G;
        if (u == 0) { /* group-uniform: next block of observations, prefetch the one after */
            bcur = bnxt;
            bnxt = block(t / G + 1);
        }
        int x;
        double xr, m;
        lk_get<MODEL, G>(bcur, u, x, xr);
        if (t == 0) {
            if constexpr (GAUSS) {
                /* log(p_1k) + SUM_k normal_lpdf(x[1] | mu_k, sigma_k): alpha_1 = p_1k (Q2) */
                const double z = (xr - ln.mu) * ln.isig;
                const double tk = ln.on ? (HHMM_NEG_LOG_SQRT_TWO_PI - ln.lsig) + (-0.5 * (z * z)) : 0.0;
                lsc += grp_sum<G>(tk);
                al = ln.on ? ln.pj : 0.0;
            } else {
                const double e = lk_emit<MODEL, G, KM>(ln, x, xr, m);
                al = ln.on ? ln.pj * e : 0.0;
            }
            al = grp_renorm<G>(al, ex);
        } else {
            const double e = lk_emit<MODEL, G, KM>(ln, x, xr, m);
            xchg(slot, al, w);
            slot ^= 1;
            lsc += m;
            al = grp_renorm_at<G>(fwd(w, e), ex, t, ln.dense);
        }
        if (t % kLChunk == 0 && st)
            ckpt(t / kLChunk) = al;
    }
    const double ll = log(grp_sum<G>(al)) + (lsc + kLn2 * ex); /* the same bits on every lane of the group */

    /* ---- backward sweep, chunk by chunk from the end ---- */
    double acc[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j)
        acc[j] = 0.0;
    double n1 = 0.0, gw = 0.0, gs1 = 0.0, gs2 = 0.0, x0 = 0.0;
    bool bad = !__builtin_isfinite(ll);
    double be = ln.on ? 1.0 : 0.0; /* beta_T uniform */
    int bex = 0;
    /* the transition into step t, with alpha_{t-1} = ap and b_t = b on this lane */
    auto transition = [&](int t, double ap, double b) {
        xchg(slot, b, w);
        slot ^= 1;
        const double d = lk_dot<KM>(w, ln.row);
        const double bn = ln.on ? d : 0.0; /* beta_{t-1}, before any renormalisation */
        const double Z = grp_sum<G>(ap * bn);
        bad |= !((Z > 0.0) & (Z < __builtin_inf()));
        const double ar = ap * fast_rcp(Z);
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if constexpr (XL) {
                if (j < K)
                    xs[j * G] = fma(ar, w[j], xs[j * G]);
            } else {
                acc[j] = fma(ar, w[j], acc[j]);
            }
        }
        be = grp_renorm_at<G>(bn, bex, t, ln.dense);
    };
    constexpr int CPB = G / kLChunk; /* chunks per observation block */
    const int nck = (Tp + kLChunk - 1) / kLChunk;
    int cb = (nck - 1) / CPB;
    LkObs<MODEL, G> ob = lk_block<MODEL, G, KM>(ln, a, cb), obp = lk_block<MODEL, G, KM>(ln, a, cb - 1);
    double ck = ckpt(nck - 1), ckn = ckpt(max(nck - 2, 0));
    double epend = 0.0; /* e of the first step of the chunk after this one */
    for (int c = nck - 1; c >= 0; --c) {
        if (c / CPB != cb) { /* group-uniform: step back one observation block */
            cb = c / CPB;
            ob = obp;
            obp = lk_block<MODEL, G, KM>(ln, a, cb - 1);
        }
        const int tc = c * kLChunk;
        const int ub = tc % G; /* the chunk's first step inside the block */
        double es[kLChunk], xv[kLChunk];
        int sym[kLChunk];
#pragma unroll
        for (int u = 0; u < kLChunk; ++u) {
            double m;
            lk_get_var<MODEL, G>(ob, ub + u, sym[u], xv[u]);
            es[u] = lk_emit<MODEL, G, KM>(ln, sym[u], xv[u], m);
        }
        /* alpha over the chunk from its checkpoint */
        double abuf[kLChunk];
        abuf[0] = ln.on ? ck : 0.0;
        ck = ckn;
        ckn = ckpt(max(c - 2, 0));
        int exb = 0;
#pragma unroll
        for (int u = 1; u < kLChunk; ++u) {
            abuf[u] = 0.0;
            if (tc + u < Tp) { /* group-uniform */
                xchg(slot, abuf[u - 1], w);
                slot ^= 1;
                abuf[u] = grp_renorm_at<G>(fwd(w, es[u]), exb, tc + u, ln.dense);
            }
        }
        /* the transition into the first step of the chunk after this one (a
         * chunk with a successor is complete: alpha_{t-1} is its last entry) */
        if (c < nck - 1)
            transition(tc + kLChunk, abuf[kLChunk - 1], epend * be);
#pragma unroll
        for (int u = kLChunk - 1; u >= 0; --u) {
            const int t = tc + u;
            if (t >= Tp) /* group-uniform */
                continue;
            /* gamma_t from the lane's own alpha_t and beta_t; the reference's
             * normalised-vector formula where the product underflows */
            const double av = abuf[u];
            const double ug = av * be;
            const double sg = grp_sum<G>(ug);
            double gm;
            if (sg > kGammaDirect) { /* group-uniform */
                bad |= !(sg < __builtin_inf());
                gm = ug * fast_rcp(sg);
            } else {
                const double sa = grp_sum<G>(av), sb = grp_sum<G>(be);
                const double un = (av / sa) * (be / sb);
                const double su = grp_sum<G>(un);
                bad |= !((su > 0.0) & (su < __builtin_inf()));
                gm = un / su;
            }
            if (t == 0)
                n1 = gm;
            if constexpr (GAUSS) {
                if (t == 0) { /* Q2: x_1 counts with weight 1 for every state */
                    x0 = xv[u];
                } else {
                    gw += gm;
                    gs1 = fma(gm, xv[u], gs1);
                    gs2 = fma(gm, xv[u] * xv[u], gs2);
                }
            } else {
                double *r = cnt + (min(max(sym[u], 1), L) - 1) * G;
                *r += gm;
            }
            if (u > 0)
                transition(t, abuf[u - 1], es[u] * be);
        }
        epend = es[0];
    }

    /* ---- the [P, ...] outputs ---- */
    const double nanv = dev_nan();
    const int64_t p = ln.p;
    if (st) {
        o.n1[p + a.P * (int64_t)ln.j] = bad ? nanv : n1;
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j < K) {
                const double v = XL ? xs[j * G] : acc[j];
                o.xi[p + a.P * ((int64_t)ln.j + (int64_t)K * j)] = bad ? nanv : ln.row[j] * v;
            }
        if constexpr (GAUSS) {
            o.w[p + a.P * (int64_t)ln.j] = bad ? nanv : 1.0 + gw;
            o.s1[p + a.P * (int64_t)ln.j] = bad ? nanv : x0 + gs1;
            o.s2[p + a.P * (int64_t)ln.j] = bad ? nanv : x0 * x0 + gs2;
        } else {
            for (int l = 0; l < L; ++l)
                o.c[p + a.P * ((int64_t)ln.j + (int64_t)K * l)] = bad ? nanv : cnt[l * G];
        }
    }
    /* any lane of the group saw a symbol outside 1..L (every lane of the wave takes part) */
    const unsigned long long hit = __ballot(xbad);
    const unsigned long long mine = ((1ull << G) - 1) << ((threadIdx.x & 63) & ~(G - 1));
    if (ln.j == 0) {
        o.loglik[p] = ll;
        if (o.status) {
            bool inv = (hit & mine) != 0;
            if (a.T)
                inv |= a.T[ln.n] < 1 || a.T[ln.n] > a.Tmax;
            o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
        }
    }
}

/* ---- host side ---- */

/* LDS bytes of one group: two exchange slots, the phi table and the count
 * table of hmm-multinom, the xi rows where the instance keeps them there. */
static size_t estep_large_group_lds(int model, int K, int L)
{
    const size_t G = (size_t)lk_G(K);
    const size_t tabs = model == HHMM_MODEL_HMM_GAUSS ? 0 : 2 * (size_t)L;
    const bool xl = estep_large_xi_lds(model == HHMM_MODEL_HMM_GAUSS, lk_KM(K));
    return ((2 + tabs) * G + (xl ? (size_t)K * G : 0)) * sizeof(double);
}

size_t lk_ckpt_workspace_bytes(const hhmm_request *r, int64_t P)
{
    return (size_t)(((int64_t)r->data.T_max + kLChunk - 1) / kLChunk) * (size_t)r->data.K * (size_t)P * sizeof(double);
}

hhmm_status check_estep_large(const hhmm_request *r, const hhmm_estep_result *o)
{
    const LkScope &sc = kEstepLargeScope;
    const hhmm_status s = stats_check_head(sc.name, r, lk_stats_model, sc.others, sc.k_lo, sc.k_hi, sc.below);
    if (s != HHMM_OK)
        return s;
    const int K = r->data.K, L = r->data.L;
    LkGeom g;
    if (r->model == HHMM_MODEL_HMM_MULTINOM && L >= 1 &&
        !lk_geometry(estep_large_group_lds(r->model, K, L), 0, lk_G(K), 1, &g)) {
        set_error("%s: L = %d: the emission table and its count table of one %d-lane group do not fit in LDS", sc.name,
                  L, lk_G(K));
        return HHMM_ERR_UNSUPPORTED;
    }
    return stats_check_tail(sc.name, r, o, sc.reads_u);
}

hhmm_status launch_estep_large(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                               hipStream_t st)
{
    const LkScope &sc = kEstepLargeScope;
    DevArgs a;
    const hhmm_status s = lk_stats_dev_args(sc, r, P, ws, &a);
    if (s != HHMM_OK)
        return s;
    LkGeom g;
    if (!lk_geometry(estep_large_group_lds(a.model, a.K, a.L), 0, lk_G(a.K), P, &g)) {
        set_error("%s: the tables of L = %d do not fit in LDS", sc.name, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const LkStatsOut o = lk_stats_out(res);
    dispatch_lk_model(a.model, a.K, [&](auto M, auto G, auto KM) { /* the instances of run_large (hhmm_m_large.hip) */
        hipLaunchKernelGGL((estep_large_kernel<M, G, KM>), g.grid, g.block, g.lds, st, a, o);
    });
    return launch_status("estep_large_kernel");
}

} // namespace hhmm
