/*
 * hhmm_pointwise_large.hip -- gfx950 kernels of the pointwise predictive
 * densities at 8 < K <= 32 (include/hhmm_pointwise.h, hhmm_pointwise_large):
 * per step the one-step-ahead predictive log density l_t of every (series,
 * draw) pair, reduced over the draws of each series to lpd_t, mean_t and
 * var_t, for hmm and hmm-multinom.
 *
 * A GROUP of G lanes owns one pair, lane j state j (the layout, the helpers and
 * the arithmetic of estep_large_kernel's forward sweep, hhmm_large.h): the
 * scaled linear-space filter with column j of A in registers, the vector
 * exchanged through the group's LDS slot, the Q2 first step for hmm, a
 * renormalisation every kLRenorm steps (every step in a dense wave).  No
 * checkpoints, no backward pass.
 *   l_t       With s_t = the group sum of alpha_t after whatever renormalisation
 *             the step did, ex the running exponent and m_t the Gaussian
 *             emission scale of the step (0 for hmm-multinom),
 *                 l_t = (log s_t - log s_{t-1}) + (kLn2 (ex_t - ex_{t-1}) + m_t)
 *                 l_1 = log s_1 + (lsc + kLn2 ex_1)
 *             from the step's own quantities, never a difference of running
 *             totals.  A step that was not renormalised has ex_t = ex_{t-1}.
 *             Under the eight-step cadence s stays within [2^-275, 32^9]
 *             (kLRenormSafeBound below, growth of at most K per step above), so
 *             |log s| < 220 and the difference of two logs is good to 5e-14
 *             absolute.  An impossible observation makes s_t = 0: l_t = -inf,
 *             and NaN (-inf minus -inf) after it, without a branch.
 *   one log   The group sum is off alpha's dependency chain, and the log is
 *   per step  not paid G times per pair-step: lane u of the group keeps s_t and
 *             the step's second term c_t = kLn2 (ex_t - ex_{t-1}) + m_t of the
 *             step with t mod G = u (two selects per step; c_t is formed at the
 *             step, so the exponent is not kept).  Once per observation block
 *             -- group-uniform, where lk_block is refilled -- every lane takes
 *             one log, gets log s_{t-1} from its neighbour in the group (lane 0
 *             from the value carried out of the block before) and stores the
 *             l_t of its step at lp[p + P t], t < T[n] only.
 *   reduction l_t always goes through memory -- the caller's lp_t, or the
 *             workspace in the same layout -- because a workgroup holds only 8
 *             or 16 pairs: tile partials would be no smaller than l_t itself.
 *             pointwise_large_reduce_kernel, on the same stream, gives W lanes
 *             to each live cell (n, t < T[n]), whose D members are contiguous
 *             at lp + P t + n D, member i on lane i mod W.  A true two-pass over
 *             the whole cell: (1) the max and the sum, (2) sum exp(l - shift)
 *             and sum (l - mean)^2, shift the max or 0 when the max is -inf.
 *             Lane partials combine by an xor butterfly (both operands of every
 *             level are mirror images: the same bits on every lane), the waves
 *             of a workgroup through LDS in wave order.  Width classes, by D:
 *                 D <= 16        W = 4
 *                 17 .. 64       W = 16
 *                 65 .. 256      W = 64   (one wave)
 *                 D > 256        W = 256  (the workgroup)
 * No floating-point atomics: the same bits on every run, with and without
 * lp_t.  A -inf member has exp(l - shift) = 0 and (l - mean) = NaN, a NaN
 * member is NaN in every sum (fmax passes it over: the shift stays finite).
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_large.h"
#include "hhmm_pointwise.h"
#include "hhmm_stats.h"

namespace hhmm {

struct PwlOut {
    double *loglik, *lp; /* lp: the caller's lp_t or the workspace, never NULL */
    int32_t *status;
};

template <int MODEL, int G, int KM>
__global__ void __launch_bounds__(kBlock) pointwise_large_kernel(const DevArgs a, const PwlOut o)
{
    HIP_DYNAMIC_SHARED(double, lds)
    constexpr bool GAUSS = LkTraits<MODEL>::kGauss;
    /* groups past the last pair redo pair P - 1 (identical values, benign
     * duplicate stores): every lane stays in the group reductions */
    const int64_t q = lk_group<G>(a.P);
    LkLane<MODEL, G, KM> ln;
    lk_setup<MODEL, G, KM>(ln, a, lds, false, q);
    const int L = GAUSS ? 0 : ln.L, Tp = ln.Tp;
    bool xbad = false; /* the data check rides on the forward sweep's loads */
    auto block = [&](int b) { return lk_block_checked<MODEL, G, KM>(ln, a, b, L, Tp, xbad); };
    double w[KM];
    int slot = 0;

    /* this lane's step of the block: s_t and c_t; the log of the last step of the block before */
    double ks = 1.0, kc = 0.0, lcarry = 0.0;
    double *const lpp = o.lp + ln.p;
    auto flush = [&](int t0) { /* the block of steps t0 .. t0 + G - 1 */
        const double ls = log(ks);
        const double up = __shfl_up(ls, 1, G);
        const double lprev = ln.j == 0 ? lcarry : up;
        lcarry = __shfl(ls, G - 1, G);
        const int t = t0 + ln.j;
        if (t < Tp)
            lpp[a.P * (int64_t)t] = (ls - lprev) + kc;
    };

    LkObs<MODEL, G> bcur, bnxt = block(0);
    bcur = bnxt;
    double al = 0.0, lsc = 0.0;
    int ex = 0;
    for (int t = 0; t < Tp; ++t) {
        const int u = t % G;
        if (u == 0) { /* group-uniform: the block before is complete; next block of observations */
            if (t > 0)
                flush(t - G);
            bcur = bnxt;
            bnxt = block(t / G + 1);
        }
        int x;
        double xr, m, c;
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
            c = lsc + kLn2 * ex;
        } else {
            const double e = lk_emit<MODEL, G, KM>(ln, x, xr, m);
            grp_exchange<G, KM>(ln.xch, slot, ln.j, al, w);
            slot ^= 1;
            lsc += m;
            const int e0 = ex;
            const double d = lk_dot<KM>(w, ln.col);
            al = grp_renorm_at<G>(ln.on ? d * e : 0.0, ex, t, ln.dense);
            c = kLn2 * (ex - e0) + m;
        }
        const double s = grp_sum<G>(al); /* off the chain: the next step does not wait for it */
        ks = ln.j == u ? s : ks;
        kc = ln.j == u ? c : kc;
    }
    flush((Tp - 1) / G * G);
    const double ll = log(grp_sum<G>(al)) + (lsc + kLn2 * ex); /* the same bits on every lane of the group */

    /* any lane of the group saw a symbol outside 1..L (every lane of the wave takes part) */
    const unsigned long long hit = __ballot(xbad);
    const unsigned long long mine = ((1ull << G) - 1) << ((threadIdx.x & 63) & ~(G - 1));
    if (ln.j == 0) {
        o.loglik[ln.p] = ll;
        if (o.status) {
            bool inv = (hit & mine) != 0;
            if (a.T)
                inv |= a.T[ln.n] < 1 || a.T[ln.n] > a.Tmax;
            o.status[ln.p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
        }
    }
}

/* ---- the reduction over the draws ---- */

struct PwlRed {
    const double *lp;
    double *lpd, *mean, *var;
    int64_t D; /* draws per series */
};

/* v over the W lanes of a cell: an xor butterfly inside the wave, then (W =
 * kBlock) the waves' values from `sm` in wave order.  The caller puts a
 * barrier between the writes and pwl_waves. */
template <int W, bool MAX>
__device__ __forceinline__ double pwl_lanes(double v)
{
#pragma unroll
    for (int off = (W < 64 ? W : 64) / 2; off > 0; off >>= 1) {
        const double r = __shfl_xor(v, off);
        v = MAX ? fmax(v, r) : v + r;
    }
    return v;
}
template <bool MAX>
__device__ __forceinline__ double pwl_waves(const double *sm)
{
    double v = sm[0];
#pragma unroll
    for (int q = 1; q < kBlock / 64; ++q)
        v = MAX ? fmax(v, sm[q]) : v + sm[q];
    return v;
}

template <int W>
__global__ void __launch_bounds__(kBlock) pointwise_large_reduce_kernel(const DevArgs a, const PwlRed o)
{
    constexpr int NW = kBlock / 64;
    __shared__ double part[4][NW];
    const int lane = threadIdx.x % W, wave = threadIdx.x >> 6;
    const int64_t cells = a.N * (int64_t)a.Tmax;
    const int64_t cell = (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W;
    const int64_t cc = min(cell, cells - 1); /* at n + N t */
    const int64_t n = cc % a.N, t = cc / a.N;
    /* a cell past the series keeps what the caller put there; its lanes read nothing
     * and stay in the shuffles and barriers (W = kBlock: uniform over the workgroup) */
    const bool live = cell < cells && t < pair_len(a, n);
    const int64_t D = live ? o.D : 0;
    const double *const l = o.lp + a.P * t + n * o.D;

    double m = dev_ninf(), s = 0.0;
    for (int64_t i = lane; i < D; i += W) {
        const double v = l[i];
        m = fmax(m, v);
        s += v;
    }
    m = pwl_lanes<W, true>(m);
    s = pwl_lanes<W, false>(s);
    if constexpr (W == kBlock) {
        if ((threadIdx.x & 63) == 0) {
            part[0][wave] = m;
            part[1][wave] = s;
        }
        __syncthreads();
        m = pwl_waves<true>(part[0]);
        s = pwl_waves<false>(part[1]);
    }
    const double Dd = (double)o.D;
    const double mean = s / Dd;
    const double shift = m == dev_ninf() ? 0.0 : m; /* every member -inf (or NaN): no shift */
    double se = 0.0, q = 0.0;
    for (int64_t i = lane; i < D; i += W) {
        const double v = l[i];
        const double dv = v - mean;
        se += exp(v - shift);
        q += dv * dv;
    }
    se = pwl_lanes<W, false>(se);
    q = pwl_lanes<W, false>(q);
    if constexpr (W == kBlock) {
        if ((threadIdx.x & 63) == 0) {
            part[2][wave] = se;
            part[3][wave] = q;
        }
        __syncthreads();
        se = pwl_waves<false>(part[2]);
        q = pwl_waves<false>(part[3]);
    }
    if (live && lane == 0) {
        o.lpd[cc] = shift + log(se / Dd);
        o.mean[cc] = mean;
        o.var[cc] = q / (Dd - 1.0);
    }
}

/* ---- host side ---- */

/* LDS bytes of one group: two exchange slots and the phi table of hmm-multinom. */
static size_t pwl_group_lds(int model, int K, int L)
{
    const size_t tab = model == HHMM_MODEL_HMM_GAUSS ? 0 : (size_t)L;
    return (2 + tab) * (size_t)lk_G(K) * sizeof(double);
}

size_t pointwise_large_workspace_bytes(const hhmm_request *r, int64_t P)
{
    return (size_t)P * (size_t)r->data.T_max * sizeof(double);
}

hhmm_status check_pointwise_large(const hhmm_request *r, const hhmm_pointwise_result *o)
{
    const LkScope &sc = kPointwiseLargeScope;
    const hhmm_status s = stats_check_head(sc.name, r, lk_stats_model, sc.others, sc.k_lo, sc.k_hi, sc.below);
    if (s != HHMM_OK)
        return s;
    const int K = r->data.K, L = r->data.L, G = lk_G(K);
    LkGeom g;
    if (r->model == HHMM_MODEL_HMM_MULTINOM && L >= 1 && !lk_geometry(pwl_group_lds(r->model, K, L), 0, G, 1, &g)) {
        set_error("%s: L = %d: (2 + L) * %d * 8 = %zu > %zu bytes: the emission table of one %d-lane group does not "
                  "fit in LDS",
                  sc.name, L, G, pwl_group_lds(r->model, K, L), kLdsLimit, G);
        return HHMM_ERR_UNSUPPORTED;
    }
    if (!o) {
        set_error("%s: result must be non-NULL", sc.name);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const char *missing = !o->loglik ? "loglik" : !o->lpd_t ? "lpd_t" : !o->mean_t ? "mean_t" : !o->var_t ? "var_t" : nullptr;
    if (missing) {
        set_error("%s: %s must be non-NULL (loglik, lpd_t, mean_t and var_t are required)", sc.name, missing);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return HHMM_OK;
}

template <int W>
static void launch_pwl_reduce(const DevArgs &a, const PwlRed &o, hipStream_t st)
{
    const int64_t cells = a.N * (int64_t)a.Tmax, cpb = kBlock / W;
    hipLaunchKernelGGL(pointwise_large_reduce_kernel<W>, dim3((unsigned)((cells + cpb - 1) / cpb)), dim3(kBlock), 0, st,
                       a, o);
}

hhmm_status launch_pointwise_large(const hhmm_request *r, const hhmm_pointwise_result *res, int64_t P, void *ws,
                                   hipStream_t st)
{
    const LkScope &sc = kPointwiseLargeScope;
    DevArgs a;
    hhmm_status s = lk_stats_dev_args(sc, r, P, nullptr, &a);
    if (s != HHMM_OK)
        return s;
    LkGeom g;
    if (!lk_geometry(pwl_group_lds(a.model, a.K, a.L), 0, lk_G(a.K), P, &g)) {
        set_error("%s: the table of L = %d does not fit in LDS", sc.name, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    double *const lp = res->lp_t ? res->lp_t : (double *)ws; /* the workspace is not touched when lp_t is given */
    const PwlOut o{res->loglik, lp, res->pair_status};
    dispatch_lk_model(a.model, a.K, [&](auto M, auto G, auto KM) { /* the instances of estep_large_kernel */
        hipLaunchKernelGGL((pointwise_large_kernel<M, G, KM>), g.grid, g.block, g.lds, st, a, o);
    });
    if ((s = launch_status("pointwise_large_kernel")) != HHMM_OK)
        return s;
    const PwlRed q{lp, res->lpd_t, res->mean_t, res->var_t, P / a.N};
    if (q.D <= 16)
        launch_pwl_reduce<4>(a, q, st);
    else if (q.D <= 64)
        launch_pwl_reduce<16>(a, q, st);
    else if (q.D <= 256)
        launch_pwl_reduce<64>(a, q, st);
    else
        launch_pwl_reduce<kBlock>(a, q, st);
    return launch_status("pointwise_large_reduce_kernel");
}

} // namespace hhmm
