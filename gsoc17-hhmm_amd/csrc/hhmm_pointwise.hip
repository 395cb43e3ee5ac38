/*
 * hhmm_pointwise.hip -- gfx950 kernels of the pointwise predictive densities
 * (include/hhmm_pointwise.h): per step the one-step-ahead predictive log
 * density l_t of every (series, draw) pair, reduced over the draws of each
 * series to lpd_t, mean_t and var_t, for hmm and hmm-multinom at K <= 8.
 *
 * One LANE owns one pair (the layout and latency rules of hhmm_step.h), and a
 * WAVE owns 64 consecutive draws of ONE series; a workgroup of nw waves is one
 * tile of 64 nw draws of that series.  Length, chunk count and the
 * observation rows are therefore uniform over the workgroup: no ragged
 * predicate inside a wave, barriers inside the chunk loop are legal, and the
 * observation addresses are scalar.  Lanes past the series' last draw redo
 * draw D - 1 and are left out of the reductions and the stores.
 *   forward   fwd_init / fwd_step with the power-of-two renorm, chunk by chunk
 *             of C = fb_chunk(K) steps, no checkpoints.  With s_t = vsum(alpha_t)
 *             after the step's renormalisation by 2^-e_t and m_t the Gaussian
 *             emission scale of the step,
 *                 l_t = (log s_t - log s_{t-1}) + (kLn2 e_t + m_t)
 *             from the step's own quantities (one log per pair and step, the
 *             previous one carried) -- not a difference of running totals,
 *             which would lose |loglik| eps per step on a long series.  s_t
 *             lies in [0.5, K), so the difference of the two logs is good to a
 *             few 1e-16 absolute.  An impossible observation makes s_t = 0:
 *             l_t = -inf, and NaN (-inf minus -inf) after it.
 *   reduction each lane leaves its chunk's C values in an LDS tile [C][64 + G]
 *             of its wave (G = 64 / C; the pad keeps the eight step rows off
 *             each other's banks).  Then G lanes own one step: each reads C of
 *             its 64 values, and log2 G __shfl_xor stages per pass give the
 *             group (1) the largest member and the sum, (2) -- with the mean
 *             at hand, a true two-pass -- sum exp(l - max) and sum (l - mean)^2.
 *             The waves of the workgroup leave these partials (max, sum exp,
 *             count, sum, M2) in LDS (two buffers by chunk parity: one barrier),
 *             and C threads merge them in wave order: the sums add, the exp
 *             sums are rescaled to the common max, M2 takes Chan's term.
 *   tiles     a series with more draws than one workgroup covers spreads over
 *             ceil(D / (64 nw)) workgroups; each writes its partials to the
 *             workspace ([tile][5][T_max][N]) and pointwise_finish_kernel
 *             merges them in tile order.  No floating-point atomics: the same
 *             bits on every run.
 * A -inf member has exp(l - max) = 0 and (l - mean) = NaN, a NaN member is NaN
 * in every sum, and an all -inf cell takes the shift 0 instead of its max:
 * the IEEE results of the contract without a branch per member.
 * lp_t stores are pair-fastest, one coalesced wave transaction per step,
 * skipped when the pointer is NULL.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_fbchunk.h"
#include "hhmm_pointwise.h"
#include "hhmm_stats.h"

namespace hhmm {

struct PwOut {
    double *loglik, *lpd, *mean, *var, *lp;
    int32_t *status;
    double *part; /* [tiles][5][Tmax][N] partials (tiles > 1) */
    int64_t D;    /* draws per series */
    int32_t tiles;
};

/* The reduction of some members of a cell: their largest value, sum exp(l -
 * shift(m)), their number, their sum and sum (l - their mean)^2. */
struct PwPart {
    double m, se, cnt, sum, m2;
};

/* the shift of the exp sums: the max, or 0 where every member is -inf (or NaN) */
__device__ __forceinline__ double pw_shift(double m) { return m == dev_ninf() ? 0.0 : m; }

/* a := a merged with b (both of at least one member), a's members first */
__device__ __forceinline__ void pw_merge(PwPart &a, const PwPart &b)
{
    const double m = fmax(a.m, b.m);
    const double ms = pw_shift(m);
    /* a side whose max is -inf holds se = 0 (or NaN) at shift 0: taken as it is */
    const double fa = a.m == dev_ninf() ? 1.0 : exp(a.m - ms);
    const double fb = b.m == dev_ninf() ? 1.0 : exp(b.m - ms);
    const double n = a.cnt + b.cnt;
    const double delta = b.sum / b.cnt - a.sum / a.cnt;
    a.m2 = (a.m2 + b.m2) + delta * delta * (a.cnt * b.cnt / n);
    a.se = a.se * fa + b.se * fb;
    a.sum = a.sum + b.sum;
    a.cnt = n;
    a.m = m;
}

/* The three reductions of a whole cell of D members. */
__device__ __forceinline__ void pw_store(const PwOut &o, int64_t cell, const PwPart &v)
{
    const double D = (double)o.D;
    o.lpd[cell] = pw_shift(v.m) + log(v.se / D);
    o.mean[cell] = v.sum / D;
    o.var[cell] = v.m2 / (D - 1.0);
}

template <int MODEL, int K>
__global__ void __launch_bounds__(kBlock) pointwise_kernel(const DevArgs a, const PwOut o)
{
    constexpr int C = fb_chunk(K);
    constexpr int KP = (K + 1) / 2;
    constexpr bool GAUSS = ModelTraits<MODEL>::kGauss;
    constexpr int G = 64 / C;  /* lanes that share one step of the reduction */
    constexpr int RS = 64 + G; /* row stride of the wave's tile */
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    /* the series and the tile of its draws: uniform over the workgroup */
    const int64_t n = blockIdx.x / o.tiles;
    const int tile = (int)(blockIdx.x - n * o.tiles);
    const int64_t wbase = ((int64_t)tile * nw + wave) * 64; /* the wave's first draw of the series */
    const bool live = wbase + lane < o.D;
    const int64_t p = n * o.D + min(wbase + lane, o.D - 1);
    int64_t np, d;
    pair_coords(a, p, np, d);

    const size_t slab_elems = GAUSS ? 0 : (size_t)a.L * KP * 64;
    double2 *const slab = lds + (size_t)wave * slab_elems + lane;
    double *const red = reinterpret_cast<double *>(lds + (size_t)nw * slab_elems);
    double *const tl = red + (size_t)wave * (C * RS);  /* this wave's [C][RS] values */
    double *const wpart = red + (size_t)nw * (C * RS); /* [2][nw][C][5] */
    PairParams<MODEL, K> pp;
    load_params<MODEL, K, false>(pp, a, d);
    if constexpr (!GAUSS)
        fill_table<K, false>(slab, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, false>(a, n);
    const int Tp = pair_len(a, n);
    const int nchunk = (Tp + C - 1) / C;
    const uint32_t po = (uint32_t)p * 8u;

    /* the reduction's view of the tile: G lanes per step, C members each */
    const int ru = lane / G, rpart = lane % G;
    const double wcnt = (double)min(max(o.D - wbase, (int64_t)0), (int64_t)64);

    double al[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        al[k] = 0.0;
    double lsc = 0.0, lprev = 0.0;
    int ex = 0;
    uint32_t xm = 0;
    Obs cur[C];
    load_chunk<MODEL, C, false>(cur, sp, 0);
    Em<K> ecur;
    emit_prob<MODEL, K>(pp, slab, a.L, cur[0], ecur);
    for (int c = 0; c < nchunk; ++c) {
        const int t0 = c * C;
        Obs nxt[C];
        load_chunk<MODEL, C, false>(nxt, sp, t0 + C);
#pragma unroll
        for (int u = 0; u < C; ++u) {
            const int t = t0 + u;
            Em<K> enx;
            emit_prob<MODEL, K>(pp, slab, a.L, (u + 1 < C) ? cur[u + 1 < C ? u + 1 : 0] : nxt[0], enx);
            if (t < Tp) {
                double lt, ls;
                if (u == 0 && c == 0) {
                    fwd_init<MODEL, K>(al, pp, ecur, cur[0], lsc, ex);
                    ls = log(vsum<K>(al));
                    lt = ls + (lsc + kLn2 * ex);
                } else {
                    const int e0 = ex;
                    lsc += ecur.m;
                    fwd_step<MODEL, K>(al, pp, ecur.e, cur[u], ex);
                    ls = log(vsum<K>(al));
                    lt = (ls - lprev) + (kLn2 * (ex - e0) + ecur.m);
                }
                lprev = ls;
                tl[u * RS + lane] = lt;
                if (o.lp && live)
                    put_out(o.lp + a.P * (int64_t)t, po, lt);
                if constexpr (!GAUSS)
                    xm = max(xm, (uint32_t)cur[u].x - 1u);
            }
            ecur = enx;
        }
        __syncthreads();
        /* this wave's 64 members of each of the chunk's steps */
        PwPart w;
        {
            double v[C];
            bool ok[C];
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int j = rpart + G * i;
                v[i] = tl[ru * RS + j];
                ok[i] = wbase + j < o.D;
            }
            double m = dev_ninf(), s = 0.0;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                m = ok[i] ? fmax(m, v[i]) : m;
                s += ok[i] ? v[i] : 0.0;
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                m = fmax(m, __shfl_xor(m, off));
                s += __shfl_xor(s, off);
            }
            const double mean = s / wcnt, ms = pw_shift(m);
            double se = 0.0, q = 0.0;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const double dv = v[i] - mean;
                se += ok[i] ? exp(v[i] - ms) : 0.0;
                q += ok[i] ? dv * dv : 0.0;
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                se += __shfl_xor(se, off);
                q += __shfl_xor(q, off);
            }
            w = PwPart{m, se, wcnt, s, q};
        }
        double *const wp = wpart + (size_t)(c & 1) * (nw * C * 5);
        if (rpart == 0) {
            double *r = wp + (wave * C + ru) * 5;
            r[0] = w.m;
            r[1] = w.se;
            r[2] = w.cnt;
            r[3] = w.sum;
            r[4] = w.m2;
        }
        __syncthreads();
        /* the workgroup's waves in order (wave 0 always has members), one thread per step */
        if ((int)threadIdx.x < C && t0 + (int)threadIdx.x < Tp) {
            const int u = threadIdx.x;
            PwPart acc{wp[u * 5], wp[u * 5 + 1], wp[u * 5 + 2], wp[u * 5 + 3], wp[u * 5 + 4]};
            for (int q = 1; q < nw; ++q) {
                const double *r = wp + (q * C + u) * 5;
                const PwPart b{r[0], r[1], r[2], r[3], r[4]};
                if (b.cnt > 0.0)
                    pw_merge(acc, b);
            }
            const int64_t cell = n + a.N * (int64_t)(t0 + u);
            if (o.tiles == 1) {
                pw_store(o, cell, acc);
            } else {
                double *r = o.part + (int64_t)tile * 5 * a.Tmax * a.N + cell;
                const int64_t st = (int64_t)a.Tmax * a.N;
                r[0] = acc.m;
                r[st] = acc.se;
                r[2 * st] = acc.cnt;
                r[3 * st] = acc.sum;
                r[4 * st] = acc.m2;
            }
        }
#pragma unroll
        for (int u = 0; u < C; ++u)
            cur[u] = nxt[u];
    }
    if (live) {
        put_out(o.loglik, po, log(vsum<K>(al)) + (lsc + kLn2 * ex));
        if (o.status) {
            bool inv = !GAUSS && xm >= (uint32_t)a.L;
            if (a.T)
                inv |= a.T[n] < 1 || a.T[n] > a.Tmax;
            o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
        }
    }
}

/* One thread per cell (n, t): the tiles' partials in tile order. */
__global__ void __launch_bounds__(kBlock) pointwise_finish_kernel(const DevArgs a, const PwOut o)
{
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t st = (int64_t)a.Tmax * a.N;
    if (cell >= st)
        return;
    const int64_t n = cell % a.N, t = cell / a.N;
    if (t >= pair_len(a, n))
        return;
    const double *r = o.part + cell;
    PwPart acc{r[0], r[st], r[2 * st], r[3 * st], r[4 * st]};
    for (int q = 1; q < o.tiles; ++q) {
        r += 5 * st;
        const PwPart b{r[0], r[st], r[2 * st], r[3 * st], r[4 * st]};
        pw_merge(acc, b);
    }
    pw_store(o, cell, acc);
}

/* Waves per workgroup and its LDS: the emission table of hmm-multinom, and 6 KiB
 * per wave that hold its tile (C (64 + 64 / C) doubles) and its partials. */
static int pointwise_waves(int model, int K, int L, size_t *lds)
{
    const size_t slab =
        model == HHMM_MODEL_HMM_MULTINOM && L > 0 ? (size_t)L * (size_t)((K + 1) / 2) * 64 * sizeof(double2) : 0;
    return waves_that_fit(slab + 6144, lds);
}

/* Tiles of 64 w draws per series (D = P / N under every pairing). */
static int64_t pointwise_tiles(const hhmm_request *r, int64_t P)
{
    size_t lds;
    const int waves = pointwise_waves(r->model, r->data.K, r->data.L, &lds);
    if (waves < 1 || r->data.n_series < 1)
        return 1;
    const int64_t D = P / r->data.n_series;
    return (D + 64 * waves - 1) / (64 * waves);
}

size_t pointwise_workspace_bytes(const hhmm_request *r, int64_t P)
{
    const int64_t tiles = pointwise_tiles(r, P);
    if (tiles <= 1)
        return 0;
    return (size_t)tiles * 5 * (size_t)r->data.n_series * (size_t)r->data.T_max * sizeof(double);
}

static bool pointwise_model(int m) { return m == HHMM_MODEL_HMM_GAUSS || m == HHMM_MODEL_HMM_MULTINOM; }

hhmm_status check_pointwise(const hhmm_request *r, const hhmm_pointwise_result *o)
{
    const hhmm_status s = stats_check_head("pointwise", r, pointwise_model,
                                           "hmm and hmm-multinom only; the coded step weights of the semisup, Tayal "
                                           "and IOHMM programs are masked or factorised, not a predictive density");
    if (s != HHMM_OK)
        return s;
    if (r->model == HHMM_MODEL_HMM_MULTINOM && r->data.K >= 1 && r->data.L >= 1) {
        size_t lds;
        if (pointwise_waves(r->model, r->data.K, r->data.L, &lds) < 1) {
            set_error("pointwise: L * ceil(K / 2) = %d * %d > 154: the emission table of one wave does not fit in LDS",
                      r->data.L, (r->data.K + 1) / 2);
            return HHMM_ERR_UNSUPPORTED;
        }
    }
    if (!o) {
        set_error("pointwise: result must be non-NULL");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const char *missing = !o->loglik ? "loglik" : !o->lpd_t ? "lpd_t" : !o->mean_t ? "mean_t" : !o->var_t ? "var_t" : nullptr;
    if (missing) {
        set_error("pointwise: %s must be non-NULL (loglik, lpd_t, mean_t and var_t are required)", missing);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return HHMM_OK;
}

template <int MODEL>
static bool launch_pointwise_m(const DevArgs &a, const PwOut &o, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    return dispatch_k(a.K, [&](auto kc) {
        hipLaunchKernelGGL((pointwise_kernel<MODEL, decltype(kc)::value>), grid, block, lds, st, a, o);
    });
}

hhmm_status launch_pointwise(const hhmm_request *r, const hhmm_pointwise_result *res, int64_t P, void *ws,
                             hipStream_t st)
{
    DevArgs a = stats_dev_args(r, P, nullptr);
    a.x = r->data.x_int;
    a.xr = r->data.x_real;
    a.phi_k = r->draws.phi_k;
    a.mu_k = r->draws.mu_k;
    a.sigma_k = r->draws.sigma_k;
    size_t lds = 0;
    const int waves = pointwise_waves(a.model, a.K, a.L, &lds);
    if (waves < 1) {
        set_error("pointwise: the table of K*L = %d*%d does not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    PwOut o{res->loglik, res->lpd_t, res->mean_t, res->var_t, res->lp_t, res->pair_status, (double *)ws, P / a.N,
            (int32_t)pointwise_tiles(r, P)};
    const dim3 grid((unsigned)(a.N * o.tiles)), block(64 * waves);
    const bool ok = a.model == HHMM_MODEL_HMM_GAUSS
                        ? launch_pointwise_m<HHMM_MODEL_HMM_GAUSS>(a, o, grid, block, lds, st)
                        : launch_pointwise_m<HHMM_MODEL_HMM_MULTINOM>(a, o, grid, block, lds, st);
    if (!ok) {
        set_error("pointwise: K = %d outside 1..%d", a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    hhmm_status s = launch_status("pointwise_kernel");
    if (s != HHMM_OK || o.tiles == 1)
        return s;
    const int64_t cells = a.N * (int64_t)a.Tmax;
    hipLaunchKernelGGL(pointwise_finish_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a,
                       o);
    return launch_status("pointwise_finish_kernel");
}

} // namespace hhmm
