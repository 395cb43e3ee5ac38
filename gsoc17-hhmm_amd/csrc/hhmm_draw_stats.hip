/*
 * hhmm_draw_stats.hip -- gfx950 kernel of the draw statistics
 * (include/hhmm_gibbs.h, include/hhmm_gibbs_gauss.h): per (series, draw) pair
 * one FFBS path z, reduced to what a conjugate parameter update needs -- z_1,
 * the transitions, and the (state, symbol) pairs (hmm-multinom, semisup, Tayal)
 * or per state the count, the sum and the sum of squares of the observations it
 * owns (the Gaussian hmm) -- at K <= 8.  Nothing is written per step.
 *
 * One kernel template; what the Gaussian hmm does differently are `if
 * constexpr` arms on ModelTraits<MODEL>::kGauss.  One LANE owns one pair (the
 * layout and latency rules of hhmm_step.h, the chunk helpers of hhmm_fbchunk.h).
 *   forward   the FFBS contract's filter, the operations of
 *             fb_kernel<.., FB_GAMMA | FB_FFBS> (fwd_chunk: per-step
 *             renormalisation, emit_prob<.., true>; Gaussian: hhmm_det_exp_tab
 *             on the workgroup's LDS copy of the 2^(j/128) table, as fb_kernel
 *             does under fb_exp2_lds): a checkpoint every C = fb_chunk(K)
 *             steps, loglik at the end.
 *   backward  chunk by chunk from the end: the filter over the chunk is
 *             recomputed from its checkpoint (bit-identical), z_t
 *             drawn by ffbs_draw's operations (draw_step) from u[p, t], the
 *             statistics taken.  No beta, no gamma, no reciprocal.
 * Accumulators: z_t is a run-time index, so nothing is indexed by it in
 * registers (that becomes scratch).  The tables are slabs in LDS, lane-fastest
 * (64 consecutive words = every bank once: conflict-free):
 *     c_kl    cs[((l - 1) * K + k) * 64 + lane]   32-bit (discrete)
 *     s1, s2  ss[(2 k + {0, 1}) * 64 + lane]      fp64, read-add-write (lane-private)
 *     w       ws[k * 64 + lane]                   32-bit (Gaussian)
 *     xi_ij   xs[(i * K + j) * 64 + lane]         32-bit
 * a 32-bit count is one ds_add_u32 per step (K^2 compare-and-add registers cost
 * 2 K^2 VALU per step on the dependent chain of the draw and, at K = 8, 64
 * VGPRs).  A count is at most T_max < 2^31.  n_1k comes from z_1 at the end.
 * Gaussian: step 1 (Q2, hmm.stan:30) belongs to every state: x_1 is added once
 * per state at the end, as estep_kernel does with x0.
 * LDS per wave: L * (1024 ceil(K/2) + 256 K) + 256 K^2 bytes, the workgroup
 * sized to fit 160 KiB; Gaussian: (K + K^2) * 256 + 2 K * 512 bytes beside the
 * workgroup's 2 KiB table, the workgroup sized for the most waves per CU.
 * The [P, ...] stores are pair-fastest: one coalesced wave transaction each.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_gibbs.h"
#include "hhmm_gibbs_gauss.h"
#include "hhmm_fbchunk.h"
#include "hhmm_stats.h"

namespace hhmm {

/* One struct per kernel-argument layout; DrawStatsOutOf picks by the model. */
struct DrawStatsOut {
    double *loglik, *n1, *xi, *c;
    int32_t *status;
};

struct DrawStatsGaussOut {
    double *loglik, *n1, *xi, *w, *s1, *s2;
    int32_t *status;
};

template <int MODEL>
using DrawStatsOutOf = std::conditional_t<ModelTraits<MODEL>::kGauss, DrawStatsGaussOut, DrawStatsOut>;

/* Bytes of LDS one wave of the Gaussian kernel needs: s1 / s2 (fp64), then w and xi (32-bit). */
constexpr size_t draw_stats_gauss_wave_lds(int K)
{
    return (size_t)2 * K * 64 * sizeof(double) + ((size_t)K + (size_t)K * K) * 64 * sizeof(uint32_t);
}

/* one more in this lane's word of a count slab */
__device__ __forceinline__ void count_one(uint32_t *w)
{
    __hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

/* v, as a value hipcc cannot trace back to its load (an empty asm: no instruction) */
__device__ __forceinline__ double opaque(double v)
{
    __asm__("" : "+v"(v));
    return v;
}

/* ffbs_draw (hhmm_fbchunk.h) with the mask of step t + 1 at z_{t+1} already decided
 * (`on`): the same operations on the same values, so the same z.  The column
 * A(., z_{t+1}) is picked from opaque copies of the entries: left to itself
 * hipcc folds the select chain over pp.A into one dynamically indexed load,
 * which moves the pair's parameters into scratch (K scratch loads per step,
 * 288 B of private segment at K = 3 up to 928 B at K = 8). */
template <int MODEL, int K>
__device__ __forceinline__ int draw_step(const PairParams<MODEL, K> &pp, const double (&f)[K], bool last, bool on,
                                         int z, double u)
{
    double w[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double az = opaque(pp.A[i][0]);
#pragma unroll
        for (int j = 1; j < K; ++j) {
            const double aj = opaque(pp.A[i][j]);
            az = (z == j) ? aj : az;
        }
        w[i] = (last | !on) ? f[i] : f[i] * az;
    }
    if (!last && z < 0)
        return -1;
    return ffbs_cat<K>(w, u);
}

template <int MODEL, int K>
__global__ void __launch_bounds__(kBlock) draw_stats_kernel(const DevArgs a, const DrawStatsOutOf<MODEL> o)
{
    constexpr int C = fb_chunk(K);
    constexpr int KP = (K + 1) / 2;
    constexpr bool GAUSS = ModelTraits<MODEL>::kGauss;
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    constexpr int MODE = FB_GAMMA | FB_FFBS;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    /* this lane's slabs.  Each arm declares the dynamic LDS array with its own
     * element type: the type's alignment decides the table copy's stores. */
    const hhmm_exp2_entry *tab = hhmm_exp2_tab;
    double *ss = nullptr;
    uint32_t *ws = nullptr, *cs = nullptr, *xs = nullptr;
    if constexpr (GAUSS) {
        HIP_DYNAMIC_SHARED(hhmm_exp2_entry, etab)
        static_assert(kExp2TabBytes % sizeof(double) == 0, "the fp64 slabs follow the table");
        for (int i = threadIdx.x; i < 128; i += blockDim.x)
            etab[i] = hhmm_exp2_tab[i];
        /* every fp64 slab first, then the count slabs */
        double *const slabs = reinterpret_cast<double *>(etab + 128);
        ss = slabs + (size_t)wave * (2 * K * 64) + lane;
        ws = reinterpret_cast<uint32_t *>(slabs + (size_t)nw * (2 * K * 64)) + (size_t)wave * ((K + K * K) * 64) + lane;
        xs = ws + K * 64;
#pragma unroll
        for (int i = 0; i < 2 * K; ++i)
            ss[i * 64] = 0.0;
#pragma unroll
        for (int i = 0; i < K + K * K; ++i)
            ws[i * 64] = 0u;
        __syncthreads();
        tab = etab;
    }

    const int64_t gwave = (int64_t)blockIdx.x * nw + wave;
    /* lanes past the last pair redo pair P-1 (identical values, benign
     * duplicate stores): every lane stays in the wave-wide reductions */
    const int64_t p = min(gwave * 64 + lane, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);

    FbLane<MODEL, K> ln;
    ln.p = p;
    ln.n = n;
    ln.L = a.L;
    ln.t0 = 0;
    ln.Tp = pair_len(a, n);
    ln.cb = 0;
    ln.q = p;
    ln.Qs = a.P;
    if constexpr (GAUSS) {
        ln.slab = nullptr;
        ln.etab = tab;
        load_params<MODEL, K, false>(ln.pp, a, d);
    } else {
        HIP_DYNAMIC_SHARED(double2, lds)
        const size_t slab_elems = (size_t)a.L * KP * 64;
        const size_t cnt_words = ((size_t)a.L * K + K * K) * 64;
        double2 *const pslab = lds + (size_t)wave * slab_elems + lane;
        cs = reinterpret_cast<uint32_t *>(lds + (size_t)nw * slab_elems) + (size_t)wave * cnt_words + lane;
        xs = cs + (size_t)a.L * K * 64;
        ln.slab = pslab;
        load_params<MODEL, K, false>(ln.pp, a, d);
        ln.pp.skip_ok &= fill_table<K, false>(pslab, a, d);
        for (int i = 0; i < a.L * K + K * K; ++i)
            cs[i * 64] = 0u;
    }
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);
    const int Tw_min = wave_min(ln.Tp);
    const int Tw_max = wave_max(ln.Tp);
    const int nfull = Tw_min / C;            /* chunks complete for every lane */
    const int nchunk = (Tw_max + C - 1) / C; /* chunks any lane needs: <= ceil(Tmax / C) checkpoint rows */

    /* ---- forward sweep: fb_kernel's FFBS filter, checkpoints only ---- */
    double ll;
    uint32_t xm = 0;
    Obs cur[C];
    {
        double al[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            al[k] = 0.0;
        double lsc = 0.0;
        int ex = 0;
        /* chunks per observation prefetch group (the grouping changes no bit).  Gaussian, K = 8: kFwdGroup = 4
         * chunks in flight beside the 8 x 8 matrix, the per-state constants and 8 exps spill 159 VGPRs; 2 none */
        constexpr int D = (GAUSS && K >= 8) ? 2 : kFwdGroup;
        Obs grp[D][C];
#pragma unroll
        for (int i = 0; i < D; ++i)
            load_chunk<MODEL, C, AUX>(grp[i], sp, i * C);
        Em<K> ecur;
        emit_prob<MODEL, K, true>(ln.pp, ln.slab, ln.L, grp[0][0], ecur, ln.etab);
        int c = 0;
        for (; c + D <= nfull; c += D) {
            Obs nxt[D][C];
#pragma unroll
            for (int i = 0; i < D; ++i)
                load_chunk<MODEL, C, AUX>(nxt[i], sp, (c + D + i) * C);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                fwd_chunk<MODEL, K, C, MODE, true>(a, ln, c + i, grp[i],
                                                   (i + 1 < D) ? grp[i + 1 < D ? i + 1 : 0][0] : nxt[0][0], ecur, al,
                                                   lsc, ex);
                if constexpr (!GAUSS)
                    xcheck_acc<C, true>(xm, grp[i], c + i, ln.Tp);
            }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int u = 0; u < C; ++u)
                    grp[i][u] = nxt[i][u];
        }
#pragma unroll
        for (int u = 0; u < C; ++u)
            cur[u] = grp[0][u];
        for (; c < nchunk; ++c) {
            Obs nxt[C];
            load_chunk<MODEL, C, AUX>(nxt, sp, (c + 1) * C);
            fwd_chunk<MODEL, K, C, MODE, false>(a, ln, c, cur, nxt[0], ecur, al, lsc, ex);
            if constexpr (!GAUSS)
                xcheck_acc<C, false>(xm, cur, c, ln.Tp);
#pragma unroll
            for (int u = 0; u < C; ++u)
                cur[u] = nxt[u];
        }
        ll = log(vsum<K>(al)) + (lsc + kLn2 * ex);
    }

    /* ---- backward sweep, chunk by chunk from the end ---- */
    bool bad = !__builtin_isfinite(ll);
    const int clast = nchunk - 1;
    load_chunk<MODEL, C, AUX>(cur, sp, clast * C);
    /* checkpoint rows are wave-uniform: a lane shorter than the wave reads
     * (unused) slots past its own last chunk, never past the allocation */
    double ck[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        ck[k] = get_tmp(a.ckpt + a.P * ((int64_t)clast * K + k), (uint32_t)p * 8u);
    /* the caller's uniforms, prefetched one chunk ahead like the observations */
    double uu[C];
#pragma unroll
    for (int u = 0; u < C; ++u)
        uu[u] = at(a.ffbs_u + a.P * (int64_t)min(clast * C + u, a.Tmax - 1), (uint32_t)p * 8u);
    Obs onext = cur[0];
    int z = -1;      /* z_{t+1}, 0-based; -1: none yet, or undefined */
    int aux1 = 0;    /* g_1 / sign_1 */
    double x0 = 0.0; /* x_1 (Gaussian) */
    for (int c = clast; c >= 0; --c) {
        const int t0 = c * C;
        Obs nxt[C];
        load_chunk<MODEL, C, AUX>(nxt, sp, (c - 1) * C);
        double un[C];
#pragma unroll
        for (int u = 0; u < C; ++u)
            un[u] = at(a.ffbs_u + a.P * (int64_t)max((c - 1) * C + u, 0), (uint32_t)p * 8u);
        double cn[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            cn[k] = get_tmp(a.ckpt + a.P * ((int64_t)max(c - 1, 0) * K + k), (uint32_t)p * 8u);
        /* the filter over the chunk from its checkpoint (bwd_chunk's recompute) */
        double abuf[C][K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            abuf[0][k] = ck[k];
        {
            int exb = 0;
            Em<K> ecur;
            emit_prob<MODEL, K, true>(ln.pp, ln.slab, ln.L, cur[1 < C ? 1 : 0], ecur, ln.etab);
#pragma unroll
            for (int u = 1; u < C; ++u) {
                Em<K> enx;
                emit_prob<MODEL, K, true>(ln.pp, ln.slab, ln.L, cur[u + 1 < C ? u + 1 : u], enx, ln.etab);
                if (t0 + u < ln.Tp)
                    fwd_step_to<MODEL, K>(abuf[u - 1], abuf[u], ln.pp, ecur.e, cur[u], exb);
                ecur = enx;
            }
        }
        /* draws of steps t0 + C - 1 .. t0 */
#pragma unroll
        for (int u = C - 1; u >= 0; --u) {
            const int t = t0 + u;
            if (t < ln.Tp) {
                const Obs &on = (u + 1 < C) ? cur[u + 1 < C ? u + 1 : u] : onext;
                const bool last = t == ln.Tp - 1;
                bool m = true; /* the forward mask of step t + 1 at z_{t+1} */
                if constexpr (ModelTraits<MODEL>::kSemisup)
                    m = semisup_mask(on.aux, z);
                if constexpr (ModelTraits<MODEL>::kTayal)
                    m = tayal_pred(on.aux, z);
                const int zt = draw_step<MODEL, K>(ln.pp, abuf[u], last, m, z, uu[u]);
                bad |= zt < 0;
                if (zt >= 0) {
                    if constexpr (GAUSS) {
                        if (t > 0) { /* step 1 is every state's (x0 below) */
                            const double x = cur[u].xr;
                            double *const sk = ss + zt * (2 * 64);
                            sk[0] = sk[0] + x;
                            sk[64] = sk[64] + x * x;
                            count_one(ws + zt * 64);
                        }
                    } else {
                        const int xc = min(max(cur[u].x, 1), a.L);
                        count_one(cs + ((xc - 1) * K + zt) * 64);
                    }
                    /* not last: z >= 0, an undefined z_{t+1} is passed on */
                    if (!last && m)
                        count_one(xs + (zt * K + z) * 64);
                }
                z = zt;
            }
        }
        if (c == 0) {
            if constexpr (GAUSS)
                x0 = cur[0].xr;
            else
                aux1 = cur[0].aux;
        }
        onext = cur[0];
#pragma unroll
        for (int u = 0; u < C; ++u) {
            cur[u] = nxt[u];
            uu[u] = un[u];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = cn[k];
    }

    /* ---- the [P, ...] outputs ---- */
    const uint32_t po = (uint32_t)p * 8u;
    const double nanv = dev_nan();
    put_out(o.loglik, po, ll);
    bool p1 = true; /* Tayal: the init factor p_1k applies at (sign_1, z_1) */
    if constexpr (ModelTraits<MODEL>::kTayal)
        p1 = tayal_init_pred(aux1, z);
#pragma unroll
    for (int k = 0; k < K; ++k)
        put_out(o.n1 + a.P * (int64_t)k, po, bad ? nanv : ((z == k) & p1) ? 1.0 : 0.0);
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i)
            put_out(o.xi + a.P * (int64_t)(i + K * j), po, bad ? nanv : (double)xs[(i * K + j) * 64]);
    if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            put_out(o.w + a.P * (int64_t)k, po, bad ? nanv : 1.0 + (double)ws[k * 64]);
            put_out(o.s1 + a.P * (int64_t)k, po, bad ? nanv : x0 + ss[(2 * k) * 64]);
            put_out(o.s2 + a.P * (int64_t)k, po, bad ? nanv : x0 * x0 + ss[(2 * k + 1) * 64]);
        }
    } else {
        for (int l = 0; l < a.L; ++l) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                put_out(o.c + a.P * ((int64_t)k + (int64_t)K * l), po, bad ? nanv : (double)cs[(l * K + k) * 64]);
        }
    }
    if (o.status) {
        bool inv = !GAUSS && xm >= (uint32_t)a.L;
        if (a.T)
            inv |= a.T[n] < 1 || a.T[n] > a.Tmax;
        o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
    }
}

/* Bytes of LDS one wave needs: the emission table and the two count tables. */
static size_t draw_stats_wave_lds(int K, int L)
{
    return (size_t)L * (size_t)((K + 1) / 2) * 64 * sizeof(double2) +
           ((size_t)L * K + (size_t)K * K) * 64 * sizeof(uint32_t);
}

/* Waves per workgroup and its LDS. */
static int draw_stats_waves(int K, int L, size_t *lds) { return waves_that_fit(draw_stats_wave_lds(K, L), lds); }

/* Waves per workgroup and its LDS: of 4, 2 and 1 waves the size that lets a CU
 * (160 KiB) hold the most waves; the larger workgroup on a tie. */
static int draw_stats_gauss_waves(int K, size_t *lds)
{
    const size_t per_wave = draw_stats_gauss_wave_lds(K);
    int best = 1;
    size_t best_waves = 0;
    for (int w = kBlock / 64; w >= 1; w /= 2) {
        const size_t cu = kLdsLimit / (kExp2TabBytes + per_wave * w) * w;
        if (cu > best_waves) {
            best_waves = cu;
            best = w;
        }
    }
    *lds = kExp2TabBytes + per_wave * best;
    return best;
}

static bool draw_stats_model(int m)
{
    return m == HHMM_MODEL_HMM_MULTINOM || m == HHMM_MODEL_HMM_MULTINOM_SEMISUP || m == HHMM_MODEL_TAYAL;
}

hhmm_status check_draw_stats(const hhmm_request *r, const hhmm_estep_result *o)
{
    const hhmm_status s = stats_check_head("draw statistics", r, draw_stats_model,
                                           "hmm-multinom, hmm-multinom-semisup and hhmm-tayal2009 only; the Gaussian "
                                           "hmm has its own entry, hhmm_draw_stats_gauss");
    if (s != HHMM_OK)
        return s;
    if (r->data.K >= 1 && r->data.L >= 1) {
        size_t lds;
        if (draw_stats_waves(r->data.K, r->data.L, &lds) < 1) {
            set_error("draw statistics: L * (4 * ceil(K / 2) + K) + K * K = %d > 640: the emission table and the "
                      "count tables of one wave do not fit in LDS",
                      r->data.L * (4 * ((r->data.K + 1) / 2) + r->data.K) + r->data.K * r->data.K);
            return HHMM_ERR_UNSUPPORTED;
        }
    }
    return stats_check_tail("draw statistics", r, o, true);
}

static bool draw_stats_gauss_model(int m) { return m == HHMM_MODEL_HMM_GAUSS; }

hhmm_status check_draw_stats_gauss(const hhmm_request *r, const hhmm_estep_result *o)
{
    const hhmm_status s = stats_check_head("Gaussian draw statistics", r, draw_stats_gauss_model,
                                           "hmm only; the discrete programs go to hhmm_draw_stats");
    if (s != HHMM_OK) /* the tables of every K <= kMaxK fit in LDS */
        return s;
    return stats_check_tail("Gaussian draw statistics", r, o, true);
}

/* One model's launch on workgroups of `waves` waves; false: no kernel at a.K (Tayal is K = 4 only). */
template <int MODEL>
static bool launch_draw_stats_m(const DevArgs &a, const DrawStatsOutOf<MODEL> &o, int waves, size_t lds,
                                hipStream_t st)
{
    const int threads = 64 * waves;
    const dim3 grid((unsigned)((a.P + threads - 1) / threads)), block(threads);
    if constexpr (ModelTraits<MODEL>::kTayal) {
        if (a.K != 4)
            return false;
        hipLaunchKernelGGL((draw_stats_kernel<MODEL, 4>), grid, block, lds, st, a, o);
        return true;
    } else {
        return dispatch_k(a.K, [&](auto kc) {
            hipLaunchKernelGGL((draw_stats_kernel<MODEL, decltype(kc)::value>), grid, block, lds, st, a, o);
        });
    }
}

hhmm_status launch_draw_stats(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws, hipStream_t st)
{
    DevArgs a = stats_dev_args(r, P, ws);
    a.x = r->data.x_int;
    a.g = r->data.g;
    a.sign = r->data.sign;
    a.phi_k = r->draws.phi_k;
    a.p_11 = r->draws.p_11;
    a.A_row = r->draws.A_row;
    a.ffbs_u = r->ffbs_u;
    DrawStatsOut o{res->loglik, res->n_1k, res->xi_ij, res->c_kl, res->pair_status};
    size_t lds = 0;
    const int waves = draw_stats_waves(a.K, a.L, &lds);
    if (waves < 1) {
        set_error("draw statistics: the tables of K*L = %d*%d do not fit in LDS", a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    bool ok = false;
    if (a.model == HHMM_MODEL_HMM_MULTINOM)
        ok = launch_draw_stats_m<HHMM_MODEL_HMM_MULTINOM>(a, o, waves, lds, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        ok = launch_draw_stats_m<HHMM_MODEL_HMM_MULTINOM_SEMISUP>(a, o, waves, lds, st);
    else if (a.model == HHMM_MODEL_TAYAL)
        ok = launch_draw_stats_m<HHMM_MODEL_TAYAL>(a, o, waves, lds, st);
    if (!ok) {
        set_error("draw statistics: model %d at K = %d has no kernel (K outside 1..%d)", a.model, a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    return launch_status("draw_stats_kernel");
}

hhmm_status launch_draw_stats_gauss(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                    hipStream_t st)
{
    DevArgs a = stats_dev_args(r, P, ws);
    a.L = 0;
    a.xr = r->data.x_real;
    a.mu_k = r->draws.mu_k;
    a.sigma_k = r->draws.sigma_k;
    a.ffbs_u = r->ffbs_u;
    DrawStatsGaussOut o{res->loglik, res->n_1k, res->xi_ij, res->w_k, res->s1_k, res->s2_k, res->pair_status};
    size_t lds = 0;
    const int waves = draw_stats_gauss_waves(a.K, &lds);
    if (!launch_draw_stats_m<HHMM_MODEL_HMM_GAUSS>(a, o, waves, lds, st)) {
        set_error("Gaussian draw statistics: K = %d outside 1..%d", a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    return launch_status("draw_stats_kernel");
}

} // namespace hhmm
