/*
 * hhmm_draw_stats_gauss.hip -- gfx950 kernel of the Gaussian draw statistics
 * (include/hhmm_gibbs_gauss.h): per (series, draw) pair one FFBS path z of
 * hmm/stan/hmm.stan, reduced to the statistics the conjugate update needs --
 * z_1, the transitions, and per state the count, the sum and the sum of squares
 * of the observations it owns -- at K <= 8.  Nothing is written per step.
 *
 * One LANE owns one pair; the schedule is draw_stats_kernel's
 * (hhmm_draw_stats.hip):
 *   forward   fwd_chunk<HMM_GAUSS, K, C, FB_GAMMA | FB_FFBS>: the FFBS
 *             contract's filter (emit_prob<.., true>, hhmm_det_exp_tab on the
 *             workgroup's LDS copy of the 2^(j/128) table, as fb_kernel does
 *             under fb_exp2_lds), a checkpoint every C = fb_chunk(K) steps,
 *             loglik at the end.
 *   backward  chunk by chunk from the end: the filter over the chunk is
 *             recomputed from its checkpoint (bit-identical), z_t drawn by
 *             draw_step from u[p, t], the statistics taken.
 * Accumulators: z_t is a run-time index, so nothing is indexed by it in
 * registers.  Four lane-fastest LDS slabs per wave (64 consecutive words:
 * every bank once):
 *     s1, s2  ss[(2 k + {0, 1}) * 64 + lane]   fp64, read-add-write: the words
 *                                             are private to their lane
 *     w       ws[k * 64 + lane]               32-bit, one ds_add_u32 per step
 *     xi      xs[(i * K + j) * 64 + lane]     32-bit, one ds_add_u32 per step
 * Step 1 (Q2, hmm.stan:30) belongs to every state: x_1 is added once per
 * state at the end, as estep_kernel does with x0; n_1k comes from z_1.
 * LDS: the table (2 KiB per workgroup) + (K + K^2) * 256 + 2 K * 512 bytes per
 * wave; draw_stats_gauss_waves sizes the workgroup for the most waves per CU.
 * The [P, ...] stores are pair-fastest: one coalesced wave transaction each.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_gibbs_gauss.h"
#include "hhmm_fbchunk.h"
#include "hhmm_drawstep.h"
#include "hhmm_stats.h"

namespace hhmm {

struct DrawStatsGaussOut {
    double *loglik, *n1, *xi, *w, *s1, *s2;
    int32_t *status;
};

/* Bytes of LDS one wave needs: s1 / s2 (fp64), then w and xi (32-bit). */
constexpr size_t draw_stats_gauss_wave_lds(int K)
{
    return (size_t)2 * K * 64 * sizeof(double) + ((size_t)K + (size_t)K * K) * 64 * sizeof(uint32_t);
}

template <int K>
__global__ void __launch_bounds__(kBlock) draw_stats_gauss_kernel(const DevArgs a, const DrawStatsGaussOut o)
{
    constexpr int MODEL = HHMM_MODEL_HMM_GAUSS;
    constexpr int C = fb_chunk(K);
    constexpr int MODE = FB_GAMMA | FB_FFBS;
    HIP_DYNAMIC_SHARED(hhmm_exp2_entry, etab)
    static_assert(kExp2TabBytes % sizeof(double) == 0, "the fp64 slabs follow the table");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < 128; i += blockDim.x)
        etab[i] = hhmm_exp2_tab[i];
    /* every fp64 slab first, then the count slabs */
    double *const slabs = reinterpret_cast<double *>(etab + 128);
    double *const ss = slabs + (size_t)wave * (2 * K * 64) + lane;
    uint32_t *const ws =
        reinterpret_cast<uint32_t *>(slabs + (size_t)nw * (2 * K * 64)) + (size_t)wave * ((K + K * K) * 64) + lane;
    uint32_t *const xs = ws + K * 64;
#pragma unroll
    for (int i = 0; i < 2 * K; ++i)
        ss[i * 64] = 0.0;
#pragma unroll
    for (int i = 0; i < K + K * K; ++i)
        ws[i * 64] = 0u;
    __syncthreads();

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
    ln.slab = nullptr;
    ln.etab = etab;
    load_params<MODEL, K, false>(ln.pp, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, false>(a, n);
    const int Tw_min = wave_min(ln.Tp);
    const int Tw_max = wave_max(ln.Tp);
    const int nfull = Tw_min / C;            /* chunks complete for every lane */
    const int nchunk = (Tw_max + C - 1) / C; /* chunks any lane needs: <= ceil(Tmax / C) checkpoint rows */

    /* ---- forward sweep: fb_kernel's FFBS filter, checkpoints only ---- */
    double ll;
    Obs cur[C];
    {
        double al[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            al[k] = 0.0;
        double lsc = 0.0;
        int ex = 0;
        /* chunks per observation prefetch group (the grouping changes no bit):
         * at K = 8 kFwdGroup = 4 chunks in flight beside the 8 x 8 matrix, the
         * per-state constants and 8 exps spill 159 VGPRs; 2 spill none */
        constexpr int D = K >= 8 ? 2 : kFwdGroup;
        Obs grp[D][C];
#pragma unroll
        for (int i = 0; i < D; ++i)
            load_chunk<MODEL, C, false>(grp[i], sp, i * C);
        Em<K> ecur;
        emit_prob<MODEL, K, true>(ln.pp, ln.slab, ln.L, grp[0][0], ecur, ln.etab);
        int c = 0;
        for (; c + D <= nfull; c += D) {
            Obs nxt[D][C];
#pragma unroll
            for (int i = 0; i < D; ++i)
                load_chunk<MODEL, C, false>(nxt[i], sp, (c + D + i) * C);
#pragma unroll
            for (int i = 0; i < D; ++i)
                fwd_chunk<MODEL, K, C, MODE, true>(a, ln, c + i, grp[i],
                                                   (i + 1 < D) ? grp[i + 1 < D ? i + 1 : 0][0] : nxt[0][0], ecur, al,
                                                   lsc, ex);
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
            load_chunk<MODEL, C, false>(nxt, sp, (c + 1) * C);
            fwd_chunk<MODEL, K, C, MODE, false>(a, ln, c, cur, nxt[0], ecur, al, lsc, ex);
#pragma unroll
            for (int u = 0; u < C; ++u)
                cur[u] = nxt[u];
        }
        ll = log(vsum<K>(al)) + (lsc + kLn2 * ex);
    }

    /* ---- backward sweep, chunk by chunk from the end ---- */
    bool bad = !__builtin_isfinite(ll);
    const int clast = nchunk - 1;
    load_chunk<MODEL, C, false>(cur, sp, clast * C);
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
    int z = -1;      /* z_{t+1}, 0-based; -1: none yet, or undefined */
    double x0 = 0.0; /* x_1 */
    for (int c = clast; c >= 0; --c) {
        const int t0 = c * C;
        Obs nxt[C];
        load_chunk<MODEL, C, false>(nxt, sp, (c - 1) * C);
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
                const bool last = t == ln.Tp - 1;
                const int zt = draw_step<MODEL, K>(ln.pp, abuf[u], last, true, z, uu[u]);
                bad |= zt < 0;
                if (zt >= 0) {
                    if (t > 0) { /* step 1 is every state's (x0 below) */
                        const double x = cur[u].xr;
                        double *const sk = ss + zt * (2 * 64);
                        sk[0] = sk[0] + x;
                        sk[64] = sk[64] + x * x;
                        count_one(ws + zt * 64);
                    }
                    /* not last: z >= 0, an undefined z_{t+1} is passed on */
                    if (!last)
                        count_one(xs + (zt * K + z) * 64);
                }
                z = zt;
            }
        }
        if (c == 0)
            x0 = cur[0].xr;
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
#pragma unroll
    for (int k = 0; k < K; ++k)
        put_out(o.n1 + a.P * (int64_t)k, po, bad ? nanv : (z == k) ? 1.0 : 0.0);
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i)
            put_out(o.xi + a.P * (int64_t)(i + K * j), po, bad ? nanv : (double)xs[(i * K + j) * 64]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        put_out(o.w + a.P * (int64_t)k, po, bad ? nanv : 1.0 + (double)ws[k * 64]);
        put_out(o.s1 + a.P * (int64_t)k, po, bad ? nanv : x0 + ss[(2 * k) * 64]);
        put_out(o.s2 + a.P * (int64_t)k, po, bad ? nanv : x0 * x0 + ss[(2 * k + 1) * 64]);
    }
    if (o.status) {
        bool inv = false;
        if (a.T)
            inv = a.T[n] < 1 || a.T[n] > a.Tmax;
        o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
    }
}

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

static bool draw_stats_gauss_model(int m) { return m == HHMM_MODEL_HMM_GAUSS; }

hhmm_status check_draw_stats_gauss(const hhmm_request *r, const hhmm_estep_result *o)
{
    const hhmm_status s = stats_check_head("Gaussian draw statistics", r, draw_stats_gauss_model,
                                           "hmm only; the discrete programs go to hhmm_draw_stats");
    if (s != HHMM_OK) /* the tables of every K <= kMaxK fit in LDS */
        return s;
    return stats_check_tail("Gaussian draw statistics", r, o, true);
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
    if (a.K < 1 || a.K > kMaxK) {
        set_error("Gaussian draw statistics: K = %d outside 1..%d", a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    size_t lds = 0;
    const int threads = 64 * draw_stats_gauss_waves(a.K, &lds);
    const dim3 grid((unsigned)((P + threads - 1) / threads)), block(threads);
    dispatch_k(a.K, [&](auto kc) {
        hipLaunchKernelGGL((draw_stats_gauss_kernel<decltype(kc)::value>), grid, block, lds, st, a, o);
    });
    return launch_status("draw_stats_gauss_kernel");
}

} // namespace hhmm
