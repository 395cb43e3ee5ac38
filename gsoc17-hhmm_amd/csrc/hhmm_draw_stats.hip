/*
 * hhmm_draw_stats.hip -- gfx950 kernel of the draw statistics
 * (include/hhmm_gibbs.h): per (series, draw) pair one FFBS path z, reduced to
 * the counts a conjugate parameter update needs -- z_1, the transitions and the
 * (state, symbol) pairs -- for hmm-multinom, semisup and Tayal at K <= 8.
 * Nothing is written per step.
 *
 * One LANE owns one pair (the layout and latency rules of hhmm_step.h, the
 * chunk helpers of hhmm_fbchunk.h).
 *   forward   the FFBS contract's filter, the operations of
 *             fb_kernel<.., FB_GAMMA | FB_FFBS> (fwd_chunk: per-step
 *             renormalisation, emit_prob<.., true>): a checkpoint every
 *             C = fb_chunk(K) steps, loglik at the end.
 *   backward  chunk by chunk from the end: the filter over the chunk is
 *             recomputed from its checkpoint (bit-identical), z_t
 *             drawn by ffbs_draw's operations (draw_step) from u[p, t], the
 *             counts taken.  No beta, no gamma, no reciprocal.
 * Accumulators: z_t is a run-time index, so nothing is indexed by it in
 * registers (that becomes scratch).  Both count tables are 32-bit slabs in LDS,
 * lane-fastest (64 consecutive words = every bank once: conflict-free):
 *     c_kl   cs[((l - 1) * K + k) * 64 + lane]
 *     xi_ij  xs[(i * K + j) * 64 + lane]
 * each step is one ds_add_u32 into each (K^2 compare-and-add registers cost
 * 2 K^2 VALU per step on the dependent chain of the draw and, at K = 8, 64
 * VGPRs).  A count is at most T_max < 2^31.  n_1k comes from z_1 at the end.
 * LDS per wave: L * (1024 ceil(K/2) + 256 K) + 256 K^2 bytes; the workgroup is
 * sized to fit 160 KiB.
 * The [P, ...] stores are pair-fastest: one coalesced wave transaction each.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_gibbs.h"
#include "hhmm_fbchunk.h"
#include "hhmm_drawstep.h"
#include "hhmm_stats.h"

namespace hhmm {

struct DrawStatsOut {
    double *loglik, *n1, *xi, *c;
    int32_t *status;
};

/* count_one and draw_step (the FFBS step on opaque copies of A: no scratch)
 * are in hhmm_drawstep.h, shared with the Gaussian kernel. */

template <int MODEL, int K>
__global__ void __launch_bounds__(kBlock) draw_stats_kernel(const DevArgs a, const DrawStatsOut o)
{
    constexpr int C = fb_chunk(K);
    constexpr int KP = (K + 1) / 2;
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    constexpr int MODE = FB_GAMMA | FB_FFBS;
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
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
    const size_t slab_elems = (size_t)a.L * KP * 64;
    const size_t cnt_words = ((size_t)a.L * K + K * K) * 64;
    double2 *const pslab = lds + (size_t)wave * slab_elems + lane;
    uint32_t *const cs = reinterpret_cast<uint32_t *>(lds + (size_t)nw * slab_elems) + (size_t)wave * cnt_words + lane;
    uint32_t *const xs = cs + (size_t)a.L * K * 64;
    ln.slab = pslab;
    load_params<MODEL, K, false>(ln.pp, a, d);
    ln.pp.skip_ok &= fill_table<K, false>(pslab, a, d);
    for (int i = 0; i < a.L * K + K * K; ++i)
        cs[i * 64] = 0u;
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
        constexpr int D = kFwdGroup;
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
    int z = -1;    /* z_{t+1}, 0-based; -1: none yet, or undefined */
    int aux1 = 0;  /* g_1 / sign_1 */
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
                    const int xc = min(max(cur[u].x, 1), a.L);
                    count_one(cs + ((xc - 1) * K + zt) * 64);
                    /* not last: z >= 0, an undefined z_{t+1} is passed on */
                    if (!last && m)
                        count_one(xs + (zt * K + z) * 64);
                }
                z = zt;
            }
        }
        if (c == 0)
            aux1 = cur[0].aux;
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
    for (int l = 0; l < a.L; ++l) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            put_out(o.c + a.P * ((int64_t)k + (int64_t)K * l), po, bad ? nanv : (double)cs[(l * K + k) * 64]);
    }
    if (o.status) {
        bool inv = xm >= (uint32_t)a.L;
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

template <int MODEL, int K>
static void launch_draw_stats_k(const DevArgs &a, const DrawStatsOut &o, dim3 grid, dim3 block, size_t lds,
                                hipStream_t st)
{
    hipLaunchKernelGGL((draw_stats_kernel<MODEL, K>), grid, block, lds, st, a, o);
}

template <int MODEL>
static bool launch_draw_stats_m(const DevArgs &a, const DrawStatsOut &o, dim3 grid, dim3 block, size_t lds,
                                hipStream_t st)
{
    return dispatch_k(a.K, [&](auto kc) {
        launch_draw_stats_k<MODEL, decltype(kc)::value>(a, o, grid, block, lds, st);
    });
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
    const int threads = 64 * waves;
    const dim3 grid((unsigned)((P + threads - 1) / threads)), block(threads);
    bool ok = false;
    if (a.model == HHMM_MODEL_HMM_MULTINOM)
        ok = launch_draw_stats_m<HHMM_MODEL_HMM_MULTINOM>(a, o, grid, block, lds, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        ok = launch_draw_stats_m<HHMM_MODEL_HMM_MULTINOM_SEMISUP>(a, o, grid, block, lds, st);
    else if (a.model == HHMM_MODEL_TAYAL && a.K == 4) {
        launch_draw_stats_k<HHMM_MODEL_TAYAL, 4>(a, o, grid, block, lds, st);
        ok = true;
    }
    if (!ok) {
        set_error("draw statistics: model %d at K = %d has no kernel (K outside 1..%d)", a.model, a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    return launch_status("draw_stats_kernel");
}

} // namespace hhmm
