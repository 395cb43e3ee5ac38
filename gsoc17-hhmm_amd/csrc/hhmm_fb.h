/*
 * hhmm_fb.h -- the forward-backward kernels of the HMM family.
 *   fb_kernel      A2/A1 emissions, A6 forward + loglik, A7 alpha, A8 backward,
 *                  A9 gamma, A12/A13 masks.  LINEAR-space
 *                  scaled recursion (K^2 FMAs per step, an exact power-of-two
 *                  renormalisation per step; no exp/log in the discrete loop);
 *                  forward checkpoints every C steps, recomputed chunk by chunk
 *                  in the backward sweep.  Tolerance 1e-9 rel.
 * Also the FB_BIG two-level backward sweep (bwd_block_big, fb_backward_big),
 * fb_sweep (shared with the parallel scan, hhmm_scan.h), fb_block and
 * fb_dense_kernel.
 */
#pragma once
#include "hhmm_fbchunk.h"

namespace hhmm {

/* FB_BIG applies to hmm-multinom's packed gamma profile with 8-step chunks. */
template <int MODEL, int K>
constexpr bool fb_big_ok()
{
    return fb_big_ok(MODEL, K);
}

/* Observation u of a kBigChunk-step block from its packed words (FB_PACK). */
__device__ __forceinline__ Obs unpack_obs(const uint32_t (&w)[kBigChunk / 8], int u)
{
    Obs o;
    o.x = (int)((w[u >> 3] >> (4 * (u & 7))) & 15u) + 1;
    o.aux = 0;
    o.xr = 0.0;
    return o;
}

/* One kBigChunk-step block of the FB_BIG backward sweep: pass 1 recomputes
 * the block's forward states from its checkpoint keeping every kGroup-th;
 * pass 2 takes the groups from the end, recomputes each group's states and
 * walks it backwards (posteriors, beta step).  go: the gamma rows' addressing
 * (TkIndexed, or a TkCursor standing on the block's last step t0 + B - 1: it
 * is stepped back once per step, predicated off or not, and left on t0 - 1). */
template <int MODEL, int K, int MODE, bool FULLB, typename GOUT>
__device__ __forceinline__ void bwd_block_big(const DevArgs &a, const FbLane<MODEL, K> &ln, int t0,
                                              const uint32_t (&w)[kBigChunk / 8], const double (&ck)[K],
                                              double (&be)[K], int &bex, GOUT &go)
{
    constexpr int B = kBigChunk, G = kGroup, NG = B / G;
    double ga[NG][K];
    double al[K];
    int exb = 0;
#pragma unroll
    for (int k = 0; k < K; ++k)
        al[k] = ga[0][k] = ck[k];
    /* pass 1; each step's emission row is fetched one step ahead, and a
     * scheduling barrier per step keeps the compiler from hoisting every
     * LDS read of the unrolled block into registers at once */
    Em<K> ecur, enx;
    emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, unpack_obs(w, 1), ecur);
#pragma unroll
    for (int u = 1; u < B; ++u) {
        if (u + 1 < B)
            emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, unpack_obs(w, u + 1 < B ? u + 1 : u), enx);
        if (FULLB || t0 + u < ln.Tp)
            fwd_step<MODEL, K>(al, ln.pp, ecur.e, unpack_obs(w, u), exb, u % fb_rp(MODE) == 0);
        if (u % G == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                ga[u / G][k] = al[k];
        }
        ecur = enx;
        __builtin_amdgcn_sched_barrier(0);
    }
    /* pass 2: emission rows re-read from LDS one step ahead (keeping a
     * group's rows in registers would cost 40 VGPRs) */
#pragma unroll
    for (int g = NG - 1; g >= 0; --g) {
        double gb[G][K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            gb[0][k] = ga[g][k];
        Em<K> e1, e2;
        emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, unpack_obs(w, g * G + 1), e1);
#pragma unroll
        for (int r = 1; r < G; ++r) {
            const int u = g * G + r;
            /* next: the following recompute step, or (after the last) the group's last step again */
            emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, unpack_obs(w, r + 1 < G ? u + 1 : g * G + G - 1), e2);
            if (FULLB || t0 + u < ln.Tp)
                fwd_step_to<MODEL, K>(gb[r - 1], gb[r], ln.pp, e1.e, unpack_obs(w, u), exb, u % fb_rp(MODE) == 0);
            e1 = e2;
        }
        /* e1 = emission of step g*G + G-1 */
#pragma unroll
        for (int r = G - 1; r >= 0; --r) {
            const int u = g * G + r;
            const int t = t0 + u;
            if (r > 0)
                emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, unpack_obs(w, r > 0 ? u - 1 : u), e2);
            if (FULLB || t < ln.Tp) {
                emit_posteriors<K, MODE>(a, ln.p, t, gb[r], be, 0.0, 0.0, go);
                if (t > ln.t0)
                    bwd_step<MODEL, K>(be, ln.pp, e1.e, unpack_obs(w, u), bex, u % fb_rp(MODE) == 0);
            }
            go.template advance<-1>();
            e1 = e2;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

/* FB_BIG backward sweep (gamma profile, packed symbols): kBigChunk-step
 * blocks from the end, each block's checkpoint and packed words prefetched
 * one block ahead. */
template <int MODEL, int K, int MODE>
__device__ __forceinline__ void fb_backward_big(const DevArgs &a, const FbLane<MODEL, K> &ln, int Tw_min, int Tw_max,
                                                double (&be)[K], int &bex)
{
    static_assert(fb_pack(MODE) && fb_base(MODE) == FB_GAMMA && !fb_ffbs(MODE), "FB_BIG: packed gamma profile");
    constexpr int B = kBigChunk, C = fb_chunk(K), NW = B / 8;
    static_assert(C == 8, "FB_BIG packs 8-step chunks");
    const int nblk = (Tw_max + B - 1) / B;
    const int nfullb = Tw_min / B;
    auto load_blk = [&](int blk, double (&ck)[K], uint32_t (&w)[NW]) {
        const int bb = max(blk, 0);
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = get_tmp(a.ckpt + ln.Qs * ((int64_t)bb * K + k), (uint32_t)ln.q * 8u);
#pragma unroll
        for (int i = 0; i < NW; ++i)
            w[i] = at(a.xpk + ln.Qs * (int64_t)(bb * NW + i), (uint32_t)ln.q * 4u);
    };
    double ck[K], ckn[K];
    uint32_t w[NW], wn[NW];
    TkIndexed go;
    load_blk(nblk - 1, ck, w);
    for (int blk = nblk - 1; blk >= 0; --blk) {
        load_blk(blk - 1, ckn, wn);
        if (blk < nfullb)
            bwd_block_big<MODEL, K, MODE, true>(a, ln, blk * B, w, ck, be, bex, go);
        else
            bwd_block_big<MODEL, K, MODE, false>(a, ln, blk * B, w, ck, be, bex, go);
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = ckn[k];
#pragma unroll
        for (int i = 0; i < NW; ++i)
            w[i] = wn[i];
    }
}

/* The forward-backward sweep of one lane over [ln.t0, ln.Tp): a whole series
 * (fb_kernel) or one T-chunk of the parallel scan (fb_scan_kernel, SURVEY §8
 * A16), which enters with the boundary vectors the scan computed: al = the
 * forward state f_{t0-1} (ignored at t0 = 0, where the model's init runs),
 * be = beta at the chunk's last step, with their log scales. */
template <int MODEL, int K, int MODE, bool SCAN, int PH = FB_PH_BOTH>
__device__ __forceinline__ void fb_sweep(const DevArgs &a, const FbLane<MODEL, K> &ln, const SeriesPtrs &sp,
                                         double (&al)[K], double lsc, double (&be)[K], double blsc)
{
    static_assert(PH == FB_PH_BOTH || (fb_big(MODE) && !SCAN), "split sweeps: FB_BIG gamma profile only");
    constexpr int C = fb_chunk(K);
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    const int64_t p = ln.p;
    const int Tw_min = wave_min(ln.Tp);
    const int Tw_max = wave_max(ln.Tp);
    const int nfull = Tw_min / C;              /* chunks complete for every lane */
    const int nchunk = (Tw_max + C - 1) / C;   /* chunks any lane needs */
    const int cb = ln.cb;

    Obs cur[C];
    if constexpr (PH != FB_PH_BWD) {
    /* ---- forward sweep ---- */
    int ex = 0;       /* sum of binary exponents removed */
    /* Full chunks go kFwdGroup at a time with the next group's observations
     * in flight: one chunk of forward steps (~40 VALU each) is far shorter
     * than an HBM round trip under load, so a one-chunk prefetch stalled
     * every chunk (the forward sweep alone measured 2.6 ms at C2 against
     * ~0.9 ms of issue).  The last, partial chunks keep the one-ahead loop. */
    constexpr int D = kFwdGroup;
    Obs grp[D][C];
#pragma unroll
    for (int i = 0; i < D; ++i)
        load_chunk<MODEL, C, AUX>(grp[i], sp, (cb + i) * C);
    Em<K> ecur;
    emit_prob<MODEL, K, fb_ffbs(MODE)>(ln.pp, ln.slab, ln.L, grp[0][0], ecur, ln.etab);
    /* whole-series sweeps over x alone check it inline (xcheck_acc) */
    constexpr bool XCHK = !SCAN && !AUX && ModelTraits<MODEL>::kDiscrete;
    uint32_t xm = 0;
    int c = cb;
    for (; c + D <= nfull; c += D) {
        Obs nxt[D][C];
#pragma unroll
        for (int i = 0; i < D; ++i)
            load_chunk<MODEL, C, AUX>(nxt[i], sp, (c + D + i) * C);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            fwd_chunk<MODEL, K, C, MODE, true>(a, ln, c + i, grp[i], (i + 1 < D) ? grp[i + 1 < D ? i + 1 : 0][0]
                                                                              : nxt[0][0], ecur, al, lsc, ex);
            if constexpr (XCHK)
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
    for (; c < nchunk; ++c) { /* < D full chunks, then the partial ones (one code copy) */
        Obs nxt[C];
        load_chunk<MODEL, C, AUX>(nxt, sp, (c + 1) * C);
        fwd_chunk<MODEL, K, C, MODE, false>(a, ln, c, cur, nxt[0], ecur, al, lsc, ex);
        if constexpr (XCHK)
            xcheck_acc<C, false>(xm, cur, c, ln.Tp);
#pragma unroll
        for (int u = 0; u < C; ++u)
            cur[u] = nxt[u];
    }
    if constexpr (XCHK)
        if (a.dc_flag && xm >= (uint32_t)ln.L)
            a.dc_flag[ln.n] = 1;
    if (!SCAN && (a.outputs & HHMM_OUT_LOGLIK) && a.loglik)
        a.loglik[p] = log(vsum<K>(al)) + (lsc + kLn2 * ex);
    } /* forward sweep */
    if constexpr (fb_base(MODE) == FB_FWD || PH == FB_PH_FWD)
        return;

    /* ---- backward sweep, chunk by chunk from the end ---- */
    int bex = 0;
    if constexpr (fb_big(MODE)) {
        fb_backward_big<MODEL, K, MODE>(a, ln, Tw_min, Tw_max, be, bex);
        return;
    }
    const int clast = nchunk - 1;
    /* observations of chunk cc: x itself, or the packed record of the forward sweep */
    auto obs_chunk = [&](Obs (&dst)[C], int cc) {
        if constexpr (fb_pack(MODE)) {
            const uint32_t w = at(a.xpk + ln.Qs * (int64_t)(max(cc, cb) - cb), (uint32_t)ln.q * 4u);
#pragma unroll
            for (int v = 0; v < C; ++v) {
                dst[v].x = (int)((w >> (4 * v)) & 15u) + 1;
                dst[v].aux = 0;
                dst[v].xr = 0.0;
            }
        } else {
            load_chunk<MODEL, C, AUX>(dst, sp, cc * C);
        }
    };
    obs_chunk(cur, clast);
    /* checkpoint rows are wave-uniform: a lane shorter than the wave reads
     * (unused) slots past its own last chunk, never past the allocation */
    double ck[K], ck_ls = 0.0;
    {
        const int cc = clast - cb;
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = get_tmp(a.ckpt + ln.Qs * ((int64_t)cc * K + k), (uint32_t)ln.q * 8u);
        if constexpr (fb_base(MODE) == FB_FULL)
            ck_ls = get_tmp(a.ckpt_ls + ln.Qs * (int64_t)cc, (uint32_t)ln.q * 8u);
    }
    /* FFBS: the caller's uniforms, prefetched one chunk ahead like the observations */
    double uu[fb_ffbs(MODE) ? C : 1], un[fb_ffbs(MODE) ? C : 1];
    if constexpr (fb_ffbs(MODE)) {
#pragma unroll
        for (int u = 0; u < C; ++u)
            uu[u] = at(a.ffbs_u + a.P * (int64_t)min(clast * C + u, a.Tmax - 1), (uint32_t)p * 8u);
    }
    Obs onext = cur[0];
    int z = -1;
    for (int c = clast; c >= cb; --c) {
        Obs nxt[C];
        obs_chunk(nxt, c - 1);
        if constexpr (fb_ffbs(MODE)) {
#pragma unroll
            for (int u = 0; u < C; ++u)
                un[u] = at(a.ffbs_u + a.P * (int64_t)max((c - 1) * C + u, 0), (uint32_t)p * 8u);
        }
        double cn[K], cn_ls = 0.0;
        {
            const int cc = max(c - 1, cb) - cb;
#pragma unroll
            for (int k = 0; k < K; ++k)
                cn[k] = get_tmp(a.ckpt + ln.Qs * ((int64_t)cc * K + k), (uint32_t)ln.q * 8u);
            if constexpr (fb_base(MODE) == FB_FULL)
                cn_ls = get_tmp(a.ckpt_ls + ln.Qs * (int64_t)cc, (uint32_t)ln.q * 8u);
        }
        if (c < nfull)
            bwd_chunk<MODEL, K, C, MODE, true>(a, ln, c, cur, ck, ck_ls, be, blsc, bex, uu, onext, z);
        else
            bwd_chunk<MODEL, K, C, MODE, false>(a, ln, c, cur, ck, ck_ls, be, blsc, bex, uu, onext, z);
        onext = cur[0];
#pragma unroll
        for (int u = 0; u < C; ++u)
            cur[u] = nxt[u];
        if constexpr (fb_ffbs(MODE)) {
#pragma unroll
            for (int u = 0; u < C; ++u)
                uu[u] = un[u];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = cn[k];
        ck_ls = cn_ls;
    }
}

/* One wave of the forward-backward: pairs [64 gwave, 64 gwave + 64) (gwave =
 * block * waves per block + wave in fb_kernel). */
template <int MODEL, int K, int MODE, int PH>
__device__ __forceinline__ void fb_block(const DevArgs &a, int64_t gwave, const hhmm_exp2_entry *etab = hhmm_exp2_tab)
{
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    /* lanes past the last pair redo pair P-1 (identical values, benign
     * duplicate stores): every lane stays in the wave-wide reductions */
    const int64_t p = min(gwave * 64 + lane, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    constexpr int KP = (K + 1) / 2;

    FbLane<MODEL, K> ln;
    ln.p = p;
    ln.n = n;
    ln.L = a.L;
    ln.t0 = 0;
    ln.Tp = pair_len(a, n);
    ln.cb = 0;
    ln.q = p;
    ln.Qs = a.P;
    ln.slab = lds + (size_t)wave * a.L * KP * 64 + lane;
    ln.etab = etab;
    load_params<MODEL, K, false>(ln.pp, a, d);
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        ln.pp.skip_ok &= fill_table<K, false>(lds + (size_t)wave * a.L * KP * 64 + lane, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);
    double al[K], be[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        al[k] = 0.0;
        be[k] = 1.0; /* unbeta_tk[T] = 1 (Q1): beta_T uniform */
    }
    if constexpr (fb_big(MODE) && !(MODE & FB_RN1)) {
        const bool dense = wave_any(!renorm_sparse_safe<MODEL, K>(ln.pp, ln.slab, a.L));
        if constexpr (PH == FB_PH_BOTH) {
            /* a wave holding a pair without the bound appends itself to the
             * list a.rnw (count, then wave ids) and leaves its sweep to
             * fb_dense_kernel (per-step renormalisation), launched right after
             * this kernel: the hot kernel carries one copy of the sweep */
            if (dense) {
                if (lane == 0) {
                    const int slot = atomicAdd(&a.rnw[0], 1);
                    a.rnw[1 + slot] = (int32_t)gwave;
                }
                return;
            }
        } else if (dense) { /* the split schedule's two launches decide alike */
            fb_sweep<MODEL, K, MODE | FB_RN1, false, PH>(a, ln, sp, al, 0.0, be, 0.0);
            return;
        }
    }
    fb_sweep<MODEL, K, MODE, false, PH>(a, ln, sp, al, 0.0, be, 0.0);
}

/* The FB_BIG waves fb_kernel listed in a.rnw, with per-step renormalisation:
 * one-wave workgroups (one emission slab each) take list entries in turn;
 * with none listed the launch reads the count and ends. */
constexpr int kDenseBlocks = 256;
template <int MODEL, int K, int MODE>
__global__ void __launch_bounds__(64) fb_dense_kernel(const DevArgs a)
{
    const int n = __builtin_amdgcn_readfirstlane(a.rnw[0]);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t gw = __builtin_amdgcn_readfirstlane(a.rnw[1 + i]);
        fb_block<MODEL, K, MODE | FB_RN1, FB_PH_BOTH>(a, gw);
    }
}

template <int MODEL, int K, int MODE, int PH = FB_PH_BOTH>
__global__ void __launch_bounds__(kBlock) fb_kernel(const DevArgs a)
{
    const hhmm_exp2_entry *etab = hhmm_exp2_tab;
    if constexpr (fb_exp2_lds<MODEL, MODE>()) {
        HIP_DYNAMIC_SHARED(hhmm_exp2_entry, t)
        for (int i = threadIdx.x; i < 128; i += blockDim.x)
            t[i] = hhmm_exp2_tab[i];
        __syncthreads();
        etab = t;
    }
    fb_block<MODEL, K, MODE, PH>(a, (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), etab);
}

} // namespace hhmm
