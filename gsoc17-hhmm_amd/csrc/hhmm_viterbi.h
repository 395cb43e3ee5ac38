/*
 * hhmm_viterbi.h -- the sequential Viterbi decoders of the HMM family.
 *   viterbi_kernel    A11 max-plus recursion in LOG space with
 *                     exactly the reference's operation order and tie rules,
 *                     log tables from the correctly rounded hhmm_cr_log
 *                     (bit-identical to the oracle); back-pointers packed
 *                     2 bits/state to HBM, backtrack in the same kernel.
 *                     Bit-exact.  One lane per pair.
 *   viterbi_sp_kernel the state-parallel decoder for few pairs with long
 *                     series: one lane per (pair, state).
 * Build with -ffp-contract=off: the Viterbi sums must round exactly as written.
 */
#pragma once
#include "hhmm_fb.h"

namespace hhmm {

/* ------------------------------------------------------------------ */
/* Viterbi                                                                */
/* ------------------------------------------------------------------ */

/* Log emission of state j at one step, bit-identical to the reference. */
template <int MODEL, int K>
__device__ __forceinline__ void emit_log(const PairParams<MODEL, K> &pp, const double2 *slab, int L,
                                         const Obs &o, double (&le)[K])
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            le[j] = gauss_lpdf<MODEL, K>(pp, o.xr, j);
    } else {
        read_table<K>(slab, o.x, L, le);
    }
}


/* One max-plus step t >= 1: delta_t(j) = max_i cand(i, j) with the
 * reference's strict '>' from -inf (first maximising i wins, NaN never
 * wins); back-pointer i packed into `word` at `slot`.
 * VALU form: the running max is one v_max_f64 (maxNum: a NaN candidate
 * leaves it unchanged, and an equal one leaves its value unchanged) and the
 * back-pointer one select on the strict compare, so each candidate costs
 * 2 adds + cmp + max + select.  Value-identical to the reference loop; the
 * back-pointer differs only where every candidate is -inf / NaN (the
 * reference leaves it unset, here 0), which the epilogue flags through
 * delta_T = -inf exactly as before. */
template <int MODEL, int K, bool NANIN = false>
__device__ __forceinline__ void vit_step(double (&dl)[K], const PairParams<MODEL, K> &pp, const double (&le)[K],
                                         const Obs &o, uint32_t &word, int slot)
{
    /* NANIN: delta_{t-1} may hold NaN -- only the step after the t = 1 row of
     * Q3.  Every later delta is a max over non-NaN candidates (delta_{t-1}
     * comes out of an fmax from -inf, and the callers' log A and log
     * emissions hold no NaN: load_vit_params, fill_table<.., VIT>), so the
     * running max can start from the first candidate instead of from
     * fmax(-inf, candidate).  It must not with a NaN candidate 0: the next
     * candidate would take the value through fmax but, failing `>` against
     * NaN, not the back-pointer. */
    constexpr int BITS = bp_bits(K);
    constexpr int STEPB = K * BITS;
    double nd[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bool on = true;
        if constexpr (ModelTraits<MODEL>::kTayal)
            on = tayal_pred(o.aux, j);
        const int sh = slot * STEPB + j * BITS;
        double best = dev_ninf();
        uint32_t argsh = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double cand;
            if constexpr (ModelTraits<MODEL>::kTayal) {
                /* (delta + log phi) [+ log A] (hhmm-tayal2009.stan:143-146) */
                cand = dl[i] + le[j];
                cand = on ? cand + pp.A[i][j] : cand;
            } else {
                /* (delta + log A) + emission (hmm.stan:111) */
                cand = (dl[i] + pp.A[i][j]) + le[j];
            }
            if (i == 0) {
                best = NANIN ? fmax(best, cand) : cand;
            } else {
                const bool gt = cand > best;
                best = fmax(best, cand);
                argsh = gt ? ((uint32_t)i << sh) : argsh;
            }
        }
        nd[j] = best;
        word |= argsh;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        dl[j] = nd[j];
}

/* Where a chunk's finished back-pointer words go: BpIndexed rebuilds the row
 * pointer from the word's row; BpCursor is a running row pointer that stands
 * on the next word's row and moves on with every word -- for chunks every lane
 * of the wave runs in full (FULLC) only, where each word is stored by the
 * whole wave, so the cursor's moves stay wave-uniform. */
struct BpIndexed {
    static constexpr bool kUniformOnly = false;
    __device__ __forceinline__ void put(const DevArgs &a, int64_t p, int row, uint32_t word)
    {
        put_tmp(a.bp + a.P * (int64_t)row, (uint32_t)p * 4u, word);
    }
};
struct BpCursor {
    static constexpr bool kUniformOnly = true;
    RowCursor<uint32_t> c;
    __device__ __forceinline__ BpCursor(const DevArgs &a, int64_t p, int row) : c(a.bp, a.P, row, p) {}
    __device__ __forceinline__ void put(const DevArgs &, int64_t, int, uint32_t word)
    {
        c.put_tmp(word);
        c.advance<1>();
    }
};

template <int MODEL, int K, int CV, bool FULLC, bool FIRST = false, typename WOUT>
__device__ __forceinline__ void vit_fwd_chunk(const DevArgs &a, int64_t p, const PairParams<MODEL, K> &pp,
                                              const double2 *slab, int Tp, int c, const Obs (&cur)[CV],
                                              const Obs &nxt0, double (&le)[K], double (&dl)[K], uint32_t &word,
                                              WOUT &wo)
{
    static_assert(FULLC || !WOUT::kUniformOnly, "a word cursor needs chunks the whole wave runs in full");
    constexpr int SPW = bp_steps_per_word(K);
    const int t0 = c * CV;
#pragma unroll
    for (int u = 0; u < CV; ++u) {
        const int t = t0 + u;
        double ln[K];
        emit_log<MODEL, K>(pp, slab, a.L, (u + 1 < CV) ? cur[u + 1 < CV ? u + 1 : 0] : nxt0, ln);
        if (FULLC || t < Tp) {
            /* FIRST: chunk 0, whose step 0 is the init row and step 1 the NaN step */
            if (FIRST && u == 1)
                vit_step<MODEL, K, true>(dl, pp, le, cur[u], word, u % SPW);
            else if (!(FIRST && u == 0))
                vit_step<MODEL, K, false>(dl, pp, le, cur[u], word, u % SPW);
            if (u % SPW == SPW - 1) {
                wo.put(a, p, t / SPW, word);
                word = 0;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            le[k] = ln[k];
    }
}
template <int MODEL, int K, int CV, bool FULLC, bool FIRST = false>
__device__ __forceinline__ void vit_fwd_chunk(const DevArgs &a, int64_t p, const PairParams<MODEL, K> &pp,
                                              const double2 *slab, int Tp, int c, const Obs (&cur)[CV],
                                              const Obs &nxt0, double (&le)[K], double (&dl)[K], uint32_t &word)
{
    BpIndexed wo;
    vit_fwd_chunk<MODEL, K, CV, FULLC, FIRST>(a, p, pp, slab, Tp, c, cur, nxt0, le, dl, word, wo);
}

/* One workgroup of the Viterbi decoder: pairs [block * blockDim, +blockDim).
 * PK: the observations come from the packed symbol words the split
 * schedule's forward launch wrote (a.xpk: one 4-bit symbol per step, one word
 * per 8-step chunk; hmm-multinom, L <= 16), 0.5 instead of 4 bytes per step. */
template <int MODEL, int K, bool PK = false>
__device__ __forceinline__ void viterbi_block(const DevArgs &a, uint32_t block)
{
    constexpr int CV = vit_chunk(K);
    constexpr bool VAUX = ModelTraits<MODEL>::kTayal; /* semisup Viterbi is unmasked (Q7) */
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t p = min((int64_t)block * blockDim.x + threadIdx.x, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);
    constexpr int KP = (K + 1) / 2;
    double2 *slab = lds + (size_t)wave * a.L * KP * 64 + lane;

    PairParams<MODEL, K> pp;
    load_vit_params<MODEL, K>(pp, a, d);
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        fill_table<K, true, true>(slab, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, VAUX>(a, n);
    static_assert(!PK || (!VAUX && !ModelTraits<MODEL>::kGauss && CV == 8), "packed symbols: 8-step chunks, x only");
    const int pkrows = (a.Tmax + CV - 1) / CV;
    auto vload = [&](Obs (&dst)[CV], const SeriesPtrs &s, int t0) {
        if constexpr (PK) {
            /* rows past a lane's own length hold padding that is never consumed */
            const int cc = min(max(t0 / CV, 0), pkrows - 1);
            const uint32_t w = at(a.xpk + a.P * (int64_t)cc, (uint32_t)p * 4u);
#pragma unroll
            for (int v = 0; v < CV; ++v) {
                dst[v].x = (int)((w >> (4 * v)) & 15u) + 1;
                dst[v].aux = 0;
                dst[v].xr = 0.0;
            }
        } else {
            load_chunk<MODEL, CV, VAUX>(dst, s, t0);
        }
    };
    const int Tw_min = wave_min(Tp);
    const int Tw_max = wave_max(Tp);
    const int nfull = Tw_min / CV;
    const int nchunk = (Tw_max + CV - 1) / CV;

    /* delta_tk[1, K] = emission of j for j = 1..K: only column K is written,
     * the others keep stanc's NaN (Q3, e.g. hmm-multinom.stan:105-106). */
    double dl[K];
    Obs cur[CV];
    vload(cur, sp, 0);
    /* chunks 1.. go kVitGroup at a time with the next group's observations in
     * flight (a one-chunk prefetch is shorter than an HBM round trip) */
    constexpr int D = kVitGroup;
    Obs grp[D][CV];
#pragma unroll
    for (int i = 0; i < D; ++i)
        vload(grp[i], sp, (1 + i) * CV);
    double le[K];
    emit_log<MODEL, K>(pp, slab, a.L, cur[0], le);
#pragma unroll
    for (int k = 0; k < K - 1; ++k)
        dl[k] = dev_nan();
    dl[K - 1] = le[K - 1];
    uint32_t word = 0;
    /* chunk 0: the t = 1 row and the NaN step (Q3) */
    vit_fwd_chunk<MODEL, K, CV, false, true>(a, p, pp, slab, Tp, 0, cur, grp[0][0], le, dl, word);
    /* decoding x itself: the data check inline (xcheck_acc) */
    constexpr bool XCHK = !PK && !ModelTraits<MODEL>::kAux && ModelTraits<MODEL>::kDiscrete;
    uint32_t xm = 0;
    if constexpr (XCHK)
        xcheck_acc<CV, false>(xm, cur, 0, Tp);
    int c = 1;
    for (; c + D <= nfull; c += D) {
        Obs nxt[D][CV];
#pragma unroll
        for (int i = 0; i < D; ++i)
            vload(nxt[i], sp, (c + D + i) * CV);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            vit_fwd_chunk<MODEL, K, CV, true>(a, p, pp, slab, Tp, c + i, grp[i],
                                              (i + 1 < D) ? grp[i + 1 < D ? i + 1 : 0][0] : nxt[0][0], le, dl, word);
            if constexpr (XCHK)
                xcheck_acc<CV, true>(xm, grp[i], c + i, Tp);
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int u = 0; u < CV; ++u)
                grp[i][u] = nxt[i][u];
    }
#pragma unroll
    for (int u = 0; u < CV; ++u)
        cur[u] = grp[0][u];
    for (; c < nchunk; ++c) { /* < D full chunks, then the partial ones (one code copy) */
        Obs nxt[CV];
        vload(nxt, sp, (c + 1) * CV);
        vit_fwd_chunk<MODEL, K, CV, false>(a, p, pp, slab, Tp, c, cur, nxt[0], le, dl, word);
        if constexpr (XCHK)
            xcheck_acc<CV, false>(xm, cur, c, Tp);
#pragma unroll
        for (int u = 0; u < CV; ++u)
            cur[u] = nxt[u];
    }
    if constexpr (XCHK)
        if (a.dc_flag && xm >= (uint32_t)a.L)
            a.dc_flag[n] = 1;
    viterbi_epilogue<K>(a, p, Tp, Tw_min, Tw_max, dl, word);
}

template <int MODEL, int K, bool PK = false>
__global__ void __launch_bounds__(kBlock) viterbi_kernel(const DevArgs a)
{
    if constexpr (!PK || (fb_big_ok<MODEL, K>() && vit_chunk(K) == 8))
        viterbi_block<MODEL, K, PK>(a, blockIdx.x);
}

/* ---- state-parallel Viterbi (few pairs, long T; C5) ------------------- *
 * One lane per (pair, state j): a pair's K <= 4 states sit in one lane quad.
 * Each step a lane fetches delta_{t-1} of the quad by DPP quad broadcasts,
 * forms its own K candidates in the reference's order and reduces them with
 * the same fmax / strict-compare rules as vit_step, so delta, the
 * back-pointers and the paths are bit-identical to the lane-per-pair decoder.
 * The per-step dependency chain is K candidates instead of K^2, which is what
 * bounds a batch too small to hide latency with other waves (250 pairs x
 * T = 1e6: 4 waves on the whole chip).  The back-pointer bits of the quad are
 * OR-reduced into the same packed word layout, so the epilogue (run by all
 * four lanes on the gathered delta_T; identical duplicate stores) and the
 * backtrack are shared. */

/* Steps per prefetched observation chunk: a multiple of the word length, two
 * Viterbi chunks deep so the (latency-bound) loads run far ahead. */
constexpr int vit_sp_chunk(int K) { return 2 * vit_chunk(K); }

template <int MODEL, int K>
struct SpLane {
    double colA[K]; /* log A[i][js] */
    double mu, isig, c0; /* gauss: state js */
    const double *slab;  /* discrete: log phi[js][.] column, stride 64 */
    const double *arow;  /* tayal: rows [sign 1 | sign 2 | other][i] of the masked column, stride 64 */
    int js;              /* state of this lane */
    int j;               /* quad position (bits only from j < K) */
};

template <int MODEL, int K>
__device__ __forceinline__ double sp_emit(const SpLane<MODEL, K> &ln, const Obs &o, int L)
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
        const double z = (o.xr - ln.mu) * ln.isig;
        const double z2 = z * z;
        return ln.c0 + (-0.5 * z2);
    } else {
        return ln.slab[(min(max(o.x, 1), L) - 1) * 64];
    }
}

/* Tayal: the masked transition column of this lane for a step's sign:
 * log A[i][js] where the mask is on, -0.0 where it is off (x + -0.0 == x for
 * every double x, so the off candidate keeps its value bit for bit). */
template <int MODEL, int K>
__device__ __forceinline__ void sp_arow(const SpLane<MODEL, K> &ln, int sign, double (&ar)[K])
{
    const int r = (sign == 1) ? 0 : (sign == 2 ? 1 : 2);
#pragma unroll
    for (int i = 0; i < K; ++i)
        ar[i] = ln.arow[(r * K + i) * 64];
}

/* Stores chunk c's back-pointer words (issued after the next chunk's loads). */
template <int K, int CS>
__device__ __forceinline__ void sp_flush_words(const DevArgs &a, int64_t p, int Tp, int c,
                                               const uint32_t (&wb)[CS / bp_steps_per_word(K)])
{
    constexpr int SPW = bp_steps_per_word(K);
#pragma unroll
    for (int i = 0; i < CS / SPW; ++i) {
        const int t = c * CS + i * SPW + SPW - 1;
        if (t < Tp)
            put_tmp(a.bp + a.P * (int64_t)(t / SPW), (uint32_t)p * 4u, wb[i]);
    }
}

template <int MODEL, int K, int CS, bool FULLC>
__device__ __forceinline__ void vit_sp_chunk_run(const DevArgs &a, const SpLane<MODEL, K> &ln, int Tp, int c,
                                                 const Obs (&cur)[CS], const Obs &nxt0, double &le, double (&ar)[K],
                                                 double &dl, uint32_t &bits,
                                                 uint32_t (&wb)[CS / bp_steps_per_word(K)])
{
    constexpr int BITS = bp_bits(K);
    constexpr int STEPB = K * BITS;
    constexpr int SPW = bp_steps_per_word(K);
    const int t0 = c * CS;
    const uint32_t jbit = (uint32_t)(ln.j * BITS);
    const bool owns = ln.j < K;
#pragma unroll
    for (int u = 0; u < CS; ++u) {
        const int t = t0 + u;
        const Obs &on1 = (u + 1 < CS) ? cur[u + 1 < CS ? u + 1 : 0] : nxt0;
        const double lnx = sp_emit<MODEL, K>(ln, on1, a.L);
        double arx[K];
        if constexpr (ModelTraits<MODEL>::kTayal)
            sp_arow<MODEL, K>(ln, on1.aux, arx);
        if (FULLC || t < Tp) {
            if (!(u == 0 && c == 0)) {
                double d[K];
                quad_gather<K>(dl, d);
                double best = dev_ninf();
                uint32_t arg = 0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    double cand;
                    if constexpr (ModelTraits<MODEL>::kTayal) {
                        /* (delta + log phi) [+ log A] (hhmm-tayal2009.stan:143-146) */
                        cand = (d[i] + le) + ar[i];
                    } else {
                        cand = (d[i] + ln.colA[i]) + le; /* (delta + log A) + emission (hmm.stan:111) */
                    }
                    if (i == 0) {
                        best = fmax(best, cand);
                    } else {
                        const bool gt = cand > best;
                        best = fmax(best, cand);
                        arg = gt ? (uint32_t)i : arg;
                    }
                }
                dl = best;
                if (owns)
                    bits |= arg << ((uint32_t)((u % SPW) * STEPB) + jbit);
            }
            if (u % SPW == SPW - 1) {
                wb[u / SPW] = quad_or(bits);
                bits = 0;
            }
        }
        le = lnx;
        if constexpr (ModelTraits<MODEL>::kTayal) {
#pragma unroll
            for (int i = 0; i < K; ++i)
                ar[i] = arx[i];
        }
    }
}

template <int MODEL, int K>
__global__ void __launch_bounds__(64) viterbi_sp_kernel(const DevArgs a)
{
    static_assert(K >= 2 && K <= 4, "state-parallel Viterbi: one lane quad per pair");
    constexpr int CS = vit_sp_chunk(K);
    constexpr bool VAUX = ModelTraits<MODEL>::kTayal; /* semisup Viterbi is unmasked (Q7) */
    HIP_DYNAMIC_SHARED(double, ldsd)
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 64 + lane;
    const int64_t p = min(g >> 2, a.P - 1);
    if (a.vs_redo && !a.vs_redo[p]) /* hhmm_vscan.h's fallback: only the pairs it flagged */
        return;
    SpLane<MODEL, K> ln;
    ln.j = (int)(g & 3);
    ln.js = min(ln.j, K - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);

    {
        PairParams<MODEL, K> pp;
        load_params<MODEL, K, true>(pp, a, d);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double v = pp.A[i][0];
#pragma unroll
            for (int jj = 1; jj < K; ++jj)
                v = (ln.js == jj) ? pp.A[i][jj] : v;
            ln.colA[i] = v;
        }
        ln.mu = ln.isig = ln.c0 = 0.0;
        if constexpr (ModelTraits<MODEL>::kGauss) {
            ln.mu = pp.mu[0];
            ln.isig = pp.isig[0];
            ln.c0 = pp.c0[0];
#pragma unroll
            for (int jj = 1; jj < K; ++jj) {
                ln.mu = (ln.js == jj) ? pp.mu[jj] : ln.mu;
                ln.isig = (ln.js == jj) ? pp.isig[jj] : ln.isig;
                ln.c0 = (ln.js == jj) ? pp.c0[jj] : ln.c0;
            }
        }
    }
    ln.slab = ldsd + lane;
    ln.arow = ldsd + (size_t)a.L * 64 + lane;
    if constexpr (ModelTraits<MODEL>::kDiscrete) {
        double *col = ldsd + lane;
        for (int l = 0; l < a.L; ++l)
            col[l * 64] = dev_cr_log(draw2<K>(a.phi_k, a, d, ln.js, l, K));
    }
    if constexpr (ModelTraits<MODEL>::kTayal) {
        double *rows = ldsd + (size_t)a.L * 64 + lane;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int i = 0; i < K; ++i)
                rows[(r * K + i) * 64] = tayal_pred(r + 1, ln.js) ? ln.colA[i] : -0.0;
    }
    const SeriesPtrs sp = series_ptrs<MODEL, VAUX>(a, n);
    const int Tw_min = wave_min(Tp);
    const int Tw_max = wave_max(Tp);
    const int nfull = Tw_min / CS;
    const int nchunk = (Tw_max + CS - 1) / CS;

    __syncthreads(); /* LDS tables written (one wave per block; orders LDS) */

    Obs cur[CS];
    load_chunk<MODEL, CS, VAUX>(cur, sp, 0);
    double le = sp_emit<MODEL, K>(ln, cur[0], a.L);
    double ar[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        ar[i] = 0.0;
    /* Q3: only column K of delta_tk[1] is written, the others stay NaN */
    double dl = (ln.js == K - 1) ? le : dev_nan();
    uint32_t bits = 0;
    constexpr int WPC = CS / bp_steps_per_word(K);
    uint32_t wb[WPC];
    for (int c = 0; c < nchunk; ++c) {
        Obs nxt[CS];
        load_chunk<MODEL, CS, VAUX>(nxt, sp, (c + 1) * CS);
        if (c > 0)
            sp_flush_words<K, CS>(a, p, Tp, c - 1, wb);
        if (c < nfull)
            vit_sp_chunk_run<MODEL, K, CS, true>(a, ln, Tp, c, cur, nxt[0], le, ar, dl, bits, wb);
        else
            vit_sp_chunk_run<MODEL, K, CS, false>(a, ln, Tp, c, cur, nxt[0], le, ar, dl, bits, wb);
#pragma unroll
        for (int u = 0; u < CS; ++u)
            cur[u] = nxt[u];
    }
    if (nchunk > 0)
        sp_flush_words<K, CS>(a, p, Tp, nchunk - 1, wb);
    double dv[K];
    quad_gather<K>(dl, dv);
    viterbi_epilogue<K, true>(a, p, Tp, Tw_min, Tw_max, dv, quad_or(bits));
}

} // namespace hhmm
