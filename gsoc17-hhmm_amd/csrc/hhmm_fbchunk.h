/*
 * hhmm_fbchunk.h -- the chunk layer of the scaled forward-backward recursion:
 * the FbMode / FbPhase profiles and the HHMM_BIG_* build knobs, the
 * renormalisation gate (renorm_sparse_safe, wave_any), the per-step outputs
 * (emit_alpha, emit_posteriors), FbLane, and one checkpoint chunk of the
 * forward sweep (fwd_chunk) and of the backward sweep (bwd_chunk, with
 * ffbs_draw), and the LDS copy of the exp2 table the Gaussian FFBS filter
 * reads (fb_exp2_lds, kExp2TabBytes).  fb_kernel (hhmm_fb.h) and the two statistics kernel
 * templates (estep_kernel in hhmm_estep.hip, draw_stats_kernel in
 * hhmm_draw_stats.hip) run their own sweeps over these chunks; the
 * statistics kernels include this header and nothing beyond it.
 */
#pragma once
#include "hhmm_step.h"

namespace hhmm {

/* ------------------------------------------------------------------ */
/* Forward / backward / posteriors                                       */
/* ------------------------------------------------------------------ */

/* FbMode, the output profile of the forward-backward kernel (compile time): hhmm_plan.h */
constexpr int fb_base(int mode) { return mode & 3; }
constexpr bool fb_ffbs(int mode) { return (mode & FB_FFBS) != 0; }
constexpr bool fb_pack(int mode) { return (mode & FB_PACK) != 0; }
constexpr bool fb_big(int mode) { return (mode & FB_BIG) != 0; }
/* steps between renormalisations */
constexpr int fb_rp(int mode);
constexpr int kFwdGroup = 4;  /* forward chunks per observation prefetch group */
constexpr int kVitGroup = 2;  /* Viterbi chunks per observation prefetch group */
#ifndef HHMM_BIG_CHUNK
#define HHMM_BIG_CHUNK 16
#endif
constexpr int kBigChunk = HHMM_BIG_CHUNK; /* checkpoint interval of FB_BIG (a multiple of fb_chunk(K) = 8) */
/* Phases of one forward-backward launch: both sweeps (the default), or the
 * split schedule's two launches (HHMM_FLAG_FB_SPLIT): the forward sweep
 * (loglik, checkpoints, packed symbols) and then the backward sweep, with the
 * Viterbi decoding the packed symbols beside the latter. */
enum FbPhase { FB_PH_BOTH = 0, FB_PH_FWD = 1, FB_PH_BWD = 2 };
/* FB_BIG renormalises every kBigRenorm-th step (every checkpoint step
 * included): the max-exponent renormalisation is ~9 VALU on each step's
 * chain, and over four steps the state only shrinks by the emission x
 * transition mass, far above the subnormal range. */
#ifndef HHMM_BIG_RENORM
#define HHMM_BIG_RENORM 4
#endif
constexpr int kBigRenorm = HHMM_BIG_RENORM;
/* the gate's bound 2^-(156 / kBigRenorm) below is a shift of at most 52 bits */
static_assert(kBigRenorm >= 3 && kBigRenorm <= 8, "HHMM_BIG_RENORM must be 3..8");
constexpr int fb_rp(int mode) { return (fb_big(mode) && !(mode & FB_RN1)) ? kBigRenorm : 1; }
/* Is the kBigRenorm-step cadence safe for this pair?  Renormalisation leaves
 * the filter's max in [0.5, 1).  One forward step keeps the max at least
 * max * min_i max_j A(i,j) phi(j,x) >= max * (min_i rowmax_i) * phi_min, one
 * backward step at least max * (min_i colmax_i) * phi_min (rowmax / colmax:
 * the largest entry of row / column i of A; phi_min: the smallest emission
 * probability).  With b = phi_min * min(rowmax, colmax) >= 2^-39, kBigRenorm = 4
 * unrenormalised steps keep the max above 2^-157, so every component down to
 * 2^-865 of it stays a normal double -- far below the 1e-250 tolerance floor,
 * as with per-step renormalisation.  Pairs with a smaller b (rare symbols,
 * near-zero transitions; the reference's log space stays finite there) make
 * their wave renormalise every step (FB_RN1), the exact per-step form. */
constexpr double kRenormSafeBound = 1.0 / (double)(1ull << (156 / kBigRenorm)); /* 2^-39 at 4 steps */
template <int MODEL, int K>
__device__ __forceinline__ bool renorm_sparse_safe(const PairParams<MODEL, K> &pp, const double2 *slab, int L)
{
    static_assert(!ModelTraits<MODEL>::kGauss, "discrete emissions only");
    double tmin = 1.0 / 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double rmax = pp.A[i][0], cmax = pp.A[0][i];
#pragma unroll
        for (int j = 1; j < K; ++j) {
            rmax = fmax(rmax, pp.A[i][j]);
            cmax = fmax(cmax, pp.A[j][i]);
        }
        tmin = fmin(tmin, fmin(rmax, cmax));
    }
    double emin = 1.0 / 0.0;
    for (int l = 1; l <= L; ++l) {
        double e[K];
        read_table<K>(slab, l, L, e);
#pragma unroll
        for (int k = 0; k < K; ++k)
            emin = fmin(emin, e[k]);
    }
    return emin * tmin >= kRenormSafeBound; /* NaN: unsafe */
}
/* true when any lane of the wave is unsafe (wave-uniform) */
__device__ __forceinline__ bool wave_any(bool v)
{
    return __builtin_amdgcn_readfirstlane((int)(__ballot(v) != 0)) != 0;
}
#ifndef HHMM_BIG_GROUP
#define HHMM_BIG_GROUP 2
#endif
constexpr int kGroup = HHMM_BIG_GROUP; /* pass 1 keeps every kGroup-th state (32 steps / groups of 4 need
                               * ~300 VGPRs: occupancy 1) */


/* Writes the forward-side outputs of step t (alpha, unalpha). */
template <int K>
__device__ __forceinline__ void emit_alpha(const DevArgs &a, int64_t p, int t, const double (&al)[K], double lsc)
{
    if ((a.outputs & HHMM_OUT_ALPHA) && a.alpha) {
        const double r = 1.0 / vsum<K>(al);
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = al[k] * r;
        store_tk<K>(a.alpha, a, p, t, v);
    }
    if ((a.outputs & HHMM_OUT_UNALPHA) && a.unalpha) {
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = log(al[k]) + lsc;
        store_tk<K>(a.unalpha, a, p, t, v);
    }
}

/* Outputs of step t once alpha_t and beta_t are known.  go: where the gamma
 * profile's rows go (TkIndexed, or the caller's TkCursor standing on step t). */
template <int K, int MODE, typename GOUT = TkIndexed>
__device__ __forceinline__ void emit_posteriors(const DevArgs &a, int64_t p, int t, const double (&al)[K],
                                                const double (&be)[K], double lsa, double lsb,
                                                const GOUT &go = GOUT())
{
    if constexpr (fb_base(MODE) == FB_GAMMA) {
        /* gamma = (alpha .* beta) / sum: the normalisations of alpha and beta
         * cancel, one division per step (hmm.stan:89-96 up to rounding) */
        if (fb_ffbs(MODE) && !a.gamma) /* FFBS alone */
            return;
        double ug[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            ug[k] = al[k] * be[k];
        double sg = vsum<K>(ug);
        double r;
        if (__builtin_expect(sg > kGammaDirect, 1)) {
            r = fast_rcp(sg);
        } else {
            /* alpha and beta nearly disjoint (e.g. the Tayal masks of Q6 on a
             * long series): form the product from the normalised vectors as
             * the reference does, so that its underflow to 0 (and gamma = NaN)
             * happens where Stan's does */
            const double ra = 1.0 / vsum<K>(al), rb = 1.0 / vsum<K>(be);
#pragma unroll
            for (int k = 0; k < K; ++k)
                ug[k] = (al[k] * ra) * (be[k] * rb);
            sg = vsum<K>(ug);
            r = 1.0 / sg;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            ug[k] = ug[k] * r;
        go.store(a.gamma, a, p, t, ug);
    } else {
        const uint32_t o = a.outputs;
        emit_alpha<K>(a, p, t, al, lsa);
        const double sb = vsum<K>(be);
        if ((o & HHMM_OUT_BETA) && a.beta) {
            const double r = 1.0 / sb;
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                v[k] = be[k] * r;
            store_tk<K>(a.beta, a, p, t, v);
        }
        if ((o & HHMM_OUT_UNBETA) && a.unbeta) {
            /* unbeta_tk[T] = 1 (Q1): every unbeta carries +1 */
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                v[k] = (log(be[k]) + lsb) + 1.0;
            store_tk<K>(a.unbeta, a, p, t, v);
        }
        if (o & (HHMM_OUT_GAMMA | HHMM_OUT_UNGAMMA)) {
            const double ra = 1.0 / vsum<K>(al), rb = 1.0 / sb;
            double ug[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                ug[k] = (al[k] * ra) * (be[k] * rb);
            if ((o & HHMM_OUT_UNGAMMA) && a.ungamma)
                store_tk<K>(a.ungamma, a, p, t, ug);
            if ((o & HHMM_OUT_GAMMA) && a.gamma) {
                const double rg = 1.0 / vsum<K>(ug);
                double v[K];
#pragma unroll
                for (int k = 0; k < K; ++k)
                    v[k] = ug[k] * rg;
                store_tk<K>(a.gamma, a, p, t, v);
            }
        }
    }
}


/* The device entry's data check done inline by a whole-series sweep that reads
 * x anyway (HHMM_PAIR_INVALID_DATA): the running max of x - 1, subtracted in
 * unsigned arithmetic (an x < 1 wraps above L; INT32_MIN, R's NA_integer_,
 * would overflow a signed x - 1), one sub and one max per symbol; steps at or past the
 * lane's own length count only on the wave's partial chunks (FULL: none). */
template <int C, bool FULL>
__device__ __forceinline__ void xcheck_acc(uint32_t &xm, const Obs (&o)[C], int c, int Tp)
{
#pragma unroll
    for (int v = 0; v < C; ++v)
        xm = max(xm, (FULL || c * C + v < Tp) ? ((uint32_t)o[v].x - 1u) : 0u);
}

/* Per-lane state of the forward-backward kernel. */
template <int MODEL, int K>
struct FbLane {
    PairParams<MODEL, K> pp;
    const double2 *slab;
    int L;
    int64_t p;   /* output pair */
    int t0;      /* first step of this lane's sweep (0, or a scan chunk's start) */
    int Tp;      /* one past its last step */
    int cb;      /* t0 / C: first checkpoint row */
    int64_t q;   /* checkpoint column (the pair, or the scan lane) */
    int64_t Qs;  /* checkpoint row stride */
    bool noinit = false; /* step 0 is not the series' first (a segment window's chunk 0) */
    int64_t n = 0;       /* the series (fb_block: the inline data check's flag) */
    const hhmm_exp2_entry *etab = hhmm_exp2_tab; /* DETEXP: the LDS copy (fb_kernel) */
};

/* One forward chunk [t0, t0+C).  FULLC: every lane of the wave has all C
 * steps (no per-step predicate).  The emission of step u+1 is fetched before
 * step u is computed (LDS latency hidden behind the K^2 FMAs). */
template <int MODEL, int K, int C, int MODE, bool FULLC>
__device__ __forceinline__ void fwd_chunk(const DevArgs &a, const FbLane<MODEL, K> &ln, int c, const Obs (&cur)[C],
                                          const Obs &nxt0, Em<K> &ecur, double (&al)[K], double &lsc, int &ex)
{
    const int t0 = c * C;
#pragma unroll
    for (int u = 0; u < C; ++u) {
        const int t = t0 + u;
        Em<K> enx;
        emit_prob<MODEL, K, fb_ffbs(MODE)>(ln.pp, ln.slab, ln.L, (u + 1 < C) ? cur[u + 1 < C ? u + 1 : 0] : nxt0,
                                           enx, ln.etab);
        if (FULLC || t < ln.Tp) {
            if (u == 0 && c == 0 && !ln.noinit) {
                fwd_init<MODEL, K>(al, ln.pp, ecur, cur[0], lsc, ex);
            } else {
                lsc += ecur.m;
                fwd_step<MODEL, K>(al, ln.pp, ecur.e, cur[u], ex, u % fb_rp(MODE) == 0);
            }
            if constexpr (fb_base(MODE) == FB_FWD) {
                emit_alpha<K>(a, ln.p, t, al, lsc + kLn2 * ex);
            } else if (u == 0 && (!fb_big(MODE) || (c - ln.cb) % (kBigChunk / C) == 0)) {
                /* checkpoint row: one per C-chunk, or one per kBigChunk steps (FB_BIG) */
                const int64_t row = fb_big(MODE) ? (c - ln.cb) / (kBigChunk / C) : (c - ln.cb);
#pragma unroll
                for (int k = 0; k < K; ++k)
                    put_tmp(a.ckpt + ln.Qs * (row * K + k), (uint32_t)ln.q * 8u, al[k]);
                if constexpr (fb_base(MODE) == FB_FULL)
                    put_tmp(a.ckpt_ls + ln.Qs * (int64_t)(c - ln.cb), (uint32_t)ln.q * 8u, lsc + kLn2 * ex);
            }
            if (fb_pack(MODE) && u == 0) {
                /* the chunk's C <= 8 symbols, 4 bits each, for the backward sweep */
                uint32_t w = 0;
#pragma unroll
                for (int v = 0; v < C; ++v)
                    w |= (((uint32_t)cur[v].x - 1u) & 15u) << (4 * v);
                at(a.xpk + ln.Qs * (int64_t)(c - ln.cb), (uint32_t)ln.q * 4u) = w;
            }
        }
        ecur = enx;
    }
}

/* FFBS draw of step t (oracle ffbs_contract): z_{T-1} ~ cat(f_{T-1}),
 * z_t ~ cat(f_t(i) * A(i, z_{t+1})) -- or f_t(i) where the model's forward mask
 * switches the transition off at (t+1, z_{t+1}).  z is 0-based, -1 = undefined. */
template <int MODEL, int K>
__device__ __forceinline__ int ffbs_draw(const PairParams<MODEL, K> &pp, const double (&f)[K], bool last,
                                         const Obs &onext, int z, double u)
{
    double w[K];
    if (last) {
#pragma unroll
        for (int i = 0; i < K; ++i)
            w[i] = f[i];
    } else {
        if (z < 0)
            return -1;
        bool on = true;
        if constexpr (ModelTraits<MODEL>::kSemisup)
            on = semisup_mask(onext.aux, z);
        if constexpr (ModelTraits<MODEL>::kTayal)
            on = tayal_pred(onext.aux, z);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double az = pp.A[i][0];
#pragma unroll
            for (int j = 1; j < K; ++j)
                az = (z == j) ? pp.A[i][j] : az;
            w[i] = on ? f[i] * az : f[i];
        }
    }
    return ffbs_cat<K>(w, u);
}

/* One backward chunk: recompute alpha over the chunk from its checkpoint,
 * then walk t = t0+C-1 .. t0 emitting the posteriors and stepping beta
 * (and drawing the FFBS state from the recomputed, bit-identical filter). */
template <int MODEL, int K, int C, int MODE, bool FULLC>
__device__ __forceinline__ void bwd_chunk(const DevArgs &a, const FbLane<MODEL, K> &ln, int c, const Obs (&cur)[C],
                                          const double (&ck)[K], double ck_ls, double (&be)[K], double &blsc,
                                          int &bex, const double (&uu)[fb_ffbs(MODE) ? C : 1], const Obs &onext,
                                          int &z)
{
    constexpr bool DETEXP = fb_ffbs(MODE);
    const int t0 = c * C;
    double abuf[C][K];
    double lsbuf[fb_base(MODE) == FB_FULL ? C : 1];
#pragma unroll
    for (int k = 0; k < K; ++k)
        abuf[0][k] = ck[k];
    lsbuf[0] = ck_ls;
    {
        double lsacc = 0.0;
        int exb = 0;
        Em<K> ecur;
        emit_prob<MODEL, K, DETEXP>(ln.pp, ln.slab, ln.L, cur[1 < C ? 1 : 0], ecur, ln.etab);
#pragma unroll
        for (int u = 1; u < C; ++u) {
            Em<K> enx;
            emit_prob<MODEL, K, DETEXP>(ln.pp, ln.slab, ln.L, cur[u + 1 < C ? u + 1 : u], enx, ln.etab);
            if (FULLC || t0 + u < ln.Tp) {
                lsacc += ecur.m;
                fwd_step_to<MODEL, K>(abuf[u - 1], abuf[u], ln.pp, ecur.e, cur[u], exb);
            }
            if constexpr (fb_base(MODE) == FB_FULL)
                lsbuf[u] = ck_ls + (lsacc + kLn2 * exb);
            ecur = enx;
        }
    }
    Em<K> ecur;
    emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[C - 1], ecur);
#pragma unroll
    for (int u = C - 1; u >= 0; --u) {
        const int t = t0 + u;
        Em<K> enx;
        emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[u > 0 ? u - 1 : 0], enx);
        if (FULLC || t < ln.Tp) {
            emit_posteriors<K, MODE>(a, ln.p, t, abuf[u], be, lsbuf[fb_base(MODE) == FB_FULL ? u : 0],
                                     blsc + kLn2 * bex);
            if constexpr (fb_ffbs(MODE)) {
                z = ffbs_draw<MODEL, K>(ln.pp, abuf[u], t == ln.Tp - 1, (u + 1 < C) ? cur[u + 1 < C ? u + 1 : u] : onext,
                                        z, uu[u]);
                at(a.z_ffbs + a.P * (int64_t)t, (uint32_t)ln.p * 4u) = z + 1;
            }
            if (t > ln.t0) {
                if constexpr (fb_base(MODE) == FB_FULL)
                    blsc += ecur.m;
                bwd_step<MODEL, K>(be, ln.pp, ecur.e, cur[u], bex);
            }
        }
        ecur = enx;
    }
}

/* fb_exp2_lds: the FFBS contract's Gaussian exps (DETEXP) read their 2^(j/128)
 * table from an LDS copy -- the Gaussian models have no emission slab, so the
 * copy sits at the start of the launch's LDS (launch_fb sizes it) */
template <int MODEL, int MODE>
constexpr bool fb_exp2_lds() { return ModelTraits<MODEL>::kGauss && fb_ffbs(MODE); }
constexpr size_t kExp2TabBytes = 128 * sizeof(hhmm_exp2_entry);

} // namespace hhmm
