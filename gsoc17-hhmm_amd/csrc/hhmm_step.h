/*
 * hhmm_step.h -- the per-step primitives of the HMM family (hmm, hmm-multinom,
 * semisup, Tayal full / lite) on gfx950: the masks, ModelTraits, the
 * observation loads (Obs, SeriesPtrs, load_chunk), the per-pair parameters
 * (PairParams, load_params, load_vit_params), the LDS emission tables
 * (fill_table, read_table, emit_prob) and one step of the scaled recursion
 * (fwd_init, fwd_step*, bwd_step*).  Every kernel of the family is built
 * from these (DESIGN.md §3.18 has the header map).
 *
 * Layout in HBM (include/hhmm.h): every array is pair-/series-/draw-fastest,
 * so one wave of 64 lanes = 64 consecutive pairs reads and writes 64
 * consecutive elements per (t, k): every global access below is a fully
 * coalesced 256 B (int32) or 512 B (fp64) wave transaction.
 *
 * One LANE owns one (series, draw) PAIR for the whole sequence; the K-state
 * vectors live in registers.  Per-pair emission tables (phi_k and log phi_k,
 * K*L doubles) live in LDS, one slab per wave, laid out
 *     slab[(l * KP + kp) * 64 + lane]  (double2: states 2kp, 2kp+1)
 * so a 16-lane ds_read_b128 group touches 16 consecutive 16-B slots = all 64
 * banks once: conflict-free for any per-lane symbol.
 *
 * Latency rules used throughout (the kernels are latency-, not issue-bound at
 * the 2 waves/SIMD the LDS tables allow): observation loads are issued
 * unconditionally (clamped index) one chunk ahead, checkpoints and
 * back-pointer words one chunk ahead, and each step's LDS emission row is
 * fetched one step ahead.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "hhmm_device.h"

namespace hhmm {

/* hmm-multinom-semisup.stan:42 -- j0 is 0-based */
__device__ __forceinline__ bool semisup_mask(int g, int j0)
{
    const int j = j0 + 1;
    return (g == 1 && (j == 1 || j == 4)) || (g == 2 && (j == 2 || j == 3));
}
/* hhmm-tayal2009.stan:62 / :109 / :144 */
__device__ __forceinline__ bool tayal_pred(int s, int j0)
{
    const int j = j0 + 1;
    return (s == 1 && (j == 2 || j == 3)) || (s == 2 && (j == 1 || j == 4));
}
/* tayal_pred for a compile-time sign class sg (1, 2, or 3 = any other sign):
 * the kernels whose wave shares one step's sign (one series under many draws,
 * C5) take the masks as constants, so the masked-off terms cost nothing. */
__host__ __device__ constexpr bool tayal_on(int sg, int j0)
{
    return (sg == 1 && (j0 == 1 || j0 == 2)) || (sg == 2 && (j0 == 0 || j0 == 3));
}
/* The flattened HHMM's transition matrix (hhmm-tayal2009.stan:36-44), as ONE
 * table both load_params (which builds A) and tayal_nz (which skips its
 * structural zeros) read: entry (i, j) is 0 (a structural zero), 1 (one), or
 * 2 + 2r + c for A_row[r][c]. */
constexpr int kTayalA[4][4] = {{0, 2, 3, 0}, {1, 0, 0, 0}, {4, 0, 0, 5}, {0, 0, 1, 0}};
/* Entry (i, j) can be nonzero.  A term with a structural zero adds exactly
 * nothing (0 x f to a linear sum of finite terms, a -inf candidate to a
 * max-plus one), so the sign-class paths skip it -- in the linear filters only
 * where the wave's parameters are probabilities (PairParams::skip_ok), so no
 * NaN or infinity can meet a skipped zero (the reference's 0 x NaN = NaN). */
__host__ __device__ constexpr bool tayal_nz(int i, int j) { return kTayalA[i][j] != 0; }
/* hhmm-tayal2009.stan:51 */
__device__ __forceinline__ bool tayal_init_pred(int s, int j0)
{
    const int j = j0 + 1;
    return (s == 1 && j == 3) || (s == 2 && j == 1);
}

template <int MODEL>
struct ModelTraits {
    static constexpr bool kGauss = (MODEL == HHMM_MODEL_HMM_GAUSS);
    static constexpr bool kSemisup = (MODEL == HHMM_MODEL_HMM_MULTINOM_SEMISUP);
    static constexpr bool kTayal = (MODEL == HHMM_MODEL_TAYAL || MODEL == HHMM_MODEL_TAYAL_LITE);
    static constexpr bool kDiscrete = !kGauss;
    static constexpr bool kAux = kSemisup || kTayal; /* needs g[] or sign[] per step */
};

/* One observation step of a series. */
struct Obs {
    int x;     /* symbol 1..L (discrete models) */
    int aux;   /* g (semisup) or sign (tayal) */
    double xr; /* real observation (gauss) */
};

/* Observation streams of one series (series-fastest arrays): uniform base
 * pointers + this lane's 32-bit series index.  A time row t is the uniform
 * pointer base + N*t, so hipcc can address it as SGPR base + VGPR offset. */
struct SeriesPtrs {
    const int32_t *x;
    const int32_t *aux;
    const double *xr;
    int64_t stride; /* N: elements between consecutive time steps */
    uint32_t n;     /* this lane's series */
    int tmax;       /* padded time extent of the arrays */
};

/* Loads the C observations of chunk [t0, t0+C).  Every load is issued
 * unconditionally from a wave-uniform time index clamped into [0, Tmax-1]: a
 * conditional load makes hipcc branch around it and drain vmcnt(0) per
 * element (cdna_hip_programming.md §5, trap (c)); rows past a lane's own
 * length are padding that is never consumed. */
template <int MODEL, int C, bool AUX>
__device__ __forceinline__ void load_chunk(Obs (&dst)[C], const SeriesPtrs &sp, int t0)
{
#pragma unroll
    for (int u = 0; u < C; ++u) {
        const int tc = min(max(t0 + u, 0), sp.tmax - 1);
        const int64_t row = (int64_t)tc * sp.stride;
        dst[u].x = 1;
        dst[u].aux = 0;
        dst[u].xr = 0.0;
        if constexpr (!ModelTraits<MODEL>::kGauss)
            dst[u].x = at(sp.x + row, sp.n * 4u);
        if constexpr (AUX)
            dst[u].aux = at(sp.aux + row, sp.n * 4u);
        if constexpr (ModelTraits<MODEL>::kGauss)
            dst[u].xr = at(sp.xr + row, sp.n * 8u);
    }
}

/* Per-pair parameters held in registers. */
template <int MODEL, int K>
struct PairParams {
    double A[K][K];  /* probability (FB) or log (Viterbi) */
    double p[K];
    double mu[K], isig[K], lsig[K], c0[K]; /* gauss: 1/sigma, log sigma, NEG_LOG_SQRT_TWO_PI - log sigma */
    bool skip_ok;    /* tayal: p_11, A_row (load_params) and phi (fill_table) all in [0, 1] */
};

template <int K>
__device__ __forceinline__ double draw1(const double *arr, const DevArgs &a, int64_t d, int k)
{
    return arr[d + a.S * (int64_t)k];
}
template <int K>
__device__ __forceinline__ double draw2(const double *arr, const DevArgs &a, int64_t d, int i, int j, int I)
{
    return arr[d + a.S * ((int64_t)i + (int64_t)I * j)];
}

/* 0 <= v <= 1 (false for NaN) */
__device__ __forceinline__ bool in01(double v) { return (v >= 0.0) & (v <= 1.0); }

/* Loads p_1k, A_ij (Tayal: expands p_11 / A_row, hhmm-tayal2009.stan:30-44)
 * and the Gaussian constants.  LOG = true puts log A in params.A.
 * Every global load is issued before the first log consumes one: with the
 * load -> correctly rounded log pairs interleaved, hipcc waits vmcnt(0) per
 * parameter, i.e. one HBM round trip per entry (K^2 + K of them) before the
 * first step. */
template <int MODEL, int K, bool LOG>
__device__ __forceinline__ void load_params(PairParams<MODEL, K> &pp, const DevArgs &a, int64_t d)
{
    if constexpr (ModelTraits<MODEL>::kTayal) {
        static_assert(K == 4, "tayal is a K = 4 model");
        const double p11 = a.p_11[d];
        const double r00 = a.A_row[d + a.S * 0], r10 = a.A_row[d + a.S * 1];
        const double r01 = a.A_row[d + a.S * 2], r11 = a.A_row[d + a.S * 3];
        const double src[6] = {0.0, 1.0, r00, r01, r10, r11}; /* kTayalA's codes */
        double A[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                A[i][j] = src[kTayalA[i][j]];
        pp.skip_ok = in01(p11) && in01(r00) && in01(r01) && in01(r10) && in01(r11);
        pp.p[0] = p11;
        pp.p[1] = 0;
        pp.p[2] = 1 - p11;
        pp.p[3] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                pp.A[i][j] = LOG ? dev_cr_log(A[i][j]) : A[i][j];
    } else {
        pp.skip_ok = false;
        double raw[K][K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            pp.p[k] = draw1<K>(a.p_1k, a, d, k);
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j)
                raw[i][j] = draw2<K>(a.A_ij, a, d, i, j, K);
        double mu[ModelTraits<MODEL>::kGauss ? K : 1], sg[ModelTraits<MODEL>::kGauss ? K : 1];
        if constexpr (ModelTraits<MODEL>::kGauss) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                sg[k] = draw1<K>(a.sigma_k, a, d, k);
                mu[k] = draw1<K>(a.mu_k, a, d, k);
            }
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j)
                pp.A[i][j] = LOG ? dev_cr_log(raw[i][j]) : raw[i][j];
        if constexpr (ModelTraits<MODEL>::kGauss) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pp.mu[k] = mu[k];
                pp.isig[k] = 1.0 / sg[k];
                pp.lsig[k] = dev_cr_log(sg[k]);
                pp.c0[k] = HHMM_NEG_LOG_SQRT_TWO_PI - pp.lsig[k];
            }
        }
    }
}

/* Fills this lane's LDS slab with phi_k (LOG: log phi_k).  Rows are fetched
 * kRowBatch at a time, all loads of a batch in flight together (a load per
 * row followed by its LDS store costs one HBM round trip per row). */
constexpr int kRowBatch = 4;

/* The lane-per-pair Viterbi (vit_step) reads log A and the log emissions with
 * every NaN entry replaced by -inf, once per pair at load time.  The
 * reference's `if (logp > delta)` from -inf ignores a NaN candidate and a
 * -inf one alike (neither moves delta or the back-pointer), so the swap
 * changes no delta and no back-pointer; and with no NaN parameter left, no
 * candidate after the Q3 step is NaN (finite or -inf terms only: an infinite
 * parameter is outside the contract), which is what lets vit_step start its
 * running max from candidate 0 instead of from -inf.  Without the swap a NaN
 * candidate 0 (A_ij[0, j] = NaN) became that start: the first finite
 * candidate then took the value but not the back-pointer. */
__device__ __forceinline__ double vit_nonan(double v) { return isnan(v) ? dev_ninf() : v; }

/* load_params<LOG> for vit_step: log A without NaN; a Gaussian state with a NaN
 * mu or sigma gets the constants that make gauss_lpdf -inf at every finite x
 * (c0 = -inf, z = (x - 0) * 0). */
template <int MODEL, int K>
__device__ __forceinline__ void load_vit_params(PairParams<MODEL, K> &pp, const DevArgs &a, int64_t d)
{
    load_params<MODEL, K, true>(pp, a, d);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j)
            pp.A[i][j] = vit_nonan(pp.A[i][j]);
    if constexpr (ModelTraits<MODEL>::kGauss) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool nan = isnan(pp.mu[k]) || isnan(pp.c0[k]) || isnan(pp.isig[k]);
            pp.mu[k] = nan ? 0.0 : pp.mu[k];
            pp.isig[k] = nan ? 0.0 : pp.isig[k];
            pp.c0[k] = nan ? dev_ninf() : pp.c0[k];
        }
    }
}

/* VIT: the table feeds vit_step (LOG only): NaN -> -inf, see vit_nonan. */
template <int K, bool LOG, bool VIT = false>
__device__ __forceinline__ bool fill_table(double2 *slab, const DevArgs &a, int64_t d)
{
    constexpr int KP = (K + 1) / 2;
    bool ok = true; /* every phi entry in [0, 1] (PairParams::skip_ok) */
    for (int l0 = 0; l0 < a.L; l0 += kRowBatch) {
        double v[kRowBatch][2 * KP];
#pragma unroll
        for (int r = 0; r < kRowBatch; ++r) {
            const int l = min(l0 + r, a.L - 1); /* clamped: a short last batch re-reads row L-1 */
#pragma unroll
            for (int k = 0; k < 2 * KP; ++k)
                v[r][k] = (k < K) ? draw2<K>(a.phi_k, a, d, k, l, K) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kRowBatch; ++r) {
            if (l0 + r < a.L) {
#pragma unroll
                for (int kp = 0; kp < KP; ++kp) {
                    double v0 = v[r][2 * kp], v1 = v[r][2 * kp + 1];
                    ok = ok && in01(v0) && in01(v1);
                    if (LOG) {
                        v0 = dev_cr_log(v0);
                        v1 = dev_cr_log(v1);
                    }
                    if (VIT) {
                        v0 = vit_nonan(v0);
                        v1 = vit_nonan(v1);
                    }
                    slab[((l0 + r) * KP + kp) * 64] = make_double2(v0, v1);
                }
            }
        }
    }
    return ok;
}

template <int K>
__device__ __forceinline__ void read_table(const double2 *slab, int x, int L, double (&e)[K])
{
    constexpr int KP = (K + 1) / 2;
    /* row x (1-based, clamped) from the slab's base one row back, so the
     * state pairs sit at non-negative immediate offsets of one address */
    const int xc = min(max(x, 1), L);
    const double2 *r = (slab - KP * 64) + xc * (KP * 64);
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
        const double2 v = r[kp * 64];
        e[2 * kp] = v.x;
        if (2 * kp + 1 < K)
            e[2 * kp + 1] = v.y;
    }
}

/* Stan's scalar normal_lpdf(y | mu_j, sigma_j) with cached c0 = C - log(sigma),
 * isig = 1/sigma: ((C - log sigma) + (-0.5 * z*z)), z = (y - mu) * isig. */
template <int MODEL, int K>
__device__ __forceinline__ double gauss_lpdf(const PairParams<MODEL, K> &pp, double y, int j)
{
    const double z = (y - pp.mu[j]) * pp.isig[j];
    const double z2 = z * z;
    return pp.c0[j] + (-0.5 * z2);
}

/* Emission of one step for the linear-space filter: e[j] (probabilities,
 * Gaussian densities divided by their max m over states) and log m. */
template <int K>
struct Em {
    double e[K];
    double m;
};

/* DETEXP: the Gaussian exp is hhmm_det_exp (FFBS contract, DESIGN.md §5: the
 * filter the draws come from is bit-reproducible by the oracle). */
template <int MODEL, int K, bool DETEXP = false>
__device__ __forceinline__ void emit_prob(const PairParams<MODEL, K> &pp, const double2 *slab, int L,
                                          const Obs &o, Em<K> &em, const hhmm_exp2_entry *etab = hhmm_exp2_tab)
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
        double lp[K];
        double m = dev_ninf();
#pragma unroll
        for (int j = 0; j < K; ++j) {
            lp[j] = gauss_lpdf<MODEL, K>(pp, o.xr, j);
            m = fmax(m, lp[j]);
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            em.e[j] = DETEXP ? hhmm_det_exp_tab(lp[j] - m, etab) : exp(lp[j] - m);
        em.m = m;
    } else {
        read_table<K>(slab, o.x, L, em.e);
        em.m = 0.0;
    }
}

/* out = e_t .* (in M_t), with the model's FORWARD transition masks (semisup
 * g_t on the current state, hmm-multinom-semisup.stan:42-44; Tayal sign_t on
 * the current state, hhmm-tayal2009.stan:62-64); no renormalisation.  in may
 * alias out. */
template <int MODEL, int K, int SG = -1>
__device__ __forceinline__ void fwd_step_raw(const double (&al)[K], double (&out)[K], const PairParams<MODEL, K> &pp,
                                             const double (&e)[K], const Obs &o)
{
    double s[K];
    if constexpr (SG > 0 && ModelTraits<MODEL>::kTayal) {
        /* the sign class is known: the off columns take the row total (the
         * same additions), the on ones the same fma chain -- the same bits */
        double tot = al[0];
#pragma unroll
        for (int i = 1; i < K; ++i)
            tot += al[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (tayal_on(SG, j)) {
                /* the structurally nonzero terms in the same order (a zero term
                 * 0 x f adds nothing to the chain: the same bits) */
                double acc = 0.0;
                bool first = true;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    if (tayal_nz(i, j)) {
                        acc = first ? al[i] * pp.A[i][j] : fma(al[i], pp.A[i][j], acc);
                        first = false;
                    }
                }
                s[j] = acc;
            } else {
                s[j] = tot;
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            out[j] = s[j] * e[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double acc = al[0] * pp.A[0][j];
#pragma unroll
        for (int i = 1; i < K; ++i)
            acc = fma(al[i], pp.A[i][j], acc);
        s[j] = acc;
    }
    if constexpr (ModelTraits<MODEL>::kAux) {
        double tot = al[0];
#pragma unroll
        for (int i = 1; i < K; ++i)
            tot += al[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            bool on;
            if constexpr (ModelTraits<MODEL>::kSemisup)
                on = semisup_mask(o.aux, j);
            else
                on = tayal_pred(o.aux, j);
            s[j] = on ? s[j] : tot;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        out[j] = s[j] * e[j];
}

/* rn: renormalise after this step (every step, except the FB_BIG gamma
 * profile's every kBigRenorm-th; the flag is a compile-time constant after
 * unrolling) */
/* F(sg) with sg a std::integral_constant: the Tayal sign class of the step
 * when every lane of the wave has the same sign (readfirstlane + ballot: a
 * wave of one series under many draws, the T-scan's chunks at C5), else -1
 * (the masks per lane).  Other models: always -1. */
template <int MODEL, typename F>
__device__ __forceinline__ void tayal_dispatch(const Obs &o, bool skip_ok, F &&f)
{
    if constexpr (ModelTraits<MODEL>::kTayal) {
        const int s0 = __builtin_amdgcn_readfirstlane(o.aux);
        if (__ballot((o.aux != s0) | !skip_ok) == 0) {
            if (s0 == 1)
                f(std::integral_constant<int, 1>());
            else if (s0 == 2)
                f(std::integral_constant<int, 2>());
            else
                f(std::integral_constant<int, 3>());
            return;
        }
    }
    f(std::integral_constant<int, -1>());
}

template <int MODEL, int K>
__device__ __forceinline__ void fwd_step_to(const double (&al)[K], double (&out)[K], const PairParams<MODEL, K> &pp,
                                            const double (&e)[K], const Obs &o, int &ex, bool rn = true)
{
    tayal_dispatch<MODEL>(o, pp.skip_ok, [&](auto sgc) { fwd_step_raw<MODEL, K, decltype(sgc)::value>(al, out, pp, e, o); });
    if (rn)
        renorm<K>(out, ex);
}

template <int MODEL, int K>
__device__ __forceinline__ void fwd_step(double (&al)[K], const PairParams<MODEL, K> &pp, const double (&e)[K],
                                         const Obs &o, int &ex, bool rn = true)
{
    fwd_step_to<MODEL, K>(al, al, pp, e, o, ex, rn);
}

/* beta_{t-1} from beta_t and step t's emission / masks. */
template <int MODEL, int K, int SG>
__device__ __forceinline__ void bwd_step_sg(double (&be)[K], const PairParams<MODEL, K> &pp, const double (&e)[K],
                                            const Obs &o)
{
    double b[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        b[i] = e[i] * be[i];
    double s[K];
    double tot = 0.0;
    if constexpr (ModelTraits<MODEL>::kTayal) {
        tot = b[0];
#pragma unroll
        for (int i = 1; i < K; ++i)
            tot += b[i];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (SG > 0 && !tayal_on(SG, j)) { /* known off: the row total alone (the same bits) */
            s[j] = tot;
            continue;
        }
        if constexpr (SG > 0 && ModelTraits<MODEL>::kTayal) {
            /* known on: row j's structurally nonzero terms in the same order */
            double acc = 0.0;
            bool first = true;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                if (tayal_nz(j, i)) {
                    acc = first ? pp.A[j][i] * b[i] : fma(pp.A[j][i], b[i], acc);
                    first = false;
                }
            }
            s[j] = acc;
            continue;
        }
        double acc = pp.A[j][0] * b[0];
#pragma unroll
        for (int i = 1; i < K; ++i)
            acc = fma(pp.A[j][i], b[i], acc);
        s[j] = acc;
    }
    if constexpr (ModelTraits<MODEL>::kTayal && SG < 0) { /* predicate on the PREVIOUS state j (Q6) */
#pragma unroll
        for (int j = 0; j < K; ++j)
            s[j] = tayal_pred(o.aux, j) ? s[j] : tot;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        be[j] = s[j];
}

template <int MODEL, int K>
__device__ __forceinline__ void bwd_step(double (&be)[K], const PairParams<MODEL, K> &pp,
                                         const double (&e)[K], const Obs &o, int &ex, bool rn = true)
{
    tayal_dispatch<MODEL>(o, pp.skip_ok, [&](auto sgc) { bwd_step_sg<MODEL, K, decltype(sgc)::value>(be, pp, e, o); });
    if (rn)
        renorm<K>(be, ex);
}

/* alpha_1 (t = 0) from the step-0 observation / emission. */
template <int MODEL, int K>
__device__ __forceinline__ void fwd_init(double (&al)[K], const PairParams<MODEL, K> &pp, const Em<K> &em,
                                         const Obs &o, double &lsc, int &ex)
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
        /* hmm.stan:30 -- log(p_1k) + SUM_k normal_lpdf(x[1] | mu_k, sigma_k) (Q2) */
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double z = (o.xr - pp.mu[k]) * pp.isig[k];
            const double z2 = z * z;
            s += HHMM_NEG_LOG_SQRT_TWO_PI;
            s -= pp.lsig[k];
            s += -0.5 * z2;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            al[k] = pp.p[k];
        lsc += s;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (ModelTraits<MODEL>::kTayal)
                al[k] = tayal_init_pred(o.aux, k) ? em.e[k] * pp.p[k] : em.e[k];
            else
                al[k] = pp.p[k] * em.e[k];
        }
    }
    renorm<K>(al, ex);
}


template <int MODEL, bool AUX>
__device__ __forceinline__ SeriesPtrs series_ptrs(const DevArgs &a, int64_t n)
{
    SeriesPtrs sp;
    sp.stride = a.N;
    sp.n = (uint32_t)n;
    sp.tmax = a.Tmax;
    sp.x = a.x;
    sp.aux = nullptr;
    if constexpr (AUX && ModelTraits<MODEL>::kSemisup)
        sp.aux = a.g;
    if constexpr (AUX && ModelTraits<MODEL>::kTayal)
        sp.aux = a.sign;
    sp.xr = a.xr;
    return sp;
}

} // namespace hhmm
