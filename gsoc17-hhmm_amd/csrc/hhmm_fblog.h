/*
 * hhmm_fblog.h -- the log-space forward-backward of the HMM family
 * (fb_log_kernel: the unalpha_tk / unbeta_tk profile).
 */
#pragma once
#include "hhmm_viterbi.h"

namespace hhmm {

/* ------------------------------------------------------------------ */
/* Log-space forward-backward (the unalpha_tk / unbeta_tk profile)       */
/* ------------------------------------------------------------------ */
/*
 * The log-scale outputs unalpha_tk / unbeta_tk keep finite values for states
 * whose probability is below the double range relative to the others (Stan
 * works in log space: e.g. hhmm-tayal2009.stan:93-119 keeps unbeta ~ -2400
 * where the linear recursion's component underflows).  When either is
 * requested the recursion runs in log space like the reference -- log A and
 * log phi tabulated once per pair, Stan's log_sum_exp per (t, j) -- with the
 * same checkpoint / recompute structure as fb_kernel.  Posteriors follow the
 * reference's formulas: alpha = softmax(unalpha), beta = softmax(unbeta),
 * ungamma = alpha .* beta, gamma = ungamma / sum (hmm.stan:60-63, 85-96).
 */
template <int K>
__device__ __forceinline__ double stan_lse(const double (&x)[K])
{
    double mx = dev_ninf();
#pragma unroll
    for (int i = 0; i < K; ++i)
        if (x[i] > mx)
            mx = x[i];
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i)
        if (x[i] != dev_ninf())
            sum += exp(x[i] - mx);
    return mx + log(sum);
}

template <int K>
__device__ __forceinline__ void stan_softmax_v(const double (&v)[K], double (&th)[K])
{
    double mx = v[0];
#pragma unroll
    for (int i = 1; i < K; ++i)
        if (v[i] > mx)
            mx = v[i];
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        th[i] = exp(v[i] - mx);
        sum += th[i];
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
        th[i] = th[i] / sum;
}

/* unalpha_1 (hmm.stan:29-30 with the Q2 summed emission; multinom :30-31;
 * Tayal :49-54).  pp.A holds log A. */
template <int MODEL, int K>
__device__ __forceinline__ void fwd_log_init(double (&u)[K], const PairParams<MODEL, K> &pp, const double (&le)[K],
                                             const Obs &o)
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
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
            u[k] = log(pp.p[k]) + s;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (ModelTraits<MODEL>::kTayal)
                u[k] = tayal_init_pred(o.aux, k) ? le[k] + log(pp.p[k]) : le[k];
            else
                u[k] = log(pp.p[k]) + le[k];
        }
    }
}

/* unalpha_t(j) = LSE_i(acc_i) with the reference's accumulator
 * (hmm.stan:37; semisup :39-44 and Tayal :60-64: transition under the mask). */
template <int MODEL, int K>
__device__ __forceinline__ void fwd_log_step(const double (&u)[K], double (&out)[K], const PairParams<MODEL, K> &pp,
                                             const double (&le)[K], const Obs &o)
{
    double nu[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double acc[K];
        if constexpr (ModelTraits<MODEL>::kAux) {
            bool on;
            if constexpr (ModelTraits<MODEL>::kSemisup)
                on = semisup_mask(o.aux, j);
            else
                on = tayal_pred(o.aux, j);
#pragma unroll
            for (int i = 0; i < K; ++i) {
                acc[i] = u[i] + le[j];
                acc[i] = on ? acc[i] + pp.A[i][j] : acc[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                acc[i] = (u[i] + pp.A[i][j]) + le[j];
        }
        nu[j] = stan_lse<K>(acc);
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        out[j] = nu[j];
}

/* unbeta_{t-1}(j) = LSE_i(acc_i): (unbeta_t(i) + log A(j,i)) + le_t(i)
 * (hmm.stan:79; semisup unmasked :84); Tayal: unbeta + log phi, + log A(j,i)
 * under the predicate on the PREVIOUS state j (hhmm-tayal2009.stan:107-111). */
template <int MODEL, int K>
__device__ __forceinline__ void bwd_log_step(double (&ub)[K], const PairParams<MODEL, K> &pp, const double (&le)[K],
                                             const Obs &o)
{
    double nb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double acc[K];
        if constexpr (ModelTraits<MODEL>::kTayal) {
            const bool on = tayal_pred(o.aux, j);
#pragma unroll
            for (int i = 0; i < K; ++i) {
                acc[i] = ub[i] + le[i];
                acc[i] = on ? acc[i] + pp.A[j][i] : acc[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                acc[i] = (ub[i] + pp.A[j][i]) + le[i];
        }
        nb[j] = stan_lse<K>(acc);
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        ub[j] = nb[j];
}

template <int K>
__device__ __forceinline__ void emit_log_posteriors(const DevArgs &a, int64_t p, int t, const double (&u)[K],
                                                    const double (&ub)[K], bool fwd_only)
{
    const uint32_t o = a.outputs;
    double al[K], be[K];
    stan_softmax_v<K>(u, al);
    if ((o & HHMM_OUT_UNALPHA) && a.unalpha)
        store_tk<K>(a.unalpha, a, p, t, u);
    if ((o & HHMM_OUT_ALPHA) && a.alpha)
        store_tk<K>(a.alpha, a, p, t, al);
    if (fwd_only)
        return;
    stan_softmax_v<K>(ub, be);
    if ((o & HHMM_OUT_UNBETA) && a.unbeta)
        store_tk<K>(a.unbeta, a, p, t, ub);
    if ((o & HHMM_OUT_BETA) && a.beta)
        store_tk<K>(a.beta, a, p, t, be);
    if (o & (HHMM_OUT_GAMMA | HHMM_OUT_UNGAMMA)) {
        double ug[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            ug[k] = al[k] * be[k];
        if ((o & HHMM_OUT_UNGAMMA) && a.ungamma)
            store_tk<K>(a.ungamma, a, p, t, ug);
        if ((o & HHMM_OUT_GAMMA) && a.gamma) {
            const double r = 1.0 / vsum<K>(ug);
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                v[k] = ug[k] * r;
            store_tk<K>(a.gamma, a, p, t, v);
        }
    }
}

template <int MODEL, int K, bool FWDONLY>
__global__ void __launch_bounds__(kBlock) fb_log_kernel(const DevArgs a)
{
    constexpr int C = fb_chunk(K);
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    constexpr int KP = (K + 1) / 2;
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t p = min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);
    double2 *slab = lds + (size_t)wave * a.L * KP * 64 + lane;
    PairParams<MODEL, K> pp;
    load_params<MODEL, K, true>(pp, a, d);
    if constexpr (ModelTraits<MODEL>::kDiscrete)
        fill_table<K, true>(slab, a, d);
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);
    const int nchunk = (wave_max(Tp) + C - 1) / C;

    double u[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        u[k] = 0.0;
    Obs cur[C];
    load_chunk<MODEL, C, AUX>(cur, sp, 0);
    for (int c = 0; c < nchunk; ++c) {
        Obs nxt[C];
        load_chunk<MODEL, C, AUX>(nxt, sp, (c + 1) * C);
#pragma unroll
        for (int v = 0; v < C; ++v) {
            const int t = c * C + v;
            if (t < Tp) {
                double le[K];
                emit_log<MODEL, K>(pp, slab, a.L, cur[v], le);
                if (t == 0)
                    fwd_log_init<MODEL, K>(u, pp, le, cur[v]);
                else
                    fwd_log_step<MODEL, K>(u, u, pp, le, cur[v]);
                if constexpr (FWDONLY) {
                    emit_log_posteriors<K>(a, p, t, u, u, true);
                } else if (v == 0) {
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        put_tmp(a.ckpt + a.P * ((int64_t)c * K + k), (uint32_t)p * 8u, u[k]);
                }
            }
        }
#pragma unroll
        for (int v = 0; v < C; ++v)
            cur[v] = nxt[v];
    }
    if ((a.outputs & HHMM_OUT_LOGLIK) && a.loglik) /* target += log_sum_exp(unalpha_tk[T]) */
        a.loglik[p] = stan_lse<K>(u);
    if constexpr (FWDONLY)
        return;

    double ub[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        ub[k] = 1.0; /* unbeta_tk[T, j] = 1 (Q1) */
    for (int c = nchunk - 1; c >= 0; --c) {
        load_chunk<MODEL, C, AUX>(cur, sp, c * C);
        double abuf[C][K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            abuf[0][k] = get_tmp(a.ckpt + a.P * ((int64_t)c * K + k), (uint32_t)p * 8u);
#pragma unroll
        for (int v = 1; v < C; ++v) {
            if (c * C + v < Tp) {
                double le[K];
                emit_log<MODEL, K>(pp, slab, a.L, cur[v], le);
                fwd_log_step<MODEL, K>(abuf[v - 1], abuf[v], pp, le, cur[v]);
            }
        }
#pragma unroll
        for (int v = C - 1; v >= 0; --v) {
            const int t = c * C + v;
            if (t < Tp) {
                emit_log_posteriors<K>(a, p, t, abuf[v], ub, false);
                if (t > 0) {
                    double le[K];
                    emit_log<MODEL, K>(pp, slab, a.L, cur[v], le);
                    bwd_log_step<MODEL, K>(ub, pp, le, cur[v]);
                }
            }
        }
    }
}

} // namespace hhmm
