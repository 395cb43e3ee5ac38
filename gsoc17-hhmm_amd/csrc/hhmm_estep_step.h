/*
 * hhmm_estep_step.h -- what one step of the E-step does, shared by the
 * lane-per-pair kernel (estep_kernel, hhmm_estep.hip: one lane sweeps a whole
 * series) and the T-scan's phase 3 (estep_scan_kernel, hhmm_estep_scan.hip: one
 * lane sweeps one T-chunk): the kernels' output structs, the transition into a
 * step (estep_transition; expect_transition for the masked programs), the
 * emission sums of a step (estep_emit_acc) and the auxiliary stream's range
 * check (auxcheck_acc).  Device code only; not part of the public ABI.
 */
#pragma once
#include <type_traits>

#include "hhmm_estep.h"
#include "hhmm_expect.h"
#include "hhmm_fbchunk.h"

namespace hhmm {

/* One struct per kernel-argument layout; EstepOutOf picks by the model. */
struct EstepOut {
    double *loglik, *n1, *xi, *c, *w, *s1, *s2;
    int32_t *status;
};

struct ExpectOut {
    double *loglik, *n1, *xi, *c;
    int32_t *status;
    int32_t ahi; /* the auxiliary stream's upper bound: G (semisup), 2 (Tayal) */
};

template <int MODEL>
using EstepOutOf = std::conditional_t<ModelTraits<MODEL>::kAux, ExpectOut, EstepOut>;

/* xi lives in LDS instead of registers (xs[(i * K + j) * 64 + lane]) where the
 * registers do not hold it: the Gaussian kernels at K >= 7, whose per-state
 * constants and exp take the room (228 VGPR spills at K = 8 otherwise); they
 * have no emission tables, so 4 waves * K^2 * 512 B <= 128 KiB is free. */
template <int MODEL, int K>
constexpr bool estep_xi_lds() { return ModelTraits<MODEL>::kGauss && K >= 7; }

/* The transition into a step with emission e: accumulates xi (without its
 * constant factor A) and returns the step's gamma in g; be: beta_t in,
 * beta_{t-1} out.  Returns Z. */
template <int MODEL, int K>
__device__ __forceinline__ double estep_transition(const PairParams<MODEL, K> &pp, const double (&ap)[K],
                                                   const double (&e)[K], double (&be)[K], double (&xi)[K][K],
                                                   double *xs, double (&g)[K])
{
    double b[K], bn[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        b[j] = e[j] * be[j];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double acc = pp.A[i][0] * b[0];
#pragma unroll
        for (int j = 1; j < K; ++j)
            acc = fma(pp.A[i][j], b[j], acc);
        bn[i] = acc;
    }
    double Z = ap[0] * bn[0];
#pragma unroll
    for (int i = 1; i < K; ++i)
        Z = fma(ap[i], bn[i], Z);
    const double r = 1.0 / Z;
    /* A is constant over the steps: xi accumulates alpha_{t-1}(i) b_t(j) / Z and
     * takes its factor A(i,j) once, at the end (estep_kernel's stores) */
    double apr[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        apr[i] = ap[i] * r;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double sj = apr[0] * pp.A[0][j];
#pragma unroll
        for (int i = 1; i < K; ++i)
            sj = fma(apr[i], pp.A[i][j], sj);
        g[j] = sj * b[j];
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if constexpr (estep_xi_lds<MODEL, K>())
                xs[(i * K + j) * 64] = fma(apr[i], b[j], xs[(i * K + j) * 64]);
            else
                xi[i][j] = fma(apr[i], b[j], xi[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
        be[i] = bn[i];
    int ex = 0;
    renorm<K>(be, ex);
    return Z;
}

/* beta_{t-1}(i) under per-lane masks, in the split form -- b divided by the
 * mask once per step, then K FMAs per row: 2K selects -- or with a select per
 * term (K^2 selects, K^2 extra adds).  The K >= 6 instances are past 256 VGPRs
 * and keep the select form: with the split form hipcc's allocation of them
 * left a dword in a private segment, which no instance may have. */
constexpr bool expect_split(int K) { return K <= 5; }

/* The adjoint transition into a step with emission e and observation o:
 * accumulates xi (without its constant factor A) and returns the step's gamma
 * in g; be: beta_t in, beta_{t-1} out.  Returns Z.  SG: the step's Tayal sign
 * class when the wave shares it (tayal_dispatch), else -1 (the masks per lane).
 * With on(j) the forward mask of step t at state j and b = e_t .* beta_t:
 *     beta_{t-1}(i) = sum_{j on} A(i,j) b(j) + sum_{j off} b(j)
 *     Z             = sum_i alpha_{t-1}(i) beta_{t-1}(i),   a = alpha_{t-1} / Z
 *     gamma_t(j)    = b(j) (on(j) ? sum_i a(i) A(i,j) : sum_i a(i))
 *     xi(i,j)      += on(j) ? a(i) b(j) : 0
 * Where every lane of the wave has the step's sign (one series under many
 * draws) the masks are compile-time constants and the structural zeros of A
 * are skipped -- only under skip_ok, see tayal_nz. */
template <int MODEL, int K, int SG>
__device__ __forceinline__ double expect_transition(const PairParams<MODEL, K> &pp, const double (&ap)[K],
                                                    const double (&e)[K], const Obs &o, double (&be)[K],
                                                    double (&xi)[K][K], double (&g)[K])
{
    constexpr bool KNOWN = SG > 0 && ModelTraits<MODEL>::kTayal;
    double b[K], bn[K];
    bool on[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        b[j] = e[j] * be[j];
        if constexpr (KNOWN)
            on[j] = tayal_on(SG, j);
        else if constexpr (ModelTraits<MODEL>::kSemisup)
            on[j] = semisup_mask(o.aux, j);
        else
            on[j] = tayal_pred(o.aux, j);
    }
    if constexpr (KNOWN) {
        /* the split form with the masks known: the same additions in the same
         * order (the per-lane form's other terms are exact zeros) -- the same
         * bits, so a pair's result does not depend on its wave's other lanes */
        static_assert(expect_split(K), "the sign-class arms mirror the split form");
        double boff = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (!on[j])
                boff += b[j];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double acc = boff;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (on[j] && tayal_nz(i, j < 4 ? j : 0))
                    acc = fma(pp.A[i][j], b[j], acc);
            bn[i] = acc;
        }
    } else if constexpr (expect_split(K)) {
        /* b split by the mask: the "on" part takes A, the "off" part is one scalar */
        double bon[K], boff = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            bon[j] = on[j] ? b[j] : 0.0;
            boff += on[j] ? 0.0 : b[j];
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double acc = fma(pp.A[i][0], bon[0], boff);
#pragma unroll
            for (int j = 1; j < K; ++j)
                acc = fma(pp.A[i][j], bon[j], acc);
            bn[i] = acc;
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double acc = 0.0;
            bool first = true;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double t = first ? pp.A[i][j] * b[j] : fma(pp.A[i][j], b[j], acc);
                const double u = first ? b[j] : acc + b[j];
                acc = on[j] ? t : u;
                first = false;
            }
            bn[i] = acc;
        }
    }
    double Z = ap[0] * bn[0];
#pragma unroll
    for (int i = 1; i < K; ++i)
        Z = fma(ap[i], bn[i], Z);
    const double r = 1.0 / Z;
    double apr[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        apr[i] = ap[i] * r;
    double tot = apr[0];
#pragma unroll
    for (int i = 1; i < K; ++i)
        tot += apr[i];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double sj = 0.0;
        bool first = true;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (KNOWN && (!on[j] || !tayal_nz(i < 4 ? i : 0, j < 4 ? j : 0)))
                continue;
            sj = first ? apr[i] * pp.A[i][j] : fma(apr[i], pp.A[i][j], sj);
            first = false;
        }
        g[j] = (on[j] ? sj : tot) * b[j];
    }
    /* A is constant over the steps: xi accumulates alpha_{t-1}(i) b_t(j) / Z over
     * the "on" steps and takes its factor A(i,j) once, at the end */
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (KNOWN && !on[j])
            continue;
        const double bm = on[j] ? b[j] : 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (KNOWN && !tayal_nz(i < 4 ? i : 0, j < 4 ? j : 0))
                continue;
            xi[i][j] = fma(apr[i], bm, xi[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
        be[i] = bn[i];
    int ex = 0;
    renorm<K>(be, ex);
    return Z;
}

/* xcheck_acc for the auxiliary stream: the running max of aux - 1 (unsigned,
 * so a value below 1 wraps above every bound) over the lane's own steps */
template <int C, bool FULL>
__device__ __forceinline__ void auxcheck_acc(uint32_t &am, const Obs (&o)[C], int c, int Tp)
{
#pragma unroll
    for (int v = 0; v < C; ++v)
        am = max(am, (FULL || c * C + v < Tp) ? ((uint32_t)o[v].aux - 1u) : 0u);
}

/* gamma of one step into the emission sums: row x of the c_kl slab (clamped
 * like the emission fetch), or the Gaussian moments. */
template <int MODEL, int K>
__device__ __forceinline__ void estep_emit_acc(double2 *cslab, int L, const Obs &o, const double (&g)[K],
                                               double (&w)[K], double (&s1)[K], double (&s2)[K])
{
    if constexpr (ModelTraits<MODEL>::kGauss) {
        const double x = o.xr, x2 = o.xr * o.xr;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            w[k] += g[k];
            s1[k] = fma(g[k], x, s1[k]);
            s2[k] = fma(g[k], x2, s2[k]);
        }
    } else {
        constexpr int KP = (K + 1) / 2;
        const int xc = min(max(o.x, 1), L);
        double2 *r = (cslab - KP * 64) + xc * (KP * 64);
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            double2 v = r[kp * 64];
            v.x += g[2 * kp];
            if (2 * kp + 1 < K)
                v.y += g[2 * kp + 1];
            r[kp * 64] = v;
        }
    }
}

} // namespace hhmm
