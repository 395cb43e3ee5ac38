/*
 * hhmm_estep_io.hip -- gfx950 kernel of the IOHMM E-step
 * (include/hhmm_estep_io.h): per (series, draw) pair the expected sufficient
 * statistics of iohmm-reg / -mix / -hmix / -hmix-lite under the coded path
 * weight, and the transition-weight gradient gw_km.  Nothing is written per
 * step.
 *
 * The coded transition A_t = softmax(u_t' w_k) is indexed by the previous
 * state only (hhmm_iohmm.h), so the path weight is a product of per-step
 * factors and the E-step is ONE forward sweep with no backward pass and no
 * checkpoints.  Step t, with the loads of step t + 1 already in flight:
 *     v_k      = u_{t+1}' w_k,   log A_{t+1} = v - LSE(v)      (t < T)
 *     lw_t(k)  = oblik_t(k) + log A_{t+1}(k)  [+ log p_1k(k) at t = 1]
 *     c_t      = LSE_k lw_t(k),  q_t = exp(lw_t - c_t),  loglik += c_t
 *     gw_k    += (q_t(k) - A_{t+1}(k)) u_{t+1}
 * and the emission sums weighted by q_t.  Every step is in log space on its
 * own: there is no running scale, so a step whose every density underflows in
 * linear space still has a finite c_t and the right q_t.  libm arithmetic
 * (hhmm_iohmm.h's IO_LIBM class; the contract is 1e-9, not bits).
 *
 * One LANE per pair, hhmm_iohmm.h's loads (coalesced; broadcast under GRID
 * pairing).  w (and b, 1/s, C - log s) sit in registers.  The accumulators sit
 * in a per-lane LDS slab laid out as c_kl is in hhmm_estep.hip (double2 i of a
 * lane at slab[i * 64 + lane]):
 *   reg, per state: the upper triangle of uu (MMAX (MMAX + 1) / 2 doubles), ux
 *        (MMAX), then (n, xx);
 *   mix, per (state, component): (mu, 1/s), (log lambda, C - log s), (n, sx),
 *        (sxx, the component's softmax numerator of the current step);
 *   gw: K * MMAX registers up to 32 of them, else behind the above in the slab.
 * A lane's results depend on nothing outside the lane.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_estep_io.h"
#include "hhmm_iohmm.h"
#include "hhmm_stats.h"

namespace hhmm {

struct EstepIoOut {
    double *loglik, *n1, *gw;
    double *nk, *uu, *ux, *xx; /* reg */
    double *nkl, *sx, *sxx;    /* mix */
    int32_t *status;
};

/* gw in registers (else in the slab) */
constexpr bool eio_gw_regs(int K, int MMAX) { return K * MMAX <= 32; }
constexpr int eio_tri(int MMAX) { return MMAX * (MMAX + 1) / 2; }
/* double2 per state of the regression slab, without gw */
constexpr int eio_reg_state(int MMAX) { return eio_tri(MMAX) / 2 + MMAX / 2 + 1; }
/* double2 per lane: the accumulators (and the mixture tables), then gw */
constexpr int eio_slab_elems(bool reg, int K, int MMAX, int L)
{
    return (reg ? K * eio_reg_state(MMAX) : K * L * 4) + (eio_gw_regs(K, MMAX) ? 0 : K * (MMAX / 2));
}
constexpr size_t eio_wave_bytes(bool reg, int K, int MMAX, int L)
{
    return (size_t)eio_slab_elems(reg, K, MMAX, L) * 64 * sizeof(double2);
}

/* m + log(sum_k exp(v_k - m)), m = max v (0 where that is -inf); e: the summands */
template <int K>
__device__ __forceinline__ double eio_lse(const double (&v)[K], double (&e)[K], double &m, double &sum)
{
    double mx = v[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        mx = fmax(mx, v[k]);
    m = (mx == dev_ninf()) ? 0.0 : mx;
    sum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        e[k] = exp(v[k] - m);
        sum += e[k];
    }
    return m + log(sum);
}

template <int FAM, int K, int MMAX>
__global__ void __launch_bounds__(kBlock) estep_io_kernel(const DevArgs a, const EstepIoOut o)
{
    constexpr bool REG = FAM == IO_REG;
    constexpr bool GWR = eio_gw_regs(K, MMAX);
    constexpr int TRI = eio_tri(MMAX);
    constexpr int MP = MMAX / 2;
    constexpr int SK = eio_reg_state(MMAX);
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const int64_t gwave = (int64_t)blockIdx.x * nw + wave;
    /* lanes past the last pair redo pair P-1 (identical values, benign duplicate stores) */
    const int64_t p = min(gwave * 64 + lane, a.P - 1);
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tp = pair_len(a, n);
    const int M = a.M, L = REG ? 0 : a.L;
    const int elems = eio_slab_elems(REG, K, MMAX, L);
    const int gw0 = REG ? K * SK : K * L * 4; /* gw's first double2 in the slab (!GWR) */
    double2 *const slab = lds + (size_t)wave * elems * 64 + lane;
    for (int i = 0; i < elems; ++i)
        slab[i * 64] = make_double2(0.0, 0.0);

    /* ---- per-pair parameters ---- */
    double lp[K], w[K][MMAX];
    double b[REG ? K : 1][MMAX], isig[REG ? K : 1], c0[REG ? K : 1];
    double gw[GWR ? K : 1][MMAX];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        lp[k] = log(a.p_1k[d + a.S * k]);
#pragma unroll
        for (int m = 0; m < MMAX; ++m) {
            w[k][m] = (m < M) ? a.w_km[d + a.S * ((int64_t)k + (int64_t)K * m)] : 0.0;
            if constexpr (REG)
                b[k][m] = (m < M) ? a.b_km[d + a.S * ((int64_t)k + (int64_t)K * m)] : 0.0;
            if constexpr (GWR)
                gw[k][m] = 0.0;
        }
        if constexpr (REG) {
            const double s = a.s_k[d + a.S * k];
            isig[k] = 1.0 / s;
            c0[k] = HHMM_NEG_LOG_SQRT_TWO_PI - log(s);
        }
    }
    if constexpr (!REG) {
        for (int k = 0; k < K; ++k)
            for (int l = 0; l < L; ++l) {
                const int64_t ix = d + a.S * ((int64_t)k + (int64_t)K * l);
                const double s = a.s_kl[ix];
                double2 *e = slab + (k * L + l) * 4 * 64;
                e[0] = make_double2(a.mu_kl[ix], 1.0 / s);
                e[64] = make_double2(log(a.lambda_kl[ix]), HHMM_NEG_LOG_SQRT_TWO_PI - log(s));
            }
    }

    /* ---- the sweep ---- */
    const int Tw_max = wave_max(Tp);
    double ll = 0.0;
    double n1[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        n1[k] = 0.0;
    double x, xn;
    double u[MMAX], un[MMAX];
    io_load<MMAX>(a, (uint32_t)n, 0, x, u);
    for (int t = 0; t < Tw_max; ++t) {
        io_load<MMAX>(a, (uint32_t)n, t + 1, xn, un); /* one step ahead */
        if (t < Tp) {
            const bool nx = t + 1 < Tp; /* else un is padding: never into a result */
            /* the transition out of step t: A_{t+1} = softmax(u_{t+1}' w_k) and its log */
            double v[K], A[K], lw[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double acc = un[0] * w[k][0];
#pragma unroll
                for (int m = 1; m < MMAX; ++m)
                    acc = fma(un[m], w[k][m], acc);
                v[k] = acc;
            }
            {
                double vm, vs;
                const double lse = eio_lse<K>(v, A, vm, vs);
                const double rs = 1.0 / vs;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    A[k] = A[k] * rs;
                    lw[k] = nx ? v[k] - lse : 0.0;
                }
            }
            /* the emission oblik_t(k) (io_emission's formulas) */
            double inv[REG ? 1 : K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double ob;
                if constexpr (REG) {
                    double mu = u[0] * b[k][0];
#pragma unroll
                    for (int m = 1; m < MMAX; ++m)
                        mu = fma(u[m], b[k][m], mu);
                    const double z = (x - mu) * isig[k];
                    ob = c0[k] + (-0.5 * (z * z));
                } else {
                    /* log lambda + normal_lpdf per component into the entry's scratch half,
                     * then the numerators exp(. - max) in its place */
                    double2 *e = slab + k * L * 4 * 64;
                    double mx = dev_ninf();
                    for (int l = 0; l < L; ++l) {
                        const double2 ms = e[(l * 4) * 64];
                        const double2 lc = e[(l * 4 + 1) * 64];
                        const double z = (x - ms.x) * ms.y;
                        const double acc = lc.x + (lc.y + (-0.5 * (z * z)));
                        reinterpret_cast<double *>(e + (l * 4 + 3) * 64)[1] = acc;
                        mx = fmax(mx, acc);
                    }
                    const double mz = (mx == dev_ninf()) ? 0.0 : mx;
                    double sum = 0.0;
                    for (int l = 0; l < L; ++l) {
                        double *sc = reinterpret_cast<double *>(e + (l * 4 + 3) * 64) + 1;
                        const double en = exp(*sc - mz);
                        sum += en;
                        *sc = en;
                    }
                    ob = mz + log(sum);
                    inv[k] = 1.0 / sum;
                }
                lw[k] = ((t == 0) ? lp[k] + ob : ob) + lw[k];
            }
            /* the step's posterior and its factor of the likelihood */
            double q[K];
            {
                double qm, qs;
                ll += eio_lse<K>(lw, q, qm, qs);
                const double rq = 1.0 / qs; /* lw = -inf (p_1k = 0): an exact 0 */
#pragma unroll
                for (int k = 0; k < K; ++k)
                    q[k] = q[k] * rq;
            }
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    n1[k] = q[k];
            }
            /* dl/dw: (q_t - A_{t+1}) u_{t+1}' */
            if (nx) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double dk = q[k] - A[k];
                    if constexpr (GWR) {
#pragma unroll
                        for (int m = 0; m < MMAX; ++m)
                            gw[k][m] = fma(dk, un[m], gw[k][m]);
                    } else {
#pragma unroll
                        for (int mp = 0; mp < MP; ++mp) {
                            double2 *g = slab + (gw0 + k * MP + mp) * 64;
                            double2 acc = *g;
                            acc.x = fma(dk, un[2 * mp], acc.x);
                            acc.y = fma(dk, un[2 * mp + 1], acc.y);
                            *g = acc;
                        }
                    }
                }
            }
            /* the emission sums */
            const double x2 = x * x;
            if constexpr (REG) {
                double pr[TRI], xu[MMAX];
                {
                    int idx = 0;
#pragma unroll
                    for (int m = 0; m < MMAX; ++m) {
                        xu[m] = x * u[m];
#pragma unroll
                        for (int m2 = m; m2 < MMAX; ++m2)
                            pr[idx++] = u[m] * u[m2];
                    }
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    double2 *s = slab + k * SK * 64;
#pragma unroll
                    for (int j = 0; j < TRI / 2; ++j) {
                        double2 acc = s[j * 64];
                        acc.x = fma(q[k], pr[2 * j], acc.x);
                        acc.y = fma(q[k], pr[2 * j + 1], acc.y);
                        s[j * 64] = acc;
                    }
#pragma unroll
                    for (int mp = 0; mp < MP; ++mp) {
                        double2 acc = s[(TRI / 2 + mp) * 64];
                        acc.x = fma(q[k], xu[2 * mp], acc.x);
                        acc.y = fma(q[k], xu[2 * mp + 1], acc.y);
                        s[(TRI / 2 + mp) * 64] = acc;
                    }
                    double2 acc = s[(SK - 1) * 64];
                    acc.x += q[k];
                    acc.y = fma(q[k], x2, acc.y);
                    s[(SK - 1) * 64] = acc;
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    double2 *e = slab + k * L * 4 * 64;
                    for (int l = 0; l < L; ++l) {
                        double2 ns = e[(l * 4 + 2) * 64];
                        double2 se = e[(l * 4 + 3) * 64];
                        /* r_t(k,l) = q_t(k) * numerator / sum; a state with q = 0 counts nothing */
                        const double r = (q[k] == 0.0) ? 0.0 : q[k] * (se.y * inv[k]);
                        ns.x += r;
                        ns.y = fma(r, x, ns.y);
                        se.x = fma(r, x2, se.x);
                        e[(l * 4 + 2) * 64] = ns;
                        e[(l * 4 + 3) * 64] = se;
                    }
                }
            }
        }
        x = xn;
#pragma unroll
        for (int m = 0; m < MMAX; ++m)
            u[m] = un[m];
    }

    /* ---- the [P, ...] outputs ---- */
    const uint32_t po = (uint32_t)p * 8u;
    const bool bad = !__builtin_isfinite(ll);
    const double nanv = dev_nan();
    put_out(o.loglik, po, ll);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        put_out(o.n1 + a.P * (int64_t)k, po, bad ? nanv : n1[k]);
#pragma unroll
        for (int m = 0; m < MMAX; ++m) {
            if (m < M) {
                double g;
                if constexpr (GWR) {
                    g = gw[k][m];
                } else {
                    const double2 acc = slab[(gw0 + k * MP + m / 2) * 64];
                    g = (m & 1) ? acc.y : acc.x;
                }
                put_out(o.gw + a.P * ((int64_t)k + (int64_t)K * m), po, bad ? nanv : g);
            }
        }
    }
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double2 *s = slab + k * SK * 64;
            const double2 nxx = s[(SK - 1) * 64];
            put_out(o.nk + a.P * (int64_t)k, po, bad ? nanv : nxx.x);
            put_out(o.xx + a.P * (int64_t)k, po, bad ? nanv : nxx.y);
            int idx = 0;
#pragma unroll
            for (int m = 0; m < MMAX; ++m) {
                if (m < M) {
                    const double2 acc = s[(TRI / 2 + m / 2) * 64];
                    put_out(o.ux + a.P * ((int64_t)k + (int64_t)K * m), po, bad ? nanv : (m & 1) ? acc.y : acc.x);
                }
#pragma unroll
                for (int m2 = m; m2 < MMAX; ++m2, ++idx) {
                    if (m2 < M) { /* both halves from the one accumulator: bitwise symmetric */
                        const double2 acc = s[(idx / 2) * 64];
                        const double val = bad ? nanv : (idx & 1) ? acc.y : acc.x;
                        put_out(o.uu + a.P * ((int64_t)k + (int64_t)K * (m + (int64_t)M * m2)), po, val);
                        if (m2 != m)
                            put_out(o.uu + a.P * ((int64_t)k + (int64_t)K * (m2 + (int64_t)M * m)), po, val);
                    }
                }
            }
        }
    } else {
        for (int k = 0; k < K; ++k)
            for (int l = 0; l < L; ++l) {
                const double2 *e = slab + (k * L + l) * 4 * 64;
                const double2 ns = e[2 * 64];
                const double2 se = e[3 * 64];
                const int64_t ix = a.P * ((int64_t)k + (int64_t)K * l);
                put_out(o.nkl + ix, po, bad ? nanv : ns.x);
                put_out(o.sx + ix, po, bad ? nanv : ns.y);
                put_out(o.sxx + ix, po, bad ? nanv : se.x);
            }
    }
    if (o.status) {
        bool inv = false;
        if (a.T)
            inv = a.T[n] < 1 || a.T[n] > a.Tmax;
        o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
    }
}

static bool estep_io_model(int m) { return m >= HHMM_MODEL_IOHMM_REG && m <= HHMM_MODEL_IOHMM_HMIX_LITE; }

/* Waves per workgroup and its LDS for a shape inside the kernel's classes. */
static int estep_io_waves(bool reg, int K, int M, int L, size_t *lds)
{
    return waves_that_fit(eio_wave_bytes(reg, K, M <= 4 ? 4 : 8, L), lds);
}

hhmm_status check_estep_io(const hhmm_request *r, const hhmm_estep_io_result *o)
{
    const char *entry = "IOHMM E-step";
    const hhmm_status s = stats_check_head(entry, r, estep_io_model,
                                           "the IOHMM programs, models 4..7, only; the HMM family has hhmm_estep and "
                                           "the masked programs hhmm_expected_stats");
    if (s != HHMM_OK)
        return s;
    const bool reg = r->model == HHMM_MODEL_IOHMM_REG;
    const int K = r->data.K, M = r->data.M, L = reg ? 0 : r->data.L;
    if (K >= 1 && M >= 1 && (reg || L >= 1)) {
        if (M > 8) {
            set_error("%s: M = %d, the lane-per-pair kernel supports M <= 8", entry, M);
            return HHMM_ERR_UNSUPPORTED;
        }
        if (L > kIoLmax) {
            set_error("%s: L = %d, the lane-per-pair kernel supports L <= %d", entry, L, kIoLmax);
            return HHMM_ERR_UNSUPPORTED;
        }
        size_t lds;
        if (estep_io_waves(reg, K, M, L, &lds) < 1) {
            set_error("%s: K = %d, M = %d, L = %d: the accumulators of one wave (%zu bytes) do not fit in LDS", entry,
                      K, M, L, eio_wave_bytes(reg, K, M <= 4 ? 4 : 8, L));
            return HHMM_ERR_UNSUPPORTED;
        }
    }
    if (!o) {
        set_error("%s: result must be non-NULL", entry);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (!o->loglik || !o->n_1k || !o->gw_km ||
        (reg ? !o->n_k || !o->uu_kmm || !o->ux_km || !o->xx_k : !o->n_kl || !o->sx_kl || !o->sxx_kl)) {
        set_error("%s: loglik, n_1k, gw_km and %s must be non-NULL", entry,
                  reg ? "n_k, uu_kmm, ux_km and xx_k" : "n_kl, sx_kl and sxx_kl");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return HHMM_OK;
}

template <int FAM, int K, int MMAX>
static bool launch_estep_io_k(const DevArgs &a, const EstepIoOut &o, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    /* a class no shape of which fits is not instantiated (check_estep_io rejects it) */
    if constexpr (eio_wave_bytes(FAM == IO_REG, K, MMAX, FAM == IO_REG ? 0 : 1) <= kLdsLimit) {
        hipLaunchKernelGGL((estep_io_kernel<FAM, K, MMAX>), grid, block, lds, st, a, o);
        return true;
    }
    return false;
}

hhmm_status launch_estep_io(const hhmm_request *r, const hhmm_estep_io_result *res, int64_t P, void *ws, hipStream_t st)
{
    DevArgs a = stats_dev_args(r, P, ws);
    const bool reg = r->model == HHMM_MODEL_IOHMM_REG;
    a.M = r->data.M;
    a.L = reg ? 0 : r->data.L;
    a.xr = r->data.x_real;
    a.u = r->data.u;
    a.w_km = r->draws.w_km;
    a.b_km = r->draws.b_km;
    a.s_k = r->draws.s_k;
    a.lambda_kl = r->draws.lambda_kl;
    a.mu_kl = r->draws.mu_kl;
    a.s_kl = r->draws.s_kl;
    const EstepIoOut o{res->loglik, res->n_1k, res->gw_km, res->n_k,    res->uu_kmm,     res->ux_km,
                       res->xx_k,   res->n_kl, res->sx_kl, res->sxx_kl, res->pair_status};
    size_t lds = 0;
    const int waves = (a.M >= 1 && a.M <= 8 && a.L <= kIoLmax) ? estep_io_waves(reg, a.K, a.M, a.L, &lds) : 0;
    if (waves < 1) {
        set_error("IOHMM E-step: the accumulators of K = %d, M = %d, L = %d do not fit in LDS", a.K, a.M, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int threads = 64 * waves;
    const dim3 grid((unsigned)((P + threads - 1) / threads)), block(threads);
    bool ok = false;
    const bool launched = dispatch_k(a.K, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (reg)
            ok = a.M <= 4 ? launch_estep_io_k<IO_REG, K, 4>(a, o, grid, block, lds, st)
                          : launch_estep_io_k<IO_REG, K, 8>(a, o, grid, block, lds, st);
        else
            ok = a.M <= 4 ? launch_estep_io_k<IO_MIX, K, 4>(a, o, grid, block, lds, st)
                          : launch_estep_io_k<IO_MIX, K, 8>(a, o, grid, block, lds, st);
    });
    if (!launched || !ok) {
        set_error("IOHMM E-step: model %d at K = %d, M = %d has no kernel", a.model, a.K, a.M);
        return HHMM_ERR_UNSUPPORTED;
    }
    return launch_status("estep_io_kernel");
}

} // namespace hhmm
