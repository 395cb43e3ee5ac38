/*
 * hhmm_estep_scan.hip -- the E-step (include/hhmm_estep.h) and the expected
 * draw statistics (include/hhmm_expect.h) as a parallel scan over T, for few
 * pairs and long series, at K <= 8: hmm, hmm-multinom, hmm-multinom-semisup and
 * hhmm-tayal2009.  Four launches on one stream:
 *   phase 1  scan_prod_kernel<.., BWD = false> (hhmm_scan.h): the forward
 *            product of every (pair, T-chunk).
 *   phase 2  scan_bound_kernel<.., ADJ = true>: the filter entering every chunk
 *            (sc_st), the loglik, and beta at every chunk's last step (sc_be).  The E-step
 *            sweeps the ADJOINT of the forward pass, beta_{t-1} = F_t beta_t,
 *            so the backward walk takes the same forward products as column
 *            maps: no backward products are formed.
 *   phase 3  estep_scan_kernel: one LANE owns one (pair, T-chunk) and runs
 *            estep_kernel's two sweeps (hhmm_estep.hip) over its chunk: forward
 *            from sc_st with a checkpoint every C = fb_chunk(K) steps, then
 *            backward from sc_be, sub-chunk by sub-chunk, with the transitions
 *            INTO its own steps t0 .. t1-1 (hhmm_estep_step.h).  The one into
 *            t0 takes alpha_{t0-1} = sc_st; the one into t1 is the next chunk's;
 *            chunk 0 has none into step 0 and forms gamma_1 and the first
 *            emission term instead.  So the chunks partition the T-1
 *            transitions and the T emission terms.  Every step divides by its
 *            own Z: the power-of-two scales of the chunk-local alpha and beta
 *            cancel, no exponent is tracked, and both are renormalised every
 *            step as in the lane kernel (phase 1 keeps scan_prod_kernel's
 *            renorm_sparse_safe cadence).
 *   reduce   estep_scan_reduce_kernel: one thread per (pair, statistic) adds
 *            the partials in chunk order, applies A(i,j) to xi once, NaNs a
 *            pair with a bad step or a non-finite loglik, writes pair_status.
 * No floating-point atomics: the same bits on every run and from both entries.
 *
 * Lane mapping of phase 3: CHUNK-fastest.  A pair's nc chunks are padded to
 * ncw = whole waves, lane g = p * ncw + c, so a wave holds 64 consecutive
 * chunks of ONE pair.  With pair-fastest lanes (fb_scan_kernel) a batch of one
 * pair would leave 63 lanes of every wave redoing lane 0's chunk; here one pair
 * fills its waves, and because a wave's partials belong to one pair it adds
 * them with a fixed xor butterfly (__shfl_xor, 6 levels; every lane ends with
 * the same bits) and lane 0 stores ONE record per wave: the partials are 64
 * times smaller than one per lane and the reduction 64 times shorter.  The
 * price: the lanes of a wave stand at different steps, so the observation
 * loads are strided by the chunk length (each lane walks its own cache lines)
 * and a wave rarely shares a Tayal sign class.  Lanes past the pair's last
 * chunk, and chunks past a ragged pair's end, sweep nothing and add exact zeros.
 *
 * Storage is estep_kernel's: xi in K^2 registers (LDS for the Gaussian kernels
 * at K >= 7), the emission table and the c_kl slab per wave in LDS (every lane
 * its own column, conflict-free 16-byte accesses), workgroups of estep_waves
 * waves.  Budget (hipcc --save-temps resource listing, gfx950): DESIGN.md §3.11c.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_estep_step.h"
#include "hhmm_scan.h"
#include "hhmm_stats.h"

namespace hhmm {

/* What phase 3 and the reduction take beside DevArgs. */
struct EsScanArgs {
    double *part;   /* [P][nwp][ns + kEstepScanTail] one record per wave of phase 3 */
    double *pa;     /* [P][K][K] each pair's A as its kernel holds it */
    int32_t ncw;    /* phase-3 lanes per pair: nc rounded up to whole waves */
    int32_t nwp;    /* ncw / 64 */
    int32_t ns;     /* statistics per pair, in the outputs' order: n_1k, xi_ij, then c_kl or w_k, s1_k, s2_k */
};

/* The reduction's outputs (both result layouts: the other family's pointers are unused). */
struct EsScanOut {
    double *loglik, *n1, *xi, *c, *w, *s1, *s2;
    int32_t *status;
    int32_t ahi; /* the auxiliary stream's upper bound: G (semisup), 2 (Tayal) */
};

/* Sum over the wave's lanes in a fixed order; every lane returns the same bits. */
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

template <int MODEL, int K>
__global__ void __launch_bounds__(kBlock) estep_scan_kernel(const DevArgs a, const EsScanArgs s)
{
    constexpr int C = fb_chunk(K);
    constexpr int KP = (K + 1) / 2;
    constexpr bool GAUSS = ModelTraits<MODEL>::kGauss;
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
    HIP_DYNAMIC_SHARED(double2, lds)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * nw + wave;
    if (gw >= a.P * (int64_t)s.nwp) /* wave-uniform; the kernel has no workgroup barrier */
        return;
    const int64_t p = gw / s.nwp;
    const int c = (int)(gw % s.nwp) * 64 + lane; /* this lane's T-chunk */
    int64_t n, d;
    pair_coords(a, p, n, d);
    const int Tpair = pair_len(a, n);
    const bool live = (int64_t)c * a.scan_cl < (int64_t)Tpair;

    FbLane<MODEL, K> ln;
    ln.p = p;
    ln.n = n;
    ln.L = a.L;
    /* a lane without steps stands on [0, 0): every step predicate is false */
    ln.t0 = live ? c * a.scan_cl : 0;
    ln.Tp = live ? (int)min((int64_t)ln.t0 + a.scan_cl, (int64_t)Tpair) : 0;
    ln.cb = ln.t0 / C;
    ln.q = gw * 64 + lane; /* checkpoint column: < P * ncw < 2^29 (estep_scan_plan) */
    ln.Qs = a.P * (int64_t)s.ncw;
    const size_t slab_elems = GAUSS ? 0 : (size_t)a.L * KP * 64;
    double2 *const pslab = lds + (size_t)wave * slab_elems + lane;
    double2 *const cslab = lds + (size_t)(nw + wave) * slab_elems + lane;
    ln.slab = pslab;
    load_params<MODEL, K, false>(ln.pp, a, d);
    if constexpr (!GAUSS) {
        if constexpr (AUX)
            ln.pp.skip_ok &= fill_table<K, false>(pslab, a, d);
        else
            fill_table<K, false>(pslab, a, d);
        for (int i = 0; i < a.L * KP; ++i)
            cslab[i * 64] = make_double2(0.0, 0.0);
    }
    constexpr bool XL = estep_xi_lds<MODEL, K>();
    double *const xs = reinterpret_cast<double *>(lds) + (size_t)wave * (K * K * 64) + lane;
    if constexpr (XL) {
#pragma unroll
        for (int i = 0; i < K * K; ++i)
            xs[i * 64] = 0.0;
    }
    const SeriesPtrs sp = series_ptrs<MODEL, AUX>(a, n);
    /* sub-chunks (checkpoint rows) any lane of the wave needs: <= scan_cl / C */
    const int nsub = (wave_max(ln.Tp - ln.t0) + C - 1) / C;
    const uint32_t qo = (uint32_t)ln.q * 8u;

    /* ---- forward sweep over the chunk: checkpoints only ---- */
    uint32_t xm = 0, am = 0;
    Obs cur[C];
    {
        double al[K];
#pragma unroll
        for (int k = 0; k < K; ++k) /* alpha_{t0-1}; chunk 0 starts from the model's init */
            al[k] = (live && c > 0) ? a.sc_st[p + a.P * ((int64_t)c * K + k)] : 0.0;
        double lsc = 0.0;
        int ex = 0;
        load_chunk<MODEL, C, AUX>(cur, sp, ln.t0);
        Em<K> ecur;
        emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[0], ecur);
        for (int r = 0; r < nsub; ++r) {
            Obs nxt[C];
            load_chunk<MODEL, C, AUX>(nxt, sp, ln.t0 + (r + 1) * C);
            fwd_chunk<MODEL, K, C, FB_GAMMA, false>(a, ln, ln.cb + r, cur, nxt[0], ecur, al, lsc, ex);
            if constexpr (!GAUSS)
                xcheck_acc<C, false>(xm, cur, ln.cb + r, ln.Tp);
            if constexpr (AUX)
                auxcheck_acc<C, false>(am, cur, ln.cb + r, ln.Tp);
#pragma unroll
            for (int u = 0; u < C; ++u)
                cur[u] = nxt[u];
        }
    }

    /* ---- backward sweep, sub-chunk by sub-chunk from the chunk's end ---- */
    double xi[K][K], be[K], n1[K], w[K], s1[K], s2[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        be[i] = live ? a.sc_be[p + a.P * ((int64_t)c * K + i)] : 1.0; /* beta at the chunk's last step */
        n1[i] = w[i] = s1[i] = s2[i] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            xi[i][j] = 0.0;
    }
    bool bad = false;
    double x0 = 0.0; /* x_1 (Gaussian) */
    int aux1 = 0;    /* g_1 / sign_1 */
    if (nsub > 0) {  /* wave-uniform */
        const int rlast = nsub - 1;
        load_chunk<MODEL, C, AUX>(cur, sp, ln.t0 + rlast * C);
        /* checkpoint rows are wave-uniform: a lane shorter than the wave reads
         * (unused) slots past its own last sub-chunk, never past the allocation */
        double ck[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = get_tmp(a.ckpt + ln.Qs * ((int64_t)rlast * K + k), qo);
        Obs onext = cur[0];
        for (int r = rlast; r >= 0; --r) {
            const int t0 = ln.t0 + r * C;
            Obs nxt[C];
            load_chunk<MODEL, C, AUX>(nxt, sp, t0 - C);
            double cn[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                cn[k] = get_tmp(a.ckpt + ln.Qs * ((int64_t)max(r - 1, 0) * K + k), qo);
            /* alpha over the sub-chunk from its checkpoint */
            double abuf[C][K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                abuf[0][k] = ck[k];
            {
                int exb = 0;
                Em<K> ecur;
                emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[1 < C ? 1 : 0], ecur);
#pragma unroll
                for (int u = 1; u < C; ++u) {
                    Em<K> enx;
                    emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[u + 1 < C ? u + 1 : u], enx);
                    if (t0 + u < ln.Tp) {
                        if constexpr (ModelTraits<MODEL>::kTayal) {
                            fwd_step_raw<MODEL, K>(abuf[u - 1], abuf[u], ln.pp, ecur.e, cur[u]);
                            renorm<K>(abuf[u], exb);
                        } else {
                            fwd_step_to<MODEL, K>(abuf[u - 1], abuf[u], ln.pp, ecur.e, cur[u], exb);
                        }
                    }
                    ecur = enx;
                }
            }
            /* transitions into steps t0 + C (the next sub-chunk's first; the next
             * T-chunk's is not this lane's: t0 + C == ln.Tp there) .. t0 + 1 */
            Em<K> ecur;
            emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, onext, ecur);
#pragma unroll
            for (int v = C; v >= 1; --v) {
                const Obs &ob = (v < C) ? cur[v < C ? v : 0] : onext;
                Em<K> enx;
                emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[v - 1 >= 1 ? v - 1 : 1 < C ? 1 : 0], enx);
                if (t0 + v < ln.Tp) {
                    double g[K];
                    double Z = 0.0;
                    if constexpr (AUX)
                        tayal_dispatch<MODEL>(ob, ln.pp.skip_ok, [&](auto sgc) {
                            Z = expect_transition<MODEL, K, decltype(sgc)::value>(ln.pp, abuf[v - 1], ecur.e, ob, be,
                                                                                  xi, g);
                        });
                    else
                        Z = estep_transition<MODEL, K>(ln.pp, abuf[v - 1], ecur.e, be, xi, xs, g);
                    bad |= !((Z > 0.0) & (Z < __builtin_inf()));
                    estep_emit_acc<MODEL, K>(cslab, a.L, ob, g, w, s1, s2);
                }
                ecur = enx;
            }
            if (r == 0 && live) {
                if (c == 0) { /* the series' first step: gamma_1 = alpha_1 .* beta_1 / their sum */
                    double Z = 0.0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        n1[k] = abuf[0][k] * be[k];
                        Z += n1[k];
                    }
                    const double rz = 1.0 / Z;
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        n1[k] *= rz;
                    bad |= !((Z > 0.0) & (Z < __builtin_inf()));
                    if constexpr (GAUSS) /* Q2: x_1 counts with weight 1 for every state */
                        x0 = cur[0].xr;
                    else
                        estep_emit_acc<MODEL, K>(cslab, a.L, cur[0], n1, w, s1, s2);
                    if constexpr (AUX)
                        aux1 = cur[0].aux;
                } else { /* the transition into the chunk's first step, from alpha_{t0-1} = sc_st */
                    double ap[K], g[K];
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        ap[k] = a.sc_st[p + a.P * ((int64_t)c * K + k)];
                    Em<K> e0;
                    emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[0], e0);
                    double Z = 0.0;
                    if constexpr (AUX)
                        tayal_dispatch<MODEL>(cur[0], ln.pp.skip_ok, [&](auto sgc) {
                            Z = expect_transition<MODEL, K, decltype(sgc)::value>(ln.pp, ap, e0.e, cur[0], be, xi, g);
                        });
                    else
                        Z = estep_transition<MODEL, K>(ln.pp, ap, e0.e, be, xi, xs, g);
                    bad |= !((Z > 0.0) & (Z < __builtin_inf()));
                    estep_emit_acc<MODEL, K>(cslab, a.L, cur[0], g, w, s1, s2);
                }
            }
            onext = cur[0];
#pragma unroll
            for (int u = 0; u < C; ++u)
                cur[u] = nxt[u];
#pragma unroll
            for (int k = 0; k < K; ++k)
                ck[k] = cn[k];
        }
    }

    /* ---- the wave's record: its 64 partials added in a fixed order, stored by lane 0 ---- */
    double *const rec = s.part + gw * (int64_t)(s.ns + kEstepScanTail);
    const bool l0 = lane == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum(n1[k]);
        if (l0)
            rec[k] = v;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double v = wave_sum(XL ? xs[(i * K + j) * 64] : xi[i][j]);
            if (l0)
                rec[K + i + K * j] = v;
        }
    if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double vw = wave_sum(w[k]), v1 = wave_sum(s1[k]), v2 = wave_sum(s2[k]);
            if (l0) {
                rec[K + K * K + k] = vw;
                rec[K + K * K + K + k] = v1;
                rec[K + K * K + 2 * K + k] = v2;
            }
        }
    } else {
        for (int l = 0; l < a.L; ++l) {
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const double2 v = cslab[(l * KP + kp) * 64];
                const double vx = wave_sum(v.x), vy = wave_sum(v.y);
                if (l0) {
                    rec[K + K * K + 2 * kp + K * l] = vx;
                    if (2 * kp + 1 < K)
                        rec[K + K * K + 2 * kp + 1 + K * l] = vy;
                }
            }
        }
    }
    const bool wbad = __ballot(bad) != 0;
    const uint32_t wxm = wave_umax(xm), wam = wave_umax(am);
    if (l0) {
        rec[s.ns + 0] = wbad ? 1.0 : 0.0;
        rec[s.ns + 1] = (double)wxm;
        rec[s.ns + 2] = (double)wam;
        rec[s.ns + 3] = (double)aux1; /* chunk 0 is lane 0 of the pair's first wave; 0 elsewhere */
        rec[s.ns + 4] = x0;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j)
                    s.pa[p * (int64_t)(K * K) + i * K + j] = ln.pp.A[i][j];
        }
    }
}

/* One thread per (pair, statistic): the pair's records added in chunk order,
 * then estep_kernel's epilogue -- A(i,j) on xi (an entry of a masked program
 * that no step switched on is 0 whatever A is; a zero in A gives an exact
 * zero), Tayal's init predicate on n_1k, the Gaussian x_1 terms, NaN for a pair
 * with a bad step or a non-finite loglik -- and pair_status. */
__global__ void __launch_bounds__(256) estep_scan_reduce_kernel(const DevArgs a, const EsScanArgs s, const EsScanOut o)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.P * (int64_t)s.ns)
        return;
    const int64_t p = g / s.ns;
    const int q = (int)(g % s.ns);
    const int K = a.K;
    const int rs = s.ns + kEstepScanTail;
    const double *rec = s.part + p * (int64_t)s.nwp * rs;
    double acc = 0.0;
    bool bad = false;
    uint32_t xm = 0, am = 0;
    for (int wv = 0; wv < s.nwp; ++wv) {
        const double *rw = rec + (int64_t)wv * rs;
        acc += rw[q];
        bad |= rw[s.ns] != 0.0;
        xm = max(xm, (uint32_t)rw[s.ns + 1]);
        am = max(am, (uint32_t)rw[s.ns + 2]);
    }
    const double ll = o.loglik[p];
    bad |= !__builtin_isfinite(ll);
    const bool gauss = a.model == HHMM_MODEL_HMM_GAUSS, tayal = a.model == HHMM_MODEL_TAYAL;
    const bool aux = tayal || a.model == HHMM_MODEL_HMM_MULTINOM_SEMISUP;
    double v = acc;
    double *dst;
    if (q < K) {
        if (tayal && !tayal_init_pred((int)rec[s.ns + 3], q)) /* the init factor p_1k applies at (sign_1, k) */
            v = 0.0;
        dst = o.n1 + a.P * (int64_t)q;
    } else if (q < K + K * K) {
        const int e = q - K, i = e % K, j = e / K;
        const double A = s.pa[p * (int64_t)(K * K) + i * K + j];
        v = (aux && acc == 0.0) ? 0.0 : A * acc;
        dst = o.xi + a.P * (int64_t)e;
    } else if (gauss) {
        const int e = q - K - K * K, k = e % K, m = e / K;
        const double x0 = rec[s.ns + 4];
        v = (m == 0 ? 1.0 : m == 1 ? x0 : x0 * x0) + acc;
        dst = (m == 0 ? o.w : m == 1 ? o.s1 : o.s2) + a.P * (int64_t)k;
    } else {
        dst = o.c + a.P * (int64_t)(q - K - K * K);
    }
    dst[p] = bad ? dev_nan() : v;
    if (q == 0 && o.status) {
        int64_t n, d;
        pair_coords(a, p, n, d);
        bool inv = !gauss && xm >= (uint32_t)a.L;
        if (aux)
            inv |= am >= (uint32_t)o.ahi;
        if (a.T)
            inv |= a.T[n] < 1 || a.T[n] > a.Tmax;
        o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
    }
}

size_t estep_scan_workspace_bytes(const hhmm_request *r, int64_t P)
{
    const EstepScanLayout w = estep_scan_layout(r->model, r->data.K, r->data.L, r->data.T_max, P,
                                                (uint32_t)r->flags | HHMM_FLAG_SCAN_FORCE);
    return w.total ? w.total + 256 : 0; /* the regions start at the first 256-byte boundary of the workspace */
}

template <int MODEL, int K>
static void launch_estep_scan_k(const DevArgs &a, const EsScanArgs &s, dim3 grid1, dim3 block1, size_t lds1,
                                dim3 grid3, dim3 block3, size_t lds3, hipStream_t st)
{
    hipLaunchKernelGGL((scan_prod_kernel<MODEL, K, false>), grid1, block1, lds1, st, a);
    hipLaunchKernelGGL((scan_bound_kernel<MODEL, K, true, true>), dim3((unsigned)a.P, 2), dim3(64 * kBoundWaves), 0, st,
                       a);
    hipLaunchKernelGGL((estep_scan_kernel<MODEL, K>), grid3, block3, lds3, st, a, s);
}

template <int MODEL, class... Args>
static bool launch_estep_scan_m(const DevArgs &a, Args &&...args)
{
    return dispatch_k(a.K, [&](auto kc) { launch_estep_scan_k<MODEL, decltype(kc)::value>(a, args...); });
}

hhmm_status launch_estep_scan(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws, hipStream_t st)
{
    const char *entry = "T-scan E-step";
    DevArgs a = stats_dev_args(r, P, ws);
    const bool gauss = a.model == HHMM_MODEL_HMM_GAUSS;
    if (gauss)
        a.L = 0; /* no tables */
    a.x = r->data.x_int;
    a.xr = r->data.x_real;
    a.phi_k = r->draws.phi_k;
    a.mu_k = r->draws.mu_k;
    a.sigma_k = r->draws.sigma_k;
    a.g = r->data.g;
    a.sign = r->data.sign;
    a.p_11 = r->draws.p_11;
    a.A_row = r->draws.A_row;
    a.flags = (uint32_t)r->flags;
    a.outputs = HHMM_OUT_LOGLIK; /* scan_bound_kernel's forward walk writes it */
    a.loglik = res->loglik;
    const EstepScanLayout w =
        estep_scan_layout(a.model, a.K, a.L, a.Tmax, P, a.flags | HHMM_FLAG_SCAN_FORCE);
    if (w.total == 0) {
        set_error("%s: no T-scan for model %d at K = %d with P = %lld pairs and T_max = %d (HHMM_FLAG_SCAN_OFF, or "
                  "2^29 (pair, chunk) lanes reached: ask for longer chunks)",
                  entry, a.model, a.K, (long long)P, a.Tmax);
        return HHMM_ERR_UNSUPPORTED;
    }
    char *b = (char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    a.scan_cl = w.sp.cl;
    a.scan_nc = w.sp.nc;
    a.sc_mf = (double *)(b + w.mf);
    a.sc_mx = (double *)(b + w.mx);
    a.sc_st = (double *)(b + w.st);
    a.sc_sl = (double *)(b + w.sl);
    a.sc_be = (double *)(b + w.be);
    a.sc_bl = (double *)(b + w.bl);
    a.ckpt = (double *)(b + w.ckpt);
    const EsScanArgs s{(double *)(b + w.part), (double *)(b + w.pa), (int32_t)w.ncw, (int32_t)w.nwp, w.ns};
    const EsScanOut o{res->loglik, res->n_1k, res->xi_ij, res->c_kl, res->w_k, res->s1_k, res->s2_k, res->pair_status,
                      a.model == HHMM_MODEL_TAYAL ? 2 : r->data.G};
    /* phase 1: scan_prod_kernel's shape (one emission table per wave) */
    size_t lds1 = 0, lds3 = 0;
    const int waves1 = waves_that_fit(gauss ? 0 : (size_t)a.L * ((a.K + 1) / 2) * 64 * sizeof(double2), &lds1);
    const int waves3 = estep_waves(a.model, a.K, a.L, &lds3);
    if (waves1 < 1 || waves3 < 1) {
        set_error("%s: the tables of K*L = %d*%d do not fit in LDS", entry, a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int64_t G1 = P * (int64_t)a.scan_nc, W3 = P * w.nwp;
    const dim3 block1(64 * waves1), grid1((unsigned)((G1 + block1.x - 1) / block1.x));
    const dim3 block3(64 * waves3), grid3((unsigned)((W3 + waves3 - 1) / waves3));
    bool ok = false;
    if (a.model == HHMM_MODEL_HMM_GAUSS)
        ok = launch_estep_scan_m<HHMM_MODEL_HMM_GAUSS>(a, s, grid1, block1, lds1, grid3, block3, lds3, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM)
        ok = launch_estep_scan_m<HHMM_MODEL_HMM_MULTINOM>(a, s, grid1, block1, lds1, grid3, block3, lds3, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        ok = launch_estep_scan_m<HHMM_MODEL_HMM_MULTINOM_SEMISUP>(a, s, grid1, block1, lds1, grid3, block3, lds3, st);
    else if (a.model == HHMM_MODEL_TAYAL && a.K == 4) {
        launch_estep_scan_k<HHMM_MODEL_TAYAL, 4>(a, s, grid1, block1, lds1, grid3, block3, lds3, st);
        ok = true;
    }
    if (!ok) {
        set_error("%s: model %d at K = %d has no kernel (K outside 1..%d)", entry, a.model, a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int64_t GR = P * (int64_t)w.ns;
    hipLaunchKernelGGL(estep_scan_reduce_kernel, dim3((unsigned)((GR + 255) / 256)), dim3(256), 0, st, a, s, o);
    return launch_status("estep_scan_kernel");
}

} // namespace hhmm
