/*
 * hhmm_estep.hip -- gfx950 kernel of the batched E-step (include/hhmm_estep.h)
 * and of the expected draw statistics (include/hhmm_expect.h): per (series,
 * draw) pair the expected sufficient statistics summed over the steps --
 * gamma_1, the pairwise posterior sum xi_ij and the emission sums -- for hmm and
 * hmm-multinom, and under the coded path weight (hhmm_gibbs.h's counts) for
 * semisup and Tayal, at K <= 8.  Nothing is written per step.
 *
 * One kernel template: the masked programs are `if constexpr` arms on kAux
 * (kTayal where only Tayal differs).  One LANE owns one pair (the layout and
 * latency rules of hhmm_step.h, the chunk helpers of hhmm_fbchunk.h).
 *   forward   fb_kernel's scaled linear-space sweep (fwd_chunk applies the
 *             masks; g / sign is loaded beside x): a checkpoint of alpha every
 *             C = fb_chunk(K) steps, loglik at the end.
 *   backward  chunk by chunk from the end: alpha over the chunk is recomputed
 *             from its checkpoint, beta is carried.  The transition into step
 *             t >= 2 takes alpha_{t-1}, so a chunk handles the transitions
 *             into its steps 2..C and into the first step of the chunk after
 *             it.  With b_t = e_t .* beta_t:
 *                 beta_{t-1}(i) = sum_j A(i,j) b_t(j)
 *                 Z             = sum_i alpha_{t-1}(i) beta_{t-1}(i)
 *                 xi(i,j)      += alpha_{t-1}(i) A(i,j) b_t(j) / Z
 *                 gamma_t(j)    = sum_i of the same terms
 *             (A(i,j) is constant over t, so the accumulator takes it once, at
 *             the end: K^2 FMAs per step; a zero in A stays an exact zero.)
 *             One reciprocal per step: dividing by Z cancels every power-of-two
 *             scale of alpha and beta, so no exponent is tracked backward.
 *             gamma_1 = alpha_1 .* beta_1 / their sum.  A step with Z == 0 or
 *             a non-finite Z, or a non-finite loglik, makes the pair's
 *             statistics NaN.
 * The masked programs take the ADJOINT of the masked forward step
 * (expect_transition; bwd_step, the programs' own backward pass, is not:
 * semisup's is unmasked, Tayal's masks on the previous state).
 * Accumulators: xi in K^2 fp64 registers (in LDS for the Gaussian kernels at
 * K >= 7, estep_xi_lds); the Gaussian sums in 3K registers; c_kl in a second
 * LDS slab per wave with the phi table's layout (slab[(l * KP + kp) * 64 +
 * lane], double2), so the update of row x_t is the emission fetch's
 * conflict-free 16-byte pattern.  Two slabs cost 2 L ceil(K/2) KiB per wave;
 * the workgroup is sized to fit 160 KiB.
 * The [P, ...] stores are pair-fastest: one coalesced wave transaction each.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_estep_step.h"
#include "hhmm_stage.h"
#include "hhmm_stats.h"

namespace hhmm {

template <int MODEL, int K>
__global__ void __launch_bounds__(kBlock) estep_kernel(const DevArgs a, const EstepOutOf<MODEL> o)
{
    constexpr int C = fb_chunk(K);
    constexpr int KP = (K + 1) / 2;
    constexpr bool GAUSS = ModelTraits<MODEL>::kGauss;
    constexpr bool AUX = ModelTraits<MODEL>::kAux;
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
    const int Tw_min = wave_min(ln.Tp);
    const int Tw_max = wave_max(ln.Tp);
    const int nfull = Tw_min / C;            /* chunks complete for every lane */
    const int nchunk = (Tw_max + C - 1) / C; /* chunks any lane needs: <= ceil(Tmax / C) checkpoint rows */

    /* ---- forward sweep: fb_kernel's (masked), checkpoints only ---- */
    double ll;
    uint32_t xm = 0, am = 0;
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
        emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, grp[0][0], ecur);
        int c = 0;
        for (; c + D <= nfull; c += D) {
            Obs nxt[D][C];
#pragma unroll
            for (int i = 0; i < D; ++i)
                load_chunk<MODEL, C, AUX>(nxt[i], sp, (c + D + i) * C);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                fwd_chunk<MODEL, K, C, FB_GAMMA, true>(a, ln, c + i, grp[i],
                                                       (i + 1 < D) ? grp[i + 1 < D ? i + 1 : 0][0] : nxt[0][0], ecur,
                                                       al, lsc, ex);
                if constexpr (!GAUSS)
                    xcheck_acc<C, true>(xm, grp[i], c + i, ln.Tp);
                if constexpr (AUX)
                    auxcheck_acc<C, true>(am, grp[i], c + i, ln.Tp);
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
            fwd_chunk<MODEL, K, C, FB_GAMMA, false>(a, ln, c, cur, nxt[0], ecur, al, lsc, ex);
            if constexpr (!GAUSS)
                xcheck_acc<C, false>(xm, cur, c, ln.Tp);
            if constexpr (AUX)
                auxcheck_acc<C, false>(am, cur, c, ln.Tp);
#pragma unroll
            for (int u = 0; u < C; ++u)
                cur[u] = nxt[u];
        }
        ll = log(vsum<K>(al)) + (lsc + kLn2 * ex);
    }

    /* ---- backward sweep, chunk by chunk from the end ---- */
    double xi[K][K], be[K], n1[K], w[K], s1[K], s2[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        be[i] = 1.0; /* beta_T uniform */
        n1[i] = w[i] = s1[i] = s2[i] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            xi[i][j] = 0.0;
    }
    bool bad = !__builtin_isfinite(ll);
    double x0 = 0.0; /* x_1 (Gaussian) */
    int aux1 = 0;    /* g_1 / sign_1 */
    const int clast = nchunk - 1;
    load_chunk<MODEL, C, AUX>(cur, sp, clast * C);
    /* checkpoint rows are wave-uniform: a lane shorter than the wave reads
     * (unused) slots past its own last chunk, never past the allocation */
    double ck[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        ck[k] = get_tmp(a.ckpt + a.P * ((int64_t)clast * K + k), (uint32_t)p * 8u);
    Obs onext = cur[0];
    for (int c = clast; c >= 0; --c) {
        const int t0 = c * C;
        Obs nxt[C];
        load_chunk<MODEL, C, AUX>(nxt, sp, (c - 1) * C);
        double cn[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            cn[k] = get_tmp(a.ckpt + a.P * ((int64_t)max(c - 1, 0) * K + k), (uint32_t)p * 8u);
        /* alpha over the chunk from its checkpoint */
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
                    /* Tayal: fwd_step_to without its sign-class dispatch (the same
                     * bits): the recompute of a chunk stays straight-line code */
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
        /* transitions into steps t0 + C (the next chunk's first) .. t0 + 1 */
        Em<K> ecur;
        emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, onext, ecur);
#pragma unroll
        for (int v = C; v >= 1; --v) {
            const Obs &ob = (v < C) ? cur[v < C ? v : 0] : onext;
            Em<K> enx;
            emit_prob<MODEL, K>(ln.pp, ln.slab, ln.L, cur[v - 1 >= 1 ? v - 1 : 1], enx);
            if (t0 + v < ln.Tp) {
                double g[K];
                double Z = 0.0;
                if constexpr (AUX)
                    tayal_dispatch<MODEL>(ob, ln.pp.skip_ok, [&](auto sgc) {
                        Z = expect_transition<MODEL, K, decltype(sgc)::value>(ln.pp, abuf[v - 1], ecur.e, ob, be, xi,
                                                                              g);
                    });
                else
                    Z = estep_transition<MODEL, K>(ln.pp, abuf[v - 1], ecur.e, be, xi, xs, g);
                bad |= !((Z > 0.0) & (Z < __builtin_inf()));
                estep_emit_acc<MODEL, K>(cslab, a.L, ob, g, w, s1, s2);
            }
            ecur = enx;
        }
        if (c == 0) { /* the first step: gamma_1 = alpha_1 .* beta_1 / their sum */
            double Z = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                n1[k] = abuf[0][k] * be[k];
                Z += n1[k];
            }
            const double r = 1.0 / Z;
#pragma unroll
            for (int k = 0; k < K; ++k)
                n1[k] *= r;
            bad |= !((Z > 0.0) & (Z < __builtin_inf()));
            if constexpr (GAUSS) /* Q2: x_1 counts with weight 1 for every state */
                x0 = cur[0].xr;
            else
                estep_emit_acc<MODEL, K>(cslab, a.L, cur[0], n1, w, s1, s2);
            if constexpr (AUX)
                aux1 = cur[0].aux;
        }
        onext = cur[0];
#pragma unroll
        for (int u = 0; u < C; ++u)
            cur[u] = nxt[u];
#pragma unroll
        for (int k = 0; k < K; ++k)
            ck[k] = cn[k];
    }

    /* ---- the [P, ...] outputs ---- */
    const uint32_t po = (uint32_t)p * 8u;
    const double nanv = dev_nan();
    put_out(o.loglik, po, ll);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bool p1 = true; /* Tayal: the init factor p_1k applies at (sign_1, k) */
        if constexpr (ModelTraits<MODEL>::kTayal)
            p1 = tayal_init_pred(aux1, k);
        put_out(o.n1 + a.P * (int64_t)k, po, bad ? nanv : p1 ? n1[k] : 0.0);
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if constexpr (AUX) /* an entry no step switched on is 0 whatever A(i,j) is */
                put_out(o.xi + a.P * (int64_t)(i + K * j), po,
                        bad ? nanv : xi[i][j] != 0.0 ? ln.pp.A[i][j] * xi[i][j] : 0.0);
            else
                put_out(o.xi + a.P * (int64_t)(i + K * j), po,
                        bad ? nanv : ln.pp.A[i][j] * (XL ? xs[(i * K + j) * 64] : xi[i][j]));
        }
    if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            put_out(o.w + a.P * (int64_t)k, po, bad ? nanv : 1.0 + w[k]);
            put_out(o.s1 + a.P * (int64_t)k, po, bad ? nanv : x0 + s1[k]);
            put_out(o.s2 + a.P * (int64_t)k, po, bad ? nanv : x0 * x0 + s2[k]);
        }
    } else {
        for (int l = 0; l < a.L; ++l) {
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const double2 v = cslab[(l * KP + kp) * 64];
                put_out(o.c + a.P * ((int64_t)(2 * kp) + (int64_t)K * l), po, bad ? nanv : v.x);
                if (2 * kp + 1 < K)
                    put_out(o.c + a.P * ((int64_t)(2 * kp + 1) + (int64_t)K * l), po, bad ? nanv : v.y);
            }
        }
    }
    if (o.status) {
        bool inv = !GAUSS && xm >= (uint32_t)a.L;
        if constexpr (AUX) /* the whole expression: `inv |= am >= ahi` on the line above moves nine listings */
            inv = xm >= (uint32_t)a.L || am >= (uint32_t)o.ahi;
        if (a.T)
            inv |= a.T[n] < 1 || a.T[n] > a.Tmax;
        o.status[p] = inv ? HHMM_PAIR_INVALID_DATA : HHMM_PAIR_OK;
    }
}

/* Waves per workgroup and its LDS: two slabs per wave for the discrete programs. */
int estep_waves(int model, int K, int L, size_t *lds)
{
    if (model == HHMM_MODEL_HMM_GAUSS) { /* K >= 7: xi in LDS (estep_xi_lds) */
        *lds = K >= 7 ? (size_t)(kBlock / 64) * K * K * 64 * sizeof(double) : 0;
        return kBlock / 64;
    }
    return waves_that_fit(2 * (size_t)L * (size_t)((K + 1) / 2) * 64 * sizeof(double2), lds);
}

static int64_t estep_chunks(int K, int Tmax) { return ((int64_t)Tmax + fb_chunk(K) - 1) / fb_chunk(K); }

size_t estep_workspace_bytes(int K, int Tmax, int64_t P)
{
    return (size_t)estep_chunks(K, Tmax) * (size_t)K * (size_t)P * sizeof(double);
}

/* Both check_*: the entry's scope, then the LDS fit of the discrete programs' two tables of one wave. */
static hhmm_status estep_check(const char *entry, const hhmm_request *r, const hhmm_estep_result *o,
                               bool (*model_ok)(int), const char *scope, const char *above = nullptr)
{
    const hhmm_status s = stats_check_head(entry, r, model_ok, scope, 1, kMaxK, "hhmm_estep", above);
    if (s != HHMM_OK)
        return s;
    size_t lds;
    if (r->model != HHMM_MODEL_HMM_GAUSS && r->data.K >= 1 && r->data.L >= 1 &&
        estep_waves(r->model, r->data.K, r->data.L, &lds) < 1) {
        set_error("%s: L * ceil(K / 2) = %d * %d > 80: the emission table and its count table of one wave "
                  "do not fit in LDS",
                  entry, r->data.L, (r->data.K + 1) / 2);
        return HHMM_ERR_UNSUPPORTED;
    }
    return stats_check_tail(entry, r, o, false);
}

static bool estep_model(int m) { return m == HHMM_MODEL_HMM_GAUSS || m == HHMM_MODEL_HMM_MULTINOM; }

hhmm_status check_estep(const hhmm_request *r, const hhmm_estep_result *o)
{
    return estep_check("E-step", r, o, estep_model, "hmm and hmm-multinom only; the semisup and Tayal backward "
                                                    "passes are not the adjoint of their forward");
}

static bool expect_model(int m)
{
    return m == HHMM_MODEL_HMM_MULTINOM || m == HHMM_MODEL_HMM_MULTINOM_SEMISUP || m == HHMM_MODEL_TAYAL;
}

hhmm_status check_expected_stats(const hhmm_request *r, const hhmm_estep_result *o)
{
    return estep_check("expected statistics", r, o, expect_model,
                       "hmm-multinom, hmm-multinom-semisup and hhmm-tayal2009 only; the Gaussian hmm has hhmm_estep");
}

/* The T-scan entries (hhmm_estep_scan.hip): the scope and the LDS fit of their
 * sequential twins, then the plan: a request it cannot chunk has no scan. */
static hhmm_status estep_scan_check(const char *entry, const hhmm_request *r, const hhmm_estep_result *o,
                                    bool (*model_ok)(int), const char *scope)
{
    const hhmm_status s = estep_check(entry, r, o, model_ok, scope, kEstepScanAbove);
    if (s != HHMM_OK)
        return s;
    const int64_t P = npairs(r);
    if (P >= 1 && r->data.T_max >= 1 &&
        estep_scan_plan(r->model, r->data.K, r->data.L, r->data.T_max, P, (uint32_t)r->flags | HHMM_FLAG_SCAN_FORCE)
                .cl == 0) {
        set_error("%s: no T-scan of P = %lld pairs x T_max = %d (HHMM_FLAG_SCAN_OFF is set, or the (pair, chunk) "
                  "lanes reach 2^29: ask for longer chunks with HHMM_FLAG_SCAN_CHUNK_LOG2)",
                  entry, (long long)P, r->data.T_max);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

hhmm_status check_estep_scan(const hhmm_request *r, const hhmm_estep_result *o)
{
    return estep_scan_check("T-scan E-step", r, o, estep_model,
                            "hmm and hmm-multinom only; the masked programs have hhmm_expected_stats_scan");
}

hhmm_status check_expected_stats_scan(const hhmm_request *r, const hhmm_estep_result *o)
{
    return estep_scan_check("T-scan expected statistics", r, o, expect_model,
                            "hmm-multinom, hmm-multinom-semisup and hhmm-tayal2009 only; the Gaussian hmm has "
                            "hhmm_estep_scan");
}

template <int MODEL>
static bool launch_estep_m(const DevArgs &a, const EstepOutOf<MODEL> &o, dim3 grid, dim3 block, size_t lds,
                           hipStream_t st)
{
    return dispatch_k(a.K, [&](auto kc) {
        hipLaunchKernelGGL((estep_kernel<MODEL, decltype(kc)::value>), grid, block, lds, st, a, o);
    });
}

/* The one launch path of both entries (`entry`: the entry's name in messages). */
static hhmm_status launch_estep_any(const char *entry, const hhmm_request *r, const hhmm_estep_result *res, int64_t P,
                                    void *ws, hipStream_t st)
{
    DevArgs a = stats_dev_args(r, P, ws);
    a.x = r->data.x_int; /* hmm and hmm-multinom */
    a.xr = r->data.x_real;
    a.phi_k = r->draws.phi_k;
    a.mu_k = r->draws.mu_k;
    a.sigma_k = r->draws.sigma_k;
    a.g = r->data.g; /* semisup (g) and Tayal (sign, p_11, A_row) */
    a.sign = r->data.sign;
    a.p_11 = r->draws.p_11;
    a.A_row = r->draws.A_row;
    const EstepOut eo{res->loglik, res->n_1k, res->xi_ij, res->c_kl, res->w_k, res->s1_k, res->s2_k, res->pair_status};
    const ExpectOut xo{res->loglik, res->n_1k, res->xi_ij, res->c_kl, res->pair_status,
                       r->model == HHMM_MODEL_TAYAL ? 2 : r->data.G};
    size_t lds = 0;
    const int waves = estep_waves(a.model, a.K, a.L, &lds);
    if (waves < 1) {
        set_error("%s: the tables of K*L = %d*%d do not fit in LDS", entry, a.K, a.L);
        return HHMM_ERR_UNSUPPORTED;
    }
    const int threads = 64 * waves;
    const dim3 grid((unsigned)((P + threads - 1) / threads)), block(threads);
    bool ok = false;
    if (a.model == HHMM_MODEL_HMM_GAUSS)
        ok = launch_estep_m<HHMM_MODEL_HMM_GAUSS>(a, eo, grid, block, lds, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM)
        ok = launch_estep_m<HHMM_MODEL_HMM_MULTINOM>(a, eo, grid, block, lds, st);
    else if (a.model == HHMM_MODEL_HMM_MULTINOM_SEMISUP)
        ok = launch_estep_m<HHMM_MODEL_HMM_MULTINOM_SEMISUP>(a, xo, grid, block, lds, st);
    else if (a.model == HHMM_MODEL_TAYAL && a.K == 4) {
        hipLaunchKernelGGL((estep_kernel<HHMM_MODEL_TAYAL, 4>), grid, block, lds, st, a, xo);
        ok = true;
    }
    if (!ok) {
        set_error("%s: model %d at K = %d has no kernel (K outside 1..%d)", entry, a.model, a.K, kMaxK);
        return HHMM_ERR_UNSUPPORTED;
    }
    return launch_status("estep_kernel");
}

hhmm_status launch_estep(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws, hipStream_t st)
{
    return launch_estep_any("E-step", r, res, P, ws, st);
}

hhmm_status launch_expected_stats(const hhmm_request *r, const hhmm_estep_result *res, int64_t P, void *ws,
                                  hipStream_t st)
{
    return launch_estep_any("expected statistics", r, res, P, ws, st);
}

} // namespace hhmm
