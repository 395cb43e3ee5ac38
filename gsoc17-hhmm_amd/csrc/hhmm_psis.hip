/*
 * hhmm_psis.hip -- gfx950 kernels of Pareto-smoothed importance sampling over
 * the draws (include/hhmm_psis.h): PSIS-LOO and the backward leave-future-out
 * estimate on top of the pointwise sweeps, and the cell operation on
 * caller-supplied log ratios.
 *
 *   suffix   (LFO) one thread per pair walks t = T_n .. 1, adds l_t to a running
 *            sum that starts at +0.0 and stores it at p + P t: pair-fastest, a
 *            coalesced transaction per step.  r_d is its negative.
 *   cells    A cell (n, t) is D contiguous members at P t + n D.  The workgroup
 *            layout is summary_kernel's: G consecutive cells gi = n + N t, each
 *            in an LDS slot of n2 = 2^ceil(log2 D) keys padded with +inf, sorted
 *            at once by the bitonic network of hhmm_sortnet.h.  W = THREADS / G
 *            lanes own one cell through every step:
 *     load    r_d (the negated source for LOO / LFO) into the slot; a NaN or
 *             infinite r_d or l_d flags the cell (NaN outputs) and is stored as
 *             +inf, so the network orders comparable values only.
 *     shift   The largest r_d is the sorted key D - 1.  x -> x - max is
 *             monotone, so subtracting it from the sorted cut and tail gives
 *             the order of the shifted keys, the contract's order; only those
 *             M + 1 <= 385 keys are needed from the network.
 *     fit     x_i = exp(tail_i) - exp(cut) goes to the slot's first M keys
 *             (M <= D / 5: clear of the tail).  The m <= 49 profile points
 *             theta_j sit on the cell's first min(W, 64) lanes; past one wave
 *             the W / 64 waves each sum a strided share of the M terms of
 *             log1p(-theta_j x_i) and lane j adds the shares in wave order.
 *             omega_j and theta_j omega_j are one lane per j; theta is their
 *             sum in j order on every lane.  k sums M log1p on min(W, 64)
 *             lanes, whose partials every lane adds in lane order.
 *     weights The M smoothed weights replace x_i in the slot.  A draw finds
 *             its rank by a binary search of its shifted r_d in the sorted
 *             tail; where the tail (or the cut) repeats that value it counts
 *             the equal members of larger index, re-read from memory, so no
 *             index array is sorted and the ties break by (r_d, d).
 *     sums    Two strided passes over the D members: the largest w_d + l_d,
 *             then the three sums.  Lane partials combine by an xor butterfly,
 *             the waves of a cell through LDS in wave order
 *             (pointwise_large_reduce_kernel's order).
 * Tiers by n2, as the summary: n2 <= 2048 packs G = 2048 / n2 cells in a
 * 256-thread workgroup (W = n2 / 8), above one cell has 1024 threads and 36 /
 * 72 / 144 KiB of LDS.  Floor: each member is read twice in the sums pass and
 * once in the load (LOO: 8 B each; LFO and psis_cells: r_d and l_d, 16 B), the
 * second and third reads out of L2.  What bounds the kernel is not HBM but the
 * network's log2(n2) (log2(n2) + 1) / 2 compare-exchange stages per key and the
 * m M log1p of the fit (DESIGN.md section 3.17d has the measurements).
 * No floating-point atomics: the same bits on every run.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_psis.h"
#include "hhmm_sortnet.h"
#include "hhmm_stage.h"
#include "hhmm_stats.h"

namespace hhmm {

constexpr int kPsisTile = 2048;  /* keys per workgroup in the packed tiers */
constexpr int kPsisMinSlot = 8;  /* smallest slot */
constexpr int kPsisMaxG = kPsisTile / kPsisMinSlot;
constexpr int kPsisMaxFit = 64;  /* m = 30 + floor(sqrt(M)) <= 49 at D <= 16384 */

struct PsisArgs {
    const double *src;  /* the log ratios' source: lr, the suffix sums or l_t */
    const double *lp;   /* the targets l_d */
    const int32_t *T;
    double *elpd, *khat, *neff;
    int64_t N, D, P, NT; /* P = N * D, NT = N * T_max cells */
    int32_t Tmax;
    int32_t neg;         /* r_d = -src (LOO, LFO) */
    int32_t n2log, G;
    int32_t M, m;        /* the tail length and the profile points of the fit */
};

/* steps of series n, 0 .. T_max */
__device__ __forceinline__ int psis_len(const int32_t *T, int64_t n, int Tmax)
{
    return T ? min(max(T[n], 0), Tmax) : Tmax;
}

__global__ void __launch_bounds__(kBlock) psis_suffix_kernel(const double *lp, double *suf, const int32_t *T, int64_t P,
                                                             int64_t D, int Tmax)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P)
        return;
    const int len = psis_len(T, p / D, Tmax);
    double acc = 0.0;
    for (int t = len - 1; t >= 0; --t) {
        acc = acc + lp[p + P * t];
        suf[p + P * t] = acc;
    }
}

/* v over the W lanes of a cell: an xor butterfly inside the wave, then the
 * waves' values from `part` in wave order.  W is uniform over the workgroup. */
template <bool MAX>
__device__ __forceinline__ double psis_reduce(double v, int W, int g, double *part)
{
    for (int off = (W < 64 ? W : 64) / 2; off > 0; off >>= 1) {
        const double r = __shfl_xor(v, off);
        v = MAX ? fmax(v, r) : v + r;
    }
    if (W > 64) {
        const int nw = W / 64;
        __syncthreads(); /* the readers of the reduction before */
        if ((threadIdx.x & 63) == 0)
            part[threadIdx.x >> 6] = v;
        __syncthreads();
        v = part[g * nw];
        for (int q = 1; q < nw; ++q)
            v = MAX ? fmax(v, part[g * nw + q]) : v + part[g * nw + q];
    }
    return v;
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) psis_cell_kernel(const PsisArgs a)
{
    extern __shared__ double keys[];     /* [G][n2], padded (sum_ph); then fitL, fitW [G][m] */
    __shared__ int64_t gbase[kPsisMaxG]; /* n*D + P*t of the cell, -1: outside the series */
    __shared__ int32_t bad[kPsisMaxG];
    __shared__ double part[THREADS];

    const int tid = threadIdx.x;
    const int G = a.G, n2log = a.n2log, n2 = 1 << n2log, E = G << n2log;
    const int D = (int)a.D, M = a.M, m = a.m;
    const int W = THREADS / G, g = tid / W, wl = tid - g * W; /* W lanes per cell */
    const int kb = g << n2log;
    const int64_t g0 = (int64_t)blockIdx.x * G;
    double *const fitL = keys + (E + (E >> 3)) + (size_t)g * m;
    double *const fitW = fitL + (size_t)G * m;
    const bool same = a.src == a.lp;

    for (int gg = tid; gg < G; gg += THREADS) {
        const int64_t gi = g0 + gg;
        int64_t base = -1;
        if (gi < a.NT) {
            const int64_t t = gi / a.N, n = gi - t * a.N;
            if (t < (int64_t)psis_len(a.T, n, a.Tmax))
                base = a.D * n + a.P * t;
        }
        gbase[gg] = base;
        bad[gg] = 0;
    }
    __syncthreads();

    /* four loads in flight per thread before the first LDS store */
    for (int i0 = tid; i0 < E; i0 += 4 * THREADS) {
        double x[4], l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + u * THREADS;
            x[u] = __builtin_inf();
            l[u] = 0.0;
            if (idx < E) {
                const int i = idx & (n2 - 1);
                const int64_t base = gbase[idx >> n2log];
                if (base >= 0 && i < D) {
                    const double v = a.src[base + i];
                    l[u] = same ? v : a.lp[base + i];
                    x[u] = a.neg ? -v : v;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + u * THREADS;
            if (idx < E) {
                const bool pad = (idx & (n2 - 1)) >= D || gbase[idx >> n2log] < 0;
                if (!pad && (!(fabs(x[u]) < __builtin_inf()) || !(fabs(l[u]) < __builtin_inf()))) {
                    bad[idx >> n2log] = 1; /* every writer stores the same value */
                    x[u] = __builtin_inf();
                }
                keys[sum_ph(idx)] = x[u];
            }
        }
    }
    __syncthreads();
    sum_sort<THREADS>(keys, E, n2, tid);

    const int64_t base = gbase[g];
    const bool ok = base >= 0 && !bad[g];
    const double mx = keys[sum_ph(kb + D - 1)];
    __syncthreads();
    /* the cut and the tail, shifted in place: still sorted */
    for (int i = wl; i <= M; i += W)
        keys[sum_ph(kb + D - M - 1 + i)] -= mx;
    __syncthreads();

    bool smooth = false;
    double kh = __builtin_inf();
    if (M >= 5) { /* uniform over the grid: D is */
        const double Md = (double)M;
        const double cut = keys[sum_ph(kb + D - M - 1)];
        const double ecut = exp(cut);
        for (int i = wl; i < M; i += W)
            keys[sum_ph(kb + i)] = exp(keys[sum_ph(kb + D - M + i)]) - ecut;
        __syncthreads();
        const double x1 = keys[sum_ph(kb)], xM = keys[sum_ph(kb + M - 1)];
        const double xstar = keys[sum_ph(kb + (M + 2) / 4 - 1)];
        auto theta_at = [&](int j) { return 1.0 / xM + (1.0 - sqrt((double)m / ((double)j + 0.5))) / (3.0 * xstar); };
        auto profile = [&](double th, double kj) { return Md * (log(-th / kj) - kj - 1.0); };
        if (W <= 64) {
            for (int j = wl; j < m; j += W) {
                const double th = theta_at(j);
                double s = 0.0;
                for (int i = 0; i < M; ++i)
                    s += log1p(-th * keys[sum_ph(kb + i)]);
                fitL[j] = profile(th, s / Md);
            }
        } else {
            const int C = W / 64, j = wl & 63, c = wl >> 6;
            const double th = theta_at(j);
            double s = 0.0;
            if (j < m)
                for (int i = c; i < M; i += C)
                    s += log1p(-th * keys[sum_ph(kb + i)]);
            part[tid] = s;
            __syncthreads();
            if (c == 0 && j < m) {
                s = part[g * W + j];
                for (int q = 1; q < C; ++q)
                    s += part[g * W + q * 64 + j];
                fitL[j] = profile(th, s / Md);
            }
        }
        __syncthreads();
        for (int j = wl; j < m; j += W) {
            const double Lj = fitL[j];
            double s = 0.0;
            for (int i = 0; i < m; ++i)
                s += exp(fitL[i] - Lj);
            fitW[j] = theta_at(j) * (1.0 / s);
        }
        __syncthreads();
        double th = 0.0;
        for (int j = 0; j < m; ++j)
            th += fitW[j];
        const int NL = W < 64 ? W : 64;
        double s = 0.0;
        if (wl < NL)
            for (int i = wl; i < M; i += NL)
                s += log1p(-th * keys[sum_ph(kb + i)]);
        part[tid] = s;
        __syncthreads();
        double k = part[g * W];
        for (int q = 1; q < NL; ++q)
            k += part[g * W + q];
        k /= Md;
        const double sigma = -k / th;
        k = (k * Md + 5.0) / (Md + 10.0);
        smooth = ok && x1 != xM && fabs(k) < __builtin_inf() && fabs(sigma) < __builtin_inf();
        if (smooth)
            kh = k;
        /* the smoothed weight of tail rank i replaces x_i (every lane is past its reads of x) */
        for (int i = wl; i < M; i += W) {
            const double lg = log1p(-((double)i + 0.5) / Md);
            const double q = k == 0.0 ? -sigma * lg : sigma * expm1(-k * lg) / k;
            const double v = log(ecut + q);
            keys[sum_ph(kb + i)] = v > 0.0 ? 0.0 : v;
        }
        __syncthreads();
    }

    const int Dn = ok ? D : 0;
    const double *const src = a.src + (base >= 0 ? base : 0);
    const double *const lpp = a.lp + (base >= 0 ? base : 0);
    const double cut = M >= 5 ? keys[sum_ph(kb + D - M - 1)] : 0.0;
    auto ratio = [&](int d) {
        const double v = src[d];
        return (a.neg ? -v : v) - mx;
    };
    auto weight = [&](int d, double r) {
        if (!smooth || !(r >= keys[sum_ph(kb + D - M)]))
            return r;
        int lo = 0, hi = M; /* the tail values <= r */
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[sum_ph(kb + D - M + mid)] <= r)
                lo = mid + 1;
            else
                hi = mid;
        }
        int at = lo - 1; /* the last of them is r itself */
        if ((lo >= 2 && keys[sum_ph(kb + D - M + lo - 2)] == r) || r == cut)
            for (int e = d + 1; e < D; ++e) /* ties: the equal members of larger index rank above */
                at -= ratio(e) == r ? 1 : 0;
        return at < 0 ? r : keys[sum_ph(kb + at)];
    };

    double am = -__builtin_inf(), bm = -__builtin_inf();
    for (int d = wl; d < Dn; d += W) {
        const double w = weight(d, ratio(d));
        am = fmax(am, w + lpp[d]);
        bm = fmax(bm, w);
    }
    am = psis_reduce<true>(am, W, g, part);
    bm = psis_reduce<true>(bm, W, g, part);
    double s1 = 0.0, s0 = 0.0, s2 = 0.0;
    for (int d = wl; d < Dn; d += W) {
        const double w = weight(d, ratio(d));
        s1 += exp((w + lpp[d]) - am);
        s0 += exp(w - bm);
        s2 += exp(2.0 * (w - bm));
    }
    s1 = psis_reduce<false>(s1, W, g, part);
    s0 = psis_reduce<false>(s0, W, g, part);
    s2 = psis_reduce<false>(s2, W, g, part);
    if (base >= 0 && wl == 0) {
        const double nan = __builtin_nan("");
        a.elpd[g0 + g] = ok ? (am + log(s1)) - (bm + log(s0)) : nan;
        a.khat[g0 + g] = ok ? kh : nan;
        a.neff[g0 + g] = ok ? s0 * s0 / s2 : nan;
    }
}

/* ---- host side ---- */

/* M = min(floor(D / 5), c), c the smallest integer with c^2 >= 9 D */
static int psis_tail(int64_t D)
{
    int64_t c = 0;
    while (c * c < 9 * D)
        ++c;
    return (int)(D / 5 < c ? D / 5 : c);
}

/* m = 30 + floor(sqrt(M)) */
static int psis_points(int M)
{
    int r = 0;
    while ((r + 1) * (r + 1) <= M)
        ++r;
    return 30 + r;
}

static hhmm_status check_psis_draws(const char *entry, int64_t D)
{
    if (D > HHMM_PSIS_MAX_DRAWS) {
        set_error("%s of D = %lld draws per series: at most %d (one cell is ordered in one workgroup's LDS)", entry,
                  (long long)D, HHMM_PSIS_MAX_DRAWS);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

/* The cell kernel over N * T_max cells of D members (device pointers). */
static hhmm_status launch_psis_cells(PsisArgs a, hipStream_t st)
{
    a.P = a.N * a.D;
    a.NT = a.N * (int64_t)a.Tmax;
    int n2log = 3;
    while (((int64_t)1 << n2log) < a.D)
        ++n2log;
    a.n2log = n2log;
    const int n2 = 1 << n2log;
    const bool big = n2 > kPsisTile;
    a.G = big ? 1 : kPsisTile / n2;
    a.M = psis_tail(a.D);
    a.m = psis_points(a.M);
    const int64_t blocks = (a.NT + a.G - 1) / a.G;
    const size_t fit = a.M >= 5 ? 2 * (size_t)a.G * (size_t)a.m * sizeof(double) : 0;
    const size_t lds = sum_lds_bytes((size_t)a.G * (size_t)n2) + fit;
    if (big) {
        /* per device, so set on every launch of this tier (the current device's) */
        const hipError_t attr =
            hipFuncSetAttribute((const void *)psis_cell_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sum_lds_bytes(HHMM_PSIS_MAX_DRAWS) + 2 * kPsisMaxFit * sizeof(double)));
        if (attr != hipSuccess) {
            set_error("psis_cell_kernel LDS attribute: %s", hipGetErrorString(attr));
            return HHMM_ERR_HIP;
        }
        hipLaunchKernelGGL(psis_cell_kernel<1024>, dim3((unsigned)blocks), dim3(1024), lds, st, a);
    } else {
        hipLaunchKernelGGL(psis_cell_kernel<kBlock>, dim3((unsigned)blocks), dim3(kBlock), lds, st, a);
    }
    return launch_status("psis_cell_kernel");
}

static bool psis_model(int m) { return m == HHMM_MODEL_HMM_GAUSS || m == HHMM_MODEL_HMM_MULTINOM; }

hhmm_status check_psis(const hhmm_request *r, const hhmm_psis_result *o)
{
    hhmm_status s = stats_check_head("PSIS", r, psis_model,
                                     "hmm and hmm-multinom only; the coded step weights of the semisup, Tayal and "
                                     "IOHMM programs are masked or factorised, not a predictive density",
                                     1, kMaxKLarge);
    if (s != HHMM_OK)
        return s;
    /* the sweep's own scope: the emission table in LDS, the pointwise outputs */
    const hhmm_pointwise_result *pw = o ? &o->pw : nullptr;
    s = r->data.K <= kMaxK ? check_pointwise(r, pw) : check_pointwise_large(r, pw);
    if (s != HHMM_OK)
        return s;
    const char *missing = !o->elpd_t ? "elpd_t" : !o->khat_t ? "khat_t" : !o->neff_t ? "neff_t" : nullptr;
    if (missing) {
        set_error("PSIS: %s must be non-NULL (elpd_t, khat_t and neff_t are required)", missing);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const int64_t P = npairs(r);
    if (P >= 1 && r->data.n_series >= 1)
        return check_psis_draws("PSIS", P / r->data.n_series);
    return HHMM_OK; /* the request check that follows names what does not fit */
}

static size_t psis_lt_bytes(const hhmm_request *r, int64_t P) { return (size_t)P * (size_t)r->data.T_max * sizeof(double); }

static size_t psis_workspace(const hhmm_request *r, int64_t P, bool lfo)
{
    const size_t sweep = r->data.K <= kMaxK ? pointwise_workspace_bytes(r, P) + psis_lt_bytes(r, P)
                                            : pointwise_large_workspace_bytes(r, P);
    return sweep + (lfo ? psis_lt_bytes(r, P) : 0);
}
size_t psis_loo_workspace_bytes(const hhmm_request *r, int64_t P) { return psis_workspace(r, P, false); }
size_t psis_lfo_workspace_bytes(const hhmm_request *r, int64_t P) { return psis_workspace(r, P, true); }

static hhmm_status launch_psis(const hhmm_request *r, const hhmm_psis_result *res, int64_t P, void *ws, hipStream_t st,
                               bool lfo)
{
    hhmm_pointwise_result pw = res->pw;
    char *w = (char *)ws;
    hhmm_status s;
    if (r->data.K <= kMaxK) {
        const size_t tiles = pointwise_workspace_bytes(r, P);
        if (!pw.lp_t)
            pw.lp_t = (double *)(w + tiles);
        s = launch_pointwise(r, &pw, P, w, st);
        w += tiles + psis_lt_bytes(r, P);
    } else {
        if (!pw.lp_t)
            pw.lp_t = (double *)w; /* where launch_pointwise_large puts l_t itself */
        s = launch_pointwise_large(r, &pw, P, w, st);
        w += psis_lt_bytes(r, P);
    }
    if (s != HHMM_OK)
        return s;
    PsisArgs a{};
    a.N = r->data.n_series;
    a.D = P / a.N;
    a.Tmax = r->data.T_max;
    a.T = r->data.T;
    a.lp = pw.lp_t;
    a.src = pw.lp_t;
    a.neg = 1;
    a.elpd = res->elpd_t;
    a.khat = res->khat_t;
    a.neff = res->neff_t;
    if (lfo) {
        double *const suf = (double *)w;
        hipLaunchKernelGGL(psis_suffix_kernel, dim3((unsigned)((P + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           (const double *)pw.lp_t, suf, a.T, P, a.D, a.Tmax);
        if ((s = launch_status("psis_suffix_kernel")) != HHMM_OK)
            return s;
        a.src = suf;
    }
    return launch_psis_cells(a, st);
}

hhmm_status launch_psis_loo(const hhmm_request *r, const hhmm_psis_result *res, int64_t P, void *ws, hipStream_t st)
{
    return launch_psis(r, res, P, ws, st, false);
}
hhmm_status launch_psis_lfo(const hhmm_request *r, const hhmm_psis_result *res, int64_t P, void *ws, hipStream_t st)
{
    return launch_psis(r, res, P, ws, st, true);
}

static hhmm_status check_psis_cells(const hhmm_psis_cells_request *r, const double *elpd, const double *khat,
                                    const double *neff)
{
    if (!r || !elpd || !khat || !neff) {
        set_error("PSIS cells: the request, elpd_t, khat_t and neff_t must be non-NULL");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_series < 1 || r->n_draws < 1 || r->T_max < 1) {
        set_error("PSIS cells needs N, D, T_max >= 1 (got N=%lld D=%lld T_max=%d)", (long long)r->n_series,
                  (long long)r->n_draws, r->T_max);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (!r->lr || !r->lp) {
        set_error("PSIS cells: lr and lp must be non-NULL");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_series > (int64_t(1) << 28) || r->n_series * (int64_t)r->T_max > (int64_t(1) << 30)) {
        set_error("PSIS cells: at most 2^28 series and 2^30 cells per call");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    return check_psis_draws("PSIS cells", r->n_draws);
}

static hhmm_status psis_cells_device_visible()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error("no HIP device visible: libhhmm has no CPU path (gfx950 required)");
        return HHMM_ERR_NO_DEVICE;
    }
    return HHMM_OK;
}

static PsisArgs psis_cells_args(const hhmm_psis_cells_request *r, double *elpd, double *khat, double *neff)
{
    PsisArgs a{};
    a.N = r->n_series;
    a.D = r->n_draws;
    a.Tmax = r->T_max;
    a.T = r->T;
    a.src = r->lr;
    a.lp = r->lp;
    a.neg = 0;
    a.elpd = elpd;
    a.khat = khat;
    a.neff = neff;
    return a;
}

} // namespace hhmm

using namespace hhmm;

extern "C" {

hhmm_status hhmm_psis_cells_workspace_size(const hhmm_psis_cells_request *req, size_t *bytes)
{
    if (!req || !bytes) {
        set_error("NULL argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    *bytes = 0;
    return HHMM_OK;
}

hhmm_status hhmm_psis_cells_device(const hhmm_psis_cells_request *req, double *elpd_t, double *khat_t, double *neff_t,
                                   void *, size_t, void *stream)
{
    hhmm_status s = check_psis_cells(req, elpd_t, khat_t, neff_t);
    if (s != HHMM_OK || (s = psis_cells_device_visible()) != HHMM_OK)
        return s;
    return launch_psis_cells(psis_cells_args(req, elpd_t, khat_t, neff_t), (hipStream_t)stream);
}

hhmm_status hhmm_psis_cells(const hhmm_psis_cells_request *req, double *elpd_t, double *khat_t, double *neff_t,
                            int device)
{
    hhmm_status s = check_psis_cells(req, elpd_t, khat_t, neff_t);
    if (s != HHMM_OK)
        return s;
    if (req->T)
        for (int64_t n = 0; n < req->n_series; ++n)
            if (req->T[n] < 1 || req->T[n] > req->T_max) {
                set_error("PSIS cells: T[%lld] = %d outside 1..T_max=%d", (long long)n, req->T[n], req->T_max);
                return HHMM_ERR_INVALID_ARGUMENT;
            }
    if ((s = psis_cells_device_visible()) != HHMM_OK)
        return s;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", device);
        return HHMM_ERR_HIP;
    }
    const size_t N = (size_t)req->n_series, NT = N * (size_t)req->T_max;
    const size_t bv = sizeof(double) * NT * (size_t)req->n_draws, bo = sizeof(double) * NT;
    double *dr = nullptr, *dl = nullptr, *dout = nullptr; /* dout: the three outputs, one after the other */
    int32_t *dT = nullptr;
    double *const host_out[3] = {elpd_t, khat_t, neff_t};
    hipError_t e = hipMalloc(&dr, bv);
    if (e == hipSuccess)
        e = hipMalloc(&dl, bv);
    if (e == hipSuccess)
        e = hipMalloc(&dout, 3 * bo);
    if (e == hipSuccess && req->T)
        e = hipMalloc(&dT, sizeof(int32_t) * N);
    if (e == hipSuccess)
        e = hipMemcpy(dr, req->lr, bv, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(dl, req->lp, bv, hipMemcpyHostToDevice);
    if (e == hipSuccess && req->T) { /* padded steps round-trip untouched */
        e = hipMemcpy(dT, req->T, sizeof(int32_t) * N, hipMemcpyHostToDevice);
        for (int q = 0; q < 3 && e == hipSuccess; ++q)
            e = hipMemcpy(dout + q * NT, host_out[q], bo, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        hhmm_psis_cells_request d = *req;
        d.T = dT;
        d.lr = dr;
        d.lp = dl;
        s = launch_psis_cells(psis_cells_args(&d, dout, dout + NT, dout + 2 * NT), nullptr);
        for (int q = 0; q < 3 && s == HHMM_OK && e == hipSuccess; ++q)
            e = hipMemcpy(host_out[q], dout + q * NT, bo, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dr);
    (void)hipFree(dl);
    (void)hipFree(dout);
    (void)hipFree(dT);
    if (e != hipSuccess) {
        set_error("PSIS cells: %s", hipGetErrorString(e));
        return (e == hipErrorOutOfMemory) ? HHMM_ERR_OUT_OF_MEMORY : HHMM_ERR_HIP;
    }
    return s;
}

} // extern "C"
