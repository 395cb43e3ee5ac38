/*
 * hhmm_summary.hip -- gfx950 reduction of the engine's pair-major outputs over
 * the draws: exact type-7 quantiles per cell and the hard state (argmax over k
 * of one quantile).  C ABI and contract in include/hhmm_summary.h.
 *
 * A cell (n, t, k) is S contiguous values at S*n + P*(t + T_max*k); the cells
 * of consecutive series at one (t, k) follow each other, so a workgroup takes
 * G consecutive groups gi = n + N*t and loads, for one k, G*S contiguous
 * values (full-line coalesced) into LDS, each cell in a slot of n2 =
 * 2^ceil(log2 S) doubles padded with +inf: the pads sort to the end, and since
 * indices above S-1 are never read, a pad can stand in only for a +inf of the
 * cell itself, the same value.  A NaN flags its cell (the cell's quantiles are
 * NaN) and is stored as +inf, so the network only ever orders comparable
 * values, with fp64 min / max (denormals kept; -0 and +0 compare equal, as
 * under <).  One bitonic network sorts all G slots at once; the Q quantiles are
 * then read off the sorted slots.  The workgroup walks k = 0 .. K-1 serially and keeps
 * the running argmax of its groups in LDS, so the hard state needs no second
 * pass and no scratch.
 *
 * Tiers by n2 (kSumTile = 2048 keys, 18 KiB of padded LDS per 256-thread
 * workgroup, so six workgroups share a CU):
 *     n2 <= 2048         G = 2048 / n2 cells per workgroup (S = 250: 8 cells)
 *     n2 = 4096 .. 16384 one cell, 1024 threads, 36 / 72 / 144 KiB of LDS
 * (S < 8 sorts in a slot of 8).  Up to three consecutive stages of the network
 * run as one pass over LDS with eight keys per thread in registers (sum_pass).
 * Floor: one read of the input (8 B per value) plus Q/S of that written; the
 * network's log2(n2) (log2(n2) + 1) / 2 compare-exchange stages per key (a
 * v_min_f64 / v_max_f64 pair each; a descending row is the ascending network on
 * the reversed row) and a barrier per pass are what bound every tier, not HBM
 * (DESIGN.md §3.10 has the measurements).
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "hhmm_summary.h"
#include "hhmm_internal.h"
#include "hhmm_sortnet.h"

namespace hhmm {

constexpr int kSumTile = 2048;   /* keys per workgroup in the packed tiers */
constexpr int kSumMinSlot = 8;   /* smallest slot: at most kSumTile / 8 groups per workgroup */
constexpr int kSumMaxG = kSumTile / kSumMinSlot;

struct SumArgs {
    const double *vf;
    const int32_t *vi;
    const int32_t *T;
    double *q;
    int32_t *am;
    int64_t N, S, P, NT; /* NT = N * T_max groups */
    int32_t Tmax, K, Q, has_arg;
    int32_t n2log, G;
    double probs[HHMM_SUMMARY_MAX_PROBS + 1]; /* [Q]: argmax_prob */
};

template <int THREADS>
__global__ void __launch_bounds__(THREADS) summary_kernel(const SumArgs a)
{
    extern __shared__ double keys[];        /* [G][n2], padded (sum_ph) */
    __shared__ int64_t gbase[kSumMaxG];     /* S*n + P*t of the group, -1: outside the series */
    __shared__ double bestv[kSumMaxG];
    __shared__ int32_t bestk[kSumMaxG];
    __shared__ int32_t nanf[kSumMaxG];
    __shared__ double sprobs[HHMM_SUMMARY_MAX_PROBS + 1];

    const int tid = threadIdx.x;
    const int G = a.G, n2log = a.n2log, n2 = 1 << n2log, E = G << n2log;
    const int S = (int)a.S;
    const int64_t g0 = (int64_t)blockIdx.x * G;
    const int nq = a.Q + a.has_arg;

    for (int g = tid; g < G; g += THREADS) {
        const int64_t gi = g0 + g;
        int64_t base = -1;
        if (gi < a.NT) {
            const int64_t t = gi / a.N, n = gi - t * a.N;
            const int len = a.T ? a.T[n] : a.Tmax;
            if (t < (int64_t)len) /* t < T_max by construction: a T[n] beyond T_max reads nothing past the array */
                base = a.S * n + a.P * t;
        }
        gbase[g] = base;
        bestk[g] = 0;
        bestv[g] = 0.0;
    }
    if (tid < nq)
        sprobs[tid] = a.probs[tid];
    __syncthreads();

    for (int k = 0; k < a.K; ++k) {
        const int64_t koff = a.P * (int64_t)a.Tmax * k;
        for (int g = tid; g < G; g += THREADS)
            nanf[g] = 0;
        __syncthreads();
        /* four loads in flight per thread before the first LDS store (E is a
         * multiple of 4 * THREADS in every tier; the bound stays checked) */
        for (int i0 = tid; i0 < E; i0 += 4 * THREADS) {
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = i0 + u * THREADS;
                x[u] = __builtin_inf();
                if (idx < E) {
                    const int i = idx & (n2 - 1);
                    const int64_t base = gbase[idx >> n2log];
                    if (base >= 0 && i < S) {
                        const int64_t at = base + koff + i;
                        x[u] = a.vf ? a.vf[at] : (double)a.vi[at];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = i0 + u * THREADS;
                if (idx < E) {
                    if (x[u] != x[u]) {
                        nanf[idx >> n2log] = 1; /* every writer stores the same value */
                        x[u] = __builtin_inf();
                    }
                    keys[sum_ph(idx)] = x[u];
                }
            }
        }
        __syncthreads();
        /* phase kk has log2(kk) stages j = kk/2 .. 1; up to three consecutive
         * stages run as one pass over LDS (eight keys per thread in registers) */
        for (int kk = 2, lk = 1; kk <= n2; kk <<= 1, ++lk) {
            int jhi = kk >> 1;
            for (int left = lk; left > 0;) {
                const int nst = left >= 3 ? 3 : left;
                if (nst == 3)
                    sum_pass<3, THREADS>(keys, E, n2, kk, jhi, tid);
                else if (nst == 2)
                    sum_pass<2, THREADS>(keys, E, n2, kk, jhi, tid);
                else
                    sum_pass<1, THREADS>(keys, E, n2, kk, jhi, tid);
                __syncthreads();
                jhi >>= nst;
                left -= nst;
            }
        }
        for (int idx = tid; idx < G * nq; idx += THREADS) {
            const int j = idx / G, g = idx - j * G;
            if (gbase[g] < 0)
                continue;
            double q;
            if (nanf[g]) {
                q = __builtin_nan("");
            } else {
                const double h = (double)(S - 1) * sprobs[j];
                const double fl = floor(h), ce = ceil(h);
                const double ylo = keys[sum_ph((g << n2log) + (int)fl)];
                const double yhi = keys[sum_ph((g << n2log) + (int)ce)];
                q = ylo;
                if (h > fl && yhi != ylo) {
                    const double gg = h - fl;
                    q = (1.0 - gg) * ylo + gg * yhi;
                }
            }
            if (j < a.Q) {
                a.q[(g0 + g) + a.NT * ((int64_t)k + (int64_t)a.K * j)] = q;
            } else if (q == q && (bestk[g] == 0 || q > bestv[g])) { /* one thread per group, k serial */
                bestv[g] = q;
                bestk[g] = k + 1;
            }
        }
        __syncthreads();
    }
    if (a.has_arg)
        for (int g = tid; g < G; g += THREADS)
            if (gbase[g] >= 0)
                a.am[g0 + g] = bestk[g];
}

hhmm_status check_summary(const hhmm_summary_request *r, const double *quantiles, const int32_t *argmax)
{
    if (!r || !quantiles) {
        set_error("NULL summary argument");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_series < 1 || r->n_draws < 1 || r->T_max < 1 || r->K < 1) {
        set_error("summary needs N, S, T_max, K >= 1 (got N=%lld S=%lld T_max=%d K=%d)", (long long)r->n_series,
                  (long long)r->n_draws, r->T_max, r->K);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_probs < 1 || r->n_probs > HHMM_SUMMARY_MAX_PROBS) {
        set_error("summary needs 1 <= n_probs <= %d (got %d)", HHMM_SUMMARY_MAX_PROBS, r->n_probs);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    for (int j = 0; j < r->n_probs; ++j)
        if (!(r->probs[j] >= 0.0 && r->probs[j] <= 1.0)) {
            set_error("summary probs[%d] = %g outside [0, 1]", j, r->probs[j]);
            return HHMM_ERR_INVALID_ARGUMENT;
        }
    if ((r->values_f64 != nullptr) == (r->values_i32 != nullptr)) {
        set_error("summary needs exactly one of values_f64 / values_i32");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    const bool arg = r->argmax_prob != -1.0;
    if (arg && !(r->argmax_prob >= 0.0 && r->argmax_prob <= 1.0)) {
        set_error("summary argmax_prob = %g is neither -1 nor in [0, 1]", r->argmax_prob);
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (arg && !argmax) {
        set_error("summary argmax_prob given but the argmax pointer is NULL");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_series > (int64_t(1) << 28) || r->n_series * (int64_t)r->T_max > (int64_t(1) << 30)) {
        set_error("summary: at most 2^28 series and 2^30 (series, step) groups per call");
        return HHMM_ERR_INVALID_ARGUMENT;
    }
    if (r->n_draws > HHMM_SUMMARY_MAX_DRAWS) {
        set_error("summary of S = %lld draws per series: at most %d (one cell is sorted in one workgroup's LDS)",
                  (long long)r->n_draws, HHMM_SUMMARY_MAX_DRAWS);
        return HHMM_ERR_UNSUPPORTED;
    }
    return HHMM_OK;
}

hhmm_status launch_summary(const hhmm_summary_request *r, double *quantiles, int32_t *argmax, hipStream_t st)
{
    SumArgs a{};
    a.vf = r->values_f64;
    a.vi = r->values_i32;
    a.T = r->T;
    a.q = quantiles;
    a.am = argmax;
    a.N = r->n_series;
    a.S = r->n_draws;
    a.P = a.N * a.S;
    a.NT = a.N * (int64_t)r->T_max;
    a.Tmax = r->T_max;
    a.K = r->K;
    a.Q = r->n_probs;
    a.has_arg = r->argmax_prob != -1.0 ? 1 : 0;
    for (int j = 0; j < a.Q; ++j)
        a.probs[j] = r->probs[j];
    a.probs[a.Q] = a.has_arg ? r->argmax_prob : 0.0;
    int n2log = 3;
    while (((int64_t)1 << n2log) < a.S)
        ++n2log;
    a.n2log = n2log;
    const int n2 = 1 << n2log;
    const bool big = n2 > kSumTile;
    a.G = big ? 1 : kSumTile / n2;
    const int64_t blocks = (a.NT + a.G - 1) / a.G;
    const size_t lds = sum_lds_bytes((size_t)a.G * (size_t)n2);
    if (big) {
        /* per device, so set on every launch of this tier (the current device's) */
        const hipError_t attr =
            hipFuncSetAttribute((const void *)summary_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sum_lds_bytes(HHMM_SUMMARY_MAX_DRAWS));
        if (attr != hipSuccess) {
            set_error("summary_kernel LDS attribute: %s", hipGetErrorString(attr));
            return HHMM_ERR_HIP;
        }
        hipLaunchKernelGGL(summary_kernel<1024>, dim3((unsigned)blocks), dim3(1024), lds, st, a);
    } else {
        hipLaunchKernelGGL(summary_kernel<256>, dim3((unsigned)blocks), dim3(256), lds, st, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("summary_kernel launch: %s", hipGetErrorString(e));
        return HHMM_ERR_HIP;
    }
    return HHMM_OK;
}

} // namespace hhmm

using namespace hhmm;

extern "C" {

hhmm_status hhmm_summary_device(const hhmm_summary_request *req, double *quantiles, int32_t *argmax, void *stream)
{
    hhmm_status s = check_summary(req, quantiles, argmax);
    if (s != HHMM_OK)
        return s;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error("no HIP device visible: libhhmm has no CPU path (gfx950 required)");
        return HHMM_ERR_NO_DEVICE;
    }
    return launch_summary(req, quantiles, argmax, (hipStream_t)stream);
}

hhmm_status hhmm_summary(const hhmm_summary_request *req, double *quantiles, int32_t *argmax, int device)
{
    hhmm_status s = check_summary(req, quantiles, argmax);
    if (s != HHMM_OK)
        return s;
    if (req->T)
        for (int64_t n = 0; n < req->n_series; ++n)
            if (req->T[n] < 1 || req->T[n] > req->T_max) {
                set_error("summary T[%lld] = %d outside 1..T_max=%d", (long long)n, req->T[n], req->T_max);
                return HHMM_ERR_INVALID_ARGUMENT;
            }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        set_error("no HIP device visible: libhhmm has no CPU path (gfx950 required)");
        return HHMM_ERR_NO_DEVICE;
    }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", device);
        return HHMM_ERR_HIP;
    }
    const bool arg = req->argmax_prob != -1.0;
    const size_t N = (size_t)req->n_series, NT = N * (size_t)req->T_max;
    const size_t nv = NT * (size_t)req->n_draws * (size_t)req->K;
    const size_t bv = nv * (req->values_f64 ? sizeof(double) : sizeof(int32_t));
    const size_t bq = sizeof(double) * NT * (size_t)req->K * (size_t)req->n_probs;
    const size_t ba = sizeof(int32_t) * NT;
    void *dv = nullptr;
    int32_t *dT = nullptr, *da = nullptr;
    double *dq = nullptr;
    hipError_t e = hipMalloc(&dv, bv);
    if (e == hipSuccess)
        e = hipMalloc(&dq, bq);
    if (e == hipSuccess && arg)
        e = hipMalloc(&da, ba);
    if (e == hipSuccess && req->T)
        e = hipMalloc(&dT, sizeof(int32_t) * N);
    if (e == hipSuccess)
        e = hipMemcpy(dv, req->values_f64 ? (const void *)req->values_f64 : (const void *)req->values_i32, bv,
                      hipMemcpyHostToDevice);
    if (e == hipSuccess && req->T) { /* padded steps round-trip untouched */
        e = hipMemcpy(dT, req->T, sizeof(int32_t) * N, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(dq, quantiles, bq, hipMemcpyHostToDevice);
        if (e == hipSuccess && arg)
            e = hipMemcpy(da, argmax, ba, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        hhmm_summary_request dr = *req;
        dr.T = dT;
        if (req->values_f64)
            dr.values_f64 = (const double *)dv;
        else
            dr.values_i32 = (const int32_t *)dv;
        s = launch_summary(&dr, dq, da, nullptr);
        if (s == HHMM_OK)
            e = hipMemcpy(quantiles, dq, bq, hipMemcpyDeviceToHost);
        if (s == HHMM_OK && e == hipSuccess && arg)
            e = hipMemcpy(argmax, da, ba, hipMemcpyDeviceToHost);
    }
    (void)hipFree(dv);
    (void)hipFree(dq);
    (void)hipFree(da);
    (void)hipFree(dT);
    if (e != hipSuccess) {
        set_error("summary: %s", hipGetErrorString(e));
        return (e == hipErrorOutOfMemory) ? HHMM_ERR_OUT_OF_MEMORY : HHMM_ERR_HIP;
    }
    return s;
}

} // extern "C"
