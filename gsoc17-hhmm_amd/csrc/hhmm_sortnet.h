/*
 * hhmm_sortnet.h -- the bitonic network over padded LDS slots that orders the
 * draws of a cell: the quantiles of hhmm_summary.hip and the importance ratios
 * of hhmm_psis.hip.  E keys lie in slots of n2 = 2^k doubles, key i at
 * sum_ph(i); every slot is sorted ascending at once with fp64 min / max (the
 * caller keeps NaN out of the keys; -0 and +0 compare equal, as under <).  Up
 * to three consecutive stages of the network run as one pass over LDS with
 * eight keys per thread in registers.  Device code only; not part of the ABI.
 */
#pragma once
#include <hip/hip_runtime.h>

namespace hhmm {

/* LDS slot of key i: one pad key per eight, so a thread's eight consecutive
 * keys (64 B) and its neighbours' fall on different banks. */
static __device__ __forceinline__ int sum_ph(int i) { return i + (i >> 3); }
constexpr size_t sum_lds_bytes(size_t keys) { return sizeof(double) * (keys + (keys >> 3)); }

/* Stages j = jhi, jhi/2, .. (NST of them) of phase kk of the bitonic network
 * over E keys in slots of n2: a thread takes the 2^NST keys that differ in
 * those stages' index bits, exchanges them in registers and writes them back.
 * They share the bit kk of their index, hence the direction. */
template <int NST, int THREADS>
static __device__ __forceinline__ void sum_pass(double *keys, int E, int n2, int kk, int jhi, int tid)
{
    constexpr int R = 1 << NST;
    const int low = jhi >> (NST - 1);
    for (int gi = tid; gi < (E >> NST); gi += THREADS) {
        const int base = ((gi & ~(low - 1)) << NST) | (gi & (low - 1));
        /* a descending group is the ascending network on the reversed row */
        const int rev = ((base & (n2 - 1)) & kk) == 0 ? 0 : R - 1;
        double r[R];
#pragma unroll
        for (int m = 0; m < R; ++m)
            r[m] = keys[sum_ph(base + (m ^ rev) * low)];
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            const int bit = 1 << (NST - 1 - s);
#pragma unroll
            for (int m = 0; m < R; ++m)
                if (!(m & bit)) {
                    const double x = r[m], y = r[m | bit];
                    r[m] = __builtin_fmin(x, y);
                    r[m | bit] = __builtin_fmax(x, y);
                }
        }
#pragma unroll
        for (int m = 0; m < R; ++m)
            keys[sum_ph(base + (m ^ rev) * low)] = r[m];
    }
}

/* The whole network: phase kk has log2(kk) stages j = kk/2 .. 1; up to three
 * consecutive stages run as one pass over LDS (eight keys per thread in
 * registers), a barrier after each.  The caller puts a barrier between its
 * stores of the keys and this.  psis_cell_kernel calls it; summary_kernel keeps
 * the same loop written out in its k loop, where the call allocates registers
 * differently (its device code is held to what it was). */
template <int THREADS>
static __device__ __forceinline__ void sum_sort(double *keys, int E, int n2, int tid)
{
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
}

} // namespace hhmm
