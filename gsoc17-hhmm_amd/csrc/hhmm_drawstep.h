/*
 * hhmm_drawstep.h -- what the draw statistics kernels share
 * (hhmm_draw_stats.hip, hhmm_draw_stats_gauss.hip): the FFBS step on opaque
 * copies of the transition matrix and the one-word LDS count.
 */
#pragma once
#include "hhmm_fbchunk.h"

namespace hhmm {

/* one more in this lane's word of a count slab */
__device__ __forceinline__ void count_one(uint32_t *w)
{
    __hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

/* v, as a value hipcc cannot trace back to its load (an empty asm: no instruction) */
__device__ __forceinline__ double opaque(double v)
{
    __asm__("" : "+v"(v));
    return v;
}

/* ffbs_draw (hhmm_fbchunk.h) with the mask of step t + 1 at z_{t+1} already decided
 * (`on`): the same operations on the same values, so the same z.  The column
 * A(., z_{t+1}) is picked from opaque copies of the entries: left to itself
 * hipcc folds the select chain over pp.A into one dynamically indexed load,
 * which moves the pair's parameters into scratch (K scratch loads per step,
 * 288 B of private segment at K = 3 up to 928 B at K = 8). */
template <int MODEL, int K>
__device__ __forceinline__ int draw_step(const PairParams<MODEL, K> &pp, const double (&f)[K], bool last, bool on,
                                         int z, double u)
{
    double w[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double az = opaque(pp.A[i][0]);
#pragma unroll
        for (int j = 1; j < K; ++j) {
            const double aj = opaque(pp.A[i][j]);
            az = (z == j) ? aj : az;
        }
        w[i] = (last | !on) ? f[i] : f[i] * az;
    }
    if (!last && z < 0)
        return -1;
    return ffbs_cat<K>(w, u);
}

} // namespace hhmm
