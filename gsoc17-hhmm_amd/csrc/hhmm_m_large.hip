/* hmm/stan/hmm.stan and hmm-multinom.stan at 8 < K <= 32: the state-parallel
 * kernels of hhmm_large.h, 16-lane groups up to K = 16 and
 * 32-lane groups above (24-state loops up to K = 24). */
#include "hhmm_lkscan.h"

namespace hhmm {

hhmm_status run_large(const DevArgs &a, hipStream_t st)
{
    return dispatch_lk_model(a.model, a.K, [&](auto M, auto G, auto KM) { return run_large_model<M, G, KM>(a, st); });
}

} // namespace hhmm
