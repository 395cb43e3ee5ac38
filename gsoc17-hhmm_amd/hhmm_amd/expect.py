"""Expected draw statistics on the GPU (include/hhmm_expect.h).

`expected_stats()` is the E-step of the programs whose forward pass is masked:
per (series, draw) pair the posterior expectation, under the CODED path weight
prod p^n_1k prod A^xi_ij prod phi^c_kl, of the counts `draw_stats()` returns
for one drawn path.  The counts follow the forward masks
(hmm-multinom-semisup.stan:42, hhmm-tayal2009.stan:51 and :62), so the backward
sweep is the adjoint of the coded forward pass -- not the programs' own
backward passes, which `estep()` refuses for that reason.  The statistics are
the exact score of the model-block log-likelihood (hhmm_amd.score) and feed
the EM point fit (hhmm_amd.baum_welch).  hmm-multinom has no mask: its
statistics are estep()'s, bit for bit.
"""
from . import _stats
from .api import load_library
from .estep import resolve_schedule
from .gibbs import MODELS, _request  # noqa: F401


def entry_name(schedule="lanes"):
    """The library entry expected_stats() calls under a resolved schedule
    (estep.resolve_schedule): "expected_stats", or "expected_stats_scan"."""
    return "expected_stats_scan" if schedule == "scan" else "expected_stats"


def expected_stats(model, data, draws, pairing="grid", device=-1, lib=None, return_status=False, schedule="auto",
                   flags=0):
    """Expected sufficient statistics of every (series, draw) pair.

    schedule ("auto", "lanes", "scan") and flags as for estep(): "scan" is the
    parallel scan over T for few pairs and long series (hhmm_expected_stats_scan).

    draws as draw_stats() takes them ({p_1k, A_ij, phi_k}; hhmm-tayal2009:
    {p_11, A_row, phi_k}).  Returns {name: array}: loglik (P,), n_1k (P, K),
    xi_ij (P, K, K), c_kl (P, K, L).  n_1k and xi_ij count only where the
    program multiplies the probability in; a structural zero of A gives an
    exact zero.  A pair whose log-likelihood is -inf or NaN has NaN
    statistics."""
    lib = lib or load_library()
    pr, res, out = _request(model, data, draws, pairing, device)
    pr.req.flags = int(flags)
    return _stats.call(lib, entry_name(resolve_schedule(pr, schedule, lib)), pr, res, out, return_status)
