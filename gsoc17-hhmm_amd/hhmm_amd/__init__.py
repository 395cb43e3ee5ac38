"""hhmm_amd -- MI355X (gfx950) engine for the HMM-family hot path of
moon1910/gsoc17-hhmm: forward filter, backward pass, smoothed posteriors and
Viterbi decoding of the Stan programs in hmm/, iohmm-*/ and tayal2009/,
evaluated for many (series x posterior draw) pairs at once.

The compute lives in libhhmm.so (C ABI: include/hhmm.h).  This package is the
host-side mirror of the reference's rstan boundary (`gqs`, shaped like
rstan::extract()) plus the synthetic-data and multi-GPU helpers used by
bench.py.
"""
from . import _abi  # noqa: F401
from .api import HHMMError, PreparedRequest, gqs, load_library, reshape_pairs  # noqa: F401
from .summary import gqs_summary, quantiles  # noqa: F401
from .estep import estep, m_step, score  # noqa: F401
from .expect import expected_stats  # noqa: F401
from .em import baum_welch  # noqa: F401
from .estep_io import em_io, estep_io, m_step_io, score_io  # noqa: F401
from .pointwise import pointwise_predictive, waic  # noqa: F401
from .psis import lfo, loo, psis_cells, psis_predictive  # noqa: F401
from .gibbs import conditional_draw, draw_stats, gibbs, stack_chains  # noqa: F401
from .gibbs_gauss import conditional_draw_gauss, draw_stats_gauss, gibbs_gauss, relabel_ordered  # noqa: F401

__version__ = "0.1.0"
