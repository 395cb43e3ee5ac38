"""CPU: the device-set sharding of hhmm_run (HHMM_DEVICE_SET; hhmm_stage.cpp
make_shards / shard_rows) covers every output element exactly once, for every
pairing, with draw splits (GRID with fewer series than shards), ragged T and
every array class (series, draws, pairs).  hhmm_selftest_shards and
hhmm_selftest_pipeline run the shard and chunk plan on host buffers only, and
stage every chunk through the library's own gather_chunk and scatter_chunk --
the functions hhmm_run's device path calls, not a copy of them -- so this runs
without a GPU, and under host ASan / UBSan in tools/sanitize.sh."""
import ctypes as C

import numpy as np
import pytest

from hhmm_amd import _abi, api, synth

CASES = [
    ("hmm-multinom", "grid", dict(N=5, S=4)),
    ("hmm-multinom", "grid", dict(N=2, S=7)),      # fewer series than shards: split the draws
    ("hmm-multinom", "zip", dict(N=6, S=6)),
    ("hmm-multinom", "block", dict(N=3, S=9)),
    ("iohmm-hmix", "grid", dict(N=3, S=5)),
    ("hhmm-tayal2009-lite", "grid", dict(N=4, S=3)),
]
# GRID requests of one draw; appended after every older case, so that the older
# cases keep their positions (their test ids carry them)
ONE_DRAW_CASES = [
    # one draw (a posterior mean): with fewer series than shards the shard is
    # draws-shaped with a single draw, which only its layout tells from a series shard
    ("hmm-multinom", "grid", dict(N=2, S=1)),
    ("hmm-multinom", "grid", dict(N=4, S=1)),
    ("iohmm-hmix", "grid", dict(N=3, S=1)),
    ("hhmm-tayal2009-lite", "grid", dict(N=5, S=1)),
    # the all-ones corner, where every shard layout coincides
    ("hmm-multinom", "grid", dict(N=1, S=1)),
    ("hmm-multinom", "zip", dict(N=1, S=1)),
    ("hmm-multinom", "block", dict(N=1, S=1)),
]
ALL_CASES = CASES + ONE_DRAW_CASES


@pytest.mark.parametrize("nshards", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("model,pairing,sizes", ALL_CASES)
def test_shards_cover_every_output_element_once(engine, model, pairing, sizes, nshards):
    data, draws = synth.GENERATORS[model](T=23, **sizes)
    data["T"] = np.array([23 - 3 * (i % 4) for i in range(sizes["N"])], dtype=np.int32)
    pars = [p for p in synth.PARS[model] if p not in ("oblik_tk",)]
    pr = api.PreparedRequest(model, data, draws, pars, pairing)
    for a in pr.out.values():
        a[...] = 0
    assert engine.hhmm_selftest_shards(C.byref(pr.req), C.byref(pr.res), nshards) == _abi.OK, \
        engine.hhmm_last_error()
    for name, a in pr.out.items():
        assert np.all(a == 1), (name, np.unique(a))


def test_shard_selftest_rejects_bad_requests(engine):
    data, draws = synth.GENERATORS["hmm-multinom"](N=2, S=3, T=5)
    pr = api.PreparedRequest("hmm-multinom", data, draws, ["loglik"])
    assert engine.hhmm_selftest_shards(C.byref(pr.req), C.byref(pr.res), 0) == _abi.ERR_INVALID_ARGUMENT
    pr.res.loglik = None
    assert engine.hhmm_selftest_shards(C.byref(pr.req), C.byref(pr.res), 2) == _abi.ERR_INVALID_ARGUMENT


PIPE_CASES = CASES + [
    ("hmm-multinom", "grid", dict(N=1, S=11)),     # one series: chunks split the draws
    ("iohmm-reg", "block", dict(N=4, S=12)),
] + ONE_DRAW_CASES


@pytest.mark.parametrize("nshards,nchunks", [(1, 1), (1, 2), (1, 3), (1, 7), (2, 3), (3, 2), (5, 4),
                                             (3, 1), (8, 1), (8, 3), (8, 7)])
@pytest.mark.parametrize("model,pairing,sizes", PIPE_CASES)
def test_pipeline_chunks_cover_every_output_element_once(engine, model, pairing, sizes, nshards, nchunks):
    """hhmm_run's host pipeline (VERDICT r5 missing 2): the chunk split of every
    device shard, the chunk layout, the staging gather (checked byte for byte in
    the library) and the scatter, on host buffers only -- every output element
    and every pair status is written exactly once, for every pairing, draw
    splits, ragged T (the outputs are staged up as well) and every array class."""
    data, draws = synth.GENERATORS[model](T=23, **sizes)
    data["T"] = np.array([23 - 3 * (i % 4) for i in range(sizes["N"])], dtype=np.int32)
    pars = [p for p in synth.PARS[model] if p not in ("oblik_tk",)]
    pr = api.PreparedRequest(model, data, draws, pars, pairing)
    for a in pr.out.values():
        a[...] = 0
    pr.status[...] = 0
    assert engine.hhmm_selftest_pipeline(C.byref(pr.req), C.byref(pr.res), nshards, nchunks) == _abi.OK, \
        engine.hhmm_last_error()
    for name, a in pr.out.items():
        assert np.all(a == 1), (name, np.unique(a))
    assert np.all(pr.status == 1)


def test_pipeline_selftest_large_rows_threaded(engine):
    """Slices above the 4 MB threading threshold: the staging copies split over
    host threads (by rows, and within one long row for contiguous slices)."""
    data, draws = synth.hmm_multinom(N=3, S=700, T=600)
    pars = ["loglik", "gamma_tk", "zstar_t"]
    pr = api.PreparedRequest("hmm-multinom", data, draws, pars, "grid")
    for a in pr.out.values():
        a[...] = 0
    assert engine.hhmm_selftest_pipeline(C.byref(pr.req), C.byref(pr.res), 1, 3) == _abi.OK
    for name, a in pr.out.items():
        assert np.all(a == 1), name
