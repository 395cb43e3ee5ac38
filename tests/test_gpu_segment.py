"""GPU: one series split along T over ranks (include/hhmm.h hhmm_segment;
SURVEY.md §8e "single very long series": each GPU scans its T-chunk, the K x K
chunk summaries are all-gathered, each GPU fixes up its prefix).

The windows' results, stitched along T, must equal the whole series: the
engine's sequential sweep and the oracle (loglik from the chained summaries,
alpha / beta / gamma per step) within tests/tolerances.py.  First in one
process, window by window (R = 1, 2, 3, 5 windows of unequal length), then
over two gloo ranks on the box's GPU through dist.gqs_tsplit."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from hhmm_amd import synth
from tolerances import compare

pytestmark = pytest.mark.gpu

PARS = ["loglik", "alpha_tk", "beta_tk", "gamma_tk"]


def _windows_in_one_process(engine, model, data, draws, R, pars=PARS, pairing="grid"):
    from hhmm_amd import segment
    T = np.atleast_2d(data["x"]).shape[-1]
    wins = segment.windows(T, R)
    runs = [segment.SegmentWindow(engine, model, segment.slice_time(data, t0, t1), draws, pars, i == 0,
                                  i == R - 1, pairing) for i, (t0, t1) in enumerate(wins)]
    sums = [w.summary().cpu().numpy() for w in runs]
    enter, leave, loglik = segment.boundaries(sums, runs[0].K)
    outs = [w.finish(enter[i], leave[i]) for i, w in enumerate(runs)]
    stitched = {k: np.concatenate([o[k] for o in outs], axis=1) for k in pars if k != "loglik"}
    stitched["loglik"] = loglik
    last = outs[-1]["loglik"]  # the last window's own loglik (phase 2 from its entering state)
    return stitched, last


@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("model", ["hmm-multinom", "hmm", "hhmm-tayal2009", "hmm-multinom-semisup"])
def test_segments_equal_the_whole_series(engine, oracle, model, R):
    import hhmm_amd
    # T = 1001: past ~1500 steps the Tayal masks drive alpha and beta onto
    # different states (Q6) and gamma's smallest components (~1e-164) carry the
    # T-scan's own ~1e-8 relative reassociation error, before they underflow to
    # NaN in the reference's formula near t = 2000; the scan's
    # own tests stop at T = 1000 for the same reason (tests/test_gpu_scan.py)
    data, draws = synth.GENERATORS[model](N=2, S=3, T=1001)
    got, last = _windows_in_one_process(engine, model, data, draws, R)
    ref = oracle.gqs(model, data, draws, pars=PARS)
    whole = hhmm_amd.gqs(model, data, draws, pars=PARS, lib=engine)
    compare("loglik", got["loglik"], ref["loglik"])
    compare("loglik", last, ref["loglik"])
    for k in ("alpha_tk", "beta_tk", "gamma_tk"):
        compare(k, got[k], whole[k])
        compare(k, got[k], ref[k])


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("K", [16, 23])
@pytest.mark.parametrize("model", ["hmm-multinom", "hmm"])
def test_segments_large_K(engine, oracle, model, K, R):
    """hmm-multinom and hmm.stan at K > 8 (the T-split stopped at K <= 8;
    VERDICT r4: hmm.stan's K is data too, hmm/stan/hmm.stan:8): the summaries come
    from the MFMA chunk products (lks_prod_kernel; hmm.stan's per-step emission
    shifts travel as each chunk's log scale) chained by lks_seg_summary_kernel,
    the finish from lks_bound_kernel + lk_fb_kernel."""
    import hhmm_amd
    kw = {"L": 9} if model == "hmm-multinom" else {}
    data, draws = synth.GENERATORS[model](N=2, S=3, T=3001, K=K, **kw)
    pars = ["loglik", "alpha_tk", "beta_tk", "gamma_tk"]
    got, last = _windows_in_one_process(engine, model, data, draws, R, pars=pars)
    ref = oracle.gqs(model, data, draws, pars=pars, nthreads=6)
    whole = hhmm_amd.gqs(model, data, draws, pars=pars, lib=engine)
    compare("loglik", got["loglik"], ref["loglik"])
    compare("loglik", last, ref["loglik"])
    for k in ("alpha_tk", "beta_tk", "gamma_tk"):
        compare(k, got[k], whole[k])
        compare(k, got[k], ref[k])


def test_segments_large_K_long_series(engine, oracle):
    """The N2 shape scaled down: one series of 10^5 steps under 4 draws at
    K = 23 over 3 windows."""
    data, draws = synth.GENERATORS["hmm-multinom"](N=1, S=4, T=100_000, K=23, L=9)
    got, _ = _windows_in_one_process(engine, "hmm-multinom", data, draws, 3, pars=["loglik", "gamma_tk"])
    ref = oracle.gqs("hmm-multinom", data, draws, pars=["loglik", "gamma_tk"], nthreads=4)
    compare("loglik", got["loglik"], ref["loglik"])
    compare("gamma_tk", got["gamma_tk"], ref["gamma_tk"])


def test_segments_long_series_few_pairs(engine, oracle):
    """Few pairs, long T: 4 pairs of one series of 2e5 steps over 4 windows,
    against the oracle."""
    data, draws = synth.GENERATORS["hmm-multinom"](N=1, S=4, T=200_000)
    got, _ = _windows_in_one_process(engine, "hmm-multinom", data, draws, 4, pars=["loglik", "gamma_tk"])
    ref = oracle.gqs("hmm-multinom", data, draws, pars=["loglik", "gamma_tk"])
    compare("loglik", got["loglik"], ref["loglik"])
    compare("gamma_tk", got["gamma_tk"], ref["gamma_tk"])


def test_segment_rejects_viterbi_outputs(engine):
    from hhmm_amd import segment
    data, draws = synth.hmm_multinom(N=1, S=2, T=50)
    with pytest.raises(ValueError, match="no segment form"):
        segment.SegmentWindow(engine, "hmm-multinom", data, draws, ["loglik", "zstar_t"], True, True)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, out_dir, model="hmm", kw=None):
    import sys
    import pathlib
    repo = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(repo / "gsoc17-hhmm_amd")]
    import torch
    import torch.distributed as dist
    from hhmm_amd import dist as hdist
    torch.cuda.set_device(0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        data, draws = synth.GENERATORS[model](N=2, S=3, T=4000, **(kw or {}))
        (t0, t1), out, loglik = hdist.gqs_tsplit(model, data, draws, ["loglik", "gamma_tk"])
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), t0=t0, t1=t1, gamma=out["gamma_tk"], loglik=loglik)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model,kw", [("hmm", {}), ("hmm-multinom", {"K": 23, "L": 9}), ("hmm", {"K": 12})],
                         ids=["hmm", "multinom-K23", "hmm-K12"])
def test_two_ranks_gqs_tsplit(engine, oracle, tmp_path, model, kw):
    """dist.gqs_tsplit at world size 2 over gloo, both ranks on the box's GPU:
    each rank's window of gamma and the loglik every rank chains from the
    gathered summaries, against the oracle's whole series (K = 23: the large-K
    summaries, 2K^2 + 3 = 1061 doubles per pair and rank)."""
    port = _free_port()
    mp.spawn(_rank, args=(2, port, str(tmp_path), model, kw), nprocs=2, join=True)
    data, draws = synth.GENERATORS[model](N=2, S=3, T=4000, **kw)
    ref = oracle.gqs(model, data, draws, pars=["loglik", "gamma_tk"])
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    assert int(parts[0]["t1"]) == int(parts[1]["t0"]) and int(parts[1]["t1"]) == 4000
    compare("loglik", parts[0]["loglik"], ref["loglik"])
    compare("loglik", parts[1]["loglik"], ref["loglik"])
    gamma = np.concatenate([p["gamma"] for p in parts], axis=1)
    compare("gamma_tk", gamma, ref["gamma_tk"])


@pytest.mark.parametrize("K", [4, 12])
def test_segment_nan_draw_is_not_bad_data(engine, oracle, K):
    """A NaN draw parameter (phi_k[1, 0, :]) is not a data-block violation: split
    over three windows, every finish call reports the pair_status hhmm_run_device
    gives the whole series, which is the oracle's -- PAIR_OK, with a NaN loglik --
    and the pairs of the other draws are bit-equal to the clean run.  (The NaN
    reaches every boundary field of the spoiled draw's pairs, so the bad-data
    marker of a segment summary must be one that parameters cannot produce.)"""
    from hhmm_amd import _abi, segment
    from test_gpu_host_pipeline import _dev
    model, S, R = "hmm-multinom", 3, 3
    data, draws = synth.hmm_multinom(N=2, S=S, T=600, K=K, L=9)
    nan = {k: np.array(v, copy=True) for k, v in draws.items()}
    nan["phi_k"][1, 0, :] = np.nan
    wins = segment.windows(600, R)
    pars = ["loglik", "gamma_tk"]

    def run(d):
        runs = [segment.SegmentWindow(engine, model, segment.slice_time(data, a, b), d, pars, i == 0, i == R - 1)
                for i, (a, b) in enumerate(wins)]
        sums = [w.summary().cpu().numpy() for w in runs]
        enter, leave, loglik = segment.boundaries(sums, K)
        return [w.finish(enter[i], leave[i]) for i, w in enumerate(runs)], loglik

    clean, ll_clean = run(draws)
    got, ll_nan = run(nan)
    whole = _dev(engine, model, data, nan, pars, "grid")
    ref = oracle.gqs(model, data, nan, pars=pars, return_status=True)
    assert np.array_equal(whole["pair_status"], ref["pair_status"])
    assert np.all(ref["pair_status"] == _abi.PAIR_OK)
    hit = np.arange(2 * S) % S == 1  # grid pairing: p = s + S n
    assert np.all(np.isnan(ref["loglik"][hit])) and np.all(np.isfinite(ref["loglik"][~hit]))
    for i in range(R):
        assert np.array_equal(got[i]["pair_status"], whole["pair_status"]), (i, got[i]["pair_status"])
        assert np.array_equal(got[i]["gamma_tk"][~hit], clean[i]["gamma_tk"][~hit])
    assert np.array_equal(ll_nan[~hit], ll_clean[~hit])
    # and the windows, stitched, are the oracle's whole series: NaN where it has NaN
    compare("loglik", ll_nan, ref["loglik"])
    compare("gamma_tk", np.concatenate([g["gamma_tk"] for g in got], axis=1), ref["gamma_tk"])


@pytest.mark.parametrize("bad_window", [0, 1, 2])
@pytest.mark.parametrize("model,K", [("hmm-multinom", 4), ("hmm-multinom", 12)])
def test_segment_bad_data_in_one_window(engine, oracle, model, K, bad_window):
    """an out-of-range symbol in ONE window's slice of one
    series.  Its summary carries segment.BAD_DATA as its log scale, so every window's finish call
    flags that series' pairs HHMM_PAIR_INVALID_DATA (not only the window that
    holds the bad step) and the chained loglik is NaN there; every other pair
    is OK and equal to the clean run."""
    from hhmm_amd import _abi, segment
    data, draws = synth.hmm_multinom(N=3, S=2, T=600, K=K, L=9)
    bad = {k: (np.array(v, copy=True) if k == "x" else v) for k, v in data.items()}
    R = 3
    wins = segment.windows(600, R)
    t0, t1 = wins[bad_window]
    bad["x"][1, (t0 + t1) // 2] = 10  # L + 1, series n = 1
    pars = ["loglik", "gamma_tk"]

    def run(d):
        runs = [segment.SegmentWindow(engine, model, segment.slice_time(d, a, b), draws, pars, i == 0, i == R - 1)
                for i, (a, b) in enumerate(wins)]
        sums = [w.summary().cpu().numpy() for w in runs]
        enter, leave, loglik = segment.boundaries(sums, K)
        return [w.finish(enter[i], leave[i]) for i, w in enumerate(runs)], loglik

    clean, ll_clean = run(data)
    got, ll_bad = run(bad)
    S = 2
    series = np.arange(3 * S) // S  # grid pairing: p = s + S n
    hit = series == 1
    for i in range(R):
        st = got[i]["pair_status"]
        assert np.all(st[hit] == _abi.PAIR_INVALID_DATA), (i, st)
        assert np.all(st[~hit] == _abi.PAIR_OK), (i, st)
        assert np.all(clean[i]["pair_status"] == _abi.PAIR_OK)
        assert np.array_equal(got[i]["gamma_tk"][~hit], clean[i]["gamma_tk"][~hit])
    assert np.all(np.isnan(ll_bad[hit])) and np.array_equal(ll_bad[~hit], ll_clean[~hit])
