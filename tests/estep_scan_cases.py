"""What tests/test_estep_scan.py and tests/test_expected_stats_scan.py share: the
E-step and the expected statistics as a parallel scan over T
(include/hhmm_estep.h hhmm_estep_scan, include/hhmm_expect.h
hhmm_expected_stats_scan; csrc/hhmm_estep_scan.hip).

Geometry, restated from csrc/hhmm_plan.h so the tests can aim at its edges: a
series is cut into T-chunks of cl steps, cl a multiple of the checkpoint
interval C = fb_chunk(K) (8 at K <= 4, else 4); a phase-3 lane owns one (pair,
chunk) and a wave 64 consecutive chunks of one pair, so a pair has
ceil(nc / 64) waves whose records the reduction adds in order.  The tests force
small chunks (HHMM_FLAG_SCAN_FORCE | HHMM_FLAG_SCAN_CHUNK_LOG2) so that short
series cross every edge: T around one, two and three chunks, nc around one wave
(64 | 65) and past the four-wave boundary walk's blocks (257).
"""
import ctypes as C
import types

import numpy as np

from hhmm_amd import _abi, _stats

TOL = 1e-9  # include/hhmm_estep.h: relative to max(1, |reference|)
SEMISUP, TAYAL = "hmm-multinom-semisup", "hhmm-tayal2009"
# (pairing, N, S): P = 5 every time
PAIRINGS = [("grid", 1, 5), ("grid", 5, 1), ("zip", 5, 5), ("block", 5, 5)]
KS = [1, 2, 4, 5, 7, 8]  # both fb_chunk values, the Gaussian xi-in-LDS instances (K >= 7)
SCAN_LANES = 262144      # csrc/hhmm_plan.h kEstepScanLanes
SCAN_TAIL = 5            # kEstepScanTail


def fb_chunk(K):
    return 8 if K <= 4 else 4


def chunk_flags(K, mult):
    """(flags, cl): forced chunks of cl = mult * C steps (mult a power of two)."""
    cl = mult * fb_chunk(K)
    return _abi.FLAG_SCAN_FORCE | _abi.flag_scan_chunk_log2(cl.bit_length() - 1), cl


def edge_lengths(cl):
    return [1, 2, cl - 1, cl, cl + 1, 2 * cl, 2 * cl + 1, 3 * cl + 3]


def worst(got, want):
    """Largest |got - want| / max(1, |want|) over the statistics; NaN and infinities must coincide."""
    w = 0.0
    for name, ref in want.items():
        out = got[name]
        assert out.shape == ref.shape, (name, out.shape, ref.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(out), np.isnan(ref)), name
        assert np.array_equal(out[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), name
        if fin.any():
            w = max(w, float(np.max(np.abs(out[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))))
    return w


def rows(stats, keep):
    return {k: v[keep] for k, v in stats.items() if k not in ("pair_status", "status")}


def shape_request(model, K, L, P, Tmax, flags=0):
    """A request that describes its shape and nothing else (planning and sizing read no arrays)."""
    r = _abi.Request()
    r.abi_version = _abi.ABI_VERSION
    r.model = _abi.MODELS[model]
    r.pairing = _abi.PAIR_ZIP
    r.flags = flags
    r.data.n_series = r.draws.n_draws = P
    r.data.K, r.data.L, r.data.T_max = K, L, Tmax
    return r


def shape_pr(model, K, L, P, Tmax, flags=0):
    """What estep.resolve_schedule reads of a PreparedRequest, without its arrays."""
    return types.SimpleNamespace(K=K, P=P, Tmax=Tmax, req=shape_request(model, K, L, P, Tmax, flags))


def plan_of(engine, model, K, L, P, Tmax, flags=0):
    cl, nc = C.c_int32(-1), C.c_int32(-1)
    r = shape_request(model, K, L, P, Tmax, flags)
    assert engine.hhmm_estep_scan_plan(C.byref(r), C.byref(cl), C.byref(nc)) == _abi.OK, engine.hhmm_last_error()
    return cl.value, nc.value


def auto_chunk(K, P, Tmax):
    """csrc/hhmm_plan.cpp estep_scan_plan left to choose: 4 C doubled until P * nc <= SCAN_LANES."""
    cl = 4 * fb_chunk(K)
    while P * -(-Tmax // cl) > SCAN_LANES and cl < 1 << 20:
        cl *= 2
    return cl, -(-Tmax // cl)


def layout_bytes(K, L, P, cl, nc, gauss=False):
    """The workspace include/hhmm_estep.h documents for hhmm_estep_scan."""
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    ncw = -(-nc // 64) * 64
    ns = K + K * K + (3 * K if gauss else K * L)
    regions = [nc * K * K * P, nc * 3 * P, nc * K * P, nc * P, nc * K * P, nc * P, (cl // fb_chunk(K)) * K * P * ncw,
               P * (ncw // 64) * (ns + SCAN_TAIL), P * K * K]
    return sum(up(8 * n) for n in regions) + 256


def device_run(engine, entry, pr, res, out, flags):
    """One run of hhmm_<entry>_device on torch's stream; the statistics on the host."""
    import torch
    pr.req.flags = int(flags)
    dv = _stats.DeviceStats(engine, entry, pr, res, {name: a.shape for name, a in out.items()})
    first = _run(dv, torch)
    return dv, first


def _run(dv, torch=None):
    if torch is None:
        import torch
    assert dv.run() == 0
    torch.cuda.synchronize()
    return dv.stats()


rerun = _run
