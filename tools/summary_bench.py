#!/usr/bin/env python3
"""Times the summary kernel alone (hhmm_summary_device on device buffers) and,
with --e2e, gqs_summary against gqs() + np.median + argmax on the host.
Prints one JSON line.

    python tools/summary_bench.py                  # the two DESIGN.md §9 kernel shapes
    python tools/summary_bench.py --e2e            # + the walk-forward end-to-end comparison
    python tools/summary_bench.py --shape 4,4096,10000,4,3

Kernel rows: median of --iters launches after --warmup, timed with events on
torch's stream over a buffer far larger than the Infinity Cache; read_TBps =
8 B * N*S*T*K / time, against the part's measured copy rate (6.29 TB/s).
"""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "gsoc17-hhmm_amd"))

COPY_TBPS = 6.29
SHAPES = [(4, 4096, 10000, 4, 3), (204, 250, 2000, 4, 1)]


def kernel_row(lib, torch, N, S, T, K, Q, warmup, iters):
    from hhmm_amd import _abi
    dev = torch.device("cuda", torch.cuda.current_device())
    v = torch.rand(N * S * T * K, dtype=torch.float64, device=dev)
    q = torch.empty(N * T * K * Q, dtype=torch.float64, device=dev)
    am = torch.empty(N * T, dtype=torch.int32, device=dev)
    req = _abi.SummaryRequest()
    req.n_series, req.n_draws, req.T_max, req.K, req.n_probs = N, S, T, K, Q
    for j, p in enumerate(np.linspace(0.1, 0.9, Q) if Q > 1 else [0.5]):
        req.probs[j] = p
    req.argmax_prob = 0.5
    req.values_f64 = v.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.hhmm_summary_device(C.byref(req), q.data_ptr(), am.data_ptr(), st)
        b.record()
        assert rc == 0, lib.hhmm_last_error().decode()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    nbytes = 8.0 * N * S * T * K
    return {"N": N, "S": S, "T": T, "K": K, "Q": Q, "ms": round(ms, 4), "ms_min": round(min(times), 4),
            "read_TBps": round(nbytes / ms / 1e9, 4), "of_copy_rate": round(nbytes / ms / 1e9 / COPY_TBPS, 4),
            "floor_ms": round(nbytes * (1 + Q / S) / COPY_TBPS / 1e9, 4)}


def e2e_row(lib, reps):
    """The walk-forward batch (204 windows x 250 draws, tayal-lite, BLOCK pairing):
    filtered in- and out-of-sample states, fused against the host reduction, interleaved."""
    import hhmm_amd
    from hhmm_amd import synth
    N, B, T, To = 204, 250, 2000, 400
    data, draws = synth.GENERATORS["hhmm-tayal2009-lite"](N=N, S=N * B, T=T, T_oos=To)
    pars = ["alpha_tk", "alpha_tk_oos"]

    def fused():
        s = hhmm_amd.gqs_summary("hhmm-tayal2009-lite", data, draws, pars, probs=(0.5,), hard=pars, pairing="block",
                                 lib=lib)
        return s["hard_alpha_tk"], s["hard_alpha_tk_oos"]

    def host():
        o = hhmm_amd.gqs("hhmm-tayal2009-lite", data, draws, pars=pars, pairing="block", lib=lib)
        out = []
        for k in pars:
            a = o[k].reshape((B, N) + o[k].shape[1:], order="F")
            out.append((np.median(a, axis=0).argmax(axis=-1) + 1).astype(np.int32))
        return out

    fused(), host()  # warm: pools, pinned buffers
    tf, th, same = [], [], True
    for _ in range(reps):
        t0 = time.perf_counter()
        f = fused()
        t1 = time.perf_counter()
        h = host()
        t2 = time.perf_counter()
        tf.append(t1 - t0)
        th.append(t2 - t1)
        same = same and all(np.array_equal(x, y) for x, y in zip(f, h))
    return {"shape": {"windows": N, "draws": B, "T": T, "T_oos": To, "K": 4}, "fused_s": round(float(np.median(tf)), 4),
            "host_s": round(float(np.median(th)), 4), "speedup": round(float(np.median(th) / np.median(tf)), 3),
            "same_states": bool(same), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="N,S,T,K,Q (repeatable; default: the two DESIGN.md shapes)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import hhmm_amd
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape] if a.shape else SHAPES
    out = {"version": lib.hhmm_version().decode(), "copy_rate_TBps": COPY_TBPS,
           "kernel": [kernel_row(lib, torch, *s, a.warmup, a.iters) for s in shapes]}
    if a.e2e:
        out["e2e"] = e2e_row(lib, a.e2e_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
