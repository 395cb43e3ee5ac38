#!/usr/bin/env python3
"""Times the IOHMM E-step (hhmm_estep_io_device) on iohmm-reg beside the
engine's loglik-only request of the same shape (hhmm_run_device with
HHMM_OUT_LOGLIK: the same transcendentals per step, none of the
accumulations): K = 3, M = 4, 65536 GRID pairs (64 series x 1024 draws) x
T = 300.  One device, device-resident inputs, events on torch's stream around
--reps launches, the two paths interleaved in one process: every round times
each of them once.  Prints one JSON line.

    python tools/estep_io_bench.py
    python tools/estep_io_bench.py --series 8 --draws 256 --T 64      # a smaller shape

The measurement runs in a child process under a time limit (--step-timeout).
"""
import argparse
import ctypes as C
import json
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "gsoc17-hhmm_amd"))


def summary(times):
    return {"ms": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "iters": len(times)}


def run_child(a):
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    N, S, T, K, M = a.series, a.draws, a.T, a.K, a.M
    P = N * S
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(20260101)
    st = torch.cuda.current_stream().cuda_stream

    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device=dev, generator=g)

    keep = {
        "x": 2.0 * rnd(T, N), "u": rnd(M, T, N),                               # [n + N t], [n + N (t + T m)]
        "p_1k": torch.softmax(rnd(K, S), 0), "w_km": 0.7 * rnd(M, K, S),       # [s + S (k + K m)]
        "b_km": rnd(M, K, S), "s_k": torch.exp(0.3 * rnd(K, S)),
    }

    def request():
        req = _abi.Request()
        req.abi_version = _abi.ABI_VERSION
        req.model = _abi.MODELS["iohmm-reg"]
        req.pairing = _abi.PAIR_GRID
        req.device = -1
        req.data.n_series, req.data.T_max, req.data.K, req.data.M = N, T, K, M
        req.draws.n_draws = S
        req.data.x_real, req.data.u = keep["x"].data_ptr(), keep["u"].data_ptr()
        for name in ("p_1k", "w_km", "b_km", "s_k"):
            setattr(req.draws, name, keep[name].data_ptr())
        return req

    def path(req, res, sizes, size_fn, run_fn):
        bufs = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        status = torch.zeros(P, dtype=torch.int32, device=dev)
        res.pair_status = status.data_ptr()
        ws = C.c_size_t(0)
        assert size_fn(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)

        def launch():
            rc = run_fn(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
            assert rc == 0, lib.hhmm_last_error().decode()
        return {"launch": launch, "loglik": bufs["loglik"], "status": status, "keep": (req, res, bufs, wbuf), "ms": []}

    ll_req = request()
    ll_req.outputs = _abi.OUT["loglik"]
    paths = {
        "loglik_only": path(ll_req, _abi.Result(), {"loglik": P}, lib.hhmm_workspace_size, lib.hhmm_run_device),
        "estep_io": path(request(), _abi.EstepIoResult(),
                         {"loglik": P, "n_1k": P * K, "gw_km": P * K * M, "n_k": P * K, "uu_kmm": P * K * M * M,
                          "ux_km": P * K * M, "xx_k": P * K},
                         lib.hhmm_estep_io_workspace_size, lib.hhmm_estep_io_device),
    }
    for i in range(a.warmup + a.iters):
        for row in paths.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                row["launch"]()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                row["ms"].append(e0.elapsed_time(e1) / a.reps)
    out = {}
    for name, row in paths.items():
        out[name] = summary(row["ms"])
        out[name].update({"loglik_mean": float(row["loglik"].mean()),
                          "loglik_finite": bool(torch.isfinite(row["loglik"]).all()),
                          "pair_failures": int((row["status"] != 0).sum())})
    ref, got = paths["loglik_only"]["loglik"], paths["estep_io"]["loglik"]
    out["loglik_worst_rel"] = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
    out["version"] = lib.hhmm_version().decode()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=64)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=400, help="launches per timed window")
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds for the measurement (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_child(a)
        return 0
    out = {"shape": {"pairs": a.series * a.draws, "series": a.series, "draws": a.draws, "T": a.T, "K": a.K, "M": a.M,
                     "reps": a.reps}}
    cmd = [sys.executable, __file__, "--child"] + [f"--{k}={getattr(a, k)}" for k in
                                                   ("series", "draws", "T", "K", "M", "warmup", "iters", "reps")]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
    except subprocess.TimeoutExpired:
        out["error"] = f"no result within {a.step_timeout} s"
        print(json.dumps(out))
        return 1
    if r.returncode != 0:
        out["error"] = f"exit status {r.returncode}"
        out["stderr"] = r.stderr[-600:]
        print(json.dumps(out))
        return 1
    out.update(json.loads(r.stdout.strip().split("\n")[-1]))
    out["estep_io_over_loglik_only"] = round(out["estep_io"]["ms"] / out["loglik_only"]["ms"], 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
