#!/usr/bin/env python3
"""Times the E-step as a parallel scan over T (hhmm_estep_scan_device,
hhmm_expected_stats_scan_device) beside the sequential entry on the same
request (hhmm_estep_device / hhmm_expected_stats_device: a lane walks a whole
series) and beside hhmm_run_device's forward-backward (loglik + gamma_tk), which
does the same sweeps through its own T-scan and writes [P, T, K] where the
E-step writes [P, K..].

    python tools/estep_scan_bench.py                 # the long-series shapes
    python tools/estep_scan_bench.py --table         # both schedules at P x T around the "auto" gate
    python tools/estep_scan_bench.py --shape multinom:8:65536

A shape is model:pairs:T with model multinom (hmm-multinom, K = 4, L = 9, one
series under `pairs` parameter sets, GRID) or tayal (hhmm-tayal2009, one series
of signs under `pairs` draws).  One device, device-resident inputs, events on
torch's stream, the paths interleaved: every round times each of them once.
Each shape runs in a child process of its own under --step-timeout seconds; a
shape that does not finish is reported as such and not tried again.  Prints one
JSON line per shape.
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

LONG = ["multinom:1:1000000", "multinom:8:1000000", "multinom:64:1000000", "tayal:250:1000000"]
TABLE = [f"multinom:{P}:{T}" for T in (8192, 65536) for P in (1, 64, 1024, 4096)]


def summary(times):
    return {"ms": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "iters": len(times)}


def run_child(a):
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    kind, P, T = a.shape.split(":")
    P, T, K, L = int(P), int(T), 4, 9
    tayal = kind == "tayal"
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(20260101)
    st = torch.cuda.current_stream().cuda_stream

    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device=dev, generator=g)

    keep = {"x": torch.randint(1, L + 1, (T,), dtype=torch.int32, device=dev, generator=g),
            "sign": torch.randint(1, 3, (T,), dtype=torch.int32, device=dev, generator=g),
            "p_1k": torch.softmax(rnd(K, P), 0), "A_ij": torch.softmax(rnd(K, K, P), 0),
            "p_11": torch.sigmoid(rnd(P)), "A_row": torch.softmax(rnd(2, 2, P), 0),
            "phi_k": torch.softmax(rnd(L, K, P), 0)}

    def request(outputs=0, flags=0):
        req = _abi.Request()
        req.abi_version = _abi.ABI_VERSION
        req.model = _abi.MODELS["hhmm-tayal2009" if tayal else "hmm-multinom"]
        req.pairing, req.device, req.outputs, req.flags = _abi.PAIR_GRID, -1, outputs, flags
        req.data.n_series, req.data.T_max, req.data.K, req.data.L = 1, T, K, L
        req.draws.n_draws = P
        req.data.x_int = keep["x"].data_ptr()
        if tayal:
            req.data.sign = keep["sign"].data_ptr()
        for name in (("p_11", "A_row", "phi_k") if tayal else ("p_1k", "A_ij", "phi_k")):
            setattr(req.draws, name, keep[name].data_ptr())
        return req

    sizes = {"loglik": P, "n_1k": P * K, "xi_ij": P * K * K, "c_kl": P * K * L}
    stem = "hhmm_expected_stats" if tayal else "hhmm_estep"

    def stats_path(entry, flags=0):
        req, res = request(flags=flags), _abi.EstepResult()
        bufs = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        status = torch.zeros(P, dtype=torch.int32, device=dev)
        res.pair_status = status.data_ptr()
        ws = C.c_size_t(0)
        assert getattr(lib, entry + "_workspace_size")(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)
        run = getattr(lib, entry + "_device")

        def launch():
            assert run(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st) == 0, lib.hhmm_last_error().decode()
        return {"launch": launch, "out": bufs, "status": status, "keep": (req, res, wbuf), "ms": [],
                "workspace_mib": round(ws.value / 2 ** 20, 1)}

    def gamma_path():
        req, res = request(_abi.OUT["loglik"] | _abi.OUT["gamma_tk"]), _abi.Result()
        bufs = {"loglik": torch.empty(P, dtype=torch.float64, device=dev),
                "gamma_tk": torch.empty(P * T * K, dtype=torch.float64, device=dev)}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        status = torch.zeros(P, dtype=torch.int32, device=dev)
        res.pair_status = status.data_ptr()
        ws = C.c_size_t(0)
        assert lib.hhmm_workspace_size(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)

        def launch():
            assert lib.hhmm_run_device(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st) >= 0, \
                lib.hhmm_last_error().decode()
        return {"launch": launch, "out": bufs, "status": status, "keep": (req, res, wbuf), "ms": [],
                "workspace_mib": round(ws.value / 2 ** 20, 1)}

    paths = {"scan": stats_path(stem + "_scan", _abi.flag_scan_chunk_log2(a.chunk_log2)), "lanes": stats_path(stem)}
    if a.gamma:
        paths["run_gamma"] = gamma_path()
    cl, nc = C.c_int32(0), C.c_int32(0)
    lib.hhmm_estep_scan_plan(C.byref(paths["scan"]["keep"][0]), C.byref(cl), C.byref(nc))
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
    out = {"shape": a.shape, "scan_plan": {"cl": cl.value, "nc": nc.value}}
    for name, row in paths.items():
        out[name] = summary(row["ms"])
        out[name].update({"workspace_mib": row["workspace_mib"], "pair_failures": int((row["status"] != 0).sum()),
                          "loglik_finite": bool(torch.isfinite(row["out"]["loglik"]).all())})
    # the two schedules on the same request: the contract's tolerance, 1e-9 relative to max(1, |value|)
    worst = 0.0
    for k in sizes:
        u, v = paths["scan"]["out"][k], paths["lanes"]["out"][k]
        worst = max(worst, float(((u - v).abs() / v.abs().clamp(min=1.0)).max()))
    out["scan_vs_lanes_worst"] = worst
    out["lanes_over_scan"] = round(out["lanes"]["ms"] / out["scan"]["ms"], 2)
    if a.gamma:
        out["scan_over_run_gamma"] = round(out["scan"]["ms"] / out["run_gamma"]["ms"], 3)
    out["version"] = lib.hhmm_version().decode()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="model:pairs:T (repeatable)")
    ap.add_argument("--table", action="store_true", help="the P x T table around the auto gate")
    ap.add_argument("--chunk-log2", type=int, default=0, help="the scan's T-chunk length 2^n (0: the plan's choice)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1, help="launches per timed window")
    ap.add_argument("--no-gamma", dest="gamma", action="store_false", help="skip hhmm_run_device's gamma_tk beside it")
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds per shape (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.shape = a.shape[0]
        run_child(a)
        return 0
    rc = 0
    for shape in a.shape or (TABLE if a.table else LONG):
        cmd = [sys.executable, __file__, "--child", f"--shape={shape}", f"--warmup={a.warmup}", f"--iters={a.iters}",
               f"--reps={a.reps}", f"--chunk-log2={a.chunk_log2}"] + ([] if a.gamma else ["--no-gamma"])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": shape, "error": f"not finished within {a.step_timeout:g} s"}), flush=True)
            return 1  # a hung device path: nothing more is started on it
        if r.returncode != 0:
            print(json.dumps({"shape": shape, "error": f"exit status {r.returncode}", "stderr": r.stderr[-600:]}),
                  flush=True)
            return 1
        print(r.stdout.strip().split("\n")[-1], flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
