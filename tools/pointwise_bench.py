#!/usr/bin/env python3
"""Times the pointwise predictive densities at 8 < K <= 32
(hhmm_pointwise_large_device, with and without lp_t) beside the route a caller
had to the same four arrays: hhmm_run_device with loglik | unalpha_tk (the
log-space kernel, [P, T, K] written), then on the device torch's logsumexp over
the states, the difference along t, and the three reductions over the draws.
hmm-multinom, L = 9, N = 4 series x D = 4096 draws (GRID pairing, P = 16384),
T = 1000, at K = 12 and K = 23 unless told otherwise; the routes interleaved in
one run, device-resident inputs, events on torch's stream.  Prints one JSON
line (--out: writes it to a file too).

    python tools/pointwise_bench.py
    python tools/pointwise_bench.py --K 12 --draws 512 --T 256      # a smaller shape
    python tools/pointwise_bench.py --out profiles/pointwise_large_bench.json

Each measurement runs in a fresh child process under its own time limit
(--step-timeout); after a child that fails or runs out of time nothing more is
started.  The child of the old route also runs the new entry once, outside the
timing, and reports the largest discrepancy between the two lp_t.
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

STEPS = ("pointwise_lp", "unalpha", "pointwise")  # per K, in this order: the old route between the two new ones


def device_request(torch, N, D, T, K, L, seed=20260101):
    """(request, kept tensors) for hmm-multinom under GRID pairing, everything on the GPU."""
    from hhmm_amd import _abi
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    keep = {
        "x": torch.randint(1, L + 1, (T, N), dtype=torch.int32, device=dev, generator=g),       # x[n + N t]
        "p_1k": torch.softmax(torch.randn((K, D), dtype=torch.float64, device=dev, generator=g), 0),
        "A_ij": torch.softmax(torch.randn((K, K, D), dtype=torch.float64, device=dev, generator=g), 0),  # [j][i][s]
        "phi_k": torch.softmax(torch.randn((L, K, D), dtype=torch.float64, device=dev, generator=g), 0),  # [l][k][s]
    }
    req = _abi.Request()
    req.abi_version = _abi.ABI_VERSION
    req.model = _abi.MODELS["hmm-multinom"]
    req.pairing = _abi.PAIR_GRID
    req.device = -1
    req.data.n_series, req.data.T_max, req.data.K, req.data.L = N, T, K, L
    req.data.x_int = keep["x"].data_ptr()
    req.draws.n_draws = D
    for name in ("p_1k", "A_ij", "phi_k"):
        setattr(req.draws, name, keep[name].data_ptr())
    return req, keep, dev


def timed(torch, launch, warmup, iters):
    times = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return {"ms": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "iters": iters}


def new_route(torch, lib, req, dev, N, P, T, with_lp):
    """(launch, buffers, workspace bytes) of hhmm_pointwise_large_device."""
    from hhmm_amd import _abi
    st = torch.cuda.current_stream().cuda_stream
    res = _abi.PointwiseResult()
    sizes = {"loglik": P, "lpd_t": N * T, "mean_t": N * T, "var_t": N * T}
    if with_lp:
        sizes["lp_t"] = P * T
    bufs = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
    for k, v in bufs.items():
        setattr(res, k, v.data_ptr())
    bufs["status"] = torch.zeros(P, dtype=torch.int32, device=dev)
    res.pair_status = bufs["status"].data_ptr()
    ws = C.c_size_t(0)
    assert lib.hhmm_pointwise_large_workspace_size(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
    wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)

    def launch():
        rc = lib.hhmm_pointwise_large_device(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
        assert rc == 0, lib.hhmm_last_error().decode()
    bufs["_keep"] = (res, wbuf)
    return launch, bufs, ws.value


def run_step(step, a):
    import math
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    N, D, T, K, L = a.series, a.draws, a.T, a.K, a.L
    P = N * D
    req, keep, dev = device_request(torch, N, D, T, K, L)
    row = {}
    if step in ("pointwise_lp", "pointwise"):
        with_lp = step == "pointwise_lp"
        launch, bufs, wsb = new_route(torch, lib, req, dev, N, P, T, with_lp)
        written = 8.0 * (P + 3 * N * T + P * T)  # l_t is written either way: to lp_t or to the workspace
        row = timed(torch, launch, a.warmup, a.iters)
        ll, status = bufs["loglik"], bufs["status"]
        row["lpd_sum"] = float(bufs["lpd_t"].sum())
    else:
        st = torch.cuda.current_stream().cuda_stream
        res = _abi.Result()
        req.outputs = _abi.OUT["loglik"] | _abi.OUT["unalpha_tk"]
        bufs = {"loglik": torch.empty(P, dtype=torch.float64, device=dev),
                "unalpha_tk": torch.empty(P * T * K, dtype=torch.float64, device=dev)}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        status = torch.zeros(P, dtype=torch.int32, device=dev)
        res.pair_status = status.data_ptr()
        ws = C.c_size_t(0)
        assert lib.hhmm_workspace_size(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wsb = ws.value
        wbuf = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        red = {}

        def launch():
            rc = lib.hhmm_run_device(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
            assert rc >= 0, lib.hhmm_last_error().decode()
            tot = torch.logsumexp(bufs["unalpha_tk"].view(K, T, P), dim=0)     # [T, P]: log sum_k exp unalpha
            lp = torch.diff(tot, dim=0, prepend=torch.zeros((1, P), dtype=tot.dtype, device=dev))
            cell = lp.view(T, N, D)                                             # the draws of a cell contiguous
            red["lp_t"] = lp
            red["lpd_t"] = torch.logsumexp(cell, dim=2) - math.log(D)
            red["mean_t"] = cell.mean(dim=2)
            red["var_t"] = cell.var(dim=2, unbiased=True)
        written = 8.0 * (P + P * T * K + 2 * P * T + 3 * N * T)  # unalpha, the log sums, their differences
        row = timed(torch, launch, a.warmup, a.iters)
        ll = bufs["loglik"]
        row["lpd_sum"] = float(red["lpd_t"].sum())
        # the two routes' l_t and reductions, outside the timing
        launch_new, nb, _ = new_route(torch, lib, req, dev, N, P, T, True)
        launch_new()
        torch.cuda.synchronize()

        def gap(x, y):
            return float(((x - y).abs() / y.abs().clamp(min=1.0)).max())
        row["lp_t_gap"] = gap(nb["lp_t"].view(T, P), red["lp_t"])
        row["reduced_gap"] = max(gap(nb[k].view(T, N), red[k]) for k in ("lpd_t", "mean_t", "var_t"))
    row.update({"output_GB": round(written / 1e9, 4), "workspace_GB": round(wsb / 1e9, 4),
                "loglik_mean": float(ll.mean()), "loglik_finite": bool(torch.isfinite(ll).all()),
                "pair_failures": int((status != 0).sum()), "version": lib.hhmm_version().decode()})
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4)
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--K", type=int, nargs="+", default=[12, 23])
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per measurement (child process)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        a.K = a.K[0]
        run_step(a.step, a)
        return 0
    out = {"shape": {"model": "hmm-multinom", "pairing": "grid", "series": a.series, "draws": a.draws,
                     "pairs": a.series * a.draws, "T": a.T, "L": a.L}}
    rc = 0
    for K in a.K:
        rows = out[f"K{K}"] = {}
        for step in STEPS:
            cmd = [sys.executable, __file__, "--step", step, f"--K={K}"] + [
                f"--{k}={getattr(a, k)}" for k in ("series", "draws", "T", "L", "warmup", "iters")]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                rows[step] = {"error": f"no result within {a.step_timeout} s"}
                rc = 1
                break
            if r.returncode != 0:
                rows[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-400:]}
                rc = 1
                break
            rows[step] = json.loads(r.stdout.strip().split("\n")[-1])
        if rc:
            break
        rows["pointwise_lp_over_unalpha"] = round(rows["pointwise_lp"]["ms"] / rows["unalpha"]["ms"], 4)
        rows["pointwise_over_unalpha"] = round(rows["pointwise"]["ms"] / rows["unalpha"]["ms"], 4)
        rows["same_lp_t"] = rows["unalpha"]["lp_t_gap"] <= 1e-9 and rows["unalpha"]["reduced_gap"] <= 1e-9
    print(json.dumps(out))
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
