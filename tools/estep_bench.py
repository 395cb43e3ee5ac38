#!/usr/bin/env python3
"""Times the batched E-step (hhmm_estep_device; hhmm_estep_large_device at
K > 8) beside the path a caller would otherwise take to the same statistics:
hhmm_run_device with loglik | gamma_tk (whose [P, T, K] output then still has
to be reduced, and which leaves xi to the host).  Both at the C2 shape
(hmm-multinom, K = 4, L = 9, 1M pairs x T = 1000, ZIP pairing) unless told
otherwise, on the same device in the same run, device-resident inputs, events
on torch's stream.  Prints one JSON line (--out: writes it to a file too).

    python tools/estep_bench.py
    python tools/estep_bench.py --pairs 65536 --T 256      # a smaller shape
    python tools/estep_bench.py --K 23 --pairs 100000 --out profiles/estep_large_bench.json   # N1's scale

Each measurement runs in a fresh child process under its own time limit
(--step-timeout); after a child that fails or runs out of time nothing more is
started.
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

STEPS = ("estep", "gamma")


def device_request(torch, P, T, K, L, seed=20260101):
    """(request, kept tensors) for hmm-multinom under ZIP pairing, everything on the GPU."""
    from hhmm_amd import _abi
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    keep = {
        "x": torch.randint(1, L + 1, (T, P), dtype=torch.int32, device=dev, generator=g),       # x[n + N t]
        "p_1k": torch.softmax(torch.randn((K, P), dtype=torch.float64, device=dev, generator=g), 0),
        "A_ij": torch.softmax(torch.randn((K, K, P), dtype=torch.float64, device=dev, generator=g), 0),  # [j][i][s]
        "phi_k": torch.softmax(torch.randn((L, K, P), dtype=torch.float64, device=dev, generator=g), 0),  # [l][k][s]
    }
    req = _abi.Request()
    req.abi_version = _abi.ABI_VERSION
    req.model = _abi.MODELS["hmm-multinom"]
    req.pairing = _abi.PAIR_ZIP
    req.device = -1
    req.data.n_series, req.data.T_max, req.data.K, req.data.L = P, T, K, L
    req.data.x_int = keep["x"].data_ptr()
    req.draws.n_draws = P
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


def run_step(step, a):
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    P, T, K, L = a.pairs, a.T, a.K, a.L
    req, keep, dev = device_request(torch, P, T, K, L)
    st = torch.cuda.current_stream().cuda_stream
    ws = C.c_size_t(0)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    if step == "estep":
        res = _abi.EstepResult()
        out = {"loglik": P, "n_1k": P * K, "xi_ij": P * K * K, "c_kl": P * K * L}
        bufs = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in out.items()}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        res.pair_status = status.data_ptr()
        entry = "hhmm_" + sys.modules["hhmm_amd.estep"].entry_name(K)
        assert getattr(lib, entry + "_workspace_size")(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)
        run_device = getattr(lib, entry + "_device")

        def launch():
            rc = run_device(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
            assert rc == 0, lib.hhmm_last_error().decode()
        written = 8.0 * sum(out.values())
    else:
        res = _abi.Result()
        req.outputs = _abi.OUT["loglik"] | _abi.OUT["gamma_tk"]
        bufs = {"loglik": torch.empty(P, dtype=torch.float64, device=dev),
                "gamma_tk": torch.empty(P * T * K, dtype=torch.float64, device=dev)}
        for k, v in bufs.items():
            setattr(res, k, v.data_ptr())
        res.pair_status = status.data_ptr()
        assert lib.hhmm_workspace_size(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
        wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)

        def launch():
            rc = lib.hhmm_run_device(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
            assert rc >= 0, lib.hhmm_last_error().decode()
        written = 8.0 * (P + P * T * K)
    row = timed(torch, launch, a.warmup, a.iters)
    ll = bufs["loglik"]
    row.update({"output_GB": round(written / 1e9, 4), "workspace_GB": round(ws.value / 1e9, 4),
                "loglik_mean": float(ll.mean()), "loglik_finite": bool(torch.isfinite(ll).all()),
                "pair_failures": int((status != 0).sum()), "version": lib.hhmm_version().decode()})
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per measurement (child process)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a)
        return 0
    out = {"shape": {"model": "hmm-multinom", "pairing": "zip", "pairs": a.pairs, "T": a.T, "K": a.K, "L": a.L}}
    rc = 0
    for step in STEPS:
        cmd = [sys.executable, __file__, "--step", step] + [f"--{k}={getattr(a, k)}" for k in
                                                            ("pairs", "T", "K", "L", "warmup", "iters")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            out[step] = {"error": f"no result within {a.step_timeout} s"}
            rc = 1
            break
        if r.returncode != 0:
            out[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-400:]}
            rc = 1
            break
        out[step] = json.loads(r.stdout.strip().split("\n")[-1])
    if rc == 0:
        out["estep_over_gamma"] = round(out["estep"]["ms"] / out["gamma"]["ms"], 4)
        out["same_loglik"] = abs(out["estep"]["loglik_mean"] - out["gamma"]["loglik_mean"]) <= 1e-9 * abs(
            out["gamma"]["loglik_mean"])
    print(json.dumps(out))
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
