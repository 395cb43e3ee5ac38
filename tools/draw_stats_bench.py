#!/usr/bin/env python3
"""Times the draw statistics (hhmm_draw_stats_device; hhmm_draw_stats_large_device
at K > 8) beside the path a caller had before it: hhmm_run_device with loglik |
z_ffbs, then a torch reduction of the [P, T] path to the same counts.  Also one
full Gibbs sweep: the uniforms, the draw statistics and the conjugate updates.
All at the C2 shape (hmm-multinom, K = 4, L = 9, 1M pairs x T = 1000, ZIP
pairing) on one device, device-resident inputs, events on torch's stream, the
paths interleaved in one process: every round times each of them once.  Prints
one JSON line.

    python tools/draw_stats_bench.py
    python tools/draw_stats_bench.py --pairs 65536 --T 256      # a smaller shape
    python tools/draw_stats_bench.py --K 23 --pairs 100000      # the large-K shape of estep_bench.py --K 23

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
sys.path.insert(0, str(ROOT / "tools"))


def stamp(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(times):
    return {"ms": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "iters": len(times)}


def run_child(a):
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    from estep_bench import device_request
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    P, T, K, L = a.pairs, a.T, a.K, a.L
    entry = "hhmm_draw_stats" if K <= 8 else "hhmm_draw_stats_large"
    req, keep, dev = device_request(torch, P, T, K, L)
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    ubuf = torch.empty(P * T, dtype=torch.float64, device=dev)

    def uniforms():
        torch.rand(P * T, dtype=torch.float64, device=dev, generator=gen, out=ubuf)
        ubuf.neg_().add_(1.0)
    uniforms()
    req.ffbs_u = ubuf.data_ptr()

    # (a) the draw statistics
    sres = _abi.EstepResult()
    sizes = {"loglik": P, "n_1k": P * K, "xi_ij": P * K * K, "c_kl": P * K * L}
    sbuf = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
    for k, v in sbuf.items():
        setattr(sres, k, v.data_ptr())
    sstat = torch.zeros(P, dtype=torch.int32, device=dev)
    sres.pair_status = sstat.data_ptr()
    ws_a = C.c_size_t(0)
    assert getattr(lib, entry + "_workspace_size")(C.byref(req), C.byref(ws_a)) == 0, lib.hhmm_last_error().decode()
    wa = torch.empty(max(ws_a.value, 256), dtype=torch.uint8, device=dev)

    stats_device = getattr(lib, entry + "_device")

    def stats():
        rc = stats_device(C.byref(req), C.byref(sres), wa.data_ptr(), wa.numel(), st)
        assert rc == 0, lib.hhmm_last_error().decode()

    # (b) the path itself, then its reduction in torch
    req_b = _abi.Request.from_buffer_copy(req)
    req_b.outputs = _abi.OUT["loglik"] | _abi.OUT["z_ffbs"]
    rres = _abi.Result()
    ll_b = torch.empty(P, dtype=torch.float64, device=dev)
    z = torch.zeros((T, P), dtype=torch.int32, device=dev)        # z[p + P t]
    rres.loglik, rres.z_ffbs = ll_b.data_ptr(), z.data_ptr()
    rstat = torch.zeros(P, dtype=torch.int32, device=dev)
    rres.pair_status = rstat.data_ptr()
    ws_b = C.c_size_t(0)
    assert lib.hhmm_workspace_size(C.byref(req_b), C.byref(ws_b)) == 0, lib.hhmm_last_error().decode()
    wb = torch.empty(max(ws_b.value, 256), dtype=torch.uint8, device=dev)

    def path():
        rc = lib.hhmm_run_device(C.byref(req_b), C.byref(rres), wb.data_ptr(), wb.numel(), st)
        assert rc >= 0, lib.hhmm_last_error().decode()

    red = {}

    def reduce():
        z0 = z.to(torch.int64) - 1
        one = torch.ones((1, 1), dtype=torch.int32, device=dev)
        red["n_1k"] = torch.zeros((K, P), dtype=torch.int32, device=dev).scatter_add_(0, z0[:1], one.expand(1, P))
        red["xi_ij"] = torch.zeros((K * K, P), dtype=torch.int32, device=dev).scatter_add_(
            0, z0[:-1] + K * z0[1:], one.expand(T - 1, P))                  # i + K j
        red["c_kl"] = torch.zeros((K * L, P), dtype=torch.int32, device=dev).scatter_add_(
            0, z0 + K * (keep["x"].to(torch.int64) - 1), one.expand(T, P))   # k + K l

    # one Gibbs sweep: uniforms + (a) + the conjugate updates, parameters written back in place
    views = {"n_1k": sbuf["n_1k"].view(K, P).t(), "xi_ij": sbuf["xi_ij"].view(K, K, P).permute(2, 1, 0),
             "c_kl": sbuf["c_kl"].view(L, K, P).permute(2, 1, 0)}
    start = {k: keep[k].clone() for k in ("p_1k", "A_ij", "phi_k")}

    def sweep():
        uniforms()
        stats()
        new = hhmm_amd.conditional_draw("hmm-multinom", views, None, gen)
        for k in start:
            keep[k].copy_(new[k].permute(*reversed(range(new[k].dim()))))

    t = {"stats": [], "path": [], "reduce": [], "sweep": []}
    same = None
    for i in range(a.warmup + a.iters):
        row = {"stats": stamp(torch, stats), "path": stamp(torch, path), "reduce": stamp(torch, reduce)}
        if same is None:  # both paths computed the same counts from the same uniforms
            same = all(bool((red[k].reshape(-1) == sbuf[k].to(torch.int32)).all()) for k in red)
        row["sweep"] = stamp(torch, sweep)
        for k in start:  # the timed paths always see the same parameters
            keep[k].copy_(start[k])
        uniforms()
        if i >= a.warmup:
            for k, v in row.items():
                t[k].append(v)
    stats()
    torch.cuda.synchronize()
    ll = sbuf["loglik"]
    out = {k: summary(v) for k, v in t.items()}
    out["path_plus_reduce"] = summary([x + y for x, y in zip(t["path"], t["reduce"])])
    out.update({"same_counts": same, "workspace_GB": {"stats": round(ws_a.value / 1e9, 4), "path": round(ws_b.value / 1e9, 4)},
                "loglik_mean": float(ll.mean()), "loglik_finite": bool(torch.isfinite(ll).all()),
                "pair_failures": int((sstat != 0).sum()) + int((rstat != 0).sum()),
                "version": lib.hhmm_version().decode()})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=420.0, help="seconds for the measurement (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_child(a)
        return 0
    K, L, C_ = a.K, a.L, (8 if a.K <= 4 or a.K > 8 else 4)
    out = {"shape": {"model": "hmm-multinom", "pairing": "zip", "pairs": a.pairs, "T": a.T, "K": K, "L": L}}
    # bytes each path moves per (pair, step): x twice (forward, backward), u, the checkpoints out and back;
    # the parent's path also writes z, and its reduction reads z and x again (temporaries not counted)
    ck = 2 * 8.0 * K / C_
    out["bytes_per_step"] = {"stats": 4 + 4 + 8 + ck, "path": 4 + 4 + 8 + ck + 4, "reduce_at_least": 4 + 4}
    if K <= 8:
        per_wave = L * (1024 * ((K + 1) // 2) + 256 * K) + 256 * K * K
        out["lds_bytes_per_wave"] = {"stats": per_wave, "path": L * 1024 * ((K + 1) // 2)}
    else:  # a group of G lanes per pair: slots, phi table, its counts and the xi rows against slots and phi table
        G = 16 if K <= 16 else 32
        out["lds_bytes_per_group"] = {"stats": G * (16 + 12 * L + 4 * K), "path": G * (16 + 8 * L)}
    # what each route writes: the statistics, or the path itself
    out["bytes_written"] = {"stats": a.pairs * (1 + K + K * K + K * L) * 8, "path": 4 * a.pairs * a.T}
    cmd = [sys.executable, __file__, "--child"] + [f"--{k}={getattr(a, k)}" for k in
                                                   ("pairs", "T", "K", "L", "warmup", "iters")]
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
    out["stats_over_path_plus_reduce"] = round(out["stats"]["ms"] / out["path_plus_reduce"]["ms"], 4)
    out["stats_over_path"] = round(out["stats"]["ms"] / out["path"]["ms"], 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
