#!/usr/bin/env python3
"""Times the Gaussian draw statistics (hhmm_draw_stats_gauss_device) beside the
path a caller had before it: hhmm_run_device with loglik | z_ffbs on hmm, then a
torch reduction of the [P, T] path and the series to the same six statistics.
Also one full Gibbs sweep: the uniforms, the draw statistics and the
Normal-Inverse-Gamma / Dirichlet updates.  hmm at K = 3 and K = 4, 1M ZIP pairs
x T = 1000 on one device, device-resident inputs, events on torch's stream, the
paths interleaved in one process per K: every round times each of them once.
Prints one JSON line.

    python tools/draw_stats_gauss_bench.py
    python tools/draw_stats_gauss_bench.py --pairs 65536 --T 256 --K 4   # a smaller shape, one K

The measurement of each K runs in a child process under a time limit (--step-timeout).
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

from draw_stats_bench import stamp, summary  # noqa: E402


def device_request(torch, P, T, K, seed=20260101):
    """(request, kept tensors, device) for hmm under ZIP pairing, everything on the GPU: states 10 apart,
    sigma about 3 (synth.hmm_gauss's parameters)."""
    from hhmm_amd import _abi
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((T, P), dtype=torch.float64, device=dev, generator=g).mul_(3.0)                 # x[n + N t]
    x.add_(torch.randint(1, K + 1, (T, P), dtype=torch.int32, device=dev, generator=g).mul_(10))
    centre = 10.0 * torch.arange(1, K + 1, dtype=torch.float64, device=dev).reshape(K, 1)
    keep = {
        "x": x,
        "p_1k": torch.softmax(torch.randn((K, P), dtype=torch.float64, device=dev, generator=g), 0),
        "A_ij": torch.softmax(torch.randn((K, K, P), dtype=torch.float64, device=dev, generator=g), 0),  # [j][i][s]
        "mu_k": centre + 0.5 * torch.randn((K, P), dtype=torch.float64, device=dev, generator=g),
        "sigma_k": 3.0 * torch.exp(0.05 * torch.randn((K, P), dtype=torch.float64, device=dev, generator=g)),
    }
    req = _abi.Request()
    req.abi_version = _abi.ABI_VERSION
    req.model = _abi.MODELS["hmm"]
    req.pairing = _abi.PAIR_ZIP
    req.device = -1
    req.data.n_series, req.data.T_max, req.data.K = P, T, K
    req.data.x_real = keep["x"].data_ptr()
    req.draws.n_draws = P
    for name in ("p_1k", "A_ij", "mu_k", "sigma_k"):
        setattr(req.draws, name, keep[name].data_ptr())
    return req, keep, dev


def run_child(a):
    import torch
    import hhmm_amd
    from hhmm_amd import _abi
    gg = sys.modules["hhmm_amd.gibbs_gauss"]
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    P, T, K = a.pairs, a.T, a.K
    req, keep, dev = device_request(torch, P, T, K)
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
    sizes = {"loglik": P, "n_1k": P * K, "xi_ij": P * K * K, "w_k": P * K, "s1_k": P * K, "s2_k": P * K}
    sbuf = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
    for k, v in sbuf.items():
        setattr(sres, k, v.data_ptr())
    sstat = torch.zeros(P, dtype=torch.int32, device=dev)
    sres.pair_status = sstat.data_ptr()
    ws_a = C.c_size_t(0)
    assert lib.hhmm_draw_stats_gauss_workspace_size(C.byref(req), C.byref(ws_a)) == 0, lib.hhmm_last_error().decode()
    wa = torch.empty(max(ws_a.value, 256), dtype=torch.uint8, device=dev)

    def stats():
        rc = lib.hhmm_draw_stats_gauss_device(C.byref(req), C.byref(sres), wa.data_ptr(), wa.numel(), st)
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
    x = keep["x"]

    def reduce():
        z0 = z.to(torch.int64) - 1
        one = torch.ones((1, 1), dtype=torch.int32, device=dev)
        red["n_1k"] = torch.zeros((K, P), dtype=torch.int32, device=dev).scatter_add_(0, z0[:1], one.expand(1, P))
        red["xi_ij"] = torch.zeros((K * K, P), dtype=torch.int32, device=dev).scatter_add_(
            0, z0[:-1] + K * z0[1:], one.expand(T - 1, P))                  # i + K j
        red["w_k"] = torch.ones((K, P), dtype=torch.int32, device=dev).scatter_add_(0, z0[1:], one.expand(T - 1, P))
        red["s1_k"] = x[:1].expand(K, P).clone().scatter_add_(0, z0[1:], x[1:])
        red["s2_k"] = (x[:1] * x[:1]).expand(K, P).clone().scatter_add_(0, z0[1:], x[1:] * x[1:])

    # one Gibbs sweep: uniforms + (a) + the conjugate updates, parameters written back in place
    views = {"n_1k": sbuf["n_1k"].view(K, P).t(), "xi_ij": sbuf["xi_ij"].view(K, K, P).permute(2, 1, 0)}
    for k in ("w_k", "s1_k", "s2_k"):
        views[k] = sbuf[k].view(K, P).t()
    names = ("p_1k", "A_ij", "mu_k", "sigma_k")
    start = {k: keep[k].clone() for k in names}
    pt = gg._prior_tensors(torch, {"mu_sigma": (5.0 * (K + 1), 0.01, 2.0, 9.0)}, torch.float64, dev)

    def sweep():
        uniforms()
        stats()
        new = gg._conditional(torch, views, pt, gen)
        for k in names:
            keep[k].copy_(new[k].permute(*reversed(range(new[k].dim()))))

    t = {"stats": [], "path": [], "reduce": [], "sweep": []}
    same, sdiff = None, None
    for i in range(a.warmup + a.iters):
        row = {"stats": stamp(torch, stats), "path": stamp(torch, path), "reduce": stamp(torch, reduce)}
        if same is None:  # both paths computed the same counts from the same uniforms
            same = all(bool((red[k].reshape(-1) == sbuf[k].to(torch.int32)).all()) for k in ("n_1k", "xi_ij", "w_k"))
            sdiff = {k: float(((red[k].reshape(-1) - sbuf[k]).abs() / sbuf[k].abs().clamp_min(1.0)).max())
                     for k in ("s1_k", "s2_k")}
        red.clear()
        row["sweep"] = stamp(torch, sweep)
        for k in names:  # the timed paths always see the same parameters
            keep[k].copy_(start[k])
        uniforms()
        if i >= a.warmup:
            for k, v in row.items():
                t[k].append(v)
    stats()
    torch.cuda.synchronize()
    ll = sbuf["loglik"]
    out = {k: summary(v) for k, v in t.items()}
    out["path_plus_reduce"] = summary([p + r for p, r in zip(t["path"], t["reduce"])])
    out.update({"same_counts": same, "sums_max_rel_diff": sdiff,
                "workspace_GB": {"stats": round(ws_a.value / 1e9, 4), "path": round(ws_b.value / 1e9, 4)},
                "loglik_mean": float(ll.mean()), "loglik_finite": bool(torch.isfinite(ll).all()),
                "pair_failures": int((sstat != 0).sum()) + int((rstat != 0).sum()),
                "version": lib.hhmm_version().decode()})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--K", type=int, default=0, help="one K (default: 3 and 4)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds for one K (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_child(a)
        return 0
    out = {"shape": {"model": "hmm", "pairing": "zip", "pairs": a.pairs, "T": a.T}, "K": {}}
    rc = 0
    for K in ([a.K] if a.K else [3, 4]):
        C_ = 8 if K <= 4 else 4
        # bytes each path moves per (pair, step): x twice (forward, backward), u, the checkpoints out and back;
        # the parent's path also writes z, and its reduction reads z and x again (temporaries not counted)
        ck = 2 * 8.0 * K / C_
        row = {"bytes_per_step": {"stats": 8 + 8 + 8 + ck, "path": 8 + 8 + 8 + ck + 4, "reduce_at_least": 4 + 8},
               "lds_bytes_per_wave": {"stats": (K + K * K) * 256 + 2 * K * 512, "path": 0}}
        out["K"][str(K)] = row
        cmd = [sys.executable, __file__, "--child", f"--K={K}"] + [f"--{k}={getattr(a, k)}" for k in
                                                                    ("pairs", "T", "warmup", "iters")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            row["error"] = f"no result within {a.step_timeout} s"
            rc = 1
            break  # nothing more is started on the device after a step that did not end
        if r.returncode != 0:
            row["error"] = f"exit status {r.returncode}"
            row["stderr"] = r.stderr[-600:]
            rc = 1
            break
        row.update(json.loads(r.stdout.strip().split("\n")[-1]))
        row["stats_over_path_plus_reduce"] = round(row["stats"]["ms"] / row["path_plus_reduce"]["ms"], 4)
        row["stats_over_path"] = round(row["stats"]["ms"] / row["path"]["ms"], 4)
    print(json.dumps(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
