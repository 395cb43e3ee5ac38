#!/usr/bin/env python3
"""Times the expected draw statistics (hhmm_expected_stats_device, the masked
adjoint sweep) on hhmm-tayal2009 beside the unmasked E-step it is built on
(hhmm_estep_device on hmm-multinom) at the same shape: K = 4, L = 9, 131072
GRID pairs (128 series x 1024 draws) x T = 1000, the same symbols.  Under GRID
pairing a wave's 64 lanes share one series, so every step's sign is wave-uniform
and the kernel takes its sign-class arms; another row times the same number of
pairs under ZIP pairing with independent signs per lane (the masks per lane),
and one hmm-multinom-semisup with random groups (per-lane masks, no dispatch).
One device, device-resident inputs, events on torch's stream around --reps
launches, the paths interleaved in one process: every round times each of them
once.  Prints one JSON line.

    python tools/expect_bench.py
    python tools/expect_bench.py --series 16 --draws 256 --T 256      # a smaller shape

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
    N, S, T, K, L = a.series, a.draws, a.T, 4, a.L
    P = N * S
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(20260101)
    st = torch.cuda.current_stream().cuda_stream

    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device=dev, generator=g)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi, shape, dtype=torch.int32, device=dev, generator=g)

    keep = {
        "x": ints(1, L + 1, T, N), "sign": ints(1, 3, T, N), "g": ints(1, 4, T, N),   # [n + N t]
        "x_zip": ints(1, L + 1, T, P), "sign_zip": ints(1, 3, T, P),
        "p_1k": torch.softmax(rnd(K, S), 0), "A_ij": torch.softmax(rnd(K, K, S), 0),   # [j][i][s]
        "p_11": torch.sigmoid(rnd(S)), "A_row": torch.softmax(rnd(2, 2, S), 0),       # [c][r][s]
        "phi_k": torch.softmax(rnd(L, K, S), 0),                                      # [l][k][s]
    }
    for name in ("p_11", "A_row", "phi_k"):  # one draw per pair for the ZIP row
        keep[name + "_zip"] = keep[name].repeat_interleave(N, dim=-1)[..., torch.randperm(P, device=dev, generator=g)]

    def request(model, pairing, n_series, n_draws, data, draws):
        req = _abi.Request()
        req.abi_version = _abi.ABI_VERSION
        req.model = _abi.MODELS[model]
        req.pairing = pairing
        req.device = -1
        req.data.n_series, req.data.T_max, req.data.K, req.data.L = n_series, T, K, L
        req.draws.n_draws = n_draws
        req.data.x_int = keep[data["x"]].data_ptr()
        if "sign" in data:
            req.data.sign = keep[data["sign"]].data_ptr()
        if "g" in data:
            req.data.g, req.data.G = keep[data["g"]].data_ptr(), 3
        for field, name in draws.items():
            setattr(req.draws, field, keep[name].data_ptr())
        return req

    sizes = {"loglik": P, "n_1k": P * K, "xi_ij": P * K * K, "c_kl": P * K * L}

    def path(req, size_fn, run_fn):
        res = _abi.EstepResult()
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

    tayal = {"p_11": "p_11", "A_row": "A_row", "phi_k": "phi_k"}
    multinom = {"p_1k": "p_1k", "A_ij": "A_ij", "phi_k": "phi_k"}
    paths = {
        "estep_multinom": path(request("hmm-multinom", _abi.PAIR_GRID, N, S, {"x": "x"}, multinom),
                               lib.hhmm_estep_workspace_size, lib.hhmm_estep_device),
        "expected_semisup": path(request("hmm-multinom-semisup", _abi.PAIR_GRID, N, S, {"x": "x", "g": "g"}, multinom),
                                 lib.hhmm_expected_stats_workspace_size, lib.hhmm_expected_stats_device),
        "expected_tayal": path(request("hhmm-tayal2009", _abi.PAIR_GRID, N, S, {"x": "x", "sign": "sign"}, tayal),
                               lib.hhmm_expected_stats_workspace_size, lib.hhmm_expected_stats_device),
        "expected_tayal_zip": path(request("hhmm-tayal2009", _abi.PAIR_ZIP, P, P, {"x": "x_zip", "sign": "sign_zip"},
                                           {k: v + "_zip" for k, v in tayal.items()}),
                                   lib.hhmm_expected_stats_workspace_size, lib.hhmm_expected_stats_device),
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
    out["version"] = lib.hhmm_version().decode()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=128)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window")
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds for the measurement (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_child(a)
        return 0
    out = {"shape": {"pairs": a.series * a.draws, "series": a.series, "draws": a.draws, "T": a.T, "K": 4, "L": a.L,
                     "reps": a.reps}}
    # bytes per (pair, step): x twice (forward, backward), the checkpoints out and back; Tayal also sign twice
    ck = 2 * 8.0 * 4 / 8
    out["bytes_per_step"] = {"estep_multinom": 4 + 4 + ck, "expected_tayal": 8 + 8 + ck}
    cmd = [sys.executable, __file__, "--child"] + [f"--{k}={getattr(a, k)}" for k in
                                                   ("series", "draws", "T", "L", "warmup", "iters", "reps")]
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
    out["tayal_over_multinom"] = round(out["expected_tayal"]["ms"] / out["estep_multinom"]["ms"], 4)
    out["semisup_over_multinom"] = round(out["expected_semisup"]["ms"] / out["estep_multinom"]["ms"], 4)
    out["tayal_zip_over_multinom"] = round(out["expected_tayal_zip"]["ms"] / out["estep_multinom"]["ms"], 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
