#!/usr/bin/env python3
"""Times PSIS-LOO and PSIS-LFO (hhmm_psis_loo_device, hhmm_psis_lfo_device)
beside the pointwise sweep they are built on (hhmm_pointwise_device up to K = 8,
hhmm_pointwise_large_device above, with lp_t: the cost of WAIC before PSIS
existed), the three entries interleaved on one device-resident request, and
beside the route a caller had to the same numbers: lp_t downloaded to the host
and the numpy restatement (tests/psis_ref.py) run cell by cell.
hmm-multinom, L = 9, N = 4 series x D = 4096 draws (GRID pairing, P = 16384),
T = 1000, at K = 4 and K = 12 unless told otherwise.  Prints one JSON line
(--out: writes it to a file too).

    python tools/psis_bench.py
    python tools/psis_bench.py --K 4 --draws 512 --T 256      # a smaller shape
    python tools/psis_bench.py --out profiles/psis_bench.json

Each step (per K: "device", then "host") runs in a fresh child process under
its own time limit (--step-timeout); after a child that fails or runs out of
time nothing more is started.

The floor of the cell kernel: every member read once, N * T * D * 8 bytes for
LOO (r_d is -l_d) and twice that for LFO (the suffix sums too), at the HBM rate
a copy reaches (--hbm-tbs, 6.3 TB/s).  The cell kernel's own time is taken as
the entry's minus the sweep's.
"""
import argparse
import ctypes as C
import json
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "gsoc17-hhmm_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

STEPS = ("device", "host")
ENTRIES = ("pointwise", "psis_loo", "psis_lfo")


def entry(torch, lib, name, req, dev, N, P, T):
    """(launch, buffers) of hhmm_<name>_device with lp_t, on torch's stream."""
    from hhmm_amd import _abi
    st = torch.cuda.current_stream().cuda_stream
    psis = name.startswith("psis")
    res = _abi.PsisResult() if psis else _abi.PointwiseResult()
    sizes = {"loglik": P, "lpd_t": N * T, "mean_t": N * T, "var_t": N * T, "lp_t": P * T}
    if psis:
        sizes.update({"elpd_t": N * T, "khat_t": N * T, "neff_t": N * T})
    bufs = {k: torch.empty(n, dtype=torch.float64, device=dev) for k, n in sizes.items()}
    for k, v in bufs.items():
        setattr(res, k, v.data_ptr())
    bufs["status"] = torch.zeros(P, dtype=torch.int32, device=dev)
    res.pair_status = bufs["status"].data_ptr()
    ws = C.c_size_t(0)
    assert getattr(lib, f"hhmm_{name}_workspace_size")(C.byref(req), C.byref(ws)) == 0, lib.hhmm_last_error().decode()
    wbuf = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=dev)
    fn = getattr(lib, f"hhmm_{name}_device")

    def launch():
        rc = fn(C.byref(req), C.byref(res), wbuf.data_ptr(), wbuf.numel(), st)
        assert rc == 0, lib.hhmm_last_error().decode()
    bufs["_keep"] = (res, wbuf)
    bufs["_workspace"] = ws.value
    return launch, bufs


def run_step(step, a):
    import torch
    import hhmm_amd
    from hhmm_amd import pointwise
    from pointwise_bench import device_request
    lib = hhmm_amd.load_library()
    assert lib.hhmm_init(1) == 0, lib.hhmm_last_error().decode()
    N, D, T, K, L = a.series, a.draws, a.T, a.K, a.L
    P = N * D
    req, _keep, dev = device_request(torch, N, D, T, K, L)
    sweep = pointwise.entry_name(K)
    row = {"version": lib.hhmm_version().decode(), "sweep": "hhmm_" + sweep + "_device"}
    if step == "device":
        runs = {name: entry(torch, lib, sweep if name == "pointwise" else name, req, dev, N, P, T) for name in ENTRIES}
        times = {name: [] for name in ENTRIES}
        for i in range(a.warmup + a.iters):  # interleaved: one launch of each per round
            for name in ENTRIES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                runs[name][0]()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
        for name in ENTRIES:
            bufs = runs[name][1]
            row[name] = {"ms": round(float(np.median(times[name])), 4), "ms_min": round(min(times[name]), 4),
                         "ms_max": round(max(times[name]), 4), "iters": a.iters,
                         "workspace_GB": round(bufs["_workspace"] / 1e9, 4),
                         "pair_failures": int((bufs["status"] != 0).sum()),
                         "lpd_sum": float(bufs["lpd_t"].sum())}
            if name != "pointwise":
                kh = bufs["khat_t"]
                row[name].update({"elpd_sum": float(bufs["elpd_t"].sum()), "khat_finite": bool(torch.isfinite(kh).all()),
                                  "khat_max": float(kh.max()), "steps_above_0.7": int((kh > 0.7).sum())})
        same = all(torch.equal(runs["pointwise"][1][k], runs[n][1][k]) for n in ENTRIES[1:]
                   for k in ("loglik", "lpd_t", "mean_t", "var_t", "lp_t"))
        row["embedded_arrays_equal"] = bool(same)
    else:
        import psis_ref
        launch, bufs = entry(torch, lib, "psis_loo", req, dev, N, P, T)
        launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp = bufs["lp_t"].cpu().numpy().reshape((P, T), order="F")   # the download a caller pays today
        t1 = time.perf_counter()
        cells = [(n, int(t)) for n in range(N) for t in np.linspace(0, T - 1, a.host_cells // N).astype(int)]
        got = {k: bufs[k].cpu().numpy().reshape((N, T), order="F") for k in ("elpd_t", "khat_t", "neff_t")}
        worst = 0.0
        t2 = time.perf_counter()
        for n, t in cells:
            rows = slice(n * D, (n + 1) * D)
            want = psis_ref.cell(-lp[rows, t], lp[rows, t])
            for k, v in zip(("elpd_t", "khat_t", "neff_t"), want):
                worst = max(worst, abs(got[k][n, t] - v) / max(1.0, abs(v)))
        t3 = time.perf_counter()
        row.update({"download_ms": round(1e3 * (t1 - t0), 3), "download_GB": round(lp.nbytes / 1e9, 4),
                    "cells_timed": len(cells), "ref_ms_per_cell": round(1e3 * (t3 - t2) / len(cells), 4),
                    "ref_ms_all_cells": round(1e3 * (t3 - t2) / len(cells) * N * T, 1),
                    "worst_discrepancy": worst})
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4)
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--K", type=int, nargs="+", default=[4, 12])
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--host-cells", type=int, default=64, help="cells the host reference is timed on")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the HBM rate of the read floor, TB/s")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per step (child process)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        a.K = a.K[0]
        run_step(a.step, a)
        return 0
    out = {"shape": {"model": "hmm-multinom", "pairing": "grid", "series": a.series, "draws": a.draws,
                     "pairs": a.series * a.draws, "T": a.T, "L": a.L}}
    floor_ms = 8.0 * a.series * a.T * a.draws / (a.hbm_tbs * 1e12) * 1e3
    out["cell_read_floor_ms"] = {"loo": round(floor_ms, 4), "lfo": round(2 * floor_ms, 4), "hbm_TBs": a.hbm_tbs}
    rc = 0
    for K in a.K:
        rows = out[f"K{K}"] = {}
        for step in STEPS:
            cmd = [sys.executable, __file__, "--step", step, f"--K={K}"] + [
                f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("series", "draws", "T", "L", "warmup", "iters",
                                                                     "host_cells")]
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
        d = rows["device"]
        for kind in ("loo", "lfo"):
            cell_ms = d["psis_" + kind]["ms"] - d["pointwise"]["ms"]
            rows[f"psis_{kind}_over_pointwise"] = round(d["psis_" + kind]["ms"] / d["pointwise"]["ms"], 4)
            rows[f"{kind}_cells_ms"] = round(cell_ms, 4)
            rows[f"{kind}_cells_over_read_floor"] = round(cell_ms / out["cell_read_floor_ms"][kind], 2)
        rows["host_route_over_psis_loo"] = round(
            (rows["host"]["download_ms"] + rows["host"]["ref_ms_all_cells"]) / d["psis_loo"]["ms"], 1)
    print(json.dumps(out))
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
