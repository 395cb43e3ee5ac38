#!/usr/bin/env python3
"""Writes tests/golden/plan_workspace.json: hhmm_workspace_size of the library
named by HHMM_LIB over a grid of HMM-family requests (no device needed).

  HHMM_LIB=gsoc17-hhmm_amd/lib/variants/libhhmm_base.so python tools/gen_plan_fixture.py

tests/test_plan.py replays the rows against the library under test, so a
change to how a request is planned or sized shows as a byte count that moved.
Run it against the library of the commit whose sizes are the reference (the
parent of a refactor), not against the tree being changed.

The grid: the five HMM-family models; K = 1, 2, 4, 5, 8 and 12 (the large-K
branch; Tayal is K = 4); L = 9, 16, 17; (pairs, T_max) on both sides of every
threshold of scan_plan, vscan_chunks and the state-parallel Viterbi; eight
output sets; the scheduling flags.  The full product is tens of thousands of
rows, so three slices of it are kept: every (model, K, shape, outputs) at
L = 9 without flags; L = 16 and 17 for hmm-multinom, the one model whose
workspace depends on L; every flag at one K per model (hmm-multinom also at
K = 2 and 12) for three output sets.  Combinations a model does not declare
are dropped.  ZIP pairing, n_series = n_draws = pairs; T_oos_max = T_max for
tayal-lite, whose Viterbi runs over the out-of-sample series.
"""
import ctypes as C
import json
import os
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "gsoc17-hhmm_amd"))
from hhmm_amd import _abi  # noqa: E402

O = _abi.OUT
FB = sum(O[k] for k in ("loglik", "unalpha_tk", "alpha_tk", "unbeta_tk", "beta_tk", "ungamma_tk", "gamma_tk",
                        "zstar_t", "logp_zstar"))
AVAILABLE = {
    "hmm": FB | O["z_ffbs"], "hmm-multinom": FB | O["z_ffbs"], "hmm-multinom-semisup": FB | O["z_ffbs"],
    "hhmm-tayal2009": FB | O["z_ffbs"],
    "hhmm-tayal2009-lite": sum(O[k] for k in ("loglik", "unalpha_tk", "alpha_tk", "unalpha_tk_oos", "alpha_tk_oos",
                                              "zstar_t", "logp_zstar")),
}
KS = {m: ([4] if "tayal" in m else [1, 2, 4, 5, 8, 12]) for m in AVAILABLE}
SHAPES = [(64, 100), (1000, 500), (250, 65536), (2048, 16384), (16383, 256), (16384, 256), (131071, 16),
          (131072, 16), (131072, 20000)]
OUTPUTS = [O["loglik"], O["loglik"] | O["gamma_tk"], O["gamma_tk"] | O["zstar_t"] | O["logp_zstar"], O["zstar_t"],
           O["gamma_tk"] | O["alpha_tk"], O["unalpha_tk"] | O["gamma_tk"], O["gamma_tk"] | O["z_ffbs"], None]
FLAGS = [_abi.FLAG_VFB_OFF, _abi.FLAG_FUSED, _abi.FLAG_FB_SPLIT, _abi.FLAG_NO_FUSE, _abi.FLAG_SCAN_FORCE,
         _abi.FLAG_SCAN_OFF, _abi.FLAG_VIT_SCAN, _abi.FLAG_VIT_SCAN_OFF, _abi.FLAG_VIT_LANES, _abi.FLAG_VIT_STATES,
         _abi.flag_scan_chunk_log2(7)]
FLAG_MODELS = [("hmm", 4), ("hmm-multinom", 2), ("hmm-multinom", 4), ("hmm-multinom", 12),
               ("hmm-multinom-semisup", 4), ("hhmm-tayal2009", 4), ("hhmm-tayal2009-lite", 4)]
COLUMNS = ["model", "K", "L", "pairs", "T_max", "T_oos_max", "outputs", "flags", "bytes"]


def request(model, K, L, pairs, T, T_oos, outputs, flags):
    """A request that describes its shape and nothing else (no arrays: sizing and planning read none)."""
    r = _abi.Request()
    r.abi_version = _abi.ABI_VERSION
    r.model = model
    r.pairing = _abi.PAIR_ZIP
    r.outputs = outputs
    r.flags = flags
    r.data.n_series = r.draws.n_draws = pairs
    r.data.K, r.data.L, r.data.T_max, r.data.T_oos_max = K, L, T, T_oos
    return r


def grid():
    """[model id, K, L, pairs, T_max, T_oos_max, outputs, flags] of every row."""
    seen, rows = set(), []

    def add(name, K, L, shape, out, flags):
        out = AVAILABLE[name] if out is None else out
        if out & ~AVAILABLE[name]:
            return
        row = (_abi.MODELS[name], K, L, shape[0], shape[1], shape[1] if name.endswith("-lite") else 0, out, flags)
        if row not in seen:
            seen.add(row)
            rows.append(list(row))

    for name in AVAILABLE:
        for K in KS[name]:
            for shape in SHAPES:
                for out in OUTPUTS:
                    add(name, K, 9, shape, out, 0)
                    if name == "hmm-multinom":
                        add(name, K, 16, shape, out, 0)
                        add(name, K, 17, shape, out, 0)
    for name, K in FLAG_MODELS:
        for shape in SHAPES:
            for out in OUTPUTS[1:4]:
                for flags in FLAGS:
                    add(name, K, 9, shape, out, flags)
    return rows


def main():
    lib = _abi.declare(C.CDLL(os.environ["HHMM_LIB"]))
    rows = grid()
    for row in rows:
        n = C.c_size_t(0)
        assert lib.hhmm_workspace_size(C.byref(request(*row)), C.byref(n)) == _abi.OK, row
        row.append(n.value)
    out = REPO / "tests" / "golden" / "plan_workspace.json"
    body = ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)
    out.write_text('{"library": %s,\n"columns": %s,\n"rows": [\n%s\n]}\n'
                   % (json.dumps(lib.hhmm_version().decode()), json.dumps(COLUMNS), body))
    print(len(rows), "rows ->", out)


if __name__ == "__main__":
    main()
