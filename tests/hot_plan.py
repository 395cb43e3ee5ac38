"""Plan-pinned runs: a GPU test that names a schedule asserts the launch plan
of its own request before it compares anything.

scan_plan takes the parallel scan over T for any batch of under 16384 pairs
with T_max >= 256 unless HHMM_FLAG_SCAN_OFF is set, and a batch of under
131072 pairs at K <= 4 decodes state-parallel unless HHMM_FLAG_VIT_LANES is
set; HHMM_FLAG_VFB / FUSED / FB_SPLIT override neither.  A test that sets one
of those flags at a small shape therefore runs the kernels it names only if
the plan says so.  hhmm_selftest_plan prints that plan and touches no device,
so the same case tables are walked by a CPU test (tests/test_hot_plan.py).
"""
import ctypes as C
import pathlib
import sys

import numpy as np

from hhmm_amd import _abi
from tolerances import PROB, RTOL, compare_all

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
from gen_plan_fixture import request  # noqa: E402

C2 = ["loglik", "gamma_tk", "zstar_t", "logp_zstar"]
# the lane-per-pair sequential sweeps at a small shape: no T-scan, no V-scan, no state-parallel decoder
LANES = _abi.FLAG_VIT_LANES | _abi.FLAG_SCAN_OFF | _abi.FLAG_VIT_SCAN_OFF
PACKED = "ckpt,ckpt_ls,xpk,rnw"
# the four schedules of the C2 request at hmm-multinom K = 4: (id, flags, the plan words they must give)
SCHEDULES = [
    ("phased", LANES | _abi.FLAG_VFB,
     dict(schedule="phased", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="sweep", scan_cl="0", vs_nc="0")),
    ("fused", LANES | _abi.FLAG_FUSED,
     dict(schedule="fused", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="sweep", scan_cl="0", vs_nc="0")),
    ("split", LANES | _abi.FLAG_FB_SPLIT,
     dict(schedule="split", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="packed", scan_cl="0", vs_nc="0")),
    ("two-kernels", LANES | _abi.FLAG_VFB_OFF,
     dict(schedule="separate", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="lanes", scan_cl="0", vs_nc="0")),
]
SCHEDULE_FLAGS = {s[0]: s[1] for s in SCHEDULES}
SCHEDULE_PLAN = {s[0]: s[2] for s in SCHEDULES}


def outputs_of(pars):
    out = 0
    for name in pars:
        out |= _abi.OUT[name]
    return out


def plan_of(engine, model, K, L, P, Tmax, pars, flags, T_oos=0):
    """The key=value words hhmm_selftest_plan prints for a request of this shape (no device, no arrays)."""
    buf = C.create_string_buffer(512)
    r = request(_abi.MODELS[model], int(K), int(L), int(P), int(Tmax), int(T_oos), outputs_of(pars), int(flags))
    assert engine.hhmm_selftest_plan(C.byref(r), buf, len(buf)) == _abi.OK, engine.hhmm_last_error()
    return dict(w.split("=", 1) for w in buf.value.decode().split())


def shape_of(model, data, draws, pairing):
    """(K, L, P, T_max, T_oos_max) as hhmm_amd.api.PreparedRequest reads them."""
    x = np.asarray(data["x_t" if model.startswith("iohmm") else "x"])
    N = 1 if x.ndim == 1 else x.shape[0]
    S = np.asarray(next(iter(draws.values()))).shape[0]
    P = N * S if pairing == "grid" else (S if pairing == "block" else N)
    T_oos = np.asarray(data["x_oos"]).shape[-1] if "x_oos" in data else 0
    return int(data["K"]), int(data.get("L", 0)), P, x.shape[-1], T_oos


def assert_plan(engine, model, data, draws, pars, flags, pairing, want_plan):
    """The plan of the request hhmm_amd.gqs would build from these arguments holds every word of want_plan."""
    K, L, P, Tmax, T_oos = shape_of(model, data, draws, pairing)
    got = plan_of(engine, model, K, L, P, Tmax, pars, flags, T_oos)
    assert {k: got[k] for k in want_plan} == dict(want_plan), (model, K, L, P, Tmax, hex(int(flags)), got)
    return got


def worst(got, ref, names):
    """Largest discrepancy of the float outputs on the scale tolerances.compare bounds by 1e-9: |a - b| over
    |b| + 1e-241 for the probabilities, over max(|b|, 1) for the log-scale outputs.  Printed for the record;
    the assertion is compare_all's."""
    w = 0.0
    for k in names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.dtype.kind != "f":
            continue
        m = np.isfinite(a) & np.isfinite(b)
        if m.any():
            scale = np.abs(b[m]) + 1e-250 / RTOL if k in PROB else np.maximum(np.abs(b[m]), 1.0)
            w = max(w, float(np.max(np.abs(a[m] - b[m]) / scale)))
    return w


def run_planned(engine, oracle, model, data, draws, pars, flags, pairing, want_plan, uniforms=None, nthreads=8,
                tag=None, ref=None):
    """Asserts want_plan, then runs the library and the oracle and compares pars + pair_status.  `ref`: the
    oracle's outputs of these very inputs where a test computed them once for several schedules."""
    import hhmm_amd
    if want_plan is not None:
        assert_plan(engine, model, data, draws, pars, flags, pairing, want_plan)
    got = hhmm_amd.gqs(model, data, draws, pars=pars, pairing=pairing, lib=engine, return_status=True, flags=flags,
                       uniforms=uniforms)
    if ref is None:
        ref = oracle.gqs(model, data, draws, pars=pars, pairing=pairing, return_status=True, nthreads=nthreads,
                         uniforms=uniforms)
    print(f"worst discrepancy {worst(got, ref, pars):.3e}" + (f" [{tag}]" if tag else ""))
    compare_all(got, ref, list(pars) + ["pair_status"])
    return got, ref
