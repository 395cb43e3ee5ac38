"""CPU: the plan of every case of tests/test_gpu_hot_sweeps.py and
tests/test_gpu_renorm_gate.py, and of the repaired schedule-named GPU tests.

hhmm_selftest_plan touches no device, so the tables those GPU modules run
are verified here first: each case's request (its own shape, outputs and
flags) gives the plan words the case pins.  A case whose flags no longer
reach the sweep it names fails here, without a GPU."""
import pytest

import test_gpu_hot_sweeps as hot
import test_gpu_renorm_gate as gate
from hhmm_amd import _abi
from hot_plan import C2, LANES, SCHEDULE_FLAGS, SCHEDULE_PLAN, assert_plan, plan_of, shape_of


@pytest.mark.parametrize("case", hot.CASES, ids=[c.id for c in hot.CASES])
def test_hot_sweep_case_plan(engine, case):
    data, draws, _ = hot.inputs(case.key)
    assert hot.symbol_L_occurs(case)
    got = assert_plan(engine, hot.MODEL, data, draws, case.pars, case.flags, case.pairing, case.plan)
    assert got["fb"] == "linear" and got["scan_cl"] == "0" and got["vs_nc"] == "0"
    assert ("xpk" in got["regions"]) == (case.key[2] <= 16)


def test_hot_sweep_table_covers_the_issue():
    ids = {c.id for c in hot.CASES}
    for sid in SCHEDULE_PLAN:
        assert {f"edge-T{T}-{sid}" for T in hot.EDGES} <= ids
        assert {f"ragged-{sid}", f"grid-{sid}", f"block-{sid}", f"P1-{sid}", f"P257-{sid}"} <= ids
        assert {f"L{L}-{sid}" for L in (1, 2, 15, 16, 17)} <= ids
    assert {f"K{K}-L{L}-{o}" for K in (1, 2, 3, 5, 6, 7, 8) for L in (2, 9, 16) for o in ("gamma", "c2")} <= ids
    assert {f"ffbs-K{K}-L{L}" for K in (4, 6) for L in (9, 16)} <= ids
    assert len(ids) == len(hot.CASES)
    # the ragged batch: the three waves the table promises
    T = hot.inputs(("ragged", 4, 9))[0]["T"]
    assert T[:64].min() == 3 and set(T[:64]) == {t for t in hot.EDGES if t <= 257}
    assert sorted(T[64:128])[-2:] == [64, 65] and (T[64:128] == 64).sum() == 63
    assert set(T[128:]) == {1, 16, 17} and (T[128:] == 1).sum() == 1
    # every shape stays small
    for c in hot.CASES:
        x = hot.inputs(c.key)[0]["x"]
        assert x.shape[1] <= 300 and x.shape[0] <= 257


@pytest.mark.parametrize("case", gate.CASES, ids=[c.id for c in gate.CASES])
def test_gate_case_plan(engine, case):
    data, draws = gate.inputs(case)
    got = assert_plan(engine, gate.MODEL, data, draws, case.pars, case.flags, case.pairing, case.plan)
    assert (got["schedule"] == "none") == (case.K > 8)


def test_gate_table_covers_every_kernel_family():
    ids = {c.id for c in gate.CASES}
    assert len(ids) == len(gate.CASES)
    for b in gate.gate_inputs.BUILDERS:
        for side in gate.gate_inputs.SIDES:
            want = set(SCHEDULE_PLAN) | {f"fb-big-K{K}" for K in (2, 3, 4)} | {f"tscan-K{K}" for K in (2, 4, 8)}
            want |= {f"large-K{K}-{o}" for K in (12, 23) for o in ("gamma", "full", "scan")}
            assert {f"{b}-{side}-{w}" for w in want} <= ids
        assert sum(c.pairing == "grid" and c.builder == b for c in gate.CASES) == 5


# ---- the shapes of the schedule-named GPU tests elsewhere in the suite: what they pin is what the plan gives ----

REPAIRED = [
    # tests/test_gpu_configs.py::test_c2_slice: 4096 pairs x T = 1000
    ("c2-slice-auto", dict(P=4096, T=1000, flags=0), dict(schedule="separate", fb="scan", vit="states")),
    # `lane` is fb_kernel beside viterbi_kernel: with the phased sweep the default (HHMM_VFB_DEFAULT) it needs VFB_OFF
    ("c2-slice-lane", dict(P=4096, T=1000, flags=SCHEDULE_FLAGS["two-kernels"]), SCHEDULE_PLAN["two-kernels"]),
    ("c2-slice-lanes-alone", dict(P=4096, T=1000, flags=LANES), SCHEDULE_PLAN["phased"]),
    ("c2-slice-lane-fused", dict(P=4096, T=1000, flags=SCHEDULE_FLAGS["fused"]), SCHEDULE_PLAN["fused"]),
    ("c2-slice-lane-split", dict(P=4096, T=1000, flags=SCHEDULE_FLAGS["split"]), SCHEDULE_PLAN["split"]),
    ("c2-slice-lane-vfb", dict(P=4096, T=1000, flags=SCHEDULE_FLAGS["phased"]), SCHEDULE_PLAN["phased"]),
    # tests/test_gpu_parity.py::test_split_schedule_ragged: 130 pairs, T_max = 300
    ("split-ragged-split", dict(P=130, T=300, flags=SCHEDULE_FLAGS["split"]), SCHEDULE_PLAN["split"]),
    ("split-ragged-vfb", dict(P=130, T=300, flags=SCHEDULE_FLAGS["phased"]), SCHEDULE_PLAN["phased"]),
    # what those two tests ran before they set SCAN_OFF: the T-scan, whatever the schedule flag
    ("before-c2-slice-lane-fused", dict(P=4096, T=1000, flags=_abi.FLAG_VIT_LANES | _abi.FLAG_FUSED),
     dict(schedule="separate", fb="scan", fb_mode="GAMMA", vit="lanes", scan_cl="32", scan_nc="32")),
    ("before-split-ragged-vfb", dict(P=130, T=300, flags=_abi.FLAG_VIT_LANES | _abi.FLAG_VFB),
     dict(schedule="separate", fb="scan", vit="lanes")),
]


def _existing_rows():
    """(id, model, K, L, P, T_max, T_oos, outputs, flags, plan) of the plan columns the other GPU modules carry."""
    import test_gpu_golden as golden
    import test_gpu_host_edges as edges
    import test_gpu_invalid_data as invalid
    import test_gpu_nan_draws as nan
    from test_golden import load
    rows = []
    for pid, (model, kw), flags, plan in nan.PATHS:
        kw = dict(kw)
        L = {"hmm": 0, "iohmm-reg": 0}.get(model, 9)
        rows.append((f"nan-{pid}", model, kw["K"], L, nan.N * nan.S, kw.get("T", nan.T), 0, nan.PARS, flags, plan))
    for sid, flags, plan in edges.WAVE_SCHEDULES:
        rows += [(f"wave-{sid}-P{P}", "hmm-multinom", 4, 9, P, 64, 0, edges.C2_PARS, flags, plan) for P in (63, 64, 65)]
    rows += [(f"invalid-c2-{sid}", "hmm-multinom", 4, 9, 512, 200, 0, invalid.C2_PARS, flags, plan)
             for sid, flags, plan in invalid.C2_ROWS]
    rows += [(f"invalid-ragged-{sid}", "hmm-multinom", 4, 9, 300, 203, 0, outs, flags, plan)
             for sid, outs, flags, plan in invalid.SCHEDULES]
    rows += [(f"invalid-extreme-{sid}", "hmm-multinom", 4, 9, 130, 70, 0, outs, flags, plan)
             for sid, outs, flags, plan in invalid.EXTREME_SCHEDULES]
    for model, schedule in golden._cases():
        if model not in golden.HMM_FAMILY:
            continue
        data, draws, outs = load(model)
        pars = [k for k in outs if k != "pair_status"]
        if schedule.startswith("scan"):
            pars = [k for k in pars if k not in ("unalpha_tk", "unbeta_tk", "unalpha_tk_oos")]
        if schedule == "phased-c2":
            pars = golden.C2
        K, L, P, T, To = shape_of(model, data, draws, "grid")
        rows.append((f"golden-{model}-{schedule}", model, K, L, P, T, To, pars, golden.SCHEDULES[schedule],
                     golden.want_plan(model, schedule, K)))
    return rows


@pytest.mark.parametrize("row", _existing_rows(), ids=[r[0] for r in _existing_rows()])
def test_plan_columns_of_the_other_gpu_modules(engine, row):
    _, model, K, L, P, T, To, pars, flags, want = row
    got = plan_of(engine, model, K, L, P, T, pars, flags, To)
    assert {k: got[k] for k in want} == dict(want), got


def test_the_phased_sweep_is_named_only_where_it_runs():
    """Every row of the tables above whose id says phased or vfb-with-the-hot-outputs pins schedule=phased."""
    for r in _existing_rows():
        if "phased" in r[0]:
            assert r[9]["schedule"] == "phased", r[0]
        if r[9].get("schedule") in ("phased", "fused", "split"):
            assert r[1] == "hmm-multinom" and r[2] == 4 and r[8] & _abi.FLAG_VIT_LANES, r[0]


@pytest.mark.parametrize("shape,want", [r[1:] for r in REPAIRED], ids=[r[0] for r in REPAIRED])
def test_repaired_tests_reach_their_schedules(engine, shape, want):
    got = plan_of(engine, "hmm-multinom", 4, 9, shape["P"], shape["T"], C2, shape["flags"])
    assert {k: got[k] for k in want} == dict(want), got
