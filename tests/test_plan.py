"""CPU: the launch plan of an HMM-family request (csrc/hhmm_plan.h), which both
workspace sizing (ws_layout) and dispatch (run_model_k) read.

* tests/golden/plan_workspace.json holds hhmm_workspace_size of the commit
  before the plan existed over a grid of requests (tools/gen_plan_fixture.py):
  the library under test must return the same bytes for every row.
* hhmm_selftest_plan prints the plan as key=value words; the pins below state,
  for one request per schedule and per forward-backward mode, what the launch
  conditions give, each with the condition it comes from.
* For every request of the grid the regions the plan names are the regions
  the workspace binding gives a pointer.
No GPU is needed: neither entry touches a device."""
import ctypes as C
import json
import pathlib
import sys

import pytest

from hhmm_amd import _abi

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
from gen_plan_fixture import request  # noqa: E402

FIXTURE = json.loads((REPO / "tests" / "golden" / "plan_workspace.json").read_text())
O = _abi.OUT
C2 = O["loglik"] | O["gamma_tk"] | O["zstar_t"] | O["logp_zstar"]
LG = O["loglik"] | O["gamma_tk"]


def plan(engine, model, outputs, flags=0, K=4, L=9, pairs=131072, T=1000, T_oos=0):
    buf = C.create_string_buffer(512)
    r = request(_abi.MODELS[model], K, L, pairs, T, T_oos, outputs, flags)
    assert engine.hhmm_selftest_plan(C.byref(r), buf, len(buf)) == _abi.OK, engine.hhmm_last_error()
    return dict(w.split("=", 1) for w in buf.value.decode().split())


def test_fixture_covers_the_grid():
    rows = FIXTURE["rows"]
    assert FIXTURE["columns"] == ["model", "K", "L", "pairs", "T_max", "T_oos_max", "outputs", "flags", "bytes"]
    assert 2000 <= len(rows) <= 6000
    assert {r[0] for r in rows} == {_abi.MODELS[m] for m in ("hmm", "hmm-multinom", "hmm-multinom-semisup",
                                                            "hhmm-tayal2009", "hhmm-tayal2009-lite")}
    assert {r[1] for r in rows} == {1, 2, 4, 5, 8, 12} and {r[2] for r in rows} == {9, 16, 17}
    assert len({(r[3], r[4]) for r in rows}) == 9 and len({r[7] for r in rows}) == 12


def test_workspace_bytes_match_the_fixture(engine):
    """Sizing is unchanged: every row's bytes are what the library before the plan returned."""
    moved = []
    for row in FIXTURE["rows"]:
        n = C.c_size_t(0)
        assert engine.hhmm_workspace_size(C.byref(request(*row[:8])), C.byref(n)) == _abi.OK
        if n.value != row[8]:
            moved.append((row, n.value))
    assert not moved, (len(moved), moved[:5])


def test_planned_regions_are_the_bound_regions(engine):
    """What the plan says its kernels touch is what bind_workspace binds, on every row of the grid."""
    buf = C.create_string_buffer(512)
    for row in FIXTURE["rows"]:
        assert engine.hhmm_selftest_plan(C.byref(request(*row[:8])), buf, len(buf)) == _abi.OK
        words = dict(w.split("=", 1) for w in buf.value.decode().split())
        if row[1] > 8:
            assert words["schedule"] == "none", row    # the large-K branch plans for itself (hhmm_large.h)
        else:
            assert words["schedule"] != "none" and words["regions"] == words["bound"], (row, words)


PACKED = "ckpt,ckpt_ls,xpk,rnw"
# (id, request, the words pinned).  hmm-multinom at K = 4, L = 9, 131072 pairs x T = 1000 unless the row says
# otherwise: no T-scan (P >= 131072), no V-scan (P >= 2048), lane-per-pair Viterbi (P >= 131072: use_vit_states).
PINS = [
    # gamma + zstar off the extra outputs, packed symbols, fbv_ok, no flags: HHMM_VFB_DEFAULT picks the phased
    # sweep, whose phase 1 checks x
    ("c2-default", dict(model="hmm-multinom", outputs=C2),
     dict(schedule="phased", fb_mode="GAMMA|PACK|BIG", vit="sweep", regions=PACKED + ",bp", checked_inline="1",
          side_stream="0", scan_cl="0", vs_nc="0")),
    # VFB_OFF: vfb_on is false and neither FUSED nor FB_SPLIT is set: two kernels, the decoder on the side stream
    # (vit && any_fwd && !NO_FUSE); fb_big_ok -> FB_BIG; both read x themselves and check it
    ("vfb-off", dict(model="hmm-multinom", outputs=C2, flags=_abi.FLAG_VFB_OFF),
     dict(schedule="separate", fb="linear", fb_mode="GAMMA|PACK|BIG", vit="lanes", side_stream="1",
          regions=PACKED + ",bp", checked_inline="1")),
    # FUSED is tested first; fbv_kernel has no inline check
    ("fused", dict(model="hmm-multinom", outputs=C2, flags=_abi.FLAG_FUSED),
     dict(schedule="fused", fb_mode="GAMMA|PACK|BIG", vit="sweep", side_stream="0", checked_inline="0")),
    # FB_SPLIT turns the default phased sweep off; the forward launch checks x, the decoder reads the packed record
    ("fb-split", dict(model="hmm-multinom", outputs=C2, flags=_abi.FLAG_FB_SPLIT),
     dict(schedule="split", fb_mode="GAMMA|PACK|BIG", vit="packed", side_stream="1", checked_inline="1")),
    # NO_FUSE turns the phased sweep off and keeps the decoder on the caller's stream
    ("no-fuse", dict(model="hmm-multinom", outputs=C2, flags=_abi.FLAG_NO_FUSE),
     dict(schedule="separate", fb_mode="GAMMA|PACK|BIG", vit="lanes", side_stream="0", checked_inline="1")),
    # L = 17 > 16: a symbol does not fit 4 bits: no xpk / rnw, so none of the shared sweeps and plain FB_GAMMA
    ("l17-no-pack", dict(model="hmm-multinom", outputs=C2, L=17),
     dict(schedule="separate", fb_mode="GAMMA", vit="lanes", side_stream="1", regions="ckpt,ckpt_ls,bp")),
    # FFBS on the packed profile: FB_GAMMA | FB_FFBS | FB_PACK (tested before FB_BIG)
    ("gamma-ffbs-multinom", dict(model="hmm-multinom", outputs=O["gamma_tk"] | O["z_ffbs"]),
     dict(schedule="separate", fb="linear", fb_mode="GAMMA|FFBS|PACK", vit="none", regions=PACKED,
          checked_inline="1", side_stream="0")),
    # alpha is an extra output: FB_FULL, and no packed symbols
    ("gamma-alpha", dict(model="hmm-multinom", outputs=O["gamma_tk"] | O["alpha_tk"]),
     dict(fb="linear", fb_mode="FULL", regions="ckpt,ckpt_ls", checked_inline="1")),
    ("gamma-alpha-ffbs", dict(model="hmm-multinom", outputs=O["gamma_tk"] | O["alpha_tk"] | O["z_ffbs"]),
     dict(fb="linear", fb_mode="FULL|FFBS", regions="ckpt,ckpt_ls")),
    # a log-scale output: the log-space recursion over both sweeps (FFBS needs the backward one), and the FFBS
    # draws from a second, linear launch, which is the one that checks x
    ("unalpha-ffbs", dict(model="hmm-multinom", outputs=O["unalpha_tk"] | O["z_ffbs"]),
     dict(fb="log", fb_mode="BOTH+FFBS", regions="ckpt,ckpt_ls", checked_inline="1")),
    # fb_log_kernel alone checks nothing inline; no backward output: forward only
    ("unalpha-only", dict(model="hmm-multinom", outputs=O["unalpha_tk"]),
     dict(fb="log", fb_mode="FWD", regions="-", checked_inline="0")),
    # no backward output: FB_FWD and no checkpoints
    ("loglik-only", dict(model="hmm-multinom", outputs=O["loglik"]),
     dict(schedule="separate", fb="linear", fb_mode="FWD", vit="none", regions="-", checked_inline="1")),
    # semisup and Tayal read g / sign beside x: no packed profile, no inline check
    ("semisup-gamma", dict(model="hmm-multinom-semisup", outputs=LG),
     dict(schedule="separate", fb_mode="GAMMA", regions="ckpt,ckpt_ls", checked_inline="0")),
    ("semisup-gamma-ffbs", dict(model="hmm-multinom-semisup", outputs=LG | O["z_ffbs"]),
     dict(fb_mode="GAMMA|FFBS", regions="ckpt,ckpt_ls", checked_inline="0")),
    ("tayal-gamma", dict(model="hhmm-tayal2009", outputs=LG),
     dict(schedule="separate", fb_mode="GAMMA", regions="ckpt,ckpt_ls", checked_inline="0")),
    # tayal-lite: in-sample forward (alpha_tk: linear), OOS forward (unalpha_tk_oos: log space), OOS Viterbi
    ("tayal-lite-oos", dict(model="hhmm-tayal2009-lite", T_oos=300,
                            outputs=O["loglik"] | O["alpha_tk"] | O["unalpha_tk_oos"] | O["zstar_t"]),
     dict(schedule="lite", fb="linear", fb_mode="FWD", oos_fb="log", vit="lanes", regions="bp", checked_inline="0",
          side_stream="0")),
    # C5's shape class, 250 pairs x long T: P < 16384 and T >= 256 -> T-scan from 4 C = 32-step chunks
    # (250 * 2048 <= 524288 lanes); P < 2048 and T >= 16384 -> V-scan in 512-step chunks
    ("c5-shape", dict(model="hmm-multinom", outputs=C2, pairs=250, T=65536),
     dict(schedule="separate", fb="scan", fb_mode="GAMMA", vit="vscan", scan_cl="32", scan_nc="2048", vs_nc="128",
          regions="ckpt,ckpt_ls,bp,scan,vscan", checked_inline="0", side_stream="1")),
    # C1's shape: small-batch T-scan; T < 16384: no V-scan; P < 131072 at K = 4: the state-parallel decoder
    ("c1-shape", dict(model="hmm-multinom", outputs=C2, pairs=1000, T=500),
     dict(schedule="separate", fb="scan", fb_mode="GAMMA", vit="states", scan_cl="32", scan_nc="16", vs_nc="0",
          regions="ckpt,ckpt_ls,bp,scan", checked_inline="0", side_stream="1")),
    # one pair fewer than 131072 takes the C2 request off the phased sweep (use_vit_states)
    ("below-lane-threshold", dict(model="hmm-multinom", outputs=C2, pairs=131071, T=16),
     dict(schedule="separate", fb_mode="GAMMA|PACK|BIG", vit="states", side_stream="1", checked_inline="1")),
    # the path alone at 131072 pairs: viterbi_kernel on the caller's stream (no forward-backward to run beside)
    ("lanes-zstar-only", dict(model="hmm-multinom", outputs=O["zstar_t"], T=16),
     dict(schedule="separate", fb="none", fb_mode="-", vit="lanes", regions="bp", side_stream="0",
          checked_inline="1")),
    # K = 5: fb_chunk = 4, so neither fb_big_ok nor fbv_ok: packed without FB_BIG, two kernels; K > 4: lanes
    ("k5-no-fbv", dict(model="hmm-multinom", outputs=C2, K=5),
     dict(schedule="separate", fb_mode="GAMMA|PACK", vit="lanes", side_stream="1", regions=PACKED + ",bp")),
    # not an HMM-family request: no plan
    ("iohmm", dict(model="iohmm-reg", outputs=O["loglik"]), dict(schedule="none", regions="-")),
]


@pytest.mark.parametrize("req,want", [p[1:] for p in PINS], ids=[p[0] for p in PINS])
def test_plan_pins(engine, req, want):
    got = plan(engine, **req)
    assert {k: got[k] for k in want} == want, got


def test_every_schedule_and_mode_is_pinned():
    """What hhmm_selftest_plan can reach (a segment window has no request of its own)."""
    assert {p[2]["schedule"] for p in PINS if "schedule" in p[2]} == {"phased", "separate", "fused", "split", "lite",
                                                                      "none"}
    assert {p[2]["fb_mode"] for p in PINS if "fb_mode" in p[2]} >= {
        "GAMMA", "FULL", "FWD", "GAMMA|FFBS", "FULL|FFBS", "GAMMA|PACK", "GAMMA|FFBS|PACK", "GAMMA|PACK|BIG",
        "BOTH+FFBS", "-"}
