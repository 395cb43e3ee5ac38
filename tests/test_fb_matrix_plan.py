"""CPU: the table of tests/fb_matrix.py is pinned, complete and not vacuous.

hhmm_selftest_plan touches no device.  Three things are shown with it and
with the oracle before tests/test_gpu_fb_matrix.py spends GPU time:

* every case's request gives the plan words the case pins;
* the ledger: the kernels a (model, K) can be asked for at the table's shapes
  are enumerated from the plan function, never from the table, and each is
  pinned by a case here or in tests/test_gpu_hot_sweeps.py -- a kernel added
  to hmm_plan later fails here until it has a case;
* the batches are what the table's docstring promises, and the oracle's
  outputs of every batch visit every state, so a kernel that dropped a state,
  a symbol or a tail chunk could not agree with them by accident."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fb_matrix as fm
import test_gpu_hot_sweeps as hot
from hhmm_amd import _abi
from hot_plan import LANES, plan_of, request

BATCHES = sorted({c.key for c in fm.CASES})


@pytest.mark.parametrize("case", fm.CASES, ids=[c.id for c in fm.CASES])
def test_case_plan(engine, case):
    kind, model, K, L = case.key
    got = plan_of(engine, model, K, L, fm.pairs_of(kind), fm.T_MAX, case.pars, case.flags,
                  fm.T_MAX if model == fm.LITE else 0)
    assert {k: got[k] for k in case.plan} == case.plan, (case.id, got)
    assert set(case.plan) >= {"schedule", "fb", "fb_mode", "oos_fb", "vit", "scan_cl", "vs_nc", "regions"}
    assert got["bound"] == got["regions"]            # every region a planned kernel touches is sized and bound


def _ledger_flags(K):
    sets = [LANES, fm.scan_forced(3), fm.STATES, fm.VSCAN, 0]
    return sets + ([fm.scan_forced(2)] if K > 4 else [])


def _ledger(engine):
    """{key: a request that gives it}: every non-empty subset of the outputs a model declares, under every flag
    set and shape of the table.  L enters hmm_plan for hmm-multinom alone (the packed profile), so the other
    discrete models are walked at L = 9 only; the output subsets are not thinned."""
    buf = C.create_string_buffer(512)
    keys, lines = {}, {}
    for model, K in fm.MODEL_K:
        bits = [_abi.OUT[n] for n in fm.ALL_PARS[model]]
        masks = [sum(b for b, on in zip(bits, sel) if on) for sel in itertools.product((0, 1), repeat=len(bits))][1:]
        for L in ((0,) if model == fm.GAUSS else (9, 17) if model == fm.MULTINOM else (9,)):
            for P in (200, 210, 150):
                r = request(_abi.MODELS[model], K, L, P, fm.T_MAX, fm.T_MAX if model == fm.LITE else 0, 0, 0)
                ref = C.byref(r)
                for flags in _ledger_flags(K):
                    r.flags = flags
                    for m in masks:
                        r.outputs = m
                        assert engine.hhmm_selftest_plan(ref, buf, 512) == _abi.OK, engine.hhmm_last_error()
                        line = buf.value
                        if line not in lines:
                            lines[line] = dict(w.split("=", 1) for w in line.decode().split())
                        keys.setdefault(fm.key_of(model, K, lines[line]), (model, K, L, P, hex(m), hex(flags)))
    return keys


def test_ledger_every_reachable_kernel_has_a_case(engine):
    pinned = {fm.key_of(c.model, c.key[2], c.plan) for c in fm.CASES}
    pinned |= {fm.key_of(hot.MODEL, c.key[1], c.plan) for c in hot.CASES}
    universe = _ledger(engine)
    missing = {k: v for k, v in universe.items() if k not in pinned}
    assert not missing, f"{len(missing)} kernel keys without a case, e.g. {sorted(missing.items())[:5]}"
    # and the universe is the size the families promise: no plan word of the key went missing on the way
    assert all(k[2] in ("separate", "lite", "phased") for k in universe)
    per = {mk: sum(1 for k in universe if k[:2] == mk) for mk in fm.MODEL_K}
    assert per[(fm.GAUSS, 1)] == 9 * 2 - 1 + 3 * 2 and per[(fm.GAUSS, 4)] == 9 * 4 - 1 + 3 * 2, per
    assert per[(fm.LITE, 4)] == 3 * 3 * 4 - 1, per
    # nothing in the table is pinned to a key the plan cannot give at its own shape
    assert {fm.key_of(c.model, c.key[2], c.plan) for c in fm.CASES} <= set(universe)


def test_table_covers_the_issue():
    ids = [c.id for c in fm.CASES]
    assert len(set(ids)) == len(ids)
    by = {}
    for c in fm.CASES:
        by.setdefault((c.model, c.key[2]), set()).add(c.id)
    for model, K in fm.MODEL_K:
        have, tag = by[(model, K)], f"{model}-K{K}"
        if model == fm.LITE:
            assert {f"{tag}-{w}" for w in ("alpha_oos+lanes", "unalpha_oos+lanes", "alpha_oos+states",
                                           "unalpha_oos+vscan", "loglik", "alpha", "unalpha", "lanes")} <= have
            continue
        L17 = "-L17" if model == fm.MULTINOM else ""
        want = {f"{tag}-{w}" for w in ("fwd-loglik", "fwd-alpha", "full", "full-ffbs", "log-fwd", "log-both",
                                       "log-both-ffbs", "scan-fwd", "scan-gamma", "scan-full", "vit+lanes")}
        want |= {f"{tag}{L17}-{w}" for w in ("gamma", "gamma-ffbs", "gamma+lanes")}     # gamma+lanes: side stream
        if K in (3, 6):
            want |= {f"{tag}-{w}" for w in ("full-beta", "full-ungamma", "full-alpha-gamma")}
            want |= {f"{tag}-{kind}-full-ffbs+lanes" for kind in ("grid", "block")}
        if K > 4:
            want |= {f"{tag}-{w}-cl4" for w in ("scan-fwd", "scan-gamma", "scan-full")}
        if 2 <= K <= 4:
            want.add(f"{tag}-vit+states")
        if K in (2, 4):
            want.add(f"{tag}-vit+vscan")
        if model == fm.MULTINOM and K in (1, 2, 3, 5, 7, 8):
            want.add(f"{tag}-gamma-ffbs-pack")
        assert want <= have, sorted(want - have)
    for c in fm.CASES:
        if "+" in c.id and c.plan["fb"] != "none" and c.plan["schedule"] == "separate":
            assert c.plan["side_stream"] == "1", c.id


@pytest.mark.parametrize("C", [4, 8])
def test_ragged_batch_is_what_the_table_promises(C):
    T = fm.ragged_lengths(C)
    Dd = fm.D
    assert T.shape == (200,) and T.max() == fm.T_MAX < 256
    assert set(T[:64]) == set(fm.wave0(C)) and len(set(fm.wave0(C))) == 15 and T[:64].min() == 1
    assert {C - 1, C, C + 1, Dd * C - 1, Dd * C, Dd * C + 1, 2 * Dd * C - 1, 2 * Dd * C, 2 * Dd * C + 1} <= set(T[:64])
    assert (T[64:128] == 2 * Dd * C).sum() == 63 and (T[64:128] == 2 * Dd * C + 1).sum() == 1
    assert T[64:128].min() // C == 2 * Dd                       # nfull: the grouped loop runs twice
    assert -(-int(T[64:128].max()) // C) == 2 * Dd + 1           # nchunk: one lane needs one chunk more
    assert set(T[128:192]) == {1, Dd * C, Dd * C + 1} and (T[128:192] == 1).sum() == 1
    assert (T[128:192] == Dd * C).sum() == 31 and (T[128:192] == Dd * C + 1).sum() == 32
    assert (T[192:] == fm.T_MAX).all() and T[192:].size == 8


@pytest.mark.parametrize("key", BATCHES, ids=["-".join(str(w) for w in k) for k in BATCHES])
def test_batch_is_not_vacuous(oracle, key):
    kind, model, K, L = key
    data, draws, uu = fm.inputs(key)
    C_ = fm.fb_chunk(K)
    if kind == "ragged":
        assert np.array_equal(data["T"], fm.ragged_lengths(C_)) and np.asarray(data["x"]).shape == (200, fm.T_MAX)
    else:
        want = [fm.T_MAX, 2 * fm.D * C_ + 1, fm.D * C_] if kind == "grid" else [2 * fm.D * C_ + 1, C_ + 1, fm.T_MAX]
        assert list(data["T"]) == want
    if model == fm.LITE:
        assert np.array_equal(data["T_oos"], data["T"]) and np.asarray(data["x_oos"]).shape[1] == fm.T_MAX
    assert uu.shape == (fm.pairs_of(kind), fm.T_MAX)
    if model != fm.GAUSS:
        assert fm.symbol_L_occurs(key)
    ref = fm.reference_all(key)
    # no pair is flagged but the length-1 series Q3 leaves undecodable at odd K >= 3 (fm.q3_flagged): exactly those
    flagged = fm.q3_flagged(key)
    assert np.array_equal(ref["pair_status"], np.where(flagged, _abi.PAIR_INVALID_BACKPOINTER, 0))
    assert flagged.sum() == (6 if kind == "ragged" and K in (3, 5, 7) else 0)
    assert np.array_equal(np.isfinite(ref["logp_zstar"]), ~flagged)
    assert not fm.reference(key, ("loglik",))["pair_status"].any()
    assert ref["loglik"].shape == (fm.pairs_of(kind),) and np.isfinite(ref["loglik"]).all()
    states = set(range(1, K + 1))

    def argmax_states(name):
        g = ref[name]
        seen = ~np.isnan(g).any(axis=2)              # the steps of each pair: the rest is never written
        return set(np.argmax(g, axis=2)[seen] + 1)

    for name in (["alpha_tk", "alpha_tk_oos"] if model == fm.LITE else ["gamma_tk"]):
        assert argmax_states(name) == states, (name, argmax_states(name))
    # Q3 pins zstar_1; every state occurs among the decoded steps after it
    z = ref["zstar_t"][:, 1:]
    assert set(z[z > 0]) == states, sorted(set(z[z > 0]))
    if model != fm.LITE:
        zf = ref["z_ffbs"]
        assert set(zf[zf > 0]) == states, sorted(set(zf[zf > 0]))
        assert np.array_equal(zf > 0, ~np.isnan(ref["gamma_tk"][:, :, 0]))    # every step of every pair holds a draw

