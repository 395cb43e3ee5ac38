"""CPU: the four "statistics per (series, draw) pair" entries -- hhmm_estep,
hhmm_draw_stats, hhmm_draw_stats_gauss, hhmm_expected_stats -- share one host
path (csrc/hhmm_stats_api.cpp stats_*, csrc/hhmm_stats.h), so the same fault
gets the same answer from each, their workspaces agree, and the request fields
an entry does not read stay ignored.  The three state-parallel entries
(hhmm_estep_large, hhmm_draw_stats_large, hhmm_pointwise_large) share that path
and their own launch helpers; their refusals are pinned word for word.  Every
check here is decided before a device is needed.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import hhmm_amd  # noqa: F401
from hhmm_amd import _abi

_estep = sys.modules["hhmm_amd.estep"]
_gibbs = sys.modules["hhmm_amd.gibbs"]
_gg = sys.modules["hhmm_amd.gibbs_gauss"]

N, S, T, K, L = 2, 3, 9, 4, 3  # K = 4: hhmm-tayal2009's only K
P = N * S
DISCRETE = ("hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009")
# entry -> (its name in messages, the models it accepts, does it read ffbs_u)
ENTRIES = {
    "estep": ("E-step", ("hmm", "hmm-multinom"), False),
    "draw_stats": ("draw statistics", DISCRETE, True),
    "draw_stats_gauss": ("Gaussian draw statistics", ("hmm",), True),
    "expected_stats": ("expected statistics", DISCRETE, False),
}
CASES = [(entry, model) for entry, (_name, models, _u) in ENTRIES.items() for model in models]


def make(model):
    g = np.random.Generator(np.random.Philox(key=4100))
    if model == "hmm":
        data = {"K": K, "x": g.normal(size=(N, T))}
        draws = {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K)),
                 "mu_k": np.sort(g.normal(size=(S, K)), axis=1), "sigma_k": g.uniform(0.5, 1.5, size=(S, K))}
        return data, draws
    data = {"K": K, "L": L, "x": g.integers(1, L + 1, size=(N, T)).astype(np.int32)}
    phi = g.dirichlet(np.full(L, 2.0), size=(S, K))
    if model == "hhmm-tayal2009":
        data["sign"] = g.integers(1, 3, size=(N, T)).astype(np.int32)
        return data, {"p_11": g.uniform(0.2, 0.8, size=S), "A_row": g.dirichlet(np.full(2, 2.0), size=(S, 2)),
                      "phi_k": phi}
    if model == "hmm-multinom-semisup":
        data["g"] = g.integers(1, 4, size=(N, T)).astype(np.int32)
        data["G"] = 3
    return data, {"p_1k": g.dirichlet(np.full(K, 2.0), size=S), "A_ij": g.dirichlet(np.full(K, 2.0), size=(S, K)),
                  "phi_k": phi}


def prepared(entry, model):
    """(PreparedRequest, EstepResult) of a request the entry accepts."""
    data, draws = make(model)
    u = np.random.Generator(np.random.Philox(key=4101)).uniform(0.1, 1.0, size=(P, T))
    if entry == "estep":
        pr, res, _out = _estep.prepare(model, data, draws, "grid")
    elif entry == "draw_stats":
        pr, res, _out = _gibbs.prepare(model, data, draws, u, "grid")
    elif entry == "draw_stats_gauss":
        pr, res, _out = _gg.prepare(data, draws, u, "grid")
    else:
        pr, res, _out = _gibbs._request(model, data, draws, "grid", -1)
    assert pr.P == P
    return pr, res


def call(engine, entry, path, req, res):
    """Status and message of hhmm_<entry> ("host") or hhmm_<entry>_device with a NULL workspace of size 0."""
    if path == "host":
        st = getattr(engine, "hhmm_" + entry)(req, res)
    else:
        st = getattr(engine, f"hhmm_{entry}_device")(req, res, None, 0, None)
    return st, engine.hhmm_last_error().decode()


def _set(field, value):
    def f(pr):
        obj = pr.req
        *path, name = field.split(".")
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, name, value)
    return f


# fault -> (change to the request, or which argument is NULL; the status; a word of the message)
FAULTS = {
    "null_request": ("req", _abi.ERR_INVALID_ARGUMENT, "request"),
    "null_result": ("res", _abi.ERR_INVALID_ARGUMENT, "result"),
    "abi_1": (_set("abi_version", 1), _abi.ERR_INVALID_ARGUMENT, "abi"),
    "model_0": (_set("model", 0), _abi.ERR_INVALID_ARGUMENT, "model id 0"),
    "model_10": (_set("model", 10), _abi.ERR_INVALID_ARGUMENT, "model id 10"),
    "K_9": (_set("data.K", 9), _abi.ERR_UNSUPPORTED, "K = 9"),
    "device_set": (_set("device", _abi.DEVICE_SET), _abi.ERR_UNSUPPORTED, "DEVICE_SET"),
}


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("entry,model", CASES)
def test_same_rejection_for_the_same_fault(engine, entry, model, fault, path):
    change, status, word = FAULTS[fault]
    pr, res = prepared(entry, model)
    req_arg, res_arg = C.byref(pr.req), C.byref(res)
    if change == "req":
        req_arg = None
    elif change == "res":
        res_arg = None
    else:
        change(pr)
    st, msg = call(engine, entry, path, req_arg, res_arg)
    assert st == status, (entry, model, fault, path, st, msg)
    assert msg.startswith(ENTRIES[entry][0] + ":") and word in msg, (entry, model, fault, path, msg)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_workspace_size_rejects_null_arguments(engine, entry):
    size = getattr(engine, f"hhmm_{entry}_workspace_size")
    pr, _res = prepared(entry, ENTRIES[entry][1][0])
    ws = C.c_size_t(0)
    assert size(None, C.byref(ws)) == _abi.ERR_INVALID_ARGUMENT
    assert size(C.byref(pr.req), None) == _abi.ERR_INVALID_ARGUMENT


def fb_chunk(k):
    return 8 if k <= 4 else 4


@pytest.mark.parametrize("k", [4, 5])  # either side of fb_chunk's change from 8 to 4
def test_workspace_sizes_agree(engine, k):
    """ceil(T_max / fb_chunk(K)) * K * P * 8 bytes from all four, whatever the model."""
    want = -(-T // fb_chunk(k)) * k * P * 8
    for entry, model in CASES:
        pr, _res = prepared(entry, model)
        pr.req.data.K = k
        ws = C.c_size_t(0)
        st = getattr(engine, f"hhmm_{entry}_workspace_size")(C.byref(pr.req), C.byref(ws))
        assert st == _abi.OK and ws.value == want, (entry, model, k, st, ws.value, want)


@pytest.mark.parametrize("entry,model", CASES)
def test_ignored_fields_stay_ignored(engine, entry, model):
    """outputs = 0, hat_rand = NULL and (where the entry reads no uniforms) ffbs_u = NULL
    pass the argument checks: without a GPU the answer is NO_DEVICE, with one the NULL
    workspace is refused -- no kernel runs either way.  The two draw entries need ffbs_u."""
    reads_u = ENTRIES[entry][2]
    pr, res = prepared(entry, model)
    pr.req.outputs = 0
    pr.req.hat_rand = None
    if not reads_u:
        pr.req.ffbs_u = None
    st, msg = call(engine, entry, "device", C.byref(pr.req), C.byref(res))
    assert st == _abi.ERR_NO_DEVICE or (st == _abi.ERR_INVALID_ARGUMENT and "workspace" in msg), (entry, model, st, msg)
    if reads_u:
        pr.req.ffbs_u = None
        for path in ("device", "host"):
            st, msg = call(engine, entry, path, C.byref(pr.req), C.byref(res))
            assert st == _abi.ERR_INVALID_ARGUMENT and "ffbs_u" in msg, (entry, model, path, st, msg)
            assert msg.startswith(ENTRIES[entry][0] + ":"), msg


# ---- the three state-parallel entries (8 < K <= 32): the refusal texts, word for word ----

_pointwise = sys.modules["hhmm_amd.pointwise"]
# entry -> hmm-multinom's first L whose tables of one group do not fit in LDS, at K = 12 (16 lanes) and K = 25 (32)
LARGE = {
    "estep_large": {12: 640, 25: 320},
    "draw_stats_large": {12: 849, 25: 418},
    "pointwise_large": {12: 1279, 25: 639},
}
# case -> (K the request is built with, the K poked into it, the model id poked into it)
LARGE_CASES = {"K8": (12, 8, None), "K33": (12, 33, None), "model": (12, None, 3), "lds_G16": (12, None, None),
               "lds_G32": (25, None, None)}


def large_prepared(entry, case):
    """(PreparedRequest, result) of an hmm-multinom request with the case's fault."""
    K0, K1, model_id = LARGE_CASES[case]
    Lx = LARGE[entry][K0] if case.startswith("lds") else L
    g = np.random.Generator(np.random.Philox(key=4102))
    data = {"K": K0, "L": Lx, "x": g.integers(1, Lx + 1, size=(N, T)).astype(np.int32)}
    draws = {"p_1k": g.dirichlet(np.full(K0, 2.0), size=S), "A_ij": g.dirichlet(np.full(K0, 2.0), size=(S, K0)),
             "phi_k": g.dirichlet(np.full(Lx, 2.0), size=(S, K0))}
    if entry == "estep_large":
        pr, res, _out = _estep.prepare("hmm-multinom", data, draws, "grid")
    elif entry == "draw_stats_large":
        u = np.random.Generator(np.random.Philox(key=4101)).uniform(0.1, 1.0, size=(P, T))
        pr, res, _out = _gibbs.prepare("hmm-multinom", data, draws, u, "grid")
    else:
        pr, res, _out = _pointwise.prepare("hmm-multinom", data, draws, "grid")
    if K1 is not None:
        pr.req.data.K = K1
    if model_id is not None:
        pr.req.model = model_id
    return pr, res


_K_RANGE = "the state-parallel kernel supports 9 <= K <= 32"
# (entry, case) -> the message, from both the host and the device entry (K8, K33: from _workspace_size too)
LARGE_TEXT = {
    ("estep_large", "K8"): f"large-K E-step: K = 8, {_K_RANGE} (hhmm_estep takes K <= 8)",
    ("estep_large", "K33"): f"large-K E-step: K = 33, {_K_RANGE}",
    ("estep_large", "model"): "large-K E-step: model 3 is not supported (hmm and hmm-multinom only; the other "
                              "programs have no state-parallel E-step)",
    ("estep_large", "lds_G16"): "large-K E-step: L = 640: the emission table and its count table of one 16-lane "
                                "group do not fit in LDS",
    ("estep_large", "lds_G32"): "large-K E-step: L = 320: the emission table and its count table of one 32-lane "
                                "group do not fit in LDS",
    ("draw_stats_large", "K8"): f"large-K draw statistics: K = 8, {_K_RANGE} (hhmm_draw_stats / "
                                "hhmm_draw_stats_gauss takes K <= 8)",
    ("draw_stats_large", "K33"): f"large-K draw statistics: K = 33, {_K_RANGE}",
    ("draw_stats_large", "model"): "large-K draw statistics: model 3 is not supported (hmm and hmm-multinom only; "
                                   "hmm-multinom-semisup and hhmm-tayal2009 are K <= 8 programs (hhmm_draw_stats))",
    ("draw_stats_large", "lds_G16"): "large-K draw statistics: L = 849: 16 * (16 + 12 * L + 4 * K) = 164032 > 163840 "
                                     "bytes: the emission table, its count table and the xi rows of one 16-lane group "
                                     "do not fit in LDS",
    ("draw_stats_large", "lds_G32"): "large-K draw statistics: L = 418: 32 * (16 + 12 * L + 4 * K) = 164224 > 163840 "
                                     "bytes: the emission table, its count table and the xi rows of one 32-lane group "
                                     "do not fit in LDS",
    ("pointwise_large", "K8"): f"large-K pointwise: K = 8, {_K_RANGE} (hhmm_pointwise takes K <= 8)",
    ("pointwise_large", "K33"): f"large-K pointwise: K = 33, {_K_RANGE}",
    ("pointwise_large", "model"): "large-K pointwise: model 3 is not supported (hmm and hmm-multinom only; the coded "
                                  "step weights of the semisup, Tayal and IOHMM programs are masked or factorised, "
                                  "not a predictive density)",
    ("pointwise_large", "lds_G16"): "large-K pointwise: L = 1279: (2 + L) * 16 * 8 = 163968 > 163840 bytes: the "
                                    "emission table of one 16-lane group does not fit in LDS",
    ("pointwise_large", "lds_G32"): "large-K pointwise: L = 639: (2 + L) * 32 * 8 = 164096 > 163840 bytes: the "
                                    "emission table of one 32-lane group does not fit in LDS",
}


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("entry,case", sorted(LARGE_TEXT))
def test_large_entries_refuse_in_these_words(engine, entry, case, path):
    pr, res = large_prepared(entry, case)
    st, msg = call(engine, entry, path, C.byref(pr.req), C.byref(res))
    assert st == _abi.ERR_UNSUPPORTED and msg == LARGE_TEXT[entry, case], (entry, case, path, st, msg)


@pytest.mark.parametrize("case", ["K8", "K33"])
@pytest.mark.parametrize("entry", sorted(LARGE))
def test_large_workspace_size_refuses_in_these_words(engine, entry, case):
    pr, _res = large_prepared(entry, case)
    ws = C.c_size_t(0)
    st = getattr(engine, f"hhmm_{entry}_workspace_size")(C.byref(pr.req), C.byref(ws))
    msg = engine.hhmm_last_error().decode()
    assert st == _abi.ERR_UNSUPPORTED and msg == LARGE_TEXT[entry, case], (entry, case, st, msg)
