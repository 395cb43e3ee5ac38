"""Reduction over draws (include/hhmm_summary.h): type-7 quantiles per cell and
the hard state, against the numpy restatement of the contract
(tests/summary_ref.py), bit for bit.

CPU: symbols, struct layouts, shape and argument checks (the C checks come
before the device check, so they answer INVALID_ARGUMENT / UNSUPPORTED with no
GPU).  gpu: the host entry (hhmm_summary) and the device entry
(hhmm_summary_device, on torch's stream) on synthetic arrays.

S values: the contract's list, plus S-1, S, S+1 at every S where the kernel
changes tier (hhmm_summary.hip): the slot of a cell is 2^ceil(log2 S) keys with
a floor of 8, 2048 / slot cells share a workgroup up to a slot of 2048, larger
slots take one 1024-thread workgroup each -- so every power of two from 8 to
8192 is a boundary (2048 -> 2049 also switches kernels).
"""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import summary_ref
from hhmm_amd import _abi, api, synth

REPO = pathlib.Path(__file__).resolve().parent.parent

S_CONTRACT = [1, 2, 3, 63, 64, 65, 250, 1000, 4096, 16384]
S_TIERS = [s + d for s in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192) for d in (-1, 0, 1)] + [16383]
S_ALL = sorted(set(S_CONTRACT + S_TIERS))


# ---------------------------------------------------------------- CPU

def test_restatement_cell_and_array_agree():
    g = np.random.Generator(np.random.Philox(key=3))
    S, N, T, K = 11, 2, 3, 2
    v = g.normal(size=(S * N, T, K))
    v[3, 1, 0] = np.nan
    probs = [0, 0.1, 1 / 3, 0.5, 1]
    q = summary_ref.quantiles(v, S, probs)
    for n in range(N):
        for t in range(T):
            for k in range(K):
                for j, p in enumerate(probs):
                    want = summary_ref.cell_quantile(v[S * n:S * (n + 1), t, k], p)
                    assert np.array_equal(q[n, t, k, j], want, equal_nan=True)
    assert np.array_equal(q[..., 3][~np.isnan(q[..., 3])],
                          np.median(v.reshape(S, N, T, K, order="F"), axis=0)[~np.isnan(q[..., 3])])
    am = summary_ref.argmax(np.array([[[1.0, 2.0, 2.0], [np.nan, np.nan, np.nan], [np.nan, -np.inf, np.nan]]]))
    assert am.tolist() == [[2, 0, 2]]


def test_symbols_load(engine):
    for name in ("hhmm_summary", "hhmm_summary_device", "hhmm_run_summary"):
        assert getattr(engine, name).restype is C.c_int


def test_struct_layout_matches_header(tmp_path):
    classes = {"hhmm_summary_request": _abi.SummaryRequest, "hhmm_summary_spec": _abi.SummarySpec,
               "hhmm_summary_result": _abi.SummaryResult}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hhmm_summary.h"', "int main(void){"]
    for st, cls in classes.items():
        src.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            src.append(f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    src.append('printf("max probs %d\\nmax draws %d\\n", HHMM_SUMMARY_MAX_PROBS, HHMM_SUMMARY_MAX_DRAWS);')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(REPO / "include"), str(c), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    lay = {tuple(r.split()[:2]): int(r.split()[2]) for r in rows if r}
    for cname, cls in classes.items():
        assert lay[(cname, "sizeof")] == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert lay[(cname, f)] == getattr(cls, f).offset, (cname, f)
    assert lay[("max", "probs")] == _abi.SUMMARY_MAX_PROBS and lay[("max", "draws")] == _abi.SUMMARY_MAX_DRAWS


def test_python_shape_checks():
    from hhmm_amd import summary
    with pytest.raises(ValueError):
        summary.make_request(np.zeros((10, 4, 2)), 3, [0.5])            # P % S != 0
    with pytest.raises(ValueError):
        summary.make_request(np.zeros((6, 4, 2)), 3, [0.5], T=[4, 4, 4])  # one length per series: N = 2
    with pytest.raises(ValueError):
        summary.make_request(np.zeros((6, 4, 2)), 3, [0.5], T=[4, 5])     # T > T_max
    with pytest.raises(ValueError):
        summary.make_request(np.zeros(6), 3, [0.5])
    req, _keep, dims, kaxis = summary.make_request(np.zeros((6, 4), dtype=np.int64), 3, [0.1, 0.9], T=[4, 1])
    assert dims == (2, 4, 1, 2) and not kaxis and req.values_i32 and not req.values_f64


def _c_request(S=4, N=1, T=2, K=1, probs=(0.5,), argmax_prob=-1.0, f64=True, i32=False):
    req = _abi.SummaryRequest()
    req.n_series, req.n_draws, req.T_max, req.K = N, S, T, K
    req.n_probs = len(probs)
    for j, p in enumerate(probs[:16]):
        req.probs[j] = p
    req.argmax_prob = argmax_prob
    n = max(S, 1) * N * T * K
    keep = [np.zeros(n), np.zeros(n, dtype=np.int32)]
    if f64:
        req.values_f64 = keep[0].ctypes.data
    if i32:
        req.values_i32 = keep[1].ctypes.data
    return req, keep


BAD = {
    "Q0": dict(probs=()),
    "Q17": dict(probs=(0.5,) * 17),
    "p_negative": dict(probs=(0.5, -0.25)),
    "p_above_1": dict(probs=(1.0000001,)),
    "p_nan": dict(probs=(float("nan"),)),
    "S0": dict(S=0),
    "both_values": dict(f64=True, i32=True),
    "no_values": dict(f64=False, i32=False),
    "argmax_prob_above_1": dict(argmax_prob=1.5),
    "argmax_prob_negative": dict(argmax_prob=-0.5),
    "argmax_prob_nan": dict(argmax_prob=float("nan")),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_reject_bad_arguments_before_the_device_check(engine, case, entry):
    req, _keep = _c_request(**BAD[case])
    q = np.zeros(64 * 17)
    am = np.zeros(64, dtype=np.int32)
    if entry == "host":
        st = engine.hhmm_summary(C.byref(req), q.ctypes.data, am.ctypes.data, -1)
    else:
        st = engine.hhmm_summary_device(C.byref(req), q.ctypes.data, am.ctypes.data, None)
    assert st == _abi.ERR_INVALID_ARGUMENT, (case, st, engine.hhmm_last_error().decode())


@pytest.mark.parametrize("entry", ["host", "device"])
def test_c_entries_too_many_draws_is_unsupported(engine, entry):
    req, _keep = _c_request(S=16385)
    q = np.zeros(64)
    if entry == "host":
        st = engine.hhmm_summary(C.byref(req), q.ctypes.data, None, -1)
    else:
        st = engine.hhmm_summary_device(C.byref(req), q.ctypes.data, None, None)
    assert st == _abi.ERR_UNSUPPORTED
    assert "16385" in engine.hhmm_last_error().decode()


def _run_summary_call(engine, pairing, outputs, summarise):
    N, S = (3, 3) if pairing == "zip" else (2, 4)
    data, draws = synth.GENERATORS["hmm-multinom"](N=N, S=S, T=10)
    pr = api.PreparedRequest("hmm-multinom", data, draws, ["loglik"], pairing)
    pr.req.outputs = outputs
    spec = _abi.SummarySpec()
    spec.n_probs = 1
    spec.probs[0] = 0.5
    spec.summarise = summarise
    spec.argmax_prob = -1.0
    res = _abi.SummaryResult()
    q = np.zeros(N * 10 * 4)
    for b in range(32):
        res.quantiles[b] = q.ctypes.data
    st = engine.hhmm_run_summary(C.byref(pr.req), C.byref(spec), C.byref(pr.res), C.byref(res))
    return st, engine.hhmm_last_error().decode()


def test_run_summary_rejects_zip(engine):
    st, msg = _run_summary_call(engine, "zip", _abi.OUT["loglik"], _abi.OUT["alpha_tk"])
    assert st == _abi.ERR_INVALID_ARGUMENT and "ZIP" in msg


def test_run_summary_rejects_per_step_output_outside_summarise(engine):
    st, msg = _run_summary_call(engine, "grid", _abi.OUT["loglik"] | _abi.OUT["gamma_tk"], _abi.OUT["alpha_tk"])
    assert st == _abi.ERR_INVALID_ARGUMENT and "summarise" in msg
    # the same request with the bit summarised passes the argument checks (no GPU: NO_DEVICE; with one: OK)
    st, msg = _run_summary_call(engine, "grid", _abi.OUT["loglik"] | _abi.OUT["gamma_tk"],
                                _abi.OUT["alpha_tk"] | _abi.OUT["gamma_tk"])
    assert st in (_abi.OK, _abi.ERR_NO_DEVICE), msg


# ---------------------------------------------------------------- GPU

def _host(engine, v, S, probs, T=None, argmax_prob=None, fill=np.nan, afill=0):
    """hhmm_summary on caller arrays pre-filled with `fill` / `afill`."""
    from hhmm_amd import summary
    v = np.asarray(v)
    N, Tm = v.shape[0] // S, v.shape[1]
    Q = np.atleast_1d(probs).size
    shape = (N, Tm, v.shape[2], Q) if v.ndim == 3 else (N, Tm, Q)
    out = np.full(shape, fill, order="F")
    oa = np.full((N, Tm), afill, dtype=np.int32, order="F") if argmax_prob is not None else None
    got = summary.quantiles(v, S, probs, T=T, argmax_prob=argmax_prob, lib=engine, out=out, out_argmax=oa)
    return got if argmax_prob is not None else (got, None)


def _device(engine, v, S, probs, T=None, argmax_prob=None, fill=np.nan, afill=0):
    """hhmm_summary_device on torch buffers, torch's current stream."""
    import torch
    from hhmm_amd import summary
    req, keep, (N, Tm, K, Q), kaxis = summary.make_request(v, S, probs, T, argmax_prob)
    dev = torch.device("cuda", torch.cuda.current_device())
    dv = torch.from_numpy(keep[0].reshape(-1, order="F").copy()).to(dev)
    if req.values_f64:
        req.values_f64 = dv.data_ptr()
    else:
        req.values_i32 = dv.data_ptr()
    dT = None
    if T is not None:
        dT = torch.from_numpy(keep[1].copy()).to(dev)
        req.T = dT.data_ptr()
    dq = torch.full((N * Tm * K * Q,), fill, dtype=torch.float64, device=dev)
    da = torch.full((N * Tm,), afill, dtype=torch.int32, device=dev)
    st = engine.hhmm_summary_device(C.byref(req), dq.data_ptr(), da.data_ptr() if argmax_prob is not None else None,
                                    torch.cuda.current_stream().cuda_stream)
    assert st == 0, engine.hhmm_last_error().decode()
    torch.cuda.synchronize()
    q = dq.cpu().numpy().reshape((N, Tm, K, Q) if kaxis else (N, Tm, Q), order="F")
    return q, (da.cpu().numpy().reshape((N, Tm), order="F") if argmax_prob is not None else None)


def _check(engine, v, S, probs, T=None, argmax_prob=None, entries=("host", "device")):
    fill, afill = -777.25, -9
    want = summary_ref.quantiles(v, S, probs, T=T, fill=fill)
    wa = None
    if argmax_prob is not None:
        qa = summary_ref.quantiles(v, S, [argmax_prob], T=T)
        wa = summary_ref.argmax(qa[..., 0] if qa.ndim == 4 else qa, T=T, fill=afill)
    for entry in entries:
        q, am = (_host if entry == "host" else _device)(engine, v, S, probs, T, argmax_prob, fill, afill)
        assert q.shape == want.shape
        bad = ~((q == want) | (np.isnan(q) & np.isnan(want)))
        assert np.array_equal(q, want, equal_nan=True), (entry, S, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        if wa is not None:
            assert np.array_equal(am, wa), (entry, S)


def _mixed(g, P, T, K):
    """Uniforms with ties, negatives and one NaN cell among untouched neighbours."""
    v = g.uniform(-1.0, 1.0, size=(P, T, K))
    v[g.uniform(size=v.shape) < 0.2] = 0.25     # ties
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("S", S_ALL)
def test_gpu_every_S(engine, S):
    """N = 3 ragged (one T[n] = 1), K = 3, three probabilities and the hard state at the median."""
    g = np.random.Generator(np.random.Philox(key=100 + S))
    N, T, K = 3, 3, 3
    v = _mixed(g, N * S, T, K)
    v[S + S // 2, 0, 1] = np.nan          # series 1, t = 0, k = 1: that cell alone becomes NaN
    _check(engine, v, S, [0.1, 0.5, 0.9], T=[3, 1, 2], argmax_prob=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("S", [250, 1000])
def test_gpu_K_axis(engine, S, K):
    g = np.random.Generator(np.random.Philox(key=7 * S + K))
    v = g.uniform(size=(5 * S, 21, K))
    _check(engine, v, S, [0.1, 0.5, 0.9], argmax_prob=0.5)
    if K == 1:
        _check(engine, v[:, :, 0], S, [0.1, 0.5, 0.9])  # [P, T] input, [N, T, Q] output


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 65, 250, 4096])
def test_gpu_layouts(engine, S):
    g = np.random.Generator(np.random.Philox(key=S))
    _check(engine, g.uniform(size=(S, 7, 3)), S, [0.5], argmax_prob=0.5)                 # N = 1
    _check(engine, g.uniform(size=(3 * S, 1, 4)), S, [0.5], T=[1, 1, 1], argmax_prob=0.5)  # T_max = 1
    T = [1, 13, 6]
    _check(engine, g.uniform(size=(3 * S, 13, 3)), S, [0.25, 0.75], T=T, argmax_prob=0.25)  # ragged
    # more groups than one workgroup holds at any S: N * T_max = 3 * 700 > 256
    if S <= 250:
        _check(engine, g.uniform(size=(3 * S, 700, 1)), S, [0.5], T=[700, 1, 333], entries=("host",))


PROBS16 = [0.0, 1.0, 0.5, 1 / 3, 1 / 3, 0.1, 0.9, 0.25, 0.75, 2 / 3, 0.01, 0.99, 0.5, 1e-300, 1 - 2.0 ** -53, 0.6]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 3, 64, 250, 251, 1000, 4096])
def test_gpu_probabilities(engine, S):
    g = np.random.Generator(np.random.Philox(key=900 + S))
    v = _mixed(g, 2 * S, 5, 3)
    assert len(PROBS16) == 16
    _check(engine, v, S, PROBS16, argmax_prob=1 / 3)
    for p in (0.0, 1.0, 0.5, 1 / 3):
        _check(engine, v, S, [p], entries=("host",))   # Q = 1


def _value_cases(g, S):
    P, T, K = 2 * S, 6, 3
    yield "uniform01", g.uniform(size=(P, T, K))
    ties = (g.uniform(size=(P, T, K)) < 0.5).astype(np.float64)
    ties[:, 0, 0] = 0.0
    ties[:, 1, 1] = 1.0
    yield "ties01", ties
    yield "negative", -g.uniform(1.0, 50.0, size=(P, T, K))
    mixed = g.normal(0, 1e3, size=(P, T, K))
    mixed[g.uniform(size=mixed.shape) < 0.1] = 0.0
    mixed[g.uniform(size=mixed.shape) < 0.1] = -0.0
    yield "mixed_sign", mixed
    inf = g.normal(size=(P, T, K))
    inf[g.uniform(size=inf.shape) < 0.3] = np.inf
    inf[g.uniform(size=inf.shape) < 0.3] = -np.inf
    inf[:, 0, 0] = np.inf
    inf[:, 0, 1] = -np.inf
    yield "inf", inf
    sub = g.integers(-40, 40, size=(P, T, K)).astype(np.float64) * 5e-324
    sub[g.uniform(size=sub.shape) < 0.2] = 2.2250738585072014e-308
    yield "subnormal", sub
    nan = g.uniform(size=(P, T, K))
    nan[S // 2, 2, 1] = np.nan
    nan[S + (S - 1), 4, 0] = np.nan
    nan[0, 5, 2] = np.nan
    nan[:S, 3, :] = np.nan             # an all-NaN row of series 0 at t = 3: hard state 0
    yield "nan", nan


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 250, 1001, 4096])
@pytest.mark.parametrize("kind", ["uniform01", "ties01", "negative", "mixed_sign", "inf", "subnormal", "nan"])
def test_gpu_values(engine, S, kind):
    g = np.random.Generator(np.random.Philox(key=S))
    v = dict(_value_cases(g, S))[kind]
    _check(engine, v, S, [0.0, 0.1, 0.5, 0.9, 1.0], argmax_prob=0.5)
    if kind == "nan":
        am = _host(engine, v, S, [0.5], argmax_prob=0.5)[1]
        assert am[0, 3] == 0 and (am[1] > 0).all()
    if kind == "ties01":   # the hard state of a tie is the first k
        am = _host(engine, np.ones((S, 2, 4)), S, [0.5], argmax_prob=0.5)[1]
        assert (am == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 64, 250, 1000])
def test_gpu_int32_input(engine, S):
    """zstar-like values 0..K with S even: x.5 medians, as R's median() of integers."""
    K = 4
    g = np.random.Generator(np.random.Philox(key=40 + S))
    z = g.integers(0, K + 1, size=(3 * S, 17), dtype=np.int32)
    z[:S // 2, 0] = 1
    z[S // 2:S, 0] = 2                  # a median of exactly 1.5
    want = summary_ref.quantiles(z, S, [0.5], T=[17, 9, 1])
    assert want[0, 0, 0] == 1.5
    _check(engine, z, S, [0.1, 0.5, 0.9], T=[17, 9, 1])
    _check(engine, z.reshape(3 * S, 17, 1), S, [0.5], argmax_prob=0.5, entries=("host",))
    assert np.array_equal(summary_ref.quantiles(z, S, [0.5])[:, :, 0],
                          np.median(z.reshape(S, 3, 17, order="F").astype(np.float64), axis=0))
