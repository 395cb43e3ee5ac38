"""RDX2 reader for the reference's tick files (SURVEY.md §8 F1 input side;
tayal2009/main.R:47-58 loads tayal2009/data/<SYM>/*.RData with `load()`).

CPU only.  A hand-serialised xts (the same layout the reference's files carry:
REALSXP matrix + dim / dimnames / index / class attributes, XDR, gzip) checks
the decoder.  The tests that decode the reference's real G.TO files and
reproduce its report's tables from them are in tests/reference_pins.py, run by
name against a checkout of the reference: the data (CC-BY-NC,
tayal2009/data/LICENSE.md) is not carried by this repository.  The report's
printed tables and the helpers around them stay here (tests/test_gpu_table4.py
uses them on synthetic legs).
"""
import gzip
import struct

import numpy as np
import pytest

from hhmm_amd import rdata


def _i(v):
    return struct.pack(">i", v)


def _flags(t, attr=False, tag=False, obj=False):
    return _i(t | (1 << 9 if attr else 0) | (1 << 10 if tag else 0) | (1 << 8 if obj else 0))


def _charsxp(s):
    b = s.encode()
    return _i(0x00040009) + _i(len(b)) + b


def _sym(name):
    return _i(rdata.SYMSXP) + _charsxp(name)


def _strsxp(vals):
    return _i(rdata.STRSXP) + _i(len(vals)) + b"".join(_charsxp(v) for v in vals)


def _real(vals, attrs=b""):
    v = np.asarray(vals, dtype=">f8")
    return _flags(rdata.REALSXP, attr=bool(attrs)) + _i(v.size) + v.tobytes() + attrs


def _pairlist(items):
    out = b""
    for tag, val in items:
        out += _flags(rdata.LISTSXP, tag=True) + _sym(tag) + val
    return out + _i(rdata.NILVALUE)


def _xts_file(name, price, size, index):
    n = len(price)
    dim = _flags(rdata.INTSXP) + _i(2) + _i(n) + _i(2)
    dimnames = _flags(rdata.VECSXP) + _i(2) + _i(rdata.NILVALUE) + _strsxp(["PRICE", "SIZE"])
    attrs = _pairlist([("dim", dim), ("dimnames", dimnames), ("index", _real(index)),
                       ("class", _strsxp(["xts", "zoo"]))])
    body = _real(np.concatenate([price, size]), attrs)
    raw = b"RDX2\nX\n" + _i(2) + _i(0x030303) + _i(0x020300) + _pairlist([(name, body)])
    return gzip.compress(raw)


def test_reader_roundtrip(tmp_path):
    price = np.array([10.0, np.nan, 10.01, 10.0, 9.99])
    size = np.array([100.0, 200.0, 300.0, np.nan, 500.0])
    index = 1.17802622e9 + np.arange(5.0)
    f = tmp_path / "2007.05.01.X.TO.RData"
    f.write_bytes(_xts_file("X.TO", price, size, index))
    objs = rdata.read_rdata(f)
    assert list(objs) == ["X.TO"]
    idx, cols = rdata.xts_columns(objs["X.TO"])
    assert list(cols) == ["PRICE", "SIZE"] and np.array_equal(idx, index)
    p, s, t = rdata.load_ticks(f)  # na.omit drops rows 2 and 4
    assert np.array_equal(p, [10.0, 10.01, 9.99]) and np.array_equal(s, [100.0, 300.0, 500.0])
    assert np.array_equal(t, index[[0, 2, 4]])


def test_reader_refuses_code(tmp_path):
    raw = b"RDX2\nX\n" + _i(2) + _i(0) + _i(0) + _flags(rdata.LISTSXP, tag=True) + _sym("f") + _i(3)
    f = tmp_path / "closure.RData"
    f.write_bytes(raw)
    with pytest.raises(ValueError):
        rdata.read_rdata(f)


# ---- The reference's printed tables for the Tayal forward (A2/A6/A7/A12 with the Q6 mask) -----
#
# Table 4 of main.pdf (main.Rmd:704-723) is table(x.ins, state.filtered.ins), where
# state.filtered.ins is the per-t which.max of the median over draws of hhmm-tayal2009-lite's
# alpha_tk (main.Rmd:436, 596-602).  Rows = bottom states 1..4, columns = U1..U9, D1..D9.
TABLE4 = np.array([
    [0, 15, 0, 810, 0, 828, 33, 0, 17, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 72, 0, 0, 2208, 0, 181, 0, 59],
    [0, 0, 0, 0, 0, 0, 0, 27, 0, 15, 0, 34, 831, 0, 846, 0, 16, 0],
    [58, 0, 158, 0, 2155, 0, 0, 22, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]])

# Table 8 of main.pdf (main.Rmd:869-907): posterior means of the same fit, printed to 2 decimals.
# p_1k = (.51, 0, .49, 0); A_ij: a12 .46, a13 .54, a21 1, a31 .09, a34 .91, a43 1.
TABLE8_P11 = 0.51
TABLE8_A_ROW = ((0.46, 0.54), (0.09, 0.91))
TABLE8_PHI = np.array([
    [.01, .02, .01, .34, .22, .35, .03, .01, .02],
    [.00, .02, .00, .05, .80, .02, .08, .00, .02],
    [.01, .00, .03, .36, .20, .39, .00, .02, .00],
    [.02, .00, .06, .02, .88, .01, .00, .01, .00]])
# A printed 0.00 is a simplex entry below 0.005, never exactly 0 (simplex[L] phi_k, lite.stan:25);
# it is floored at the midpoint of [0, 0.005) and each row renormalised.
PHI_FLOOR = 0.0025


def table8_draw():
    phi = np.where(TABLE8_PHI == 0.0, PHI_FLOOR, TABLE8_PHI)
    phi = phi / phi.sum(axis=1, keepdims=True)
    return {"p_11": np.array([TABLE8_P11]), "A_row": np.array([TABLE8_A_ROW]), "phi_k": phi[None]}


def table8_flat(draw):
    """hhmm-tayal2009-lite.stan:34-48: the transformed-parameters expansion."""
    p11, (r1, r2) = draw["p_11"][0], draw["A_row"][0]
    p_1k = np.array([[p11, 0.0, 1.0 - p11, 0.0]])
    A = np.zeros((1, 4, 4))
    A[0, 0, 1], A[0, 0, 2], A[0, 1, 0], A[0, 2, 0], A[0, 2, 3], A[0, 3, 2] = r1[0], r1[1], 1, r2[0], r2[1], 1
    return p_1k, A


def tabulate(feature, state):
    """table(x.ins, state) laid out like Table 4: [state, feature]."""
    t = np.zeros((4, 18), dtype=np.int64)
    np.add.at(t, (state - 1, feature - 1), 1)
    return t


def table_agreement(got):
    """Observations whose (feature, state) cell is shared with Table 4: sum of cell-wise minima."""
    return int(np.minimum(got, TABLE4).sum())
