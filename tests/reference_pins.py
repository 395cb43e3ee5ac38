"""Pins against the reference's own tick data (tayal2009/data, CC-BY-NC):
not part of the suite, because the data is not part of this repository.

The reference ships Thomson Reuters tick files under a licence this project
does not carry, so nothing of them (or derived from them) is stored here, and
pytest does not collect this module by default.  With a checkout of the
reference at hand, run it by name and point it at the data folder:

    HHMM_REFERENCE_DATA=<reference>/tayal2009/data python -m pytest tests/reference_pins.py -q

The real G.TO files are decoded (hhmm_amd.rdata) and pushed through the
feature oracle, which must agree with the R-semantics transcription
(tests/test_features.py) on real ticks; the zig-zag count, Table 4 and the
Tayal forward of the reference's rendered report (tayal2009/main.pdf) are
reproduced from them; and the walk-forward task list has the reference's 204
windows.  The data is read in place, never copied.  The tables themselves
(printed in the report) and the helpers live in tests/test_rdata.py.
"""
import os
import pathlib

import numpy as np
import pytest

from hhmm_amd import rdata, walkforward as W
from test_rdata import TABLE4, table8_draw, table8_flat, table_agreement, tabulate

if not os.environ.get("HHMM_REFERENCE_DATA"):
    pytest.skip("set HHMM_REFERENCE_DATA to the reference's tayal2009/data folder", allow_module_level=True)
DATA = pathlib.Path(os.environ["HHMM_REFERENCE_DATA"])


def test_real_ticks_through_feature_oracle(oracle):
    import test_features
    files = sorted((DATA / "G.TO").glob("*.RData"))[:3]
    price, size, time = rdata.load_ticks(files)
    assert price.size > 10_000
    assert (size == np.round(size)).all()  # integer volumes: R's long-double sum is exact in double
    got = oracle.extract_features(price, size, time, alpha=0.25)
    test_features._assert_same(got, test_features.transcribe(price, size, time, 0.25))


# tayal2009/main.Rmd:65-74 -- the data set and windows its rendered report (main.pdf) uses
RMD_DAYS = ("2007.05.04", "2007.05.07", "2007.05.08", "2007.05.09", "2007.05.10", "2007.05.11")
RMD_INS = "2007-05-04 09:30:00/2007-05-10 16:30:00"
RMD_OOS = "2007-05-11 09:30:00/2007-05-11 16:30:00"


def test_in_sample_zigzag_count_matches_report(oracle):
    """Reference-held pin for F1: main.Rmd:410 prints nrow(zig.ins), and the
    rendered tayal2009/main.pdf reads "In-sample dataset reduced to 8386
    zig-zags".  The chain is the report's own: load() + rbind + na.omit of the
    six files (:386-395), extract_features(tdata, 0.25) (:405), zig[ins] with
    the index in America/Toronto (:406, main.R:52)."""
    from hhmm_amd import features as F
    files = [DATA / "G.TO" / f"{d}.G.TO.RData" for d in RMD_DAYS]
    price, size, time = rdata.load_ticks(files)
    legs = oracle.extract_features(price, size, time, alpha=0.25)
    when = time[F.index_ticks(legs, price)]
    assert int(F.xts_window(when, RMD_INS).sum()) == 8386
    assert int(F.xts_window(when, RMD_OOS).sum()) > 0


# Column sums of Table 4 ("tab:tseg-filtered-ins") of the rendered tayal2009/main.pdf:
# main.Rmd:704-723 prints table(x.ins, state.filtered.ins) with the rows labelled by
# expand.grid(1:9, c("U", "D")), i.e. feature codes 1..9 = U1..U9 and 10..18 = D1..D9.
# Summed over the four states they are the in-sample count of each leg feature.
TABLE4_U = (58, 15, 158, 810, 2155, 828, 33, 49, 17)
TABLE4_D = (15, 72, 34, 831, 2209, 846, 181, 16, 59)


def test_in_sample_feature_histogram_matches_report_table4(oracle):
    """Second reference-held pin for F1, symbol by symbol: the per-feature counts
    of the same 8386 in-sample zig-zags pin the leg coding of
    feature-extraction.R:92-110, and the (x, sign) split of tayal2009/main.R:85-89
    (sign = 1 for codes 1..9 = U, x = code; sign = 2 for 10..18 = D, x = code - 9)."""
    from hhmm_amd import features as F
    files = [DATA / "G.TO" / f"{d}.G.TO.RData" for d in RMD_DAYS]
    price, size, time = rdata.load_ticks(files)
    legs = oracle.extract_features(price, size, time, alpha=0.25)
    ins = F.xts_window(time[F.index_ticks(legs, price)], RMD_INS)
    counts = np.bincount(legs["feature"][ins], minlength=19)
    assert counts[0] == 0 and counts.size == 19
    assert tuple(counts[1:10]) == TABLE4_U
    assert tuple(counts[10:19]) == TABLE4_D
    assert sum(TABLE4_U) + sum(TABLE4_D) == 8386
    x, sign = legs["x"][ins], legs["sign"][ins]
    assert tuple(np.bincount(x[sign == 1], minlength=10)[1:]) == TABLE4_U
    assert tuple(np.bincount(x[sign == 2], minlength=10)[1:]) == TABLE4_D


def _gto_legs(oracle):
    from hhmm_amd import features as F
    files = [DATA / "G.TO" / f"{d}.G.TO.RData" for d in RMD_DAYS]
    price, size, time = rdata.load_ticks(files)
    legs = oracle.extract_features(price, size, time, alpha=0.25)
    when = time[F.index_ticks(legs, price)]
    return legs, F.xts_window(when, RMD_INS), F.xts_window(when, RMD_OOS)


def test_tayal_forward_reproduces_report_table4(oracle):
    """Pins the oracle's Tayal forward to the reference's own output.  The report's chain on
    CPU: six G.TO files -> extract_features -> in-sample / OOS windows (main.Rmd:405-446) ->
    hhmm-tayal2009-lite at Table 8's posterior means -> which.max(alpha_tk) per t, tabulated
    against the 18 features.  A point estimate stands in for the median over 250 draws, so a
    few observations near a decision boundary may move (U6, U8); every other cell must agree,
    including the Q6-mask cells where up legs go to the bear state 1 (U2/U4/U6/U7/U9) and the
    single D5 observation in state 4."""
    legs, ins, oos = _gto_legs(oracle)
    feat, x, sign = legs["feature"][ins], legs["x"][ins], legs["sign"][ins]
    assert feat.size == 8386 and np.array_equal(feat, np.where(sign == 1, x, x + 9))
    data = {"K": 4, "L": 9, "x": x, "sign": sign, "x_oos": legs["x"][oos], "sign_oos": legs["sign"][oos]}
    draw = table8_draw()
    out = oracle.gqs("hhmm-tayal2009-lite", data, draw, pars=["alpha_tk", "alpha_tk_oos", "zstar_t"])
    got = tabulate(feat, np.argmax(out["alpha_tk"][0], axis=1) + 1)
    assert got.sum() == 8386
    agree = table_agreement(got)
    assert agree >= 8350, (agree, got)
    # the 16 features other than U6 and U8 land exactly where the report put them
    exact = [c for c in range(18) if c not in (5, 7)]
    assert np.array_equal(got[:, exact], TABLE4[:, exact]), got
    assert got[1, 13] == 2208 and got[3, 13] == 1  # D5: 2208 in state 2, one in state 4
    assert got[0, 5] + got[2, 5] == 828 and got[0, 5] >= 800  # U6 mostly in state 1, as the report
    assert got[2, 7] + got[3, 7] == 49  # U8 split between states 3 and 4, as the report
    print(f"Table 4 agreement {agree} / 8386; U6 {got[:, 5]}, U8 {got[:, 7]}")

    # The check discriminates: without the sign mask (the transition applied for every j and the
    # initial distribution for every j, i.e. the plain multinomial HMM of hmm-multinom.stan at the
    # same expanded parameters) the table falls apart.
    p_1k, A = table8_flat(draw)
    plain = oracle.gqs("hmm-multinom", {"K": 4, "L": 9, "x": x},
                       {"p_1k": p_1k, "A_ij": A, "phi_k": draw["phi_k"]}, pars=["alpha_tk"])
    nomask = table_agreement(tabulate(feat, np.argmax(plain["alpha_tk"][0], axis=1) + 1))
    print(f"no-mask agreement {nomask} / 8386")
    assert nomask < 5000, nomask


def test_table4_point_oracle_vs_numpy_transcription(oracle):
    """The same real-data request through the independent pure-Python transcription
    (tests/oracle_numpy.py): every in-sample and OOS output of the lite model agrees with the
    C oracle, so the Table 4 pin above covers both restatements."""
    import oracle_numpy as onp
    from tolerances import compare
    legs, ins, oos = _gto_legs(oracle)
    x, sign, xo, so = legs["x"][ins], legs["sign"][ins], legs["x"][oos], legs["sign"][oos]
    data = {"K": 4, "L": 9, "x": x, "sign": sign, "x_oos": xo, "sign_oos": so}
    draw = table8_draw()
    pars = ["loglik", "unalpha_tk", "alpha_tk", "unalpha_tk_oos", "alpha_tk_oos", "zstar_t", "logp_zstar"]
    got = oracle.gqs("hhmm-tayal2009-lite", data, draw, pars=pars)
    ref = onp.tayal_lite(x.size, x, sign, xo.size, xo, so, draw["p_11"][0], draw["A_row"][0], draw["phi_k"][0])
    for name in pars:
        compare(name, np.asarray(got[name])[0], np.asarray(ref[name]))


def test_reference_task_list_has_204_windows(oracle):
    """12 stocks x (22 - 6 + 1) windows (test-strategy.R:45-59); the first
    task's in/out-of-sample data through the oracle's extractor."""
    tasks = W.window_tasks(DATA)
    assert len(tasks) == 204 and len({t["stock"] for t in tasks}) == 12
    w = W.load_window(tasks[0], extract=oracle.extract_features)
    assert w["x"].size > 1000 and w["x_oos"].size > 100
    for k in ("x", "x_oos"):
        assert w[k].min() >= 1 and w[k].max() <= 9
    for k in ("sign", "sign_oos"):
        assert set(np.unique(w[k])) <= {1, 2}
