"""The five "statistics per (series, draw) pair" entries past one workgroup and one chunk group.

hhmm_estep, hhmm_expected_stats, hhmm_draw_stats, hhmm_draw_stats_gauss and hhmm_estep_io are lane-per-pair
kernels that address a pair by gwave = blockIdx.x * nw + wave, carve a per-wave LDS slab at wave * elems
and (all but the IOHMM E-step) run fb_kernel's grouped forward loop.  Their own test files cover every K
and L, the chunk edges and the abnormal pairs at one small batch geometry; this module runs P = 577 pairs
(tests/batch_geometry.py: a few base pairs gathered wave by wave) so that

  * blockIdx.x > 0 meets wave > 0 in every LDS class (4, 3, 2 and 1 waves per workgroup), the last pair has
    a wave of its own and, at 4 waves, two waves of the last workgroup are spare lanes only;
  * ragged waves go through the group loop: nfull = D (one group, D + 2 tail chunks) and nfull = D + 1 (the
    hand-over inside the full chunks), the shorter lanes reading checkpoint rows past their last chunk;
  * a wave of every length from 1 up, with a NaN draw, an impossible series and (device entry) an invalid
    series, sits between them, and a wave of one pair 64 times.

Each case asserts
  (a) every one of the 577 results against the reference of its base pair under the entry's own rule:
      1e-9 relative to max(1, |reference|), NaN and infinities in the same places; the two draw entries,
      as in their own files, against the statistics of the engine's own z_ffbs on the same batch, counts
      exact (s1_k / s2_k of the Gaussian one within T 2^-52 sum |x_t| / sum x_t^2);
  (b) position independence, bit for bit: every copy of a base pair equals that pair's result when the entry
      runs on the base pairs alone (so every copy equals every other);
  (c) the device entry returns the host entry's bits, and pair_status is PAIR_INVALID_DATA exactly on the
      copies of the invalid base pair.

Waves per workgroup (the id of a case ends in it; test_cases_state_their_waves pins them to the sizing
functions as tests/batch_geometry.py restates them), and what was measured when this module was written
(MI355X; the worst (a) discrepancy of each case is printed before it is asserted):

  estep           hmm-multinom (K, L) = (4, 9) 4 waves, (4, 12) 3, (4, 16) 2, (8, 16) 1: 5.1e-14, 1.4e-13,
                  1.3e-13, 3.8e-14.  hmm K = 3, 6, 7, 8, always 4 waves (K = 7, 8: xi in LDS on every wave):
                  3.3e-13, 3.0e-13, 9.5e-14, 1.5e-13.  (b) held bit for bit in all eight.
  expected_stats  semisup (4, 9) 4 waves, (6, 8) 3, (4, 16) 2, (8, 16) 1: 6.5e-14, 4.5e-15, 8.3e-14, 1.2e-14.
                  Tayal (4, 9) 4 waves, (4, 16) 2: 3.1e-14, 3.5e-14.  (b) held bit for bit in all six, the
                  sign-class arm of the uniform waves against the per-lane masks included.
  draw_stats      hmm-multinom, semisup and Tayal at K = 4 with L = 9 (4 waves), 16 (3), 25 (2), 40 (1), and
                  semisup (6, 4) 4 waves: every count equal, loglik equal to the engine's own in every bit
                  (discrepancy 0) in all thirteen.  (b) held bit for bit.
  draw_stats_gauss  K = 3 (4 waves), 7 (2 waves), 8 (1 wave, D = 2) -- draw_stats_gauss_waves picks of 4, 2 and
                  1 waves the size that lets a CU hold the most, which is not 4 at K = 7 and 8: counts equal,
                  loglik discrepancy 0, s1_k / s2_k at most 0.094 of their bound.  (b) held bit for bit.
  estep_io        iohmm-reg (K, M) = (4, 4) 4 waves, (6, 3) 3, (7, 4) 2, (2, 7) 3, (3, 6) 2, (5, 8) 1 with gw
                  in the slab: 3.4e-15, 1.8e-15, 2.7e-15, 9.9e-15, 4.9e-15, 6.9e-15.  Mixtures (K, L, M) =
                  iohmm-mix (3, 2, 3) 4 waves, iohmm-hmix (4, 3, 4) 3, iohmm-hmix-lite (5, 2, 5) 2 with gw in
                  the slab, iohmm-mix (4, 8, 7) 1: 1.4e-15, 1.9e-15, 2.0e-15, 3.4e-15.  (b) held bit for bit.

A workgroup always launches its full complement of waves, and lanes past the last pair redo pair P - 1.  So
in a 4-wave class the small batches of the entries' own files do run waves 1-3 as spare lanes, and a slab
offset that lets a spare wave write through a live wave's slab is seen there already; what those files
cannot see is an offset wrong in a class none of their shapes is in (the 3-wave class of estep and
expected_stats), one that only separates live waves, a wrong gwave past the first workgroup, and anything
in the group loop of draw_stats at K <= 4.
"""
import functools

import numpy as np
import pytest

import batch_geometry as bg
import hhmm_amd
from hhmm_amd import _abi

TOL = 1e-9
P = bg.P_BATCH
MULTINOM, SEMISUP, TAYAL = "hmm-multinom", "hmm-multinom-semisup", "hhmm-tayal2009"


def _case(entry, model, waves, K, L=0, M=0):
    shape = "K%d" % K + ("-L%d" % L if L else "") + ("-M%d" % M if M else "")
    return pytest.param(entry, model, K, L, M, waves, id="%s-%s-%s-%dw" % (entry, model, shape, waves))


CASES = [
    # estep: hmm-multinom by L * ceil(K / 2): <= 20: 4 waves, <= 26: 3, <= 40: 2, <= 80: 1; hmm always 4,
    # K = 7 and 8 with xi in LDS on every wave
    _case("estep", MULTINOM, 4, 4, 9), _case("estep", MULTINOM, 3, 4, 12), _case("estep", MULTINOM, 2, 4, 16),
    _case("estep", MULTINOM, 1, 8, 16),
    _case("estep", "hmm", 4, 3), _case("estep", "hmm", 4, 6), _case("estep", "hmm", 4, 7), _case("estep", "hmm", 4, 8),
    # expected_stats: the same rule
    _case("expected_stats", SEMISUP, 4, 4, 9), _case("expected_stats", SEMISUP, 3, 6, 8),
    _case("expected_stats", SEMISUP, 2, 4, 16), _case("expected_stats", SEMISUP, 1, 8, 16),
    _case("expected_stats", TAYAL, 4, 4, 9), _case("expected_stats", TAYAL, 2, 4, 16),
    # draw_stats: 1024 L ceil(K / 2) + 256 (L K + K K) bytes per wave against 160 KiB
    *[_case("draw_stats", m, w, 4, L) for m in (MULTINOM, SEMISUP, TAYAL)
      for L, w in ((9, 4), (16, 3), (25, 2), (40, 1))],
    _case("draw_stats", SEMISUP, 4, 6, 4),
    # draw_stats_gauss: of 4, 2 and 1 waves the size that lets a CU hold the most; K = 8 takes D = 2
    _case("draw_stats_gauss", "hmm", 4, 3), _case("draw_stats_gauss", "hmm", 2, 7),
    _case("draw_stats_gauss", "hmm", 1, 8),
    # estep_io: the slab of eio_slab_elems double2 per lane; (5, 8) and (5, 2, 5) keep gw in the slab
    _case("estep_io", "iohmm-reg", 4, 4, M=4), _case("estep_io", "iohmm-reg", 3, 6, M=3),
    _case("estep_io", "iohmm-reg", 2, 7, M=4), _case("estep_io", "iohmm-reg", 3, 2, M=7),
    _case("estep_io", "iohmm-reg", 2, 3, M=6), _case("estep_io", "iohmm-reg", 1, 5, M=8),
    _case("estep_io", "iohmm-mix", 4, 3, 2, 3), _case("estep_io", "iohmm-hmix", 3, 4, 3, 4),
    _case("estep_io", "iohmm-hmix-lite", 2, 5, 2, 5), _case("estep_io", "iohmm-mix", 1, 4, 8, 7),
]


@functools.lru_cache(maxsize=None)
def base_of(entry, model, K, L, M):
    """The base pairs of a case and the layout of its batch: made once, shared, read-only."""
    base = bg.make_base(entry, {"model": model, "K": K, "L": L, "M": M}, seed=100 * K + 10 * L + M)
    idx = bg.layout(P, bg.base_classes(base))
    for v in list(base["data"].values()) + list(base["draws"].values()) + [base["u"], base["T"], idx]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return base, idx


@functools.lru_cache(maxsize=None)
def base_reference(entry, model, K, L, M):
    """The numpy reference of the base pairs (the three expected-statistics entries): once per case."""
    ref = bg.reference(base_of(entry, model, K, L, M)[0])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def names_of(stats):
    return [k for k in stats if k not in ("status", "pair_status")]


# ---------------------------------------------------------------- CPU: the harness

SMALL = {"estep": {"model": "hmm", "K": 5}, "expected_stats": {"model": TAYAL, "K": 4, "L": 5},
         "draw_stats": {"model": SEMISUP, "K": 4, "L": 5}, "draw_stats_gauss": {"model": "hmm", "K": 3},
         "estep_io": {"model": "iohmm-mix", "K": 3, "L": 2, "M": 3}}


@pytest.mark.parametrize("entry", bg.ENTRIES)
def test_gather_commutes_with_the_reference(oracle, entry):
    """reference(gather(base, idx)) == reference(base)[idx]: the gather means what the GPU tests assume."""
    base = bg.make_base(entry, SMALL[entry], seed=3)
    idx = np.random.Generator(np.random.Philox(key=11)).integers(0, base["B"], size=12)
    idx[:3] = [base["roles"]["nan"], base["B"] - 1, base["roles"]["nan"]]           # repeats, the abnormal ones
    whole = bg.reference(base, oracle.gqs)
    part = bg.reference(bg.gather(base, idx), oracle.gqs)
    assert set(part) == set(whole)
    for name, v in whole.items():
        assert part[name].shape == (12,) + v.shape[1:], name
        assert np.array_equal(part[name], v[idx], equal_nan=True), name
    # the abnormal pairs are what they claim, the others finite
    nan = np.arange(base["B"]) == base["roles"]["nan"]
    imp = np.arange(base["B"]) == base["roles"].get("impossible", -1)
    for name, v in whole.items():
        flat = v.reshape(base["B"], -1)
        assert np.isnan(flat[nan]).all() and np.isfinite(flat[~nan & ~imp]).all(), name
        assert (flat[imp] == -np.inf).all() if name == "loglik" else np.isnan(flat[imp]).all(), name


@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("D", [2, 4])
def test_layout_meets_the_wave_conditions(C, D):
    lens, roles = bg.base_lengths(C, D)
    assert lens.size <= 32 and lens.max() == 2 * D * C + C + 3
    classes = bg.classes_of(lens, C, D, roles.values())
    idx = bg.layout(P, classes)
    assert idx.shape == (P,) and idx.min() >= 0 and idx.max() < lens.size
    waves = [lens[idx[64 * j:64 * j + 64]] for j in range(10)]
    assert [w.size for w in waves] == [64] * 9 + [1]
    kinds = set()
    for j, w in enumerate(waves[:9]):
        members = set(idx[64 * j:64 * j + 64].tolist())
        if j % 3 == 0:
            assert set(w.tolist()) <= set(bg.long_lengths(C, D)) and not members & set(roles.values())
            assert w.min() >= D * C and w.max() > w.min()                         # nfull >= D, ragged
            kinds.add("handover" if (w.min() // C) % D else "group")
            if (w.min() // C) % D == 0:                                           # more than one tail chunk
                assert -(-w.max() // C) - w.min() // C > 1
        elif j % 3 == 1:
            assert members == set(range(lens.size))                               # everything
            assert w.min() == 1 and {1, 2, C, C + 1} <= set(w.tolist())
        else:
            assert len(members) == 1 and not members & set(roles.values())
            kinds.add("uniform")
    assert kinds == {"group", "handover", "uniform"}
    # every abnormal pair only in class-1 waves
    for j in range(10):
        if j % 3 != 1:
            assert not set(idx[64 * j:64 * j + 64].tolist()) & set(roles.values())


def test_last_pair_has_a_wave_of_its_own():
    """P = 577 = 9 * 64 + 1; and what that means for a workgroup of 4, 3, 2 and 1 waves."""
    assert P % 64 == 1 and (P - 1) // 64 == 9 and (P - 2) // 64 == 8
    for nw, full, rest in ((4, 2, 65), (3, 3, 1), (2, 4, 65), (1, 9, 1)):
        groups = -(-P // (64 * nw))
        assert groups == full + 1 and P - 64 * nw * full == rest


@pytest.mark.parametrize("entry,model,K,L,M,waves", CASES)
def test_cases_state_their_waves(entry, model, K, L, M, waves):
    assert bg.waves_per_workgroup(entry, model, K, L, M) == waves
    if entry == "estep_io":
        assert bg.gw_in_slab(K, M) == ((K, M) in ((5, 8), (5, 5)))


def test_every_entry_meets_every_lds_class_it_has():
    seen = {}
    for c in CASES:
        entry, _model, _K, _L, _M, waves = c.values
        seen.setdefault(entry, set()).add(waves)
    assert seen == {"estep": {1, 2, 3, 4}, "expected_stats": {1, 2, 3, 4}, "draw_stats": {1, 2, 3, 4},
                    "draw_stats_gauss": {1, 2, 4}, "estep_io": {1, 2, 3, 4}}


# ---------------------------------------------------------------- GPU

def host(engine, req):
    e, m, d, w, u = req["entry"], req["model"], req["data"], req["draws"], req["u"]
    kw = dict(lib=engine, return_status=True)
    if e == "estep":
        return hhmm_amd.estep(m, d, w, "zip", **kw)
    if e == "expected_stats":
        return hhmm_amd.expected_stats(m, d, w, "zip", **kw)
    if e == "draw_stats":
        return hhmm_amd.draw_stats(m, d, w, u, "zip", **kw)
    if e == "draw_stats_gauss":
        return hhmm_amd.draw_stats_gauss(d, w, u, "zip", **kw)
    return hhmm_amd.estep_io(m, d, w, "zip", **kw)


def device(engine, req):
    import stats_devrun as sd
    from test_estep_io import DeviceEstepIo
    e, m, d, w, u = req["entry"], req["model"], req["data"], req["draws"], req["u"]
    if e == "estep":
        dv = sd.DeviceEstep(engine, m, d, w, "zip")
    elif e == "expected_stats":
        dv = sd.DeviceExpect(engine, m, d, w, "zip")
    elif e == "draw_stats":
        dv = sd.DeviceDrawStats(engine, m, d, w, u, "zip")
    elif e == "draw_stats_gauss":
        dv = sd.DeviceDrawStatsGauss(engine, d, w, u, "zip")
    else:
        dv = DeviceEstepIo(engine, m, d, w, "zip")
    assert dv.run() == 0
    return dv.stats()


def against_reference(engine, base, idx, big, got):
    """(a); returns the worst relative discrepancy seen."""
    from test_estep import worst
    entry = base["entry"]
    if entry in ("estep", "expected_stats", "estep_io"):
        ref = base_reference(entry, base["model"], base["K"], base["L"], base["M"])
        want = {k: v[idx] for k, v in ref.items()}
        assert set(want) == set(names_of(got))
        w = worst(got, want)
        assert w <= TOL, (entry, w)
        return w
    gqs = functools.partial(hhmm_amd.gqs, lib=engine)
    want = bg.reference(big, gqs)
    ll = want.pop("loglik")
    if entry == "draw_stats":
        import test_draw_stats as t
        t.compare(got, want, ll, entry)
    else:
        import test_draw_stats_gauss as t
        b1, b2 = t.bounds(big["data"], "zip", P, P)
        t.compare(got, want, ll, b1, b2, entry)
    return worst({"loglik": got["loglik"]}, {"loglik": ll})


@pytest.mark.gpu
@pytest.mark.parametrize("entry,model,K,L,M,waves", CASES)
def test_gpu_batch_geometry(engine, entry, model, K, L, M, waves):
    base, idx = base_of(entry, model, K, L, M)
    roles = base["roles"]
    big = bg.gather(base, idx)
    alone = host(engine, base)
    got = host(engine, big)
    names = names_of(got)
    assert alone["status"] == 0 and got["status"] == 0
    assert not alone["pair_status"].any() and not got["pair_status"].any()

    # (a) every pair against the reference of its base pair
    w = against_reference(engine, base, idx, big, got)
    print("%s %s K=%d L=%d M=%d (%d waves): worst (a) discrepancy %.3g" % (entry, model, K, L, M, waves, w))
    # the abnormal pairs show what the entry's own tests require of them; their neighbours are finite
    nan, imp = idx == roles["nan"], idx == roles.get("impossible", -1)
    assert nan.sum() >= 9 and (imp.sum() >= 9 or "impossible" not in roles)
    for name in names:
        flat = got[name].reshape(P, -1)
        assert np.isnan(flat[nan]).all() and np.isfinite(flat[~nan & ~imp]).all(), name
        assert (flat[imp] == -np.inf).all() if name == "loglik" else np.isnan(flat[imp]).all(), name

    # (b) position independence, bit for bit
    for name in names:
        assert bg.same_bits(got[name], alone[name][idx]), (name, "differs from the base pairs run alone")

    # (c) the device entry is the host entry; it flags exactly the copies of the invalid pair
    dreq, hit = bg.device_request(base, idx)
    assert hit.sum() >= 9
    dev = device(engine, dreq)
    assert (dev["pair_status"][hit] == _abi.PAIR_INVALID_DATA).all() and not dev["pair_status"][~hit].any()
    for name in names:
        assert bg.same_bits(dev[name][~hit], got[name][~hit]), (name, "device entry differs from the host entry")
