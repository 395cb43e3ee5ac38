"""GPU: the phased sweep's running row pointers (RowCursor, csrc/hhmm_device.h)
at every place where a cursor's walk and the rows it may touch part ways.

vfb_kernel reaches its per-step rows -- gamma's K rows, zstar, the per-block
checkpoint / packed-symbol / back-pointer records in the backward sweep, x's
rows, the packed-symbol row and the back-pointer word rows in the Viterbi's
group loop -- by stepping a wave-uniform pointer one row per step.  A cursor
moves on every step of the wave, also where some lanes' access is predicated
off, and may stand before row 0 or past the last row; the cases below are the
shapes where that matters:

  edges    T on both sides of the 4-step back-pointer word, the 8-step chunk,
           the 16-step block and the two-chunk group loop (which starts at
           chunk 1 and needs its prefetched group inside x: T >= 40 runs it
           once), with P = 1 (63 tail lanes clamped to pair 0), 63, 65 (two
           waves) and 257 (two workgroups);
  ragged   lengths 1, 7, 16, 17 and 40 inside one wave: the wave's blocks are
           all partial for some lane, the cursors walk 48 rows for every lane,
           and a series of length 1 sits next to one of length T_max;
  dense    an emission entry of 2^-45 in every draw of wave 0 fails the
           renormalisation gate, so vfb_dense_kernel runs that wave's backward
           sweep (the same cursors) beside wave 1 in vfb_kernel;
  4 GiB    140000 pairs x T = 1000 through the device entry: gamma is 4.48 GB,
           state 3's rows cross byte offset 2^32 at t = 834 / 835, and the
           zstar and record rows pass 2^31 bytes -- 64-bit cursor arithmetic.

Every case asserts the phased plan of its own request first (tests/hot_plan.py)
and compares with the CPU oracle at tests/tolerances.py: loglik and gamma_tk
within tolerance, zstar_t, logp_zstar and pair_status exact."""
import functools

import numpy as np
import pytest

import gate_inputs
from hhmm_amd import synth
from hot_plan import C2, SCHEDULE_FLAGS, SCHEDULE_PLAN, assert_plan, plan_of, run_planned
from tolerances import compare_all

pytestmark = pytest.mark.gpu

MODEL, K, L = "hmm-multinom", 4, 9
FLAGS, PLAN = SCHEDULE_FLAGS["phased"], SCHEDULE_PLAN["phased"]
EDGE_T = [1, 2, 15, 16, 17, 31, 32, 33, 47]
EDGE_P = [1, 63, 65, 257]
RAGGED_T = [40, 1, 7, 16, 17]        # T_max first: pair 0 has 40 steps, pair 1 one


@functools.lru_cache(maxsize=None)
def uniform(P, T):
    return synth.hmm_multinom(N=P, S=P, T=T, K=K, L=L)


@pytest.mark.parametrize("P", EDGE_P)
@pytest.mark.parametrize("T", EDGE_T)
def test_block_and_word_edges(engine, oracle, T, P):
    data, draws = uniform(P, T)
    run_planned(engine, oracle, MODEL, data, draws, C2, FLAGS, "zip", PLAN, tag=f"T{T}-P{P}")


def test_group_loop_runs_with_cursors_then_hands_over(engine, oracle):
    """T = 40 is the first length at which the Viterbi's group loop runs (chunks 1, 2 with chunks 3, 4 prefetched
    through the x cursor, which ends on row 40 = T_max, one past the last); T = 47 and 57 leave it one and three
    chunks, partial ones included, for the clamped chunk-by-chunk loop."""
    for T in (40, 57):
        data, draws = uniform(65, T)
        run_planned(engine, oracle, MODEL, data, draws, C2, FLAGS, "zip", PLAN, tag=f"T{T}")


def test_ragged_lengths_inside_one_wave(engine, oracle):
    data, draws = synth.hmm_multinom(N=70, S=70, T=40, K=K, L=L)
    Tn = np.array([RAGGED_T[i % len(RAGGED_T)] for i in range(70)], dtype=np.int32)
    assert Tn[0] == 40 and Tn[1] == 1 and Tn[:64].min() < Tn[:64].max() and Tn[64:].max() == 40
    data["T"] = Tn
    run_planned(engine, oracle, MODEL, data, draws, C2, FLAGS, "zip", PLAN, tag="ragged")


def test_dense_wave(engine, oracle):
    """Wave 0 (draws 0..63) holds phi[.., state 1, symbol L] = 2^-45 < 2^-39: its backward sweep runs in
    vfb_dense_kernel with per-step renormalisation; wave 1 (6 pairs) stays in vfb_kernel."""
    data, draws = synth.hmm_multinom(N=70, S=70, T=33, K=K, L=L)
    draws = {k: np.array(v, dtype=np.float64) for k, v in draws.items()}
    gate_inputs._set_column(draws["phi_k"][:64, 1, :], L - 1, 2.0 ** -45)
    assert draws["phi_k"][0, 1, L - 1] == 2.0 ** -45
    b = gate_inputs.gate_b(draws)
    assert (b[:64] < gate_inputs.BOUND).all() and (b[64:] >= gate_inputs.BOUND).all()
    assert (np.asarray(data["x"])[:64] == L).any(), "the rare symbol occurs in the dense wave"
    run_planned(engine, oracle, MODEL, data, draws, C2, FLAGS, "zip", PLAN, tag="dense")


def test_rows_past_4_gib(engine, oracle):
    import torch
    from devrun import DeviceRequest
    U, P, T = 2048, 140000, 1000
    data, draws = synth.hmm_multinom(N=U, S=U, T=T, K=K, L=L)
    tile = np.arange(P) % U
    big = {"K": K, "L": L, "x": np.asarray(data["x"])[tile]}
    big_draws = {k: np.asarray(v)[tile] for k, v in draws.items()}
    got_plan = plan_of(engine, MODEL, K, L, P, T, C2, FLAGS)
    assert {k: got_plan[k] for k in PLAN} == dict(PLAN), got_plan
    assert K * T * P * 8 > 2 ** 32 and (3 * T + 834) * P * 8 < 2 ** 32 <= (3 * T + 835) * P * 8
    run = DeviceRequest(engine, MODEL, big, big_draws, C2, pairing="zip", flags=FLAGS)
    assert run.run() >= 0
    assert int((run.status != 0).sum()) == 0
    # 48 of the unique pairs: pair 0, the one pair P - 1 is a copy of, and 46 spread over the rest
    last = (P - 1) % U
    uniq = sorted({0, last} | set(range(17, U, U // 46)))[:48]
    assert len(uniq) == 48 and 0 in uniq and last in uniq
    sub = {"K": K, "L": L, "x": np.asarray(data["x"])[uniq]}
    sub_draws = {k: np.asarray(v)[uniq] for k, v in draws.items()}
    ref = oracle.gqs(MODEL, sub, sub_draws, pars=C2, pairing="zip", return_status=True, nthreads=8)
    # each in the first tile, one in the middle and the last whole tile; pair P - 1 among them
    for shift in (0, (P // U // 2) * U, (P // U - 1) * U, (P - 1) - last):
        idx = np.array(uniq) + shift
        if shift == (P - 1) - last:
            idx = idx[idx < P]
            assert idx[-1] == P - 1 or (P - 1) in idx
        keep = [uniq.index(int(i) % U) for i in idx]
        got = {k: run.host_pairs(k, idx) for k in C2}
        got["pair_status"] = run.status[torch.as_tensor(idx, device=run.dev)].cpu().numpy()
        compare_all(got, {k: np.asarray(ref[k])[keep] for k in C2 + ["pair_status"]}, C2 + ["pair_status"])
    # every copy of a unique pair gives the same bits, on both sides of the crossing
    g = run.out["gamma_tk"]
    assert bool(torch.equal(g[:, :, :U], g[:, :, (P // U - 1) * U:(P // U) * U]))
    z = run.out["zstar_t"]
    assert bool(torch.equal(z[:, :U], z[:, (P // U - 1) * U:(P // U) * U]))
    assert bool(torch.equal(g[:, :, P - 1], g[:, :, last])) and bool(torch.equal(z[:, P - 1], z[:, last]))
