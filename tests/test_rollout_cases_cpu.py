"""The conditions tests/test_gpu_rollout_edges.py rests on, checked without a device: the horizon table covers the host scheduler's
case analysis (asserted on run_length, the rule restated in tests/rollout_cases.py), the position sets are what their names say
(oracle), the fp64 reference alone leaves at most a tenth of the sweep's trials out as near ties, and the reference's one-turn rotated
trial is the net's value of the greedy afterstate with the turn bit of the side now to move."""
import numpy as np
import pytest

import outcome_ref as OR
import rollout_cases as RC
import rollout_ref as R
import search_ref as S
from oracle import oracle as O


@pytest.fixture(scope="module")
def W():
    w = RC.weights()
    assert w.size == O.N_PARAMS
    return w


def test_the_rules():
    assert [RC.run_length(0, r) for r in (False, True)] == [8, 8]
    assert [RC.run_length(M, False) for M in range(1, 18)] == [1, 2, 3, 4, 5, 6, 7, 8, 3, 5, 1, 6, 1, 7, 5, 8, 1]
    assert [RC.run_length(M, True) for M in range(1, 18)] == [1, 1, 2, 3, 4, 5, 6, 7, 8, 3, 5, 1, 6, 1, 7, 5, 8]
    assert all(RC.run_length(M, r, plies=2) == 1 for M in range(0, 30) for r in (False, True))
    for M in range(1, 60):                               # the rule's purpose: every seated trial's M-th turn ends a run
        for rot in (False, True):
            Rn, D = RC.run_length(M, rot), M - rot
            assert 1 <= Rn <= 8 and (D < 1 or D % Rn == 0) and not any(D >= 1 and D % q == 0 for q in range(Rn + 1, 9))
    assert [RC.default_lanes(N) for N in (1, 255, 256, 257, 740, 65536, 65537, 10 ** 6)] == [256, 256, 256, 512, 768, 65536, 65536, 65536]
    assert [RC.fan_size(T) for T in (1, 5, 35, 36, 37, 73)] == [1, 5, 35, 36, 36, 36]
    d = RC.first_dice(73)
    assert d[:36].tolist() == [[a, b] for a in range(1, 7) for b in range(1, 7)]
    assert (d[36:72] == d[:36]).all() and d[72].tolist() == [1, 1] and d.dtype == np.int32


def test_horizons_cover_the_schedule():
    H = RC.HORIZONS
    assert len(H) == len(set(H)) and 16 <= len(H) <= 20 and all(1 <= M <= 25 for M, _ in H)
    assert {RC.run_length(M, r) for M, r in H} == set(range(1, 9))
    D = lambda M, r: M - (1 if r else 0)
    prime = lambda n: n > 1 and all(n % q for q in range(2, n))
    assert (1, True) in H and D(1, True) < 1 and (1, False) in H
    for rot in (False, True):
        assert any(r == rot and prime(D(M, r)) and D(M, r) > 8 and RC.run_length(M, r) == 1 for M, r in H), rot
        for runs in (2, 3):                              # exactly two and three full runs of 8
            assert any(r == rot and D(M, r) == 8 * runs and RC.run_length(M, r) == 8 for M, r in H), (rot, runs)
    assert set(RC.REF_HORIZONS) <= set(H) and set(RC.REF_HORIZONS) == {(1, True), (1, False), (2, True), (11, False)}
    assert RC.SWEEP_T > 36 and RC.SWEEP_T % 36 and RC.SWEEP_OFFSET > 0


def _no_move(s, player):
    st = O.State.from28(s, player)
    if any(O.legal_moves(st, player, die) for die in range(1, 7)):
        return False
    for a in range(1, 7):
        for b in range(1, 7):
            c = S.distinct_afterstates(s, player, a, b)   # (a doubles roll without a move: one empty sequence, the board itself)
            if not (len(c) == 0 or (len(c) == 1 and (c[0] == s).all())):
                return False
    return True


def test_census_of_the_positions(W):
    st, tu, kind = RC.positions()
    assert len(st) == 20 and kind.tolist() == ["start"] + ["g10"] * 6 + ["forced"] * 10 + ["over"] * 2 + ["bar"]
    assert (kind[:RC.N_LIVE] != "forced").all() and set(kind[:RC.N_LIVE]) == {"start", "g10"}
    pts = OR.points_many(st)
    assert ((pts != 0) == (kind == "over")).all() and pts[kind == "over"].tolist() == [1, -2]
    assert ((st[:, :24] * (st[:, :24] > 0)).sum(1) + st[:, 24] + st[:, 26] == 15).all()
    assert ((-st[:, :24] * (st[:, :24] < 0)).sum(1) + st[:, 25] + st[:, 27] == 15).all()
    assert set(tu.tolist()) == {0, 1} and len({s.tobytes() for s in st}) == 20
    # the bar position: a pass for every ordered pair, for the side that is to move
    b = int(np.nonzero(kind == "bar")[0][0])
    assert st[b][24] == 1 and tu[b] == 0 and _no_move(st[b], 0) and not _no_move(OR.START, 0)
    # the forced positions end on their first turn for the rolls forced_positions() names: every roll, the last one for a roll with a 1
    fst, ftu, fpts, names = OR.forced_positions()
    f0 = int(np.nonzero(kind == "forced")[0][0])
    assert (st[f0:f0 + 10] == fst).all() and (tu[f0:f0 + 10] == ftu).all()
    for p in range(10):
        for i in range(36):
            d1, d2 = RC.first_dice(36)[i]
            v, turns, trunc, near, board = OR.trial_with_board(W, fst[p], ftu[p], RC.SEED, 1000 + i, i, 1, True)
            ends = p < 9 or d1 == 1 or d2 == 1
            assert not near and turns == 1 and trunc == (not ends), (names[p], i)
            assert OR.points(board) == (fpts[p] if ends else 0), (names[p], i)
    # the start position and the fixture boards play on after any first roll
    for p in range(RC.N_LIVE):
        for i in range(36):
            assert R.trial(W, st[p], tu[p], RC.SEED, i, i, 1, True)[2], (p, i)


def test_census_of_the_seat_loop_batch(W):
    st, tu, kind = RC.skip_heavy()
    assert len(st) == 40 and (kind[3::4] != "over").all() and (kind[3::4] != "forced").all()
    skipped = (kind == "over") | (kind == "forced")
    assert skipped.sum() >= 30 and skipped.mean() >= 0.75 and (kind == "late").sum() == 9 and (kind == "forced8").sum() == 1
    pts = OR.points_many(st)
    assert ((pts != 0) == (kind == "over")).all()
    for p in np.nonzero(skipped)[0]:
        v, turns, points = RC.known_result(st[p], kind[p])
        for i in (0, 7, 35):                             # (every pair: test_census_of_the_positions)
            got = OR.trial_with_board(W, st[p], tu[p], RC.SEED, 50 + i, i, 0, True)
            assert (got[0], got[1], OR.points(got[4])) == (v, turns, points), (p, i)
    lst, ltu = RC.late_boards(9)
    assert (lst[:, 26:28] >= 8).all() and (lst[:, 26:28] <= 10).all() and (OR.points_many(lst) == 0).all()
    for p in range(9):                                   # live: no first roll ends the game
        assert all(R.trial(W, lst[p], ltu[p], RC.SEED, i, i, 1, True)[2] for i in range(36)), p


@pytest.mark.parametrize("M,rotate", RC.REF_HORIZONS)
def test_near_tie_cap_of_the_reference(M, rotate):
    """The GPU sweep compares its trials with the reference off near ties and asks for 90 % of them: the reference alone must leave no
    more than 10 % out, for the exact calls of the sweep."""
    ref = RC.sweep_reference(M, rotate)
    assert ref["near_tie"].shape == (RC.N_LIVE, RC.SWEEP_T)
    share = float(ref["near_tie"].mean())
    print(f"horizon ({M}, {rotate}): near ties in {share:.4f} of {ref['near_tie'].size} trials, "
          f"{int(ref['truncated'].sum())} truncated")
    assert share <= 0.10
    assert (ref["turns"][ref["truncated"]] == M).all() and ref["truncated"].any()
    if M <= 2:                                           # (no live position ends within two turns)
        assert ref["truncated"].all()


def test_reference_one_turn_rotated_trial(W):
    """M = 1 with rotation: the net's value of the greedy afterstate of pair i % 36 with the turn bit of the side now to move -- on the
    live positions and on the bar position, whose afterstate is the board itself."""
    st, tu, kind = RC.positions()
    for p in list(range(RC.N_LIVE)) + [int(np.nonzero(kind == "bar")[0][0])]:
        mover = int(tu[p])
        for i in (0, 7, 20, 35, 36, 72):
            d1, d2 = RC.first_dice(i + 1)[i]
            assert (d1, d2) == (1 + (i % 36) // 6, 1 + (i % 36) % 6)
            cand = S.distinct_afterstates(st[p], mover, int(d1), int(d2))
            if len(cand):
                v = S.net(W, cand, mover)
                after = cand[int(np.argmax(v) if mover == 0 else np.argmin(v))]
            else:
                after = st[p]
            val, turns, trunc, _ = R.trial(W, st[p], mover, RC.SEED, 500 + i, i, max_plies=1, rotate=True)
            assert trunc and turns == 1 and val == float(S.net(W, after, 1 - mover)[0]), (p, i)
            assert val != float(S.net(W, after, mover)[0])
