"""The 2-ply expectimax search on the MI355X (bgamd_env_step_search) against the fp64 CPU reference (tests/search_ref.py): kept
candidates, 1- and 2-ply values and the choice at full width, the top-K filter, chunk invariance and determinism, the flags, and
the strength of 2-ply over 1-ply in head-to-head play."""
import math
import os

import numpy as np
import pytest

import search_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _greedy_positions(bg, weights, n, seed):
    """n positions reached by a seeded greedy run from the start position (lanes stopped at different plies)."""
    env = bg.VecGame(max(n, 64), seed=seed)
    env.load_weights(weights)
    st, tu = [], []
    for k in range(n):
        env.step_greedy()
        st.append(env.states()[k].cpu().numpy()); tu.append(int(env.turns()[k]))
    env.close()
    return np.array(st, np.int32), np.array(tu, np.int32)


def _lanes(bg, golden_dir, weights, n_greedy, n_g10, seed):
    st1, tu1 = _greedy_positions(bg, weights, n_greedy, seed)
    g10 = np.load(os.path.join(golden_dir, "g10_arbitrary_boards.npz"))
    idx = np.arange(n_g10) * (len(g10["boards"]) // n_g10)
    st2, tu2 = g10["boards"][idx], g10["dice"][idx, 0]
    rng = np.random.RandomState(seed)
    dice1 = rng.randint(1, 7, (n_greedy, 2))
    st = np.concatenate([st1, st2]).astype(np.int32)
    tu = np.concatenate([tu1, tu2]).astype(np.int32)
    dice = np.concatenate([dice1, g10["dice"][idx, 1:]]).astype(np.int32)
    return st, tu, dice


def _setup(bg, weights, st, tu, dice, n=None, slot_weights=None):
    env = bg.VecGame(n or len(st))
    env.load_weights(weights)
    if slot_weights is not None:
        env.load_weights(slot_weights, slot=1)
    if n and n > len(st):
        reps = -(-n // len(st))
        st, tu, dice = np.tile(st, (reps, 1))[:n], np.tile(tu, reps)[:n], np.tile(dice, (reps, 1))[:n]
    env.set_states(st, tu)
    env.set_dice(dice)
    return env


def _check_against_reference(env, weights, st, tu, dice, top_k, k_ties=False):
    states, v1, v2, kept = (x.cpu().numpy() for x in env.search_candidates())
    after = env.states().cpu().numpy()
    n_pass = n_term = 0
    for i in range(len(st)):
        r = S.search(weights, st[i], int(tu[i]), int(dice[i, 0]), int(dice[i, 1]), top_k)
        n_pass += r["passes"]; n_term += int(r["terminal"].sum())
        k = int(kept[i])
        assert k == len(r["states"]), (i, k, len(r["states"]))
        if k == 0:
            continue
        got = {tuple(s): (a, b) for s, a, b in zip(states[i, :k], v1[i, :k], v2[i, :k])}
        want = {tuple(s): (a, b) for s, a, b in zip(r["states"], r["v1"], r["v2"])}
        if set(got) != set(want):
            # the filter: only candidates tied at the K-th place may differ
            assert k_ties, i
            kth = np.sort(r["v1"])[::-1][k - 1] if tu[i] == 0 else np.sort(r["v1"])[k - 1]
            for s in set(got) ^ set(want):
                v = got[s][0] if s in got else want[s][0]
                assert abs(v - kth) <= 1e-5, (i, v, kth)
        for s in set(got) & set(want):
            assert abs(got[s][0] - want[s][0]) <= 1e-5, (i, got[s][0], want[s][0])
            assert abs(got[s][1] - want[s][1]) <= 1e-5, (i, got[s][1], want[s][1])
        # the choice: the reference's, unless its best two V2 lie within 2e-5
        v2r = np.array(r["v2"])
        srt = np.sort(v2r)[::-1] if tu[i] == 0 else np.sort(v2r)
        chosen = tuple(r["states"][r["choice"]])
        if tuple(after[i]) != chosen:
            assert len(srt) > 1 and abs(srt[0] - srt[1]) <= 2e-5, i
            assert tuple(after[i]) in want
    return n_pass, n_term


def test_parity_at_full_width(bg, golden_dir, weights):
    st, tu, dice = _lanes(bg, golden_dir, weights, 64, 64, seed=11)
    env = _setup(bg, weights, st, tu, dice)
    env.step_search(top_k=0, roll=False, auto_reset=False, no_flip=True)
    n_pass, n_term = _check_against_reference(env, weights, st, tu, dice, 0)
    assert n_pass > 0 and n_term > 0, (n_pass, n_term)
    lc = env.last_choice()
    _, _, v2, kept = (x.cpu().numpy() for x in env.search_candidates())
    val = lc["value"].cpu().numpy()
    for i in range(len(st)):
        if kept[i]:
            assert val[i] in set(v2[i, :kept[i]].tolist())
    env.close()


def test_top_k_1_is_the_greedy_step(bg, weights):
    n = 65536
    src = bg.VecGame(n, seed=5)
    src.load_weights(weights)
    src.run_greedy(12)
    st, tu = src.states().cpu().numpy(), src.turns().cpu().numpy()
    src.close()
    dice = np.random.RandomState(5).randint(1, 7, (n, 2)).astype(np.int32)
    a = _setup(bg, weights, st, tu, dice)
    b = _setup(bg, weights, st, tu, dice)
    a.step_search(top_k=1, roll=False, auto_reset=False)
    b.step_greedy(roll=False, auto_reset=False)
    _, v1, _, kept = a.search_candidates()
    term = (kept > 0) & ((v1[:, 0] == 1.0) | (v1[:, 0] == 0.0))
    same = (a.states() == b.states()).all(dim=1)
    assert bool(same[~term].all()), int((~same[~term]).sum())
    f = a.flags()
    won = ((f & 16) != 0) & (((f >> 5) & 1) == torch.as_tensor(tu, device=f.device))
    assert bool(won[term].all())
    a.close(); b.close()


def test_top_k_8_filter_against_reference(bg, golden_dir, weights):
    st, tu, dice = _lanes(bg, golden_dir, weights, 128, 128, seed=23)
    env = _setup(bg, weights, st, tu, dice)
    env.step_search(top_k=8, roll=False, auto_reset=False, no_flip=True)
    _check_against_reference(env, weights, st, tu, dice, 8, k_ties=True)
    env.close()


def test_chunk_invariance_and_determinism(bg, golden_dir, weights):
    st, tu, dice = _lanes(bg, golden_dir, weights, 32, 32, seed=3)
    small = _setup(bg, weights, st, tu, dice)
    big = _setup(bg, weights, st, tu, dice, n=65536)
    for e in (small, big):
        e.step_search(top_k=8, roll=False, auto_reset=False)
    ls, lb = small.last_choice(), big.last_choice()
    for k in ("seq", "seq_len", "chosen", "value"):
        assert torch.equal(ls[k][:64], lb[k][:64]), k
    assert torch.equal(small.states(), big.states()[:64])
    assert torch.equal(small.search_candidates()[2], big.search_candidates()[2][:64])
    small.close(); big.close()

    envs = []
    for _ in range(2):
        e = bg.VecGame(16384, seed=77)
        e.load_weights(weights)
        for _ in range(40):
            e.step_search(top_k=8)
        envs.append(e)
    assert torch.equal(envs[0].states(), envs[1].states())
    assert torch.equal(envs[0].turns(), envs[1].turns())
    l0, l1 = envs[0].last_choice(), envs[1].last_choice()
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    assert envs[0].stats()["games_finished"] > 0                     # games finished and restarted along the way
    for e in envs:
        e.close()


def test_flags(bg, golden_dir, weights):
    from backgammon_env import _capi
    st, tu, dice = _lanes(bg, golden_dir, weights, 32, 32, seed=41)
    # only_player: the other side's lanes are untouched
    env = _setup(bg, weights, st, tu, dice)
    before = env.snapshot().clone()
    env.step_search(top_k=4, roll=False, auto_reset=False, only_player=0)
    after = env.snapshot()
    idle = torch.as_tensor(tu, device=after.device) == 1
    assert torch.equal(before[idle], after[idle])
    assert not torch.equal(before[~idle][:, :28], after[~idle][:, :28])
    env.close()
    # slot 1: the search evaluates with the slot-1 weights
    w1 = (weights * np.float32(0.9) + np.float32(0.01)).astype(np.float32)
    env = _setup(bg, weights, st[:16], tu[:16], dice[:16], slot_weights=w1)
    env.step_search(top_k=4, roll=False, auto_reset=False, no_flip=True, slot=1)
    _check_against_reference(env, w1, st[:16], tu[:16], dice[:16], 4, k_ties=True)
    env.close()
    # finished lanes without auto-reset stay finished
    env = bg.VecGame(4096, seed=9)
    env.load_weights(weights)
    for _ in range(400):
        env.step_search(top_k=2, auto_reset=False)
        if bool(((env.flags() & 4) != 0).sum() > 64):
            break
    fin = (env.flags() & 4) != 0
    assert int(fin.sum()) > 0
    s0 = env.states()[fin].clone()
    env.step_search(top_k=2, auto_reset=False)
    assert bool(((env.flags() & 4) != 0)[fin].all()) and torch.equal(env.states()[fin], s0)
    # a ring log set: refused
    env.record_ring(8)
    rc = env._lib.bgamd_env_step_search(env._h, _capi.ROLL | _capi.AUTO_RESET, 8, None)
    assert rc == -1                                  # BGAMD_E_INVALID
    env.record_ring(None)
    env.close()
    # 65 536 lanes, top_k = 8: no error flag, no arena overflow
    env = bg.VecGame(65536, seed=13)
    env.load_weights(weights)
    for _ in range(3):
        env.step_search(top_k=8)
    s = env.stats()
    assert s["error_flags"] == 0, s
    env.close()


def test_two_ply_beats_one_ply(bg, weights):
    from backgammon_env.arena import head_to_head
    env = bg.VecGame(4096, seed=2024)
    r = head_to_head(env, weights, weights, plies_a=2, plies_b=1, top_k=8)
    n = r["games"]
    se = math.sqrt(0.25 / n)
    print("2-ply (top_k 8) vs 1-ply, tdgammonNEW100k: %d games, win rate %.4f (se %.4f)" % (n, r["win_rate"], se))
    assert n >= 8192
    assert r["win_rate"] > 0.5 + 3 * se, r
    env.close()
