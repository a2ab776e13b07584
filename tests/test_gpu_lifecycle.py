"""Creation, re-creation and teardown of everything a handle owns on the MI355X (csrc/bg_devmem.h: one owner of device memory per env
and per learner).  One env of 256 lanes and one of 1 lane go through every feature that allocates on first use or grows on demand,
with the rollout's trial env destroyed and re-created in between; both are destroyed, created again and taken through the same calls.
Nothing here knows what the right answers are -- the other GPU tests do -- only that they are the same bits every time."""
import ctypes as C

import numpy as np
import pytest

import rollout_cases as RC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = RC.SEED
TRIALS = 5


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items() if torch.is_tensor(v)}


def _scalar_enumerate(one, player, d1, d2):
    """bgamd_game_enumerate on a one-lane env, as Game._enumerate calls it (no pooled env: this one is destroyed with the pass)"""
    cap = 4096
    st, sq, ln = np.empty((cap, 28), np.int32), np.empty((cap, 4, 2), np.int8), np.empty((cap,), np.int32)
    k = one._lib.bgamd_game_enumerate(one._h, player, d1, d2, *(x.ctypes.data_as(C.c_void_p) for x in (st, sq, ln)), cap)
    assert 0 < k <= cap, k
    return {"states": st[:k].copy(), "seq": sq[:k].copy(), "len": ln[:k].copy()}


def _one_pass(bg, weights, st, tu):
    """-> {name: {field: array}}: every output of one env's life"""
    out = {}
    env = bg.VecGame(256, seed=11)
    one = bg.VecGame(1, seed=11, arena_rows=32768)
    env.load_weights(weights)
    roll = lambda tag, **kw: out.__setitem__(tag, _np(env.rollout(st, tu, TRIALS, seed=SEED, per_trial=True, outcomes=True, **kw)))

    roll("rollout_256", lanes=256)
    env.step_search(top_k=2)                                         # first use: the search's buffers, the scratch env
    out["search"] = dict(states=env.states().cpu().numpy(), value=env.last_choice()["value"].cpu().numpy(), info=np.array(env.search_info()))
    pre, turn, dice = env.states(), env.turns(), env.dice()          # the greedy move from here is the move to analyse from here
    env.step_greedy(roll=False, auto_reset=False, no_flip=True)
    played = env.states()
    env.set_states(pre, turn)
    env.set_dice(dice)
    out["analysis"] = _np(env.analyze_moves(played, top_k=2))        # first use: the analysis' buffers
    roll("rollout_512", lanes=512)                                   # the trial env destroyed and re-created ...
    f, m = env.evaluate_preroll(st, tu)                              # first use: the pre-roll buffers
    out["preroll"] = dict(f=f.cpu().numpy(), mean=m.cpu().numpy())
    roll("rollout_vr", lanes=512, variance_reduction=True)           # ... what the luck-adjusted rollout adds
    roll("rollout_grouped", lanes=512, groups=[0, 0, 1])             # ... and the group table
    env.step_sampled(1.0)                                            # first use: the sampled step's two buffers
    out["sampled"] = dict(states=env.states().cpu().numpy(), info=np.array(env.sample_info()))
    roll("rollout_256_again", lanes=256)                             # ... and re-created once more
    out["enumerate"] = _scalar_enumerate(one, 0, 3, 1)               # first use: the scalar surface's staging
    out["enumerate_doubles"] = _scalar_enumerate(one, 0, 2, 2)       # a longer list: its device copy grows
    for e in (env, one):
        assert e.stats()["error_flags"] == 0
        e.close()
    return out


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def test_envs_recreated_give_the_same_bits(weights):
    import backgammon_env as bg
    st, tu = RC.late_boards(3)
    first = _one_pass(bg, weights, st, tu)
    # the trial env went 256 -> 512 -> 256 lanes with every first-use group allocated in between: the same rollout, the same bits
    assert first["rollout_256"]["trial_value"].shape == (3, TRIALS)
    _assert_same(first["rollout_256"], first["rollout_256_again"], "rollout after two re-creations of the trial env")
    assert (first["analysis"]["status"] == 0).any() and len(first["enumerate_doubles"]["len"]) > len(first["enumerate"]["len"])
    # both envs destroyed and created again with the same seeds: every output of the second life equals the first
    second = _one_pass(bg, weights, st, tu)
    assert sorted(first) == sorted(second)
    for name in first:
        _assert_same(first[name], second[name], name)


def test_learner_created_and_destroyed(weights):
    """A learner of four slots with the delayed update switched on once, created and destroyed twice.  (The delayed replay's own buffers
    come with its first one-launch step, which takes 512 slots: tests/test_gpu_round4.py runs and destroys such learners.)"""
    from backgammon_env.learner import DeviceTDLambdaLearner
    for _ in range(2):
        L = DeviceTDLambdaLearner(weights, max_games=4)
        L.set_delay(1)
        assert L.theta.cpu().numpy().tobytes() == np.asarray(weights, np.float32).tobytes()
        del L
