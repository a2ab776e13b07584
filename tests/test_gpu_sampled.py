"""The temperature-sampled step on the MI355X (bgamd_env_step_sampled / _run_sampled / _sample_info: csrc/bg_sample.h and GreedyRun),
held lane by lane to the exact model tests/sample_model.py fed with the device's own rows and float32 values:
  (a) the rule: the played board, key and reported value are the model's winner on every lane outside the near-tie set (counted, at most
      1 %), twins play the smaller key, T = 1e-30 plays an arg-max, lanes without a move stay put -- lane counts 1, 63, 65, 257, 1 000,
      four temperatures, the checkpoint and a table that ties candidates exactly;
  (b) sample_info() against the counts recomputed from choice_spread() and last_choice();
  (c) T = 0 is step_greedy bit for bit; finished and only_player lanes are untouched;
  (d) independence of the lane count, the split over envs, run against steps, replay, the weight slot;
  (e) the ring log and want_index work as they do for the greedy step; error codes; the drivers end to end.
tests/test_sample_model_cpu.py holds the conditions these rest on (the model itself, the lane set's shapes, the near-tie census)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_model as SM
import search_lanes as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHOICE = ("chosen", "count", "seq", "seq_len", "value")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _np(x):
    return x.cpu().numpy()


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _table(net, weights):
    return weights if net == "ckpt" else L.dyadic()


def _snap(env):
    out = {k: _np(v) for k, v in env.last_choice().items()}
    out.update(states=_np(env.states()), turns=_np(env.turns()), dice=_np(env.dice()), flags=_np(env.flags()), stats=env.stats())
    return out


def _same(a, b, what, keys=None, la=slice(None), lb=slice(None)):
    for k in keys or a.keys():
        if k == "stats":                                                       # (the node counters depend on how a run's launches are fused)
            for c in ("steps", "games_finished", "p1_wins", "rows_evaluated", "error_flags"):
                assert a[k][c] == b[k][c], (what, c, a[k], b[k])
            continue
        x, y = a[k][la], b[k][lb]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        same = x.reshape(len(x), -1).view(np.uint8) == y.reshape(len(y), -1).view(np.uint8)
        assert same.all(), (what, k, "lanes", np.where(~same.all(1))[0][:8].tolist())


# ---- (a), (b): one sampled step from the lane set, every result as numpy, once per (net, lanes, T) -------------------------------------------

_steps, _ks = {}, {}


def _step(bg, weights, net, n, T):
    if (net, n, T) not in _steps:
        st, tu, dice = (x[:n] for x in SM.lane_set())
        env = bg.VecGame(n, seed=SM.SEED)
        env.load_weights(_table(net, weights))
        env.set_states(st, tu)
        env.set_dice(dice)
        env.step_sampled(T, roll=False, auto_reset=False, no_flip=True)
        info, ust, uval = (_np(x) for x in env.unique_rows())
        out = _snap(env)
        out.update(info=info, ust=np.ascontiguousarray(ust, dtype=np.int32), uval=uval, sample_info=env.sample_info(),
                   spread={k: (_np(v) if hasattr(v, "cpu") else v) for k, v in env.choice_spread().items()})
        assert out["stats"]["error_flags"] == 0
        env.close()
        _steps[(net, n, T)] = out
    return _steps[(net, n, T)]


def _row_k(gid, row):
    """the integer of a row's u (game id gid, ply 0): a function of the planes alone, shared by every net and temperature"""
    key = (gid, row.tobytes())
    if key not in _ks:
        _ks[key] = SM.uniform_int(SM.SEED, gid, 0, row)
    return _ks[key]


def _key_seq(key, mover, d1, d2):
    """the (origin, destination) pairs a key stands for (csrc/bg_staged.h: pass | four 5-bit origins | length)"""
    ln, pas = key & 7, (key >> 23) & 1
    dA, dB = (d2, d1) if pas else (d1, d2)
    seq = np.full((4, 2), -1, np.int8)
    for k in range(ln):
        o = (key >> (18 - 5 * k)) & 31
        die = dB if k & 1 else dA
        seq[k] = (o, min(25, max(0, o - die if mover else o + die)))
    return seq, ln


@pytest.mark.parametrize("n", SM.LANE_COUNTS)
@pytest.mark.parametrize("net", ["ckpt", "dyadic"])
def test_rule_lane_by_lane(bg, weights, net, n):
    st, tu, dice = (x[:n] for x in SM.lane_set())
    for T in SM.TEMPERATURES:
        r = _step(bg, weights, net, n, T)
        game, key = r["info"][:, 0], r["info"][:, 1] & 0x7FFFFFFF
        assert ((r["info"][:, 1] >> 31) == tu[game]).all()
        order = np.argsort(game, kind="stable")
        bounds = np.searchsorted(game[order], np.arange(n + 1))
        planes = SM.planes(r["ust"])
        left_out = twins = moved = left_best = 0
        for i in range(n):
            idx = order[bounds[i]:bounds[i + 1]]
            if len(idx) == 0:                                                  # no move (the oracle agrees): the board stays, nothing is chosen
                assert len(SM.candidates(i)[0]) == 0 and (r["states"][i] == st[i]).all() and r["chosen"][i] == -1, (T, i)
                continue
            assert {s.tobytes() for s in r["ust"][idx]} == {s.tobytes() for s in SM.candidates(i)[0]}, (T, i)
            ks = np.array([_row_k(i, planes[j]) for j in idx], np.int64)
            m = SM.lane(planes[idx], key[idx], r["uval"][idx], tu[i], SM.SEED, i, 0, T, ks=ks)
            a = SM.mover_side(r["uval"][idx], tu[i])
            moved += 1
            left_best += int(_u32(r["value"][i]).item() != _u32(r["uval"][idx][np.argmax(a)]).item())
            has_twin = len({s.tobytes() for s in r["ust"][idx]}) < len(idx)
            twins += has_twin
            if T == 1e-30:                                                     # an arg-max, whatever the noise says
                assert _u32(r["value"][i]).item() == _u32(r["uval"][idx][np.argmax(a)]).item(), (T, i)
            if m["near"]:
                left_out += 1
                continue
            w = idx[m["winner"]]
            assert (r["states"][i] == r["ust"][w]).all(), (T, i, "board")
            assert _u32(r["value"][i]) == _u32(r["uval"][w]), (T, i, "value")
            seq, ln = _key_seq(int(key[w]), int(tu[i]), int(dice[i, 0]), int(dice[i, 1]))
            assert r["seq_len"][i] == ln and (r["seq"][i] == seq).all(), (T, i, "key")
            if has_twin:                                                       # of the copies of the played afterstate: the smallest key
                same = [j for j in idx if (r["ust"][j] == r["ust"][w]).all()]
                assert key[w] == min(key[j] for j in same), (T, i, "twin")
        print(net, "lanes", n, "T", T, "with a move", moved, "left out", left_out, "twin lanes", twins, "left the arg-max", left_best)
        assert left_out <= 0.01 * n
        if n == 1000:
            assert twins >= 20
        # (b) sample_info: lanes with a move, lanes whose played value is not their best value -- the same from choice_spread and last_choice
        sp = r["spread"]
        has = sp["count"] > 0
        assert r["sample_info"] == [moved, left_best]
        assert r["sample_info"] == [int(has.sum()), int((_u32(r["value"])[has] != _u32(sp["best"])[has]).sum())]
        if T == 1e-30:
            assert r["sample_info"][1] == 0
        if T == 1.0 and n >= 63:
            assert r["sample_info"][1] > 0.2 * moved                           # at T = 1 the draw is nearly uniform: it does sample


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------

def test_temperature_zero_is_the_greedy_step(bg, weights):
    a, b = bg.VecGame(257), bg.VecGame(257)
    for e in (a, b):
        e.load_weights(weights)
    with pytest.raises(bg.BgamdError) as err:                                 # nothing sampled yet
        b.sample_info()
    assert err.value.code == -1
    for t in range(3):
        a.step_greedy(want_index=(t == 2))
        b.step_sampled(0.0, want_index=(t == 2))
        _same(_snap(a), _snap(b), ("step", t))
    a.run_greedy(5)
    b.run_sampled(5, 0.0)
    _same(_snap(a), _snap(b), "run")
    assert a.stats() == b.stats()                                             # the same launches: every counter alike
    with pytest.raises(bg.BgamdError):                                        # T = 0 samples nothing: still nothing to report
        b.sample_info()
    a.close(); b.close()


def test_finished_and_only_player_lanes_are_untouched(bg, weights):
    n = 65
    st, tu, dice = (x[:n].copy() for x in SM.lane_set())
    st[:5] = 0; st[:5, 23] = 1; st[:5, 26] = 14; st[:5, 0] = -1; st[:5, 27] = 14; tu[:5] = 0; dice[:5] = (1, 2)     # bears its last checker off
    env = bg.VecGame(n)
    env.load_weights(weights)
    env.set_states(st, tu)
    env.set_dice(dice)
    env.step_sampled(0.05, roll=False, auto_reset=False)
    one = _snap(env)
    assert (one["flags"][:5] & 5 == 5).all() and (one["states"][:5, 26] == 15).all()
    env.step_sampled(0.05, roll=True, auto_reset=False)
    two = _snap(env)
    _same(one, two, "finished lanes", keys=("states", "turns", "flags") + CHOICE, la=slice(0, 5), lb=slice(0, 5))
    assert (two["states"][5:] != one["states"][5:]).any()
    # only PLAYER1's lanes take part: the others keep board, turn, dice and their last choice; PLAYER1's play what they play in a full step
    full, part = bg.VecGame(n), bg.VecGame(n)
    for e in (full, part):
        e.load_weights(weights)
        e.set_states(st, tu)
        e.set_dice(dice)
    before = _snap(part)
    full.step_sampled(0.05, roll=False, auto_reset=False)
    part.step_sampled(0.05, roll=False, auto_reset=False, only_player=0)
    f, p = _snap(full), _snap(part)
    p1 = np.where(tu == 0)[0]; p2 = np.where(tu == 1)[0]
    _same(p, before, "PLAYER2 idle", keys=("states", "turns", "dice", "flags") + CHOICE, la=p2, lb=p2)
    _same(p, f, "PLAYER1 plays", keys=("states", "turns", "flags") + CHOICE, la=p1, lb=p1)
    assert part.sample_info()[0] == int((f["chosen"][p1] >= 0).sum())
    for e in (env, full, part):
        e.close()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------

def _fresh(bg, weights, n=257, slot=0, **kw):
    env = bg.VecGame(n, **kw)
    env.load_weights(weights, slot=slot)
    return env


def test_split_over_two_envs(bg, weights):
    """the same game ids in one env and split over two by lane_offset: the noise is keyed by the game id, not the lane"""
    n, cut, T = 257, 128, 0.05
    one = _fresh(bg, weights, n)
    lo, hi = _fresh(bg, weights, cut, lane_offset=0, lane_stride=n), _fresh(bg, weights, n - cut, lane_offset=cut, lane_stride=n)
    for t in range(7):
        for e in (one, lo, hi):
            e.step_sampled(T)
        a, x, y = _snap(one), _snap(lo), _snap(hi)
        keys = ("states", "turns", "dice", "flags") + CHOICE
        _same(a, x, ("low half", t), keys=keys, la=slice(0, cut))
        _same(a, y, ("high half", t), keys=keys, la=slice(cut, n))
    assert one.sample_info()[0] == lo.sample_info()[0] + hi.sample_info()[0]
    assert one.sample_info()[1] == lo.sample_info()[1] + hi.sample_info()[1] > 0
    for e in (one, lo, hi):
        e.close()


@pytest.mark.parametrize("auto_reset", [True, False])
def test_run_is_its_steps(bg, weights, auto_reset):
    T = 0.05
    for k in (1, 2, 7):
        run, steps = _fresh(bg, weights), _fresh(bg, weights)
        for e in (run, steps):                       # a few greedy steps first: the lanes are at different plies
            e.run_greedy(3)
        run.run_sampled(k, T, auto_reset=auto_reset)
        info = np.zeros(2, np.int64)
        for _ in range(k):
            steps.step_sampled(T, auto_reset=auto_reset)
            info += steps.sample_info()
        _same(_snap(run), _snap(steps), ("run of", k))
        assert run.sample_info() == info.tolist() and info[1] > 0
        run.close(); steps.close()


def test_dense_mode_replays_and_slots_agree(bg, weights):
    T = 0.05
    a, b = _fresh(bg, weights), _fresh(bg, weights)
    for e in (a, b):
        e.run_sampled(4, T, precision=bg.F16X2)
        e.step_sampled(T, precision=bg.F32_DENSE)
    _same(_snap(a), _snap(b), "dense replay")
    assert a.sample_info() == b.sample_info() and a.sample_info()[1] > 0
    # F32_DENSE values are the dense chain's, not the incremental net's: the rule on the device's own values still holds
    info, ust, uval = (_np(x) for x in a.unique_rows())
    ch = _snap(a)
    played = {(int(g), _u32(v).item()) for g, v in zip(info[:, 0], uval)}
    assert all((i, _u32(ch["value"][i]).item()) in played for i in range(a.n) if ch["chosen"][i] >= 0)
    s0, s1 = _fresh(bg, weights), _fresh(bg, weights, slot=1)
    for t in range(4):
        s0.step_sampled(T)
        s1.step_sampled(T, slot=1)
        _same(_snap(s0), _snap(s1), ("slot", t))
    for e in (a, b, s0, s1):
        e.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------

def test_ring_log_and_want_index(bg, weights):
    """The ring logs the pre-move row of every sampled step -- the rows a stepwise env without a log stands on before each step (the moves
    are the same moves: the noise does not depend on the log) -- and the end records of the games that end.  want_index names the sampled
    sequence's reference-order index and the list's length."""
    n, k, T = 257, 12, 0.25
    ring, plain = _fresh(bg, weights, n), _fresh(bg, weights, n)
    rows, end = ring.record_ring(16)
    ring.run_sampled(k, T)
    for t in range(k):
        pre = bg.pack_rows(plain.states(), plain.turns())
        plain.step_sampled(T)
        assert torch.equal(rows[t], pre), t
        over = (plain.flags() & 1) != 0
        assert torch.equal(end[t] != 0, over), t
    _same(_snap(ring), _snap(plain), "ring")
    ring.record_ring(None)
    ring.close(); plain.close()
    st, tu, dice = (x[:n] for x in SM.lane_set())
    env = _fresh(bg, weights, n)
    env.set_states(st, tu)
    env.set_dice(dice)
    env.step_sampled(T, roll=False, auto_reset=False, no_flip=True, want_index=True)
    r = _snap(env)
    other = 0
    for i in range(n):
        cand, seq, ln = SM.candidates(i)
        assert r["count"][i] == len(cand), i
        if len(cand) == 0:
            assert r["chosen"][i] == -1
            continue
        c = int(r["chosen"][i])
        assert (cand[c] == r["states"][i]).all() and ln[c] == r["seq_len"][i] and (seq[c] == r["seq"][i]).all(), i
        other += c != 0
    assert other > n // 4
    env.close()


def test_refused_temperatures(bg, weights):
    env = _fresh(bg, weights, 63)
    before = _snap(env)
    for T in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        for call in (lambda: env.step_sampled(T), lambda: env.run_sampled(2, T)):
            with pytest.raises(bg.BgamdError) as err:
                call()
            assert err.value.code == -1, T
    _same(before, _snap(env), "refused")
    with pytest.raises(bg.BgamdError):
        env.sample_info()
    env.close()


def test_drivers_refuse_epsilon_beside_temperature(bg, weights):
    from backgammon_env import analysis, arena
    from backgammon_env.learner import ContinuousSelfPlay, play_round
    a, b = _fresh(bg, weights, 63), _fresh(bg, weights, 63)
    with pytest.raises(ValueError):
        play_round(a, max_plies=8, epsilon=0.1, temperature=0.05)
    with pytest.raises(ValueError):
        analysis.error_rate(a, b, 1, epsilon=0.1, temperature=0.05)
    with pytest.raises(ValueError):
        arena.head_to_head(a, weights, weights, max_turns=1, epsilon=0.1, temperature=0.05)
    sp = ContinuousSelfPlay(a, ring_steps=16)
    with pytest.raises(ValueError):
        sp.play(4, epsilon=0.1, temperature=0.05)
    sp.play(4, temperature=0.05)                                              # ... and plays without it
    assert a.sample_info()[0] > 0
    sp.close()
    rows, lengths, won = play_round(b, max_plies=8, temperature=0.05)
    assert rows.shape[1] == 63 and b.sample_info()[0] > 0
    r = arena.head_to_head(b, weights, weights, max_turns=4, temperature=0.05)
    assert r["games"] >= 0 and b.sample_info()[0] > 0
    a.close(); b.close()


_ERROR_RATE = """
import os, sys
sys.path[:0] = [%r, %r]
import numpy as np
import backgammon_env as bg
from backgammon_env import analysis
w = np.fromfile(%r, dtype=np.float32)
player, judge = bg.VecGame(256, seed=1), bg.VecGame(256, seed=1)
player.load_weights(w); judge.load_weights(w)
hot = analysis.error_rate(player, judge, turns=8, temperature=0.05)
info = player.sample_info()
player.reset()
cold = analysis.error_rate(player, judge, turns=8)
assert hot["total"]["illegal"] == 0 and cold["total"]["illegal"] == 0
assert hot["lane_turns"] == 256 * 8 and info[0] > 0 and info[1] > 0
assert cold["total"]["error_rate"] < hot["total"]["error_rate"] < 0.1, (cold["total"], hot["total"])
print("error_rate greedy %%.6f sampled %%.6f" %% (cold["total"]["error_rate"], hot["total"]["error_rate"]))
"""


def test_error_rate_and_training_example_end_to_end(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32")
    script = tmp_path / "sampled_error_rate.py"
    script.write_text(_ERROR_RATE % (ROOT, os.path.join(ROOT, "backgammon-engine_amd"), golden))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and "error_rate greedy" in r.stdout, r.stdout + r.stderr
    args = [sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "256", "--rounds", "2", "--max-plies", "200",
            "--arena", "64", "--health-rows", "2048", "--temperature", "0.05"]
    r = subprocess.run(args, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("round ") and " health: " in ln]) == 2, r.stdout
