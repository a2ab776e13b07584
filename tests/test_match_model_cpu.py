"""CPU checks of match play on the cubeful rollouts (include/bgamd.h, bgamd_env_rollout_match):
  (1) tests/match_model.py against a second statement of the rule, written as one function with nothing shared, over every entry of
      four tables' thresholds and over a set of trials;
  (2) closed forms;
  (3) five deliberately wrong models are told apart from it on the same test set;
  (4) the C++ threshold table and refusals of csrc/bg_match_plan.h (tests/sanitize/match_plan_driver.cpp, built plainly and with
      AddressSanitizer + UBSan, each run as its own program) against the model bit for bit;
  (5) the conditions tests/test_gpu_rollout_match.py rests on, under the fp64 rollout reference: every class of match history occurs
      in its configurations, and still does when every mean moves by the value tolerance;
  (6) plumbing that fails without the feature."""
import ctypes
import inspect
import itertools
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cube_cases as CC
import cube_model as CM
import match_cases as MC
import match_model as MM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
INF = float("inf")


def random_tables():
    """three seeded tables of 6, 7 and 8 points: two monotone (a side that needs fewer points, or whose opponent needs more, is better
    off) and complementary, one of independent uniform entries -- not monotone, not complementary: its window is often empty"""
    rng = np.random.RandomState(5)
    out = []
    for M in (6, 8):
        lead = np.sort(rng.uniform(0.02, 0.3, M))             # the worth of being d points ahead, growing with d
        met = np.array([[min(1.0, max(0.0, 0.5 + np.sign(b - a) * lead[abs(b - a)] * (1.0 + 1.0 / (a + b + 2)))) for b in range(M)]
                        for a in range(M)])
        met = np.where(np.arange(M)[:, None] > np.arange(M)[None, :], 1.0 - met.T, met)
        out.append(MM.table(met, np.sort(rng.uniform(0.0, 0.5, M))[::-1]))
    out.append(MM.table(rng.uniform(0.0, 1.0, (7, 7)), rng.uniform(0.0, 1.0, 7)))
    return out


TABLES = [MC.J7] + random_tables()
SHARES = (0.0, 0.5, 0.37, 1.0)


# ---- (1) a second statement ---------------------------------------------------------------------------------------------------------------

def restated(tab, ws, turns, points, value, too_good_at, max_cube, hold, c0, o0, a1, a2, state, bug=None):
    """One loop over the turns with the thresholds worked out in place, plain ints and floats; the table is read through `chance`
    alone.  -> (cube, owner, dropped, passed, doubles, dead, mwc, ended).  bug: one of the wrong models of (3), else the rule."""
    def chance(me, you, post):                                 # me / you: points to go (<= 0: the match is over)
        if me < 1:
            return 1.0
        if you < 1:
            return 0.0
        if post and bug != "met after the Crawford game":
            if you == 1:
                return tab.met_pc[me - 1]
            if me == 1:
                return 1.0 - tab.met_pc[you - 1]
        return tab.met[me - 1][you - 1]

    post = state in (1, 2)
    c, o, dropped, passed, n, dead = c0, o0, -1, 0, 0, False
    for k, (mover, mean, over) in enumerate(turns):
        side = mover + 1
        mine, yours = (a1, a2) if side == 1 else (a2, a1)
        if dropped != -1 or over or c >= max_cube or o not in (0, side) or (hold and k == 0):
            continue
        if state == 1 and bug != "doubling in the Crawford game":
            continue
        if c >= mine and bug != "offering a dead cube":
            dead = True
            continue
        win1, lose1 = chance(mine - c, yours, post), chance(mine, yours - c, post)
        win2, lose2 = chance(mine - c - c, yours, post), chance(mine, yours - c - c, post)
        spread, risk, gain = win2 - lose2, lose1 - lose2, win2 - win1
        if spread <= 0.0 or risk + gain <= 0.0:
            continue
        take_point = (win1 - lose2) / spread
        opening = risk / (risk + gain)
        double_point = opening + ws * (take_point - opening)
        if not all(map(math.isfinite, (take_point, opening, double_point))):
            continue
        w = mean if side == 1 else 1.0 - mean
        if double_point <= w <= too_good_at:
            if w > take_point:
                dropped, passed = k, 3 - side
            else:
                c, o, n = c + c, 3 - side, n + 1
    if dropped == -1 and points == 0:
        x = float(np.float32(value))
        if bug == "money formula at truncation":
            return c, o, dropped, passed, n, dead, c * (2.0 * x - 1.0), 0
        return c, o, dropped, passed, n, dead, x * chance(a1 - c, a2, post) + (1.0 - x) * chance(a1, a2 - c, post), 0
    if dropped != -1:
        stake = (c + c if bug == "a pass pays 2c" else c) * (1 if passed == 2 else -1)
    else:
        stake = c * points
    left1, left2 = (a1 - stake, a2) if stake > 0 else (a1, a2 + stake)
    return c, o, dropped, passed, n, dead, chance(left1, left2, post), (1 if left1 < 1 else (-1 if left2 < 1 else 0))


def restated_thresholds(tab, ws, state, c, a, b):
    """through `restated`: the means at which a single turn of PLAYER1 starts to double and to be passed are searched by bisection on
    the float line, so this shares no formula with the model -- used on a sample of the entries; the formula below on all"""
    post = state in (1, 2)

    def chance(me, you):
        if me < 1:
            return 1.0
        if you < 1:
            return 0.0
        if post and you == 1:
            return tab.met_pc[me - 1]
        if post and me == 1:
            return 1.0 - tab.met_pc[you - 1]
        return tab.met[me - 1][you - 1]
    win1, lose1, win2, lose2 = chance(a - c, b), chance(a, b - c), chance(a - 2 * c, b), chance(a, b - 2 * c)
    if not win2 - lose2 > 0.0 or not (lose1 - lose2) + (win2 - win1) > 0.0:
        return INF, INF
    t = (win1 - lose2) / (win2 - lose2)
    o = (lose1 - lose2) / ((lose1 - lose2) + (win2 - win1))
    return o + ws * (t - o), t


def test_thresholds_against_the_restatement_over_every_entry():
    n = degenerate = 0
    for tab, ws in itertools.product(TABLES, SHARES):
        got = MM.threshold_table(tab, ws)
        assert len(got) == 2 * MM.levels(tab.M) * tab.M * tab.M
        for (s, c, a, b), v in got.items():
            assert v == restated_thresholds(tab, ws, s, c, a, b), (s, c, a, b)
            n += 1
            degenerate += v[0] == INF
            assert (v[0] == INF) == (v[1] == INF) and (v[0] == INF or (math.isfinite(v[0]) and math.isfinite(v[1])))
    assert n > 4000 and 0 < degenerate < n
    # the table that is not monotone meets the degenerate branch where a monotone one does not: a live cube in a normal game
    live = lambda tab: [v[0] == INF for (s, c, a, b), v in MM.threshold_table(tab, 0.5).items() if s == 0 and 2 * c < min(a, b)]
    assert any(live(TABLES[3])) and not any(live(TABLES[0])) and not any(live(TABLES[1]))


def _scores(M, rng):
    a1, a2 = int(rng.randint(1, M + 1)), int(rng.randint(1, M + 1))
    return MM.Score(a1, a2, int(rng.randint(1, 3)) if min(a1, a2) == 1 else 0)


def _test_set():
    """(table, window_share, turns, points, value, rule, start value, start owner, score): means a few ulps and a little away from
    each threshold of the turn's own entry, both movers, every owner, every state, every ending -- and the reference's own trials of
    the GPU cases"""
    out = []
    rng = np.random.RandomState(17)
    rules = [CM.Rule(1.0, 0.0, 1.0, 64), CM.Rule(1.0, 0.0, 0.9, 4), CM.Rule(1.0, 0.0, 1.0, 8, False, True), MC.RULE]
    for tab, ws in itertools.product(TABLES, SHARES[:3]):
        marks = {0.0, 1.0, 0.3, 0.5, 0.9}
        for v in MM.threshold_table(tab, ws).values():
            if v[0] != INF and rng.rand() < 0.05:
                marks |= {t for x in v if 0.0 <= x <= 1.0 for t in (x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, 1.0)))}
        marks = sorted(marks)
        for _ in range(140):
            first = int(rng.randint(2))
            turns = []
            for k in range(int(rng.randint(1, 7))):
                mover = (first + k) % 2
                w = marks[int(rng.randint(len(marks)))]
                turns.append((mover, w if mover == 0 else 1.0 - w, False))
            out.append((tab, ws, turns, int(rng.choice([0, 1, 2, 3, -1, -2, -3])), float(np.float32(rng.rand())),
                        rules[int(rng.randint(len(rules)))], int(rng.choice([1, 1, 2, 4])), int(rng.randint(3)), _scores(tab.M, rng)))
    for (rotate, T), config in itertools.product(CC.SHAPES, MC.CONFIGS):
        for p, row in enumerate(CC.reference(rotate, T, CC.HORIZON)):
            out += [(config[1], config[2], turns, points, value, MC.RULE, config[6][p], config[7][p], MC.scores(config)[p])
                    for turns, points, value, _ in row]
    return out


@pytest.fixture(scope="module")
def test_set():
    return _test_set()


def _model(case):
    tab, ws, turns, points, value, rule, c0, o0, score = case
    thr = lambda s, c, a, b: MM.thresholds(tab, ws, s, c, a, b)
    played, mwc, ended = MM.trial(tab, turns, points, value, rule, score, thr, c0, o0)
    r = played.rec
    return (r.cube, r.owner, r.dropped, r.passed, r.doubles, played.dead, mwc, ended)


def _restated(case, bug=None):
    tab, ws, turns, points, value, rule, c0, o0, score = case
    return restated(tab, ws, turns, points, value, rule.too_good_at, rule.max_cube, rule.hold_turn0, c0, o0, *score, bug=bug)


def test_model_against_the_restatement(test_set):
    assert len(test_set) > 2000
    for case in test_set:
        assert _model(case) == _restated(case), case[2:]
    seen = [_model(case) for case in test_set]
    assert any(s[2] >= 0 for s in seen) and any(s[4] >= 2 for s in seen) and any(s[5] for s in seen) and {s[7] for s in seen} == {-1, 0, 1}


def test_statistics_order():
    rng = np.random.RandomState(3)
    for T in (1, 36, 40, 64, 65, 200):
        q = [float(x) for x in rng.choice([0.0, 1.0, 0.25, 0.594, 0.37, 0.81], T)]
        m, se = MM.statistics(q)
        assert abs(m - math.fsum(q) / T) <= T * 2.0 ** -50
        want = math.sqrt(math.fsum((e - math.fsum(q) / T) ** 2 for e in q) / (T * (T - 1))) if T > 1 else 0.0
        assert abs(se - want) <= 1e-12 * want + T * 2.0 ** -50
        assert MM.paired(q, q) == (0.0, 0.0)


# ---- (2) closed forms ---------------------------------------------------------------------------------------------------------------------

def test_no_decision_at_double_match_point():
    for tab in TABLES + [MC.J1]:
        thr = lambda s, c, a, b: MM.thresholds(tab, 0.5, s, c, a, b)
        for state, mover, w, owner in itertools.product((1, 2), (0, 1), (0.0, 0.3, 0.5, 0.7, 1.0), (0, 1, 2)):
            played = MM.play([(mover, w, False), (1 - mover, w, False)], MC.RULE, MM.Score(1, 1, state), thr, 1, owner)
            assert played.rec == CM.start(1, owner) and not played.events
            assert MM.payoff(tab, played.rec, 1, 1.0, MM.Score(1, 1, state)) == (1.0, 1)
            assert MM.payoff(tab, played.rec, -3, 0.0, MM.Score(1, 1, state)) == (0.0, -1)


def test_two_away_two_away_on_a_symmetric_table():
    for tab in TABLES[:3]:
        assert tab.met[1][0] == 1.0 - tab.met[0][1]
        for ws in SHARES:
            double_at, pass_at = MM.thresholds(tab, ws, 0, 1, 2, 2)
            assert pass_at == tab.met[0][1]
            assert double_at == 0.5 + ws * (pass_at - 0.5)         # open == 0.5 exactly
        assert MM.thresholds(tab, 0.0, 0, 1, 2, 2)[0] == 0.5


def test_a_side_that_loses_the_match_on_losing_c_points_opens_at_zero():
    n = 0
    for tab in TABLES:
        for s, l, a in itertools.product((0, 2), range(MM.levels(tab.M)), range(1, tab.M + 1)):
            c = 1 << l
            for b in range(1, c + 1):                              # the opponent needs no more than c
                double_at, pass_at = MM.thresholds(tab, 0.0, s, c, a, b)
                if double_at != INF:
                    assert double_at == 0.0, (s, c, a, b)
                    n += 1
    assert n > 50


def test_payoff_by_hand():
    tab = MC.J7
    rec = CM.start(2, 0)
    # a gammon with the cube on 2 at 3-away ends the match; so do 6 points: what lies beyond the length is worth nothing
    assert MM.payoff(tab, rec, 2, 1.0, MM.Score(3, 5, 0)) == (1.0, 1) and MM.payoff(tab, rec, 3, 1.0, MM.Score(3, 5, 0)) == (1.0, 1)
    assert MM.payoff(tab, rec, 1, 1.0, MM.Score(3, 5, 0)) == (tab.met[0][4], 0)
    assert MM.payoff(tab, rec, -1, 0.0, MM.Score(3, 5, 0)) == (tab.met[2][2], 0)
    # a pass pays the cube before the double; after the Crawford game the trailer reads met_pc
    assert MM.payoff(tab, rec._replace(dropped=0, passed=1), 0, 0.5, MM.Score(1, 4, 2)) == (1.0 - tab.met_pc[1], 0)
    assert MM.payoff(tab, rec._replace(dropped=0, passed=2), 0, 0.5, MM.Score(4, 1, 2)) == (tab.met_pc[1], 0)
    assert MM.payoff(tab, CM.start(1, 0), 0, 0.25, MM.Score(2, 2, 0))[0] == 0.25 * tab.met[0][1] + 0.75 * tab.met[1][0]
    # c x 3 beyond 32 bits
    assert MM.payoff(tab, CM.start(2 ** 30, 0), -3, 0.0, MM.Score(7, 7, 0)) == (0.0, -1)


# ---- (3) wrong models ---------------------------------------------------------------------------------------------------------------------

BUGS = ["doubling in the Crawford game", "offering a dead cube", "met after the Crawford game", "a pass pays 2c",
        "money formula at truncation"]


@pytest.mark.parametrize("bug", BUGS)
def test_wrong_models_are_told_apart(test_set, bug):
    assert sum(_model(case) != _restated(case, bug) for case in test_set) > 0, bug


# ---- (4) the C++ table and refusals ---------------------------------------------------------------------------------------------------------

def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "match_plan_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("match_plan")
    return [(build_driver(d / "match_plan_driver"), None),
            (build_driver(d / "match_plan_driver_san", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer")), SAN_ENV)]


def run(exe, mode, text, extra_env):
    r = subprocess.run([exe, mode], env={**os.environ, **(extra_env or {})}, input=text, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    return r.stdout.splitlines()


def test_cpp_table_against_the_model_bit_for_bit(drivers):
    for exe, env in drivers:
        for tab, ws in itertools.product(TABLES + [MC.J1, MC.janowski(64)], (0.5, 0.37)):
            text = "%d %s\n" % (tab.M, ws.hex()) + " ".join(x.hex() for row in tab.met for x in row) + "\n" + " ".join(x.hex() for x in tab.met_pc)
            lines = run(exe, "table", text + "\n", env)
            want = MM.threshold_table(tab, ws)
            L = MM.levels(tab.M)
            assert lines[0].split() == ["layout", str(tab.M), str(L), "0", str(tab.M ** 2), str((tab.M ** 2 + tab.M + 1) // 2 * 2),
                                        str((tab.M ** 2 + tab.M + 1) // 2 * 2 + 4 * L * tab.M ** 2)]
            assert len(lines) == 1 + len(want)
            order = [(s, 1 << l, a, b) for s in (0, 2) for l in range(L) for a in range(1, tab.M + 1) for b in range(1, tab.M + 1)]
            for key, line in zip(order, lines[1:]):
                w = line.split()
                assert tuple(map(int, w[:4])) == key
                got = (float.fromhex(w[4]), float.fromhex(w[5]))
                assert got == want[key] and [g.hex() for g in got] == [x.hex() for x in want[key]], (key, got, want[key])


def setting_refusal(flags, M, has_tables, ws, k, v):
    """bg_match_plan.h's check_setting restated: the first rule broken, in its order"""
    if flags & ~1:
        return 1
    if not 1 <= M <= 64:
        return 2
    if not has_tables:
        return 3
    if 0 <= k < M * M + M and not 0.0 <= v <= 1.0:
        return 4
    if not 0.0 <= ws <= 1.0:
        return 5
    return 0


def call_refusal(on, cube_flags, flags):
    if not on:
        return 0
    if not cube_flags & 1:
        return 1
    if cube_flags & 2:
        return 2
    return 0 if flags & 256 else 3


def test_cpp_refusals_and_their_precedence(drivers):
    nan = float("nan")
    broken = [dict(flags=2), dict(flags=3), dict(M=0), dict(M=65), dict(M=-1), dict(has=0), dict(k=0, v=1.5), dict(k=0, v=-0.1),
              dict(k=3, v=nan), dict(k=7, v=INF), dict(k=4 * 4 + 3, v=2.0), dict(ws=nan), dict(ws=-0.25), dict(ws=1.25), dict(ws=INF)]
    fine = [dict(), dict(M=1), dict(M=64), dict(k=0, v=0.0), dict(k=19, v=1.0), dict(ws=0.0), dict(ws=1.0), dict(flags=0), dict(k=20, v=7.0)]
    cases = broken + fine + [{**a, **b} for a, b in itertools.combinations(broken, 2)]
    req = [(c.get("flags", 1), c.get("M", 4), c.get("has", 1), c.get("ws", 0.5), c.get("k", -1), c.get("v", 0.5)) for c in cases]
    want = [setting_refusal(*q) for q in req]
    assert all(w > 0 for w in want[:len(broken)]) and not any(want[len(broken):len(broken) + len(fine)]) and set(want) == {0, 1, 2, 3, 4, 5}
    calls = list(itertools.product((0, 1), range(8), (0, 128, 256, 384)))
    sizes = [(M, P, N, on) for M in (1, 2, 3, 4, 5, 7, 8, 9, 33, 64) for P, N, on in ((3, 108, 1), (3, 108, 0), (65536, 2 ** 31 - 1, 1))]
    for exe, env in drivers:
        got = run(exe, "setting", "".join("%d %d %d %s %d %s\n" % (f, M, h, repr(ws), k, repr(v)) for f, M, h, ws, k, v in req), env)
        assert list(map(int, got)) == want
        got = run(exe, "call", "".join("%d %d %d\n" % c for c in calls), env)
        assert list(map(int, got)) == [call_refusal(*c) for c in calls]
        got = run(exe, "sizes", "".join("%d %d %d %d\n" % s for s in sizes), env)
        for (M, P, N, on), line in zip(sizes, got):
            L = MM.levels(M)
            assert list(map(int, line.split())) == [L, (M * M + M + 1) // 2 * 2 + 4 * L * M * M, P if on else 0, N if on else 0]
    assert {call_refusal(*c) for c in calls} == {0, 1, 2, 3}
    assert [MM.levels(M) for M in (1, 2, 3, 4, 5, 8, 9, 64)] == [0, 1, 2, 2, 3, 3, 4, 6]


# ---- (5) the conditions the GPU tests rest on ------------------------------------------------------------------------------------------------

def test_every_class_occurs_under_the_reference():
    trials_of = lambda rotate, T: CC.reference(rotate, T, CC.HORIZON)
    for tol in (0.0, CC.MEAN_TOL):
        got = MC.full_census(trials_of, tol)
        print("tol %.0e:" % tol, got)
        for c in MC.CLASSES:
            assert got.get(c, 0) >= 1, (c, tol, got)


def test_configurations_are_valid_and_the_cube_setting_is_ignored():
    for config in MC.CONFIGS:
        assert all(MM.valid(s, config[1].M) for s in MC.scores(config)), config[0]
    assert not MM.valid(MM.Score(1, 3, 0), 7) and not MM.valid(MM.Score(2, 3, 1), 7) and not MM.valid(MM.Score(2, 8, 0), 7)
    # under the money rule MC.RULE never doubles
    for rotate, T in CC.SHAPES:
        for row in CC.reference(rotate, T, CC.HORIZON):
            assert all(CM.play(t[0], MC.RULE) == CM.start() for t in row)


# ---- (6) plumbing ------------------------------------------------------------------------------------------------------------------------------

NEW = ("bgamd_env_rollout_match", "bgamd_env_rollout_match_results", "bgamd_env_rollout_match_thresholds")


def test_match_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from backgammon_env import _capi
    src = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    assert re.search(r"\bBGAMD_MATCH_ON\s*=\s*1\b", src)
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in {n for n, _, _ in _capi.SYMBOLS}, name
    assert _capi.MATCH_ON == 1
    assert os.path.exists(os.path.join(ROOT, "backgammon-engine_amd", "csrc", "bg_match_plan.h"))
    # host-side argument checks need no device
    assert lib.bgamd_env_rollout_match(None, 1, ctypes.c_int64(1), None, None, ctypes.c_double(0.5), None, None, None) == -1
    assert lib.bgamd_env_rollout_match_thresholds(None, 0, ctypes.c_int64(1), 2, 2, None) == -1


def test_python_surface(tmp_path):
    import backgammon_env as bg
    from backgammon_env import analysis
    from backgammon_env.match import Match, MatchTable
    assert "match" in inspect.signature(bg.VecGame.rollout).parameters and bg.VecGame.PAIRED_WHICH["mwc"] == 4
    assert "match" in inspect.signature(analysis.cube_action).parameters and callable(bg.VecGame.rollout_match_read)
    # the package's table is the one the cases restate
    for M, want in ((7, MC.J7), (1, MC.J1)):
        t = MatchTable.janowski(M)
        assert t.M == M and t.met.tolist() == want.met and t.met_pc.tolist() == want.met_pc
        for a1, a2, s in itertools.product(range(-1, M + 1), range(-1, M + 1), (0, 1, 2)):
            assert t.after(a1, a2, s) == MM.after(want, a1, a2, s)
    # load: JSON and plain text give the table back bit for bit
    t = MatchTable.janowski(5)
    (tmp_path / "t.json").write_text(json.dumps({"met": t.met.tolist(), "met_pc": t.met_pc.tolist()}))
    (tmp_path / "t.txt").write_text("# a table\n" + "\n".join(" ".join(repr(x) for x in row) for row in t.met.tolist()) + "\n"
                                    + ", ".join(repr(x) for x in t.met_pc.tolist()) + "\n")
    for name in ("t.json", "t.txt"):
        u = MatchTable.load(str(tmp_path / name))
        assert u.met.tolist() == t.met.tolist() and u.met_pc.tolist() == t.met_pc.tolist()
    (tmp_path / "bad.txt").write_text("0.5 0.5 0.5")
    for bad in (lambda: MatchTable.load(str(tmp_path / "bad.txt")), lambda: MatchTable([[0.5, 1.5], [0.5, 0.5]], [0.5, 0.5]),
                lambda: MatchTable([[0.5]], [0.5, 0.5]), lambda: MatchTable.janowski(65)):
        with pytest.raises(ValueError):
            bad()
    # the state is derived where the score says it, and asked for where it does not
    m = Match(t, [3, 2], [5, 4])
    assert [x.tolist() for x in m.per_position(2)] == [[3, 2], [5, 4], [0, 0]] and m.window_share == 0.5
    with pytest.raises(ValueError):
        Match(t, 1, 3)
    assert [x.tolist() for x in Match(t, 1, 3, state=2).per_position(3)] == [[1, 1, 1], [3, 3, 3], [2, 2, 2]]
