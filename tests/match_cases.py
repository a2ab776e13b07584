"""The cases of the match play tests.  No device, no torch.  Shared by tests/test_match_model_cpu.py, which computes under the fp64
rollout reference (tests/cube_cases.py: its three positions, shapes and horizon) the conditions the GPU tests rest on -- every class
of match history occurs, with room to spare --, and tests/test_gpu_rollout_match.py, which asserts the same census on the device.

The table is MatchTable.janowski(7) restated here (the package is not imported: no torch), and janowski(1) for double match point.
The cube setting of every case is RULE: its double_at and pass_at would stop every double if they were read (1.0 and 0.0: the roller
never reaches 1.0, and every double would be passed) -- a match ignores them; nobody is too good, and the cube stops at 4.

  2-2         2-away / 2-away, the cube in the centre: the contact position's roller stands at 0.5945 against a take point of
              met[0][1] = 0.5944 (too near to count: the census takes what is robust), a take makes the cube dead for both sides; the
              bear-off's roller (0.98) doubles and PLAYER1 passes at turn 0
  5-5         5-away / 5-away with max_cube 4 and a narrow window (0.1: double_at 0.523): takes, and redoubles when the lead changes
  2-3         PLAYER1 2-away, PLAYER2 3-away: the trailer's take point in the roller's w is 0.445, PLAYER2 passes at turn 0
  crawford    1-away / 3-away in the Crawford game: no decision
  post        1-away against 4-, 3- and 4-away after the Crawford game: the leader's cube is dead, the 4-away trailer doubles at its
              first turn (from 0.25 on, passed above 0.5), the 3-away trailer meets an entry without thresholds (winning 1 and winning 2
              points are worth the same 0.5: doubling gains nothing, the window is empty)
  post 3-1    the same from the other seat: PLAYER1 trails 4-, 2- and 3-away
  dmp         double match point on a one-point table (M = 1): no decision, the MWC is the win
  gammon      5-away / 3-away with a 2-cube in PLAYER1's hands: the bear-off's roller has no access, wins 2 or, with a gammon, 4 points:
              a gammon times the cube ends the match, a point beyond its length"""
import itertools

import cube_cases as CC
import cube_model as CM
import match_model as MM

RULE = CM.Rule(double_at=1.0, pass_at=0.0, too_good_at=1.0, max_cube=4)


def janowski(M):
    met = [[0.5] * M for _ in range(M)]
    for a in range(1, M + 1):
        for b in range(a + 1, M + 1):
            v = min(1.0, max(0.0, 0.5 + 0.85 * float(b - a) / float(a + b + 6)))
            met[a - 1][b - 1], met[b - 1][a - 1] = v, 1.0 - v
    return MM.Table(M, met, [0.5 ** ((k + 1) // 2) for k in range(1, M + 1)])


J7, J1 = janowski(7), janowski(1)

# (name, table, window_share, away1 [3], away2 [3], state [3], start values [3], start owners [3])
CONFIGS = [
    ("2-2", J7, 0.5, [2, 2, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1], [0, 0, 0]),
    ("5-5", J7, 0.1, [5, 5, 5], [5, 5, 5], [0, 0, 0], [1, 1, 1], [0, 0, 0]),
    ("2-3", J7, 0.5, [2, 2, 2], [3, 3, 3], [0, 0, 0], [1, 1, 1], [0, 0, 0]),
    ("crawford", J7, 0.5, [1, 1, 1], [3, 3, 3], [1, 1, 1], [1, 1, 1], [0, 0, 0]),
    ("post", J7, 0.5, [1, 1, 1], [4, 3, 4], [2, 2, 2], [1, 1, 1], [0, 0, 0]),
    ("post 3-1", J7, 0.5, [4, 2, 3], [1, 1, 1], [2, 2, 2], [1, 1, 1], [0, 0, 0]),
    ("dmp", J1, 0.5, [1, 1, 1], [1, 1, 1], [1, 2, 1], [1, 1, 1], [0, 0, 0]),
    ("gammon", J7, 0.5, [5, 5, 5], [3, 3, 3], [0, 0, 0], [2, 2, 2], [1, 1, 1]),
]
CLASSES = ("Crawford game", "dead cube", "double / take", "pass by PLAYER1", "pass by PLAYER2", "redouble",
           "post-Crawford trailer doubling at its first turn", "match ended by a gammon times the cube", "points beyond the match length",
           "truncated payoff", "degenerate entry")


def scores(config):
    _, _, _, a1, a2, st, _, _ = config
    return [MM.Score(*x) for x in zip(a1, a2, st)]


def model_thr(config):
    """the model's threshold function of a config"""
    tab, ws = config[1], config[2]
    return lambda state, c, a, b: MM.thresholds(tab, ws, state, c, a, b)


def census(trials, config, thr, tol=0.0):
    """trials [P][T] of cube_cases.ref_trial's tuples -> {class: count}; tol > 0: a trial counts for a class only if it belongs to it
    however its means move, each on its own, by -tol, 0 or +tol (every decision is monotone in its mean)"""
    out = {}
    sc = scores(config)
    for p, row in enumerate(trials):
        for turns, points, value, _ in row:
            live = [k for k, t in enumerate(turns) if not t[2]]
            sure = None
            for moves in itertools.product((0.0,) if tol == 0.0 else (-tol, 0.0, tol), repeat=len(live)):
                moved = list(turns)
                for k, d in zip(live, moves):
                    moved[k] = (turns[k][0], turns[k][1] + d, False)
                played = MM.play(moved, RULE, sc[p], thr, config[6][p], config[7][p])
                cl = MM.classes(played, moved, points, sc[p], config[6][p])
                sure = cl if sure is None else sure & cl
            for c in sure:
                out[c] = out.get(c, 0) + 1
    return out


def full_census(trials_of, tol=0.0, thr_of=model_thr):
    """the union over CONFIGS and cube_cases.SHAPES: trials_of(rotate, T) -> [P][T]; thr_of(config) -> the threshold function"""
    out = {}
    for config in CONFIGS:
        for rotate, T in CC.SHAPES:
            for c, n in census(trials_of(rotate, T), config, thr_of(config), tol).items():
                out[c] = out.get(c, 0) + n
    return out
