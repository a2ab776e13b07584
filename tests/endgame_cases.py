"""End-game positions for the board rules, and their census (no device, no torch).

helpers.random_boards kind 1 keeps PLAYER1 on 19..24 and PLAYER2 on 1..6, so "the mover bears off with an opposing checker inside its home
board" hardly occurs in fixture G10 -- the class where SURVEY Q1 makes the two sides differ: PLAYER2's overrun (die > origin) is denied by
a checker of EITHER colour on the points origin+1..7, PLAYER1's (die > 25 - origin) only by its own checkers on origin+1..24.  This set
asks for that and for the rest of the end of the game: exact bear-offs and overruns, stragglers that come home and then bear off, a checker
on the bar while the others are home, hits inside the home board, borne-off counts 0..14 crossing 3|4, 7|8 and 11|12, and the fifteenth
checker leaving with dice unplayed, as a single game, a gammon and a backgammon.

  cases()            -> (state28 int32 [N, 28], mover int32 [N], dice int32 [N, 2]): a seeded draw plus hand-built boards, N <= 4096.
                        Every board has 15 checkers a side and is not over.  About 35 % of the drawn rolls are doubles.
  enumerate_oracle() -> per lane (sequences, afterstates, legalMoves for the dice 1..6, the die of every move of every sequence)
  lane_classes(...)  -> the names of the classes below that one lane belongs to, decided from the oracle's answer
  census(set)        -> {class: lanes}, the set's total number of sequences, per-lane class sets; CLASSES lists every class, MIN_LANES
                        is the condition (tests/test_endgame_cases_cpu.py): each class holds at least 8 lanes.
  probes(set)        -> int32 [P, 6] rows (lane, kind, player, die, origin, destination): the fixed tryMove probes of every lane, each
                        sent to a fresh copy of the lane's position; PROBE_KINDS names the kinds.

Classes.  "above o" are the points the reference's overrun rule looks at: o+1..24 for PLAYER1, o+1..7 for PLAYER2.  An overrun candidate
is a checker of a mover who is all home with an empty bar, on a point nearer to the edge than the die.  *_P1 / *_P2: suffixed per mover.
  overrun*   exact (a legal bear-off with the exact die); overrun_ok (a legal overrun, no opposing checker above its origin);
             overrun_ok_oppbehind (a legal overrun with an opposing checker above its origin: PLAYER1 only);
             overrun_denied_oppbehind (a denied candidate with an opposing checker and none of its own above it: PLAYER2 only);
             overrun_denied_only_point7_P2 (the same, the only such checker on point 7); overrun_denied_own_higher (a denied candidate
             with one of its own above it); must_move_inside (a die with no exact checker, a checker farther out, and a legal move inside
             the home board); home_blocked (all home; zero sequences, or one empty sequence on doubles)
  shape*     comes_home_then_off (a checker outside home, bar empty, and a sequence that bears off); on_bar_rest_home (on the bar,
             every other checker home: nothing bears off -- four sixes take the entering checker to the last point and no further, so a
             turn that enters and bears off does not exist); overrun_opens_midturn (a sequence's second or later move is an overrun that
             was not legal at the root); short_nonwinning (the longest sequence that does not win is shorter than the dice, not empty);
             plain_contact_in_home / dbl_contact_in_home (an opposing checker on the mover's six home points and a sequence that bears
             off); hit_and_off (an afterstate with a hit and a checker borne off)
  counts     plain_off1, plain_off2, dbl_off1 .. dbl_off4 (an afterstate that bears off exactly that many); off_root_0 .. off_root_14;
             off_cross_3_4, _7_8, _11_12 (root at or below, an afterstate above); off_reaches_15; stack_ge8_dec (a point with 8 or more
             that an afterstate takes below 8); stack_4_3 (a point with 4 or more taken to 3 or fewer); dup_afterstates; one_distinct
  ends*      win (an afterstate with 15 off); win_dice_left_plain (a winning sequence of one move on a plain roll), win_dice_left_dbl1 /
             _dbl2 / _dbl3 (a winning sequence of three / two / one moves on doubles); win_beside_nonwin; all_win
  results    win_points_1_P1 .. win_points_3_P2 (outcome_ref.points of a winning afterstate, per winner); win_bg_bar, win_bg_home (the
             backgammon with the loser on the bar / with the bar empty and a checker in the winner's home)

Census of the committed set under the oracle (`python tests/endgame_cases.py` prints it; fixture G12 holds the unmodified reference's
answers on exactly these lanes):
lanes 2648 (1800 drawn, 848 hand-built), doubles 1079, sequences 40481, distinct afterstates 10278; lanes per class, the smallest 11:
  exact_P1                           392   win_dice_left_plain_P1              96   off_root_5                          90
  exact_P2                           365   win_dice_left_plain_P2              71   off_root_6                         119
  overrun_ok_P1                      539   win_dice_left_dbl1_P1               44   off_root_7                          90
  overrun_ok_P2                      209   win_dice_left_dbl1_P2               39   off_root_8                          98
  overrun_denied_own_higher_P1       209   win_dice_left_dbl2_P1               97   off_root_9                         106
  overrun_denied_own_higher_P2       314   win_dice_left_dbl2_P2               37   off_root_10                         89
  must_move_inside_P1                332   win_dice_left_dbl3_P1               67   off_root_11                        164
  must_move_inside_P2                321   win_dice_left_dbl3_P2               35   off_root_12                        368
  home_blocked_P1                     15   win_beside_nonwin_P1                11   off_root_13                        545
  home_blocked_P2                    166   win_beside_nonwin_P2                13   off_root_14                        420
  comes_home_then_off_P1             123   all_win_P1                         405   off_cross_3_4                       92
  comes_home_then_off_P2              95   all_win_P2                         241   off_cross_7_8                      102
  on_bar_rest_home_P1                 82   overrun_ok_oppbehind_P1             75   off_cross_11_12                    141
  on_bar_rest_home_P2                 76   overrun_denied_oppbehind_P2        201   off_reaches_15                     670
  overrun_opens_midturn_P1           447   overrun_denied_only_point7_P2       35   stack_ge8_dec                       95
  overrun_opens_midturn_P2           160   plain_off1                         762   stack_4_3                          344
  short_nonwinning_P1                 18   plain_off2                         334   dup_afterstates                   1632
  short_nonwinning_P2                104   dbl_off1                           324   one_distinct                      1307
  plain_contact_in_home_P1           197   dbl_off2                           284   win_points_1_P1                    273
  plain_contact_in_home_P2           119   dbl_off3                           153   win_points_2_P1                     45
  dbl_contact_in_home_P1             175   dbl_off4                           145   win_points_3_P1                     98
  dbl_contact_in_home_P2              93   off_root_0                         230   win_points_1_P2                    135
  hit_and_off_P1                      54   off_root_1                          83   win_points_2_P2                     43
  hit_and_off_P2                      38   off_root_2                          89   win_points_3_P2                     76
  win_P1                             416   off_root_3                          68   win_bg_bar                         109
  win_P2                             254   off_root_4                          89   win_bg_home                         66
tryMove probes: 20 132; by message 9421 accepted, 4425 "Invalid origin", 1214 "Destination out of range", 2404 "Cannot move in that
direction.", 1152 "Move does not match dice.", 495 "Invalid destination.", 1021 "Cannot bear off from jail".  "Origin out of range" is
never given: the reference tests the origin first and refuses every origin outside 0..25 as "Invalid origin".
The wrong readings of tests/rules_ref.py differ from the oracle on 239 (h), 90 (i), 40 (j), 1017 (k), 1112 (l), 768 (m), 122 (n), 670 (o)
and 204 (p) of these lanes.

Measured on the MI355X on this set (tests/test_gpu_rules_endgame.py, its NETS-MAX lines; integer results are bit-exact; 26 tests in
11.2 s, the slowest 3.4 s): max |gpu - fp64| over the 10 881 rows the greedy step hands to the value net, per parity family of
tests/nets.py, against the 1e-5 bound --
  ckpt 4.99e-07   xavier 6.49e-08   ckpt_x4 2.67e-06   w1_x16 1.26e-06   normal 1.01e-06   normal_w1_x8 1.32e-06   loguniform 5.36e-07
the 2-ply search's v1 of every kept candidate 4.99e-07, evaluate_preroll on 128 roots (2662 rolls compared) 3.52e-07 (checkpoint).  The
sampled step at T = 0.05 left no lane out as a near tie; the rollouts' reference marks 3 and 4 of 864 trials.
"""
import numpy as np

SEED = 1207
N_RANDOM = 1800
MIN_LANES = 8
MAX_SEQUENCES = 80000

_SUFFIXED = ["exact", "overrun_ok", "overrun_denied_own_higher", "must_move_inside", "home_blocked",
             "comes_home_then_off", "on_bar_rest_home", "overrun_opens_midturn", "short_nonwinning", "plain_contact_in_home",
             "dbl_contact_in_home", "hit_and_off",
             "win", "win_dice_left_plain", "win_dice_left_dbl1", "win_dice_left_dbl2", "win_dice_left_dbl3", "win_beside_nonwin", "all_win"]
CLASSES = tuple([k + s for k in _SUFFIXED for s in ("_P1", "_P2")]
                + ["overrun_ok_oppbehind_P1", "overrun_denied_oppbehind_P2", "overrun_denied_only_point7_P2"]
                + ["plain_off1", "plain_off2", "dbl_off1", "dbl_off2", "dbl_off3", "dbl_off4"]
                + ["off_root_%d" % k for k in range(15)]
                + ["off_cross_3_4", "off_cross_7_8", "off_cross_11_12", "off_reaches_15", "stack_ge8_dec", "stack_4_3",
                   "dup_afterstates", "one_distinct"]
                + ["win_points_%d_P%d" % (k, p) for p in (1, 2) for k in (1, 2, 3)] + ["win_bg_bar", "win_bg_home"])

PROBE_KINDS = ("exact", "overrun_far", "overrun_near", "wrong_end", "from_outside", "bar_to_off", "point_while_on_bar", "direction",
               "dice_mismatch", "blocked", "forward", "origin_m1", "origin_26", "dest_m1", "dest_26")


def mirror(st):
    """The same position with the sides exchanged: point p <-> 25 - p, signs flipped, bars and borne-off counts swapped."""
    st = np.asarray(st)
    out = np.empty_like(st)
    out[..., :24] = -st[..., 23::-1]
    out[..., 24], out[..., 25], out[..., 26], out[..., 27] = st[..., 25], st[..., 24], st[..., 27], st[..., 26]
    return out


_OFF_DRAW = [0] * 5 + list(range(1, 14)) * 2 + [14] * 6 + [12, 13, 13]
_OOFF_DRAW = [0] * 10 + list(range(1, 15))


def _random_board(rng):
    """One board from the side of a mover who is PLAYER1 (home 19..24, bears off to 25); the caller mirrors it for PLAYER2."""
    board = np.zeros(24, dtype=np.int32)
    off = int(_OFF_DRAW[rng.randint(len(_OFF_DRAW))])
    b = 1 if rng.rand() < 0.12 and off < 14 else 0
    own = 15 - off - b
    n_out = int((0, 0, 0, 0, 1, 1, 2, 3)[rng.randint(8)]) if own > 1 else 0
    n_out = min(n_out, own - 1)
    # the opponent first: 0-3 points inside the mover's home (point 18, the mirror of 7, included), blots and made points
    ooff = int(_OOFF_DRAW[rng.randint(len(_OOFF_DRAW))])
    obar = int((0, 0, 0, 0, 0, 1, 1, 2, 3, 4)[rng.randint(10)])
    opp = 15 - ooff - obar
    if opp < 0:
        obar, opp = 0, 15 - ooff
    k_in = int((0, 0, 1, 1, 2, 3)[rng.randint(6)]) if rng.rand() < 0.6 else 0
    for p in rng.permutation(np.arange(17, 24))[:k_in]:
        k = min(opp, int((1, 1, 2, 3)[rng.randint(4)]))
        board[p] = -k; opp -= k
    # the mover: stragglers on 1..18 (mostly near home), the rest on 1..6 of the free home points -- up to 15 on one point
    for _ in range(n_out):
        p = int(rng.randint(11, 18)) if rng.rand() < 0.75 else int(rng.randint(0, 18))
        if board[p] < 0:
            p = next(q for q in range(p, -1, -1) if board[q] >= 0) if (board[:p + 1] >= 0).any() else None
        if p is None:
            continue
        board[p] += 1; own -= 1
    free_home = [p for p in range(18, 24) if board[p] == 0]
    if own and not free_home:
        return None
    pts = rng.choice(free_home, int(rng.randint(1, len(free_home) + 1)), replace=False) if own else []
    if own and rng.rand() < 0.2:
        pts = pts[:1]
    for c in range(own):
        board[int(pts[c] if c < len(pts) and rng.rand() < 0.7 else pts[rng.randint(len(pts))])] += 1
    # the opponent's rest: its own home 1..6, sometimes a few points elsewhere
    free = [p for p in range(0, 17) if board[p] == 0]
    if opp and not free:
        return None
    where = [p for p in free if p < 6] or free
    if rng.rand() < 0.3:
        where = free
    for c in range(opp):
        board[int(where[rng.randint(len(where))])] -= 1
    return np.concatenate([board, [b, obar, off, ooff]]).astype(np.int32)


def _hand_built():
    """The classes a random draw reaches too rarely, from the side of a mover who is PLAYER1; every board is used for both movers (the
    overrun rules differ, so the two lanes of a board may fall into different classes).  -> list of (state28, d1, d2)"""
    out = []

    def add(own, opp, d1, d2, b=0, ob=0, ooff=None):
        """own / opp: {point: count}; the mover's missing checkers are borne off, the opponent's as well unless ooff is given -- then
        they stand on its points 1 and 2"""
        board = np.zeros(24, dtype=np.int32)
        for p, v in own.items():
            board[p - 1] += v
        for p, v in opp.items():
            if p > 24 or board[p - 1] > 0:                   # off the board, or the point is the mover's: no such board
                return
            board[p - 1] -= v
        off = 15 - b - sum(own.values())
        rest = 15 - ob - sum(opp.values())
        if ooff is not None or rest > 14:
            ooff = 14 if ooff is None else ooff
            board[0] -= (rest - ooff + 1) // 2; board[1] -= (rest - ooff) // 2
            rest = ooff
        assert 0 <= off <= 14 and 0 <= rest <= 14, (own, opp, off, rest)
        out.append((np.concatenate([board, [b, ob, off, rest]]).astype(np.int32), d1, d2))

    for d in range(2, 7):
        for o in range(26 - d, 25):                          # an overrun candidate on o, die d
            for x in range(19, 25):
                if x != o:
                    add({o: 2}, {x: 1}, d, 1 + (d + x) % 6)              # a blot of the opponent's beside it, either side
                    add({o: 1, min(24, o + 1): 1}, {x: 2}, d, d)
            add({o: 2}, {18: 1}, d, d)                                    # only on point 18, the mirror of 7
            add({o: 1}, {18: 2}, 7 - d if 7 - d > 25 - o else d, d)
            for h in range(19, 25):
                if h != o:
                    add({o: 1, h: 2}, {}, d, 1 + (d + h) % 6)            # one of its own on the other side
    # all home and blocked on every die: made points on every destination inside, and the overrun denied (or no checker near enough)
    for d1, d2 in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (1, 3), (3, 3), (2, 3)):
        add({19: 3}, {19 + d1: 2, 19 + d2: 2}, d1, d2)
        add({19: 2, 20: 2}, {19 + d1: 2, 19 + d2: 2, 20 + d1: 2, 20 + d2: 2}, d1, d2) if 20 not in (19 + d1, 19 + d2) else None
        add({19: 1, 20 + max(d1, d2): 1}, {19 + d1: 2, 19 + d2: 2}, d1, d2) if 20 + max(d1, d2) < 25 and 20 + max(d1, d2) not in (19 + d1, 19 + d2) else None
    # a sequence that does not win and is shorter than the dice: one move, then blocked
    for d1, d2 in ((1, 2), (2, 1), (2, 2), (1, 1), (3, 1), (1, 3), (3, 3), (2, 4)):
        add({19: 2, 24: 1}, {19 + d1 + d2: 2, 19 + 2 * max(d1, d2): 2} if d1 != d2 else {19 + 2 * d1: 2}, d1, d2)
        add({19: 3}, {19 + d1 + d2: 3} if 19 + d1 + d2 < 25 else {24: 2}, d1, d2)
    # the last checkers leave: single game, gammon, backgammon on the bar and in the winner's home, with one to three dice unplayed
    for k in (1, 2, 3, 4):
        for d in (1, 3, 6):
            for res in ("single", "gammon", "bg_bar", "bg_home"):
                ob = 2 if res == "bg_bar" else 0
                oppd = {19: 1} if res == "bg_home" and d != 6 else ({24: 1} if res == "bg_home" else {})
                own = {25 - d: k} if 25 - d not in oppd else {23: k}
                add(own, oppd, d, d, ob=ob, ooff=3 if res == "single" else 0)
                add(own, oppd, d, 1 + d % 6, ob=ob, ooff=1 if res == "single" else 0) if k <= 2 else None
    # a win beside a sequence that does not win: two checkers left, one die bears off and the other may move the far one inside
    for d1, d2 in ((6, 1), (1, 6), (5, 2), (2, 5), (4, 4), (3, 3), (6, 2), (3, 5)):
        add({19: 1, 25 - d1: 1} if 25 - d1 != 19 else {19: 1, 24: 1}, {}, d1, d2, ooff=0)
        add({20: 1, 23: 1}, {24: 1}, d1, d2, ooff=0)
        add({19: 2, 22: 1, 24: 1}, {}, d1, d1, ooff=2)
    # heavy stacks that a turn takes below 8 and from 4 to 3, hits inside the home on the way off, a checker on the bar
    for d in range(1, 7):
        add({25 - d: 9}, {}, d, d)
        add({25 - d: 8, 19: 1}, {}, d, 1 + d % 6)
        add({25 - d: 4}, {}, d, d)
        add({19: 1, 25 - d: 2} if d != 6 else {19: 3}, {19 + d: 1} if d < 6 and 19 + d != 25 - d else {20: 1}, d, d, ooff=0)
        add({24: 1}, {d: 1} if d > 2 else {}, 24 - d if 24 - d <= 6 else d, d, b=1)
        add({18 - d + 1: 1, 24: 1}, {19: 1}, d, d)                       # comes home with a hit on 19, then bears off
        add({}, {d: 1}, d, d, b=1, ob=1)
        add({19: 1}, {}, 6, 6, b=1) if d == 1 else None
    for d in (4, 5, 6):                                                  # from the bar to the last point on doubles: nothing bears off
        add({24: 1}, {}, d, d, b=1)
        add({24: 2}, {d: 1}, d, d, b=1)
    for d in (1, 2, 3):                                                  # a checker on the bar, the others home: no bear-off before it is home
        add({24: 2, 23: 1}, {}, d, 6, b=1)
    return [x for x in out if x is not None]


def cases():
    """-> (state28 int32 [N, 28], mover int32 [N], dice int32 [N, 2]), the same arrays on every call"""
    rng = np.random.RandomState(SEED)
    st, mv, dc = [], [], []
    while len(st) < N_RANDOM:
        s = _random_board(rng)
        mover = int(rng.randint(2))
        d1, d2 = int(rng.randint(1, 7)), int(rng.randint(1, 7))
        if rng.rand() < 0.22:                                # with the 1 in 6 by chance: about 35 % doubles
            d2 = d1
        if s is None:
            continue
        st.append(mirror(s) if mover else s); mv.append(mover); dc.append((d1, d2))
    for s, d1, d2 in _hand_built():
        for mover in (0, 1):
            st.append(mirror(s) if mover else s); mv.append(mover); dc.append((d1, d2))
    st, mv, dc = np.array(st, dtype=np.int32), np.array(mv, dtype=np.int32), np.array(dc, dtype=np.int32)
    assert len(st) <= 4096
    assert (np.clip(st[:, :24], 0, None).sum(1) + st[:, 24] + st[:, 26] == 15).all()
    assert (np.clip(-st[:, :24], 0, None).sum(1) + st[:, 25] + st[:, 27] == 15).all()
    assert (st[:, 24:] >= 0).all() and (st[:, 26:] < 15).all()
    return st, mv, dc


def enumerate_oracle(st, mv, dc):
    """The oracle's answer for every lane: -> list of (seqs as lists of (origin, dest), states [C, 28], [legal_moves(mover, die) for die
    1..6], the die of every move as lists parallel to seqs).  On a plain roll the sequences that play d1 first come first; their number
    is counted move by move, with the oracle's own tryMove and legalMoves."""
    from oracle import oracle as O
    out = []
    for i in range(len(st)):
        pl, d1, d2 = int(mv[i]), int(dc[i, 0]), int(dc[i, 1])
        s = O.State.from28(st[i], pl)
        q, ln, a = O.evaluate_turn_sequences(s, pl, d1, d2)
        seqs = O.sequences_as_lists(q, ln)
        if d1 == d2:
            dies = [[d1] * len(x) for x in seqs]
        else:
            first = 0
            for o, d in O.legal_moves(s, pl, d1):
                t = s.copy()
                ok, _ = O.try_move(t, pl, d1, o, d)
                assert ok
                first += max(1, len(O.legal_moves(t, pl, d2)))
            dies = [([d1, d2] if k < first else [d2, d1])[:len(x)] for k, x in enumerate(seqs)]
        out.append((seqs, a, [O.legal_moves(s, pl, die) for die in range(1, 7)], dies))
    return out


def lane_classes(s28, mover, d1, d2, seqs, states, moves, dies):
    """seqs, states, moves (legalMoves of the dice 1..6 at the root) and dies as enumerate_oracle returns them.  -> set of class names"""
    import outcome_ref as OC
    s28 = np.asarray(s28)
    sign = 1 if mover == 0 else -1
    sfx = "_P%d" % (mover + 1)
    off_d = 25 if mover == 0 else 0
    own = {p: int(s28[p - 1]) * sign for p in range(1, 25) if s28[p - 1] * sign > 0}
    opp = {p for p in range(1, 25) if s28[p - 1] * sign < 0}
    home = range(19, 25) if mover == 0 else range(1, 7)
    dist = (lambda p: 25 - p) if mover == 0 else (lambda p: p)
    above = (lambda o: range(o + 1, 25)) if mover == 0 else (lambda o: range(o + 1, 8))
    b, off, oppbar = int(s28[24 + mover]), int(s28[26 + mover]), int(s28[25 - mover])
    all_home = b == 0 and all(p in home for p in own)
    doubles = d1 == d2
    n, ndice = len(seqs), 4 if d1 == d2 else 2
    c = {"off_root_%d" % off}
    if all_home:
        for die in sorted({d1, d2}):
            legal = set(moves[die - 1])
            if any(dist(o) == die and (o, off_d) in legal for o in own):
                c.add("exact" + sfx)
            for o in own:
                if dist(o) >= die:
                    continue
                opp_above, own_above = [p for p in above(o) if p in opp], [p for p in above(o) if p in own]
                if (o, off_d) in legal:
                    c.add(("overrun_ok_oppbehind" if opp_above else "overrun_ok") + sfx)
                elif own_above:
                    c.add("overrun_denied_own_higher" + sfx)
                else:
                    assert opp_above, (s28, mover, die, o)
                    c.add("overrun_denied_oppbehind" + sfx)
                    if opp_above == [7]:
                        c.add("overrun_denied_only_point7" + sfx)
            if (not any(dist(o) == die for o in own) and any(dist(o) > die for o in own)
                    and any(d != off_d for _, d in legal)):
                c.add("must_move_inside" + sfx)
        if n == 0 or (n == 1 and not seqs[0]):
            c.add("home_blocked" + sfx)
    if b > 0 and all(p in home for p in own):
        c.add("on_bar_rest_home" + sfx)
    if not n:
        return c
    aoff = states[:, 26 + mover]
    gained = aoff - off
    hits = states[:, 25 - mover] - oppbar
    wins = aoff == 15
    if (gained > 0).any():
        if b == 0 and not all_home:
            c.add("comes_home_then_off" + sfx)
        assert b == 0                                        # (see on_bar_rest_home)
        if any(p in opp for p in home):
            c.add(("dbl" if doubles else "plain") + "_contact_in_home" + sfx)
    for q, dq in zip(seqs, dies):
        for k in range(1, len(q)):
            o, d = q[k]
            if d == off_d and dq[k] > dist(o) and (o, d) not in moves[dq[k] - 1]:
                c.add("overrun_opens_midturn" + sfx)
    lens = np.array([len(q) for q in seqs])
    if (~wins).any() and 1 <= lens[~wins].max() < ndice:
        c.add("short_nonwinning" + sfx)
    if ((hits > 0) & (gained > 0)).any():
        c.add("hit_and_off" + sfx)
    for k in range(1, ndice + 1):
        if (gained == k).any():
            c.add("%s_off%d" % ("dbl" if doubles else "plain", k))
    for lo in (3, 7, 11):
        if off <= lo and (aoff > lo).any():
            c.add("off_cross_%d_%d" % (lo, lo + 1))
    for p, k in own.items():
        if p in home and k >= 8 and (states[:, p - 1] * sign < 8).any():
            c.add("stack_ge8_dec")
        if p in home and k >= 4 and (states[:, p - 1] * sign <= 3).any():
            c.add("stack_4_3")
    distinct = len({tuple(int(v) for v in r) for r in states})
    if n > distinct:
        c.add("dup_afterstates")
    if distinct == 1:
        c.add("one_distinct")
    if wins.any():
        c.update(("off_reaches_15", "win" + sfx))
        c.add(("win_beside_nonwin" if (~wins).any() else "all_win") + sfx)
        left = {ndice - int(k) for k in lens[wins]}
        if not doubles and 1 in left:
            c.add("win_dice_left_plain" + sfx)
        for k in (1, 2, 3):
            if doubles and k in left:
                c.add("win_dice_left_dbl%d%s" % (k, sfx))
        for r in states[wins]:
            pts = OC.points(r)
            assert pts * sign > 0
            c.add("win_points_%d%s" % (abs(pts), sfx))
            if abs(pts) == 3:
                c.add("win_bg_bar" if r[25 - mover] > 0 else "win_bg_home")
    return c


def census(case_set, answers=None):
    """-> ({class: lanes}, total sequences, per-lane class sets).  answers: enumerate_oracle's list, when the caller has it already."""
    st, mv, dc = case_set
    answers = answers if answers is not None else enumerate_oracle(st, mv, dc)
    counts = {k: 0 for k in CLASSES}
    per_lane, total = [], 0
    for i, (seqs, states, moves, dies) in enumerate(answers):
        cl = lane_classes(st[i], int(mv[i]), int(dc[i, 0]), int(dc[i, 1]), seqs, states, moves, dies)
        for k in cl:
            counts[k] += 1
        per_lane.append(cl)
        total += len(seqs)
    return counts, total, per_lane


def u32_for(k, n):
    """The smallest choice_u32 with which the random step picks index k of n sequences (index = choice_u32 * n >> 32)"""
    k, n = int(k), int(n)
    u = ((k << 32) + n - 1) // n
    assert 0 <= k < n and u < 2 ** 32 and (u * n) >> 32 == k
    return u


ROLLOUT_TRIALS = 36


def rollout_lanes(case_set, per_lane):
    """24 lanes for rollouts played to the end: for each of the six results two lanes with 13 or 14 off whose every sequence (on the
    lane's own dice) wins with it and with no other, and twelve lanes late in the game (both sides with 8 or more off, the mover at most
    11, no bar) that take several turns."""
    st, mv, dc = case_set
    lanes = []
    for p in (1, 2):
        for k in (1, 2, 3):
            want = {"all_win_P%d" % p, "win_points_%d_P%d" % (k, p)}
            others = {"win_points_%d_P%d" % (j, p) for j in (1, 2, 3) if j != k}
            lanes += [i for i in range(len(st)) if want <= per_lane[i] and not (others & per_lane[i]) and st[i, 25 + p] >= 13][:2]
    late = [i for i in range(len(st)) if st[i, 26] >= 8 and st[i, 27] >= 8 and st[i, 24] == 0 and st[i, 25] == 0
            and st[i, 26 + mv[i]] <= 11 and i not in lanes]
    lanes += late[:24 - len(lanes)]
    assert len(lanes) == 24
    return np.array(lanes)


def scalar_lanes(st, k=64):
    """k lanes with both bars empty (the scalar surface sets a position through setGameBoard / setBorneOffPieces, which reach no bar),
    spread evenly over the set"""
    free = np.nonzero((st[:, 24] == 0) & (st[:, 25] == 0))[0]
    return free[np.linspace(0, len(free) - 1, k).astype(np.int64)]


def scalar_surface_check(mod, g12, lanes):
    """The lanes through the scalar Game surface of `mod` (the Python package or the compiled module of the same name), against fixture
    G12 as np.load gives it: setGameBoard / setBorneOffPieces, evaluateTurnSequences, legalMoves for the six dice, the first two and the
    last of the lane's tryMove probes on clones, and is_game_over after the first and the last sequence that bears off and the first
    that wins, played move by move through tryMove.  -> (sequences played, games they ended)"""
    p = [mod.Player("a", mod.PlayerType.PLAYER1), mod.Player("b", mod.PlayerType.PLAYER2)]
    seq_off = np.concatenate([[0], np.cumsum(g12["n_seq"])])
    mv_off = np.concatenate([[0], np.cumsum(g12["n_moves"].ravel())])
    pr, code = g12["probes"].astype(np.int64), g12["probe_code"]
    after_at = np.cumsum(code == 0) - 1                       # row of probe_after, for the probes that succeeded
    played = ended = 0

    def position(g):
        return list(g.getGameBoard()) + [g.getJailedCount(0), g.getJailedCount(1), g.getBornOffCount(0), g.getBornOffCount(1)]

    for i in lanes:
        root = g12["boards"][i].astype(np.int64).tolist()
        pl, d1, d2 = int(g12["mover"][i]), int(g12["dice"][i, 0]), int(g12["dice"][i, 1])
        g = mod.Game(0)
        g.setPlayers(p[0], p[1])
        g.setGameBoard(root[:24])
        g.setBorneOffPieces(0, root[26]); g.setBorneOffPieces(1, root[27])
        assert position(g) == root and g.is_game_over() == (False, -1), i
        r = slice(seq_off[i], seq_off[i + 1])
        seqs, states = g.evaluateTurnSequences(pl, d1, d2)
        want = [[(int(o), int(d)) for o, d in x[:n]] for x, n in zip(g12["seqs"][r], g12["seq_len"][r])]
        assert [[tuple(m) for m in q] for q in seqs] == want, i
        assert np.array_equal(np.asarray(states).reshape(-1, 28), g12["states"][r]), i
        for die in range(1, 7):
            j = i * 6 + die - 1
            assert [tuple(m) for m in g.legalMoves(pl, die)] == [tuple(m) for m in g12["moves"][mv_off[j]:mv_off[j + 1]].tolist()], (i, die)
        mine = np.nonzero(pr[:, 0] == i)[0]
        for j in sorted(set(mine[:2].tolist() + mine[-1:].tolist())):
            _, kind, player, die, o, d = pr[j].tolist()
            c = g.clone()
            ok, msg = c.tryMove(p[player], die, o, d)
            assert (ok, msg) == (code[j] == 0, str(g12["messages"][code[j]])), (i, PROBE_KINDS[kind], msg)
            assert position(c) == (g12["probe_after"][after_at[j]].tolist() if ok else root), (i, PROBE_KINDS[kind])
        bears, wins = np.nonzero(g12["over"][r] >= 0)[0], np.nonzero(g12["over"][r] >= 1)[0]
        for k in sorted(set(bears[:1].tolist() + bears[-1:].tolist() + wins[:1].tolist())):     # the first, the last, the first that wins
            c = g.clone()
            row = seq_off[i] + k
            for (o, d), die in zip(want[k], g12["seq_dies"][row].tolist()):
                assert c.tryMove(p[pl], die, o, d) == (True, ""), (i, k)
            assert position(c) == g12["states"][row].tolist(), (i, k)
            over = int(g12["over"][row])
            assert c.is_game_over() == ((True, over - 1) if over else (False, -1)), (i, k)
            played += 1; ended += over > 0
        assert position(g) == root, i
    return played, ended


def probes(case_set):
    """The tryMove probes of every lane, from the position alone (seeded): -> int32 [P, 6] rows (lane, kind, player, die, origin, dest).
    Whether a probe is legal is not decided here: the reference's tryMove accepts every bear-off from a point of the mover's,
    so an overrun the rules deny, a bear-off to the wrong end and one from outside the home board are all sent and all recorded."""
    st, mv, dc = case_set
    rng = np.random.RandomState(SEED + 1)
    K = {k: j for j, k in enumerate(PROBE_KINDS)}
    rows = []
    for i in range(len(st)):
        pl = int(mv[i])
        sign = 1 if pl == 0 else -1
        off_d, wrong_d, bar_o = (25, 0, 0) if pl == 0 else (0, 25, 25)
        own = [p for p in range(1, 25) if st[i, p - 1] * sign > 0]
        dist = (lambda p: 25 - p) if pl == 0 else (lambda p: p)
        inside = sorted((p for p in own if dist(p) <= 6), key=dist)
        outside = [p for p in own if dist(p) > 6]

        def add(kind, die, o, d, player=pl):
            rows.append((i, K[kind], player, int(die), int(o), int(d)))

        if inside:
            p = inside[rng.randint(len(inside))]
            add("exact", dist(p), p, off_d)
            far, near = inside[-1], inside[0]
            if dist(far) < 6:
                add("overrun_far", rng.randint(dist(far) + 1, 7), far, off_d)
            if near != far and dist(near) < 6:
                add("overrun_near", rng.randint(dist(near) + 1, 7), near, off_d)
            add("wrong_end", rng.randint(1, 7), p, wrong_d)
            if st[i, 24 + pl] > 0:
                add("point_while_on_bar", dist(p), p, off_d)
        if outside:
            add("from_outside", rng.randint(1, 7), outside[rng.randint(len(outside))], off_d)
        who = pl if st[i, 24 + pl] > 0 or st[i, 25 - pl] == 0 else 1 - pl       # a side that is on the bar, where there is one
        add("bar_to_off", rng.randint(1, 7), 0 if who == 0 else 25, 25 if who == 0 else 0, player=who)
        if own:
            p = own[rng.randint(len(own))]
            die = int(rng.randint(1, 7))
            if 1 <= p - sign * die <= 24:
                add("direction", die, p, p - sign * die)
            if 1 <= p + sign * die <= 24:
                add("dice_mismatch", 1 + die % 6, p, p + sign * die)
            held = [(o, k) for o in own for k in range(1, 7) if 1 <= o + sign * k <= 24 and st[i, o + sign * k - 1] * sign <= -2]
            if held:
                o, k = held[rng.randint(len(held))]
                add("blocked", k, o, o + sign * k)
            if 1 <= p + sign * die <= 24:
                add("forward", die, p, p + sign * die)
        anyp = own[0] if own else 12
        die = int(rng.randint(1, 7))
        if i % 4 == 0:                                       # one of the four per lane, in turn
            add("origin_m1", die, -1, 5)
        elif i % 4 == 1:
            add("origin_26", die, 26, 20)
        elif i % 4 == 2:
            add("dest_m1", die, anyp, -1)
        else:
            add("dest_26", die, anyp, 26)
    return np.array(rows, dtype=np.int32)


def probe_oracle(case_set, pr):
    """The oracle's tryMove on every probe, each on a fresh copy: -> (code int32 [P], resulting state int32 [P, 28])"""
    from oracle import oracle as O
    st, mv, _ = case_set
    inv = {v: k for k, v in O.ERR_MESSAGES.items()}
    code, after = np.zeros(len(pr), dtype=np.int32), np.zeros((len(pr), 28), dtype=np.int32)
    for j, (i, _, pl, die, o, d) in enumerate(pr.tolist()):
        s = O.State.from28(st[i], int(mv[i]))
        ok, msg = O.try_move(s, pl, die, o, d)
        code[j], after[j] = inv[msg], s.to28()
        assert ok == (code[j] == 0)
    return code, after


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    cs = cases()
    ans = enumerate_oracle(*cs)
    cnt, total, _ = census(cs, ans)
    dbl = int((cs[2][:, 0] == cs[2][:, 1]).sum())
    print("lanes %d (%d drawn, %d hand-built), doubles %d, sequences %d, distinct afterstates %d" % (
        len(cs[0]), N_RANDOM, len(cs[0]) - N_RANDOM, dbl, total, sum(len({tuple(r) for r in a[1].tolist()}) for a in ans)))
    names = list(CLASSES)
    rows = (len(names) + 2) // 3
    for r in range(rows):
        print("  " + "   ".join("%-32s %5d" % (names[k], cnt[names[k]]) for k in (r, r + rows, r + 2 * rows) if k < len(names)).rstrip())
    print("short:", {k: v for k, v in cnt.items() if v < MIN_LANES})
    pr = probes(cs)
    code, _ = probe_oracle(cs, pr)
    print("probes %d; per message:" % len(pr), np.bincount(code, minlength=8).tolist())
    print("per kind:", {k: int((pr[:, 1] == j).sum()) for j, k in enumerate(PROBE_KINDS)})
