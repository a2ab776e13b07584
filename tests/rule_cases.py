"""Bar-heavy positions for the board rules, and their census (no device, no torch).

helpers.random_boards never puts more than 2 checkers on a bar and the fixtures harvested from play hold a handful of lanes with 3.  This
set asks for what they leave out: bar counts 0..15 on both sides, entries on doubles that use three or four dice, entries that leave
checkers on the bar, hits that carry a bar count into the third and fourth count plane (3 -> 4, 7 -> 8) and entries that borrow out of
them (4 -> 3, 8 -> 7).

  cases()            -> (state28 int32 [N, 28], mover int32 [N], dice int32 [N, 2]): a seeded draw plus hand-built boards, N <= 4096.
                        Every board has 15 checkers a side and is not over.  About half the rolls are doubles.
  lane_classes(...)  -> the names of the classes below that one lane belongs to, decided from the oracle's enumeration
  census(set)        -> {class: lanes} and the set's total number of sequences; CLASSES lists every class, MIN_LANES is the condition
                        (tests/test_rule_cases_cpu.py): each class holds at least 8 lanes.

Classes (b = the mover's bar, ob = the opponent's, both at the root):
  bar_1 .. bar_8, bar_9_15, bar_15; obar_0 .. obar_8, obar_9_14; both_bars_ge3
  doubles   dbl_blocked (one empty sequence); dbl_enter{1,2,3}_full (b = e, some sequence plays all four dice);
            dbl_enter{1,2,3}_stuck (b = e, the bar is emptied and the longest sequence is shorter than 4);
            dbl_enter4_b4; dbl_enter4_b5plus (the bar is still occupied after the turn)
  plain     plain_both_blocked (zero sequences); plain_first_only_b1 / _b2plus, plain_second_only_b1 / _b2plus (one die enters);
            plain_both_enter_b2; plain_both_enter_b3plus (bar still occupied); plain_b1_other_elsewhere (b = 1 enters and the other die
            moves another checker)
  hits      entry_hits_blot; hits1_obar3plus, hits2_obar3plus, hits3plus_obar3plus (an afterstate with that many hits, ob >= 3);
            obar_cross_3_4, obar_cross_7_8 (ob <= 3 / 7 and an afterstate above it); bar_cross_4_3, bar_cross_8_7 (b >= 4 / 8 and an
            afterstate below it)
  after     dup_afterstates (more sequences than distinct afterstates); one_distinct (exactly one distinct afterstate)

Census of the committed set under the oracle (`python tests/rule_cases.py` prints it; fixture G11 holds the unmodified reference's
answers on exactly these lanes): 3198 lanes (2560 drawn, 638 hand-built), 1637 doubles rolls, 34 387 sequences, 11 630 distinct afterstates;
lanes per class, the smallest 36:
  bar_1                      623   obar_6                     247   plain_first_only_b2plus    158
  bar_2                      418   obar_7                     346   plain_second_only_b1        52
  bar_3                      342   obar_8                     185   plain_second_only_b2plus   160
  bar_4                      282   obar_9_14                  751   plain_both_enter_b2        117
  bar_5                      176   both_bars_ge3             1514   plain_both_enter_b3plus    661
  bar_6                      181   dbl_blocked                262   plain_b1_other_elsewhere   213
  bar_7                      167   dbl_enter1_full            188   entry_hits_blot           1099
  bar_8                      220   dbl_enter2_full            175   hits1_obar3plus            753
  bar_9_15                   605   dbl_enter3_full            157   hits2_obar3plus            290
  bar_15                     216   dbl_enter1_stuck           117   hits3plus_obar3plus         80
  obar_0                     348   dbl_enter2_stuck            36   obar_cross_3_4             218
  obar_1                     193   dbl_enter3_stuck            37   obar_cross_7_8             265
  obar_2                     223   dbl_enter4_b4              109   bar_cross_4_3              504
  obar_3                     422   dbl_enter4_b5plus          467   bar_cross_8_7              276
  obar_4                     182   plain_both_blocked         114   dup_afterstates           1245
  obar_5                     241   plain_first_only_b1         40   one_distinct              2276
The wrong readings of tests/rules_ref.py differ from the oracle on 1920 (a), 600 (b), 263 (c), 1712 (d), 2613 (e), 1099 (f) and 942 (g)
of these lanes.

Measured on the MI355X on this set (tests/test_gpu_rules_bar.py, its NETS-MAX lines; integer results are bit-exact): max |gpu - fp64|
over the 11 791 rows the greedy step hands to the value net, per parity family of tests/nets.py, against the 1e-5 bound --
  ckpt 1.75e-07   xavier 6.74e-08   ckpt_x4 9.33e-07   w1_x16 7.99e-07   normal 9.75e-07   normal_w1_x8 1.67e-06   loguniform 6.59e-07
the 2-ply search's v1 of every kept candidate 1.75e-07, evaluate_preroll on 128 roots (2639 rolls compared) 1.61e-07 (checkpoint).
"""
import numpy as np

SEED = 1103
N_RANDOM = 2560
N_RICH = 384                                   # the last of the random lanes: see _random_board
MIN_LANES = 8

_BAR = ["bar_%d" % k for k in range(1, 9)] + ["bar_9_15", "bar_15"]
_OBAR = ["obar_%d" % k for k in range(0, 9)] + ["obar_9_14"]
CLASSES = tuple(_BAR + _OBAR + ["both_bars_ge3",
                                "dbl_blocked", "dbl_enter1_full", "dbl_enter2_full", "dbl_enter3_full",
                                "dbl_enter1_stuck", "dbl_enter2_stuck", "dbl_enter3_stuck", "dbl_enter4_b4", "dbl_enter4_b5plus",
                                "plain_both_blocked", "plain_first_only_b1", "plain_first_only_b2plus", "plain_second_only_b1",
                                "plain_second_only_b2plus", "plain_both_enter_b2", "plain_both_enter_b3plus", "plain_b1_other_elsewhere",
                                "entry_hits_blot", "hits1_obar3plus", "hits2_obar3plus", "hits3plus_obar3plus",
                                "obar_cross_3_4", "obar_cross_7_8", "bar_cross_4_3", "bar_cross_8_7",
                                "dup_afterstates", "one_distinct"])

def mirror(st):
    """The same position with the sides exchanged: point p <-> 25 - p, signs flipped, bars and borne-off counts swapped."""
    st = np.asarray(st)
    out = np.empty_like(st)
    out[..., :24] = -st[..., 23::-1]
    out[..., 24], out[..., 25], out[..., 26], out[..., 27] = st[..., 25], st[..., 24], st[..., 27], st[..., 26]
    return out


def _scatter(rng, board, free, n, sign, lo, hi, max_points):
    """n checkers of one side on at most max_points of the free points lo..hi (0-based, inclusive); -> checkers placed"""
    cand = [p for p in range(lo, hi + 1) if free[p]]
    if n <= 0 or not cand or max_points <= 0:
        return 0
    k = min(len(cand), max_points, n)
    pts = rng.choice(cand, int(rng.randint(1, k + 1)), replace=False)
    for c in range(n):
        p = int(pts[c] if c < len(pts) else pts[rng.randint(len(pts))])
        board[p] += sign
        free[p] = False
    return n


_BAR_DRAW = [0] * 3 + list(range(1, 9)) * 3 + list(range(9, 16)) + [15, 15]
_OBAR_DRAW = [0] * 4 + list(range(1, 9)) * 3 + list(range(9, 15)) * 2 + [15]


def _random_board(rng, rich=False):
    """One board from the side of a mover who is PLAYER1 (enters on points 1..6); the caller mirrors it for PLAYER2.  rich: few checkers
    on the mover's bar and all the others on the board, on up to eight points -- long lists after the entries."""
    b, ob = int(_BAR_DRAW[rng.randint(len(_BAR_DRAW))]), int(_OBAR_DRAW[rng.randint(len(_OBAR_DRAW))])
    if rich:
        b = int((1, 1, 2, 3)[rng.randint(4)])
    board = np.zeros(24, dtype=np.int32)
    own, opp = 15 - b, 15 - ob
    kind = rng.randint(10)                                   # 0 closed board, 1-2 five-point board, else a mix
    if kind == 0 and opp >= 12:
        want = ["point"] * 6
    elif kind <= 2 and opp >= 10:
        want = ["point"] * 5 + [("blot", "own", "gap")[rng.randint(3)]]
        rng.shuffle(want)
    else:
        want = [("point", "blot", "blot", "own", "gap", "gap")[rng.randint(6)] for _ in range(6)]
    for p, w in enumerate(want):
        if w == "point" and opp >= 2:
            k = 2 + int(rng.randint(2)) if opp >= 3 else 2
            board[p] = -k; opp -= k
        elif w == "blot" and opp >= 1:
            board[p] = -1; opp -= 1
        elif w == "own" and own >= 1:
            k = min(own, 1 + int(rng.randint(3)))
            board[p] = k; own -= k
    free = [board[p] == 0 for p in range(24)]
    for p in range(6):
        free[p] = False                                      # the entry points keep what was drawn for them
    # the rest: scattered over points 7..24 or borne off.  Few points for the mover, so that the lists stay short
    k_own = int(rng.randint(0, own + 1)) if rng.rand() < 0.8 else 0
    if own == 15 - b and own > 14:
        k_own = max(k_own, 1)
    if rich:
        k_own = own
    own -= _scatter(rng, board, free, k_own, +1, 6, 23, int(rng.randint(3, 9)) if rich else int(rng.randint(1, 7)))
    k_opp = int(rng.randint(0, opp + 1)) if rng.rand() < 0.8 else 0
    if opp > 14:
        k_opp = max(k_opp, opp - 14)
    opp -= _scatter(rng, board, free, k_opp, -1, 6, 23, int(rng.randint(1, 7)))
    if own > 14 or opp > 14:                                 # nowhere to put them: the board would be over
        return None
    return np.concatenate([board, [b, ob, own, opp]]).astype(np.int32)


def _hand_built():
    """The classes a random draw does not reach (or reaches too rarely), from the side of a mover who is PLAYER1; every board is used for
    both movers.  -> list of (state28, d1, d2)"""
    out = []

    def add(points, b, ob, d1, d2, opp_extra=None):
        board = np.zeros(24, dtype=np.int32)
        for p, v in points.items():
            board[p - 1] = v
        own = 15 - b - int(np.clip(board, 0, None).sum())
        opp = 15 - ob - int(np.clip(-board, 0, None).sum())
        if opp_extra is not None and opp > 0:                # the opponent's remaining checkers on a far point that nobody reaches
            k = min(opp, opp_extra[1]); board[opp_extra[0] - 1] -= k; opp -= k
        assert 0 <= own <= 14 and 0 <= opp <= 14, (points, b, ob, own, opp)
        out.append((np.concatenate([board, [b, ob, own, opp]]).astype(np.int32), d1, d2))

    # doubles, entered e and then stuck: the entered checkers run along d, 2d, 3d, ... into an opponent point at m * d, every other
    # checker of the mover is borne off (e * (m - 1) < 4 moves in all) or sits right in front of that point
    for d in range(1, 7):
        for e, m in ((1, 2), (1, 3), (1, 4), (2, 2), (3, 2)):
            if m * d > 24:
                continue
            for ob in (0, 3, 7):
                add({m * d: -2}, e, ob, d, d, opp_extra=(24, 6))
            if (m - 1) * d > 6 and e * (m - 1) < 3:          # a checker that was there already: one die more, then stuck
                add({m * d: -2, (m - 1) * d: 1} if m > 2 else {m * d: -2}, e, 4, d, d)
    # hits in a chain from the bar with the opponent's bar already heavy: blots on d, 2d, 3d, 4d (doubles) and on d1, d1 + d2 (plain)
    for d in (1, 2, 3, 4, 5, 6):
        for ob in (3, 5, 7):
            for b in (1, 2, 4):
                add({k * d: -1 for k in range(1, 5) if k * d <= 24}, b, ob, d, d, opp_extra=(24 if 4 * d < 24 else 23, 4))
    for d1, d2 in ((1, 2), (2, 1), (3, 5), (6, 4), (5, 6), (4, 1)):
        for ob in (2, 3, 6, 7):
            for b in (1, 2, 4, 8):
                add({d1: -1, d2: -1, d1 + d2: -1, 20: 2}, b, ob, d1, d2, opp_extra=(24, 5))
    # one die enters, the other is blocked, with one and with many on the bar; the free die then moves a checker elsewhere or nothing
    for d1, d2 in ((1, 2), (2, 1), (3, 6), (6, 3), (5, 4), (4, 5), (2, 6), (6, 1)):
        for b in (1, 2, 3, 9):
            add({d2: -2, d1 + d2: -3, 15: 2}, b, 3, d1, d2, opp_extra=(24, 5))       # only the first die enters
            add({d1: -2, d1 + d2: -2}, b, 0, d1, d2, opp_extra=(23, 5))              # only the second
    # b = 15 and the opponent's bar heavy as well
    for d1, d2 in ((1, 1), (2, 5), (6, 6), (4, 3), (3, 3), (5, 1)):
        add({d1: -1}, 15, 9, d1, d2)
        add({d2: -2}, 15, 12, d1, d2)
    return out


def cases():
    """-> (state28 int32 [N, 28], mover int32 [N], dice int32 [N, 2]), the same arrays on every call"""
    rng = np.random.RandomState(SEED)
    st, mv, dc = [], [], []
    while len(st) < N_RANDOM:
        rich = len(st) >= N_RANDOM - N_RICH
        s = _random_board(rng, rich)
        mover = int(rng.randint(2))
        d1, d2 = int(rng.randint(1, 7)), int(rng.randint(1, 7))
        if rng.rand() < 0.4 or (rich and s is not None and s[24] >= 2):   # (two or three to enter and then a free choice: doubles)
            d2 = d1
        if s is None:
            continue
        st.append(mirror(s) if mover else s); mv.append(mover); dc.append((d1, d2))
    for i, (s, d1, d2) in enumerate(_hand_built()):
        for mover in (0, 1):
            st.append(mirror(s) if mover else s); mv.append(mover); dc.append((d1, d2))
    st, mv, dc = np.array(st, dtype=np.int32), np.array(mv, dtype=np.int32), np.array(dc, dtype=np.int32)
    assert len(st) <= 4096
    assert (np.clip(st[:, :24], 0, None).sum(1) + st[:, 24] + st[:, 26] == 15).all()
    assert (np.clip(-st[:, :24], 0, None).sum(1) + st[:, 25] + st[:, 27] == 15).all()
    assert (st[:, 24:] >= 0).all() and (st[:, 26:] < 15).all()
    return st, mv, dc


def lane_classes(s28, mover, d1, d2, seqs, states, enters1, enters2):
    """seqs: the lane's ordered sequences as lists of (origin, dest); states [C, 28] their afterstates; enters1 / enters2: whether
    legalMoves(die) is non-empty at the root for d1 / d2 -- all of them the oracle's.  -> set of class names"""
    b, ob = int(s28[24 + mover]), int(s28[25 - mover])
    bar_o = 0 if mover == 0 else 25
    c = set()
    if 1 <= b <= 8:
        c.add("bar_%d" % b)
    if b >= 9:
        c.add("bar_9_15")
    if b == 15:
        c.add("bar_15")
    if ob <= 8:
        c.add("obar_%d" % ob)
    elif ob <= 14:
        c.add("obar_9_14")
    if b >= 3 and ob >= 3:
        c.add("both_bars_ge3")
    n = len(seqs)
    longest = max((len(q) for q in seqs), default=0)
    ab = states[:, 24 + mover] if n else np.zeros(0, dtype=np.int32)
    aob = states[:, 25 - mover] if n else np.zeros(0, dtype=np.int32)
    if d1 == d2 and b >= 1:
        if n == 1 and longest == 0:
            c.add("dbl_blocked")
        elif b <= 3:
            assert (ab == 0).all()                           # an open entry point stays open: the bar empties
            c.add("dbl_enter%d_%s" % (b, "full" if longest == 4 else "stuck"))
        elif b == 4:
            c.add("dbl_enter4_b4")
        else:
            assert (ab == b - 4).all()
            c.add("dbl_enter4_b5plus")
    if d1 != d2 and b >= 1:
        if n == 0:
            c.add("plain_both_blocked")
        elif enters1 and not enters2:
            c.add("plain_first_only_b1" if b == 1 else "plain_first_only_b2plus")
        elif enters2 and not enters1:
            c.add("plain_second_only_b1" if b == 1 else "plain_second_only_b2plus")
        elif b == 2:
            c.add("plain_both_enter_b2")
        elif b >= 3:
            c.add("plain_both_enter_b3plus")
        if b == 1 and any(len(q) == 2 and q[0][0] == bar_o and q[1][0] != q[0][1] for q in seqs):
            c.add("plain_b1_other_elsewhere")
    if b >= 1:
        for q in seqs:
            if q and q[0][0] == bar_o and int(s28[q[0][1] - 1]) == (-1 if mover == 0 else 1):
                c.add("entry_hits_blot")
                break
    if n:
        hits = aob - ob
        if ob >= 3:
            if (hits == 1).any():
                c.add("hits1_obar3plus")
            if (hits == 2).any():
                c.add("hits2_obar3plus")
            if (hits >= 3).any():
                c.add("hits3plus_obar3plus")
        if ob <= 3 and (aob >= 4).any():
            c.add("obar_cross_3_4")
        if ob <= 7 and (aob >= 8).any():
            c.add("obar_cross_7_8")
        if b >= 4 and (ab <= 3).any():
            c.add("bar_cross_4_3")
        if b >= 8 and (ab <= 7).any():
            c.add("bar_cross_8_7")
        distinct = len({tuple(int(v) for v in r) for r in states})
        if n > distinct:
            c.add("dup_afterstates")
        if distinct == 1:
            c.add("one_distinct")
    return c


def enumerate_oracle(st, mv, dc):
    """The oracle's answer for every lane: -> list of (seqs as lists, states [C, 28], [legal_moves(mover, die) for die 1..6])"""
    from oracle import oracle as O
    out = []
    for i in range(len(st)):
        pl, d1, d2 = int(mv[i]), int(dc[i, 0]), int(dc[i, 1])
        s = O.State.from28(st[i], pl)
        q, ln, a = O.evaluate_turn_sequences(s, pl, d1, d2)
        out.append((O.sequences_as_lists(q, ln), a, [O.legal_moves(s, pl, die) for die in range(1, 7)]))
    return out


def reference_game(rb, p1, p2, s28):
    """A Game of the reference's pybind11 module `rb` (players p1, p2) that holds the position s28, bar counts included.  The binding has
    no setter for the bar, but setGameBoard replaces the 24 points only and leaves the bar counts alone, so setGameBoard + tryMove hits
    build them: PLAYER1's bar first, by bar1 + bar2 hits of a PLAYER2 that has nothing on the bar; then PLAYER2's, by bar2 entries of
    PLAYER1 that hit, each of which takes one checker off PLAYER1's bar again."""
    bar1, bar2 = int(s28[24]), int(s28[25])
    g = rb.Game(0)
    g.setPlayers(p1, p2)
    hit_p1 = [0] * 24
    hit_p1[1], hit_p1[2] = 1, -1                             # PLAYER2 moves 3 -> 2 onto PLAYER1's blot
    for _ in range(bar1 + bar2):
        g.setGameBoard(hit_p1)
        ok, msg = g.tryMove(p2, 1, 3, 2)
        assert ok, msg
    hit_p2 = [0] * 24
    hit_p2[0] = -1                                           # PLAYER1 enters with a 1 onto PLAYER2's blot
    for _ in range(bar2):
        g.setGameBoard(hit_p2)
        ok, msg = g.tryMove(p1, 1, 0, 1)
        assert ok, msg
    assert (g.getJailedCount(0), g.getJailedCount(1)) == (bar1, bar2)
    g.setGameBoard([int(v) for v in s28[:24]])
    g.setBorneOffPieces(0, int(s28[26])); g.setBorneOffPieces(1, int(s28[27]))
    return g


def census(case_set, answers=None):
    """-> ({class: lanes}, total sequences, per-lane class sets).  answers: enumerate_oracle's list, when the caller has it already."""
    st, mv, dc = case_set
    answers = answers if answers is not None else enumerate_oracle(st, mv, dc)
    counts = {k: 0 for k in CLASSES}
    per_lane, total = [], 0
    for i, (seqs, states, moves) in enumerate(answers):
        d1, d2 = int(dc[i, 0]), int(dc[i, 1])
        cl = lane_classes(st[i], int(mv[i]), d1, d2, seqs, states, bool(moves[d1 - 1]), bool(moves[d2 - 1]))
        for k in cl:
            counts[k] += 1
        per_lane.append(cl)
        total += len(seqs)
    return counts, total, per_lane


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    cs = cases()
    cnt, total, _ = census(cs)
    print("lanes %d, doubles %d, sequences %d" % (len(cs[0]), int((cs[2][:, 0] == cs[2][:, 1]).sum()), total))
    for k in CLASSES:
        print("  %-26s %5d%s" % (k, cnt[k], "" if cnt[k] >= MIN_LANES else "   <-- short"))
