"""The board rules once more, in plain Python on int counts, with deliberately wrong variants (no device, no torch, no ctypes).

Written from the reference's behaviour as SURVEY.md §8(a) describes it (rows a3-a10 and the notes Q1-Q6), not from oracle/bg_oracle.c:
a second, independent reading that tests/test_rule_cases_cpu.py holds to the oracle on every lane of tests/rule_cases.py.  Each wrong
variant is one plausible misreading of the bar rules; the same test asserts that it differs from the oracle on at least 8 lanes of the
set, which is what makes the set worth running on the device.

A state is a list of 28 ints: 24 points (PLAYER1 positive, PLAYER2 negative), bar1, bar2, off1, off2.  Origins and destinations are the
reference's: 0 / 25 are PLAYER1's / PLAYER2's bar as an origin, 25 / 0 their bear-off as a destination.

Variants (`wrong=`):
  "a"  other checkers may move while the bar is still occupied, once one checker has entered in this turn
  "b"  a doubles turn ends when the bar is empty
  "c"  a blocked doubles roll yields zero sequences instead of one empty sequence
  "d"  bar counts kept modulo 8 (the top count plane lost)
  "e"  bar counts kept modulo 4
  "f"  an entering checker does not hit: the blot leaves the point but never reaches the bar
  "g"  the second-die-first block is dropped when both dice enter from the bar
"""

VARIANTS = ("a", "b", "c", "d", "e", "f", "g")


def _can_bear_off(s, player, die, origin):
    """a5 with Q1: bar empty, every checker home, and an overrun only when nothing sits behind -- PLAYER1's overrun is blocked by its own
    checkers on the higher points, PLAYER2's by ANY checker on the points origin+1..7."""
    if s[24 + player] != 0:
        return False
    if player == 0:
        if any(s[p - 1] > 0 for p in range(1, 19)):
            return False
        if die > 25 - origin and any(s[p - 1] > 0 for p in range(origin + 1, 25)):
            return False
    else:
        if any(s[p - 1] < 0 for p in range(7, 25)):
            return False
        if die > origin and any(s[p - 1] != 0 for p in range(origin + 1, 8)):
            return False
    return True


def legal_moves(s, player, die, entered=False, wrong=None):
    """a6: origins 0..25 ascending, the destination clamped to 0..25.  entered: a checker has entered in this turn (variant "a" only)."""
    sign = 1 if player == 0 else -1
    bar_origin = 0 if player == 0 else 25
    on_bar = s[24 + player] > 0
    out = []
    for o in range(26):
        if on_bar and o != bar_origin and not (wrong == "a" and entered):
            continue
        if o == bar_origin:
            if not on_bar:
                continue
        elif not (1 <= o <= 24 and s[o - 1] * sign > 0):
            continue
        d = min(25, max(0, o + sign * die))
        if d == 0 or d == 25:
            ok = _can_bear_off(s, player, die, o)
        else:
            ok = s[d - 1] * sign >= -1
        if ok:
            out.append((o, d))
    return out


def _wrap(s, wrong):
    if wrong == "d":
        s[24] &= 7; s[25] &= 7
    elif wrong == "e":
        s[24] &= 3; s[25] &= 3
    return s


def apply_move(s, player, o, d, wrong=None):
    """a7 for a move that legal_moves listed: leave the bar or the point, hit a blot, land -- or bear off.  -> a new state"""
    s = list(s)
    sign = 1 if player == 0 else -1
    if d == 0 or d == 25:
        s[26 + player] += 1
        s[o - 1] -= sign
        return s
    from_bar = o == 0 or o == 25
    if from_bar:
        s[24 + player] -= 1
    else:
        s[o - 1] -= sign
    if s[d - 1] * sign == -1:
        s[d - 1] = 0
        if not (wrong == "f" and from_bar):
            s[25 - player] += 1
    s[d - 1] += sign
    return _wrap(s, wrong)


def turn_sequences(s, player, d1, d2, wrong=None):
    """a8-a10 with Q2-Q4: -> (ordered sequences as lists of (origin, dest), their afterstates as lists of 28 ints)"""
    s = _wrap(list(s), wrong)
    bar_origin = 0 if player == 0 else 25
    seqs, states = [], []
    if d1 != d2:
        orders = [(d1, d2), (d2, d1)]
        if wrong == "g" and s[24 + player] > 0 and legal_moves(s, player, d1) and legal_moves(s, player, d2):
            orders = orders[:1]
        for da, db in orders:
            for m1 in legal_moves(s, player, da, wrong=wrong):
                s1 = apply_move(s, player, m1[0], m1[1], wrong)
                nxt = legal_moves(s1, player, db, entered=m1[0] == bar_origin, wrong=wrong)
                if not nxt:
                    seqs.append([m1]); states.append(s1)
                for m2 in nxt:
                    seqs.append([m1, m2]); states.append(apply_move(s1, player, m2[0], m2[1], wrong))
        return seqs, states
    had_bar = s[24 + player] > 0

    def dfs(cur, depth, path, entered):
        moves = legal_moves(cur, player, d1, entered=entered, wrong=wrong)
        if depth == 4 or not moves or (wrong == "b" and had_bar and depth > 0 and cur[24 + player] == 0):
            seqs.append(list(path)); states.append(cur)
            return
        for m in moves:
            path.append(m)
            dfs(apply_move(cur, player, m[0], m[1], wrong), depth + 1, path, entered or m[0] == bar_origin)
            path.pop()

    dfs(s, 0, [], False)
    if wrong == "c" and seqs == [[]]:
        return [], []
    return seqs, states
