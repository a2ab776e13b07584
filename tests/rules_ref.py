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
and of the end-game rules (ENDGAME_VARIANTS; tests/test_endgame_cases_cpu.py holds them to the set of tests/endgame_cases.py):
  "h"  PLAYER2's overrun judged by PLAYER1's rule: only its own checkers on origin+1..7 deny it
  "i"  PLAYER1's overrun judged by PLAYER2's rule: a checker of either colour on origin+1..24 denies it
  "j"  PLAYER2's block range ends at point 6, not 7
  "k"  an overrun is always legal          "l"  an overrun is never legal
  "m"  bear-off allowed with a checker outside the home board
  "n"  bear-off allowed from a point while the mover is on the bar
  "o"  play goes on after the fifteenth checker is off: the turn passes and the game is not over (turn_end)
  "p"  no hit inside the mover's home board: an opposing blot there blocks like a made point
"""

VARIANTS = ("a", "b", "c", "d", "e", "f", "g")
ENDGAME_VARIANTS = ("h", "i", "j", "k", "l", "m", "n", "o", "p")
MESSAGES = ("", "Invalid origin", "Origin out of range", "Destination out of range", "Cannot move in that direction.",
            "Move does not match dice.", "Invalid destination.", "Cannot bear off from jail")


def _can_bear_off(s, player, die, origin, wrong=None):
    """a5 with Q1: bar empty, every checker home, and an overrun only when nothing sits behind -- PLAYER1's overrun is blocked by its own
    checkers on the higher points, PLAYER2's by ANY checker on the points origin+1..7."""
    if s[24 + player] != 0 and wrong != "n":
        return False
    outside = range(1, 19) if player == 0 else range(7, 25)
    sign = 1 if player == 0 else -1
    if wrong != "m" and any(s[p - 1] * sign > 0 for p in outside):
        return False
    if die > (25 - origin if player == 0 else origin):
        if wrong in ("k", "l"):
            return wrong == "k"
        above = range(origin + 1, 25) if player == 0 else range(origin + 1, 7 if wrong == "j" else 8)
        either = player == 1                                  # PLAYER2's rule looks at both colours, PLAYER1's at its own
        if (wrong == "h" and player == 1) or (wrong == "i" and player == 0):
            either = not either
        if any((s[p - 1] != 0) if either else (s[p - 1] * sign > 0) for p in above):
            return False
    return True


def legal_moves(s, player, die, entered=False, wrong=None):
    """a6: origins 0..25 ascending, the destination clamped to 0..25.  entered: a checker has entered in this turn (variant "a" only)."""
    sign = 1 if player == 0 else -1
    bar_origin = 0 if player == 0 else 25
    on_bar = s[24 + player] > 0
    out = []
    home = range(19, 25) if player == 0 else range(1, 7)
    for o in range(26):
        if on_bar and o != bar_origin and not (wrong == "a" and entered):
            if wrong == "n" and 1 <= o <= 24 and s[o - 1] * sign > 0 and not 1 <= o + sign * die <= 24 and _can_bear_off(s, player, die, o, wrong):
                out.append((o, min(25, max(0, o + sign * die))))
            continue
        if o == bar_origin:
            if not on_bar:
                continue
        elif not (1 <= o <= 24 and s[o - 1] * sign > 0):
            continue
        d = min(25, max(0, o + sign * die))
        if d == 0 or d == 25:
            ok = _can_bear_off(s, player, die, o, wrong)
        else:
            ok = s[d - 1] * sign >= (0 if wrong == "p" and d in home else -1)
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


def turn_end(after, player, wrong=None):
    """a4 after a turn of `player` that left `after`: -> (over, winner or -1, the side to move next: the winner's turn stays)"""
    if wrong != "o":
        for pl in (0, 1):
            if after[26 + pl] == 15:
                return True, pl, player
    return False, -1, 1 - player


def try_move(s, player, die, o, d):
    """a7 / Q6, the reference's order of checks: -> (message, the state afterwards -- unchanged where the move is refused)"""
    sign = 1 if player == 0 else -1
    bar_origin = 0 if player == 0 else 25
    if s[24 + player] > 0:
        valid = o == bar_origin
    else:
        valid = 1 <= o <= 24 and s[o - 1] * sign > 0
    if not valid:
        return MESSAGES[1], list(s)                           # (out-of-range origins end here: message 2 is never given)
    if not 0 <= d <= 25:
        return MESSAGES[3], list(s)
    if d in (0, 25):                                          # Q6: either end, any die, no look at the rest of the board
        if o in (0, 25):
            return MESSAGES[7], list(s)
        t = list(s)
        t[26 + player] += 1
        t[o - 1] -= sign
        return "", t
    if (d - o) * sign < 0:
        return MESSAGES[4], list(s)
    if die != abs(d - o):
        return MESSAGES[5], list(s)
    if s[d - 1] * sign < -1:
        return MESSAGES[6], list(s)
    return "", apply_move(s, player, o, d)
