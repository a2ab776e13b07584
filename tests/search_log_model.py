"""An exact model of the search log's entry (csrc/bg_search_log.h, bgamd_env_set_search_log in include/bgamd.h): what one search step of
either kind writes for one lane, or that it writes nothing.  numpy and integers only: no net is evaluated -- the kept candidates' values
come from the caller (the device's own, or any float32 numbers), so what is modelled is the RULE, bit for bit.

A lane is: its board (reference layout, 28 ints), its mover, whether it is live and takes part (not finished, not left out by
BGAMD_ONLY_P1/P2), and the step's kept list -- the kept candidates' reference-order indices, their states, the bit patterns of their v1 and
V2 and their terminal flags, in any order.  The step's kind is `filtered` (bgamd_env_step_search_filtered) or plain; the margin has done
its work when the kept list is handed in, so the only class it leaves to tell is "kept one candidate" (a singleton: not searched).
search_model.choose picks the played candidate."""
import numpy as np

import sample_model as P
import search_model as M

TURN_BIT = 1 << 31
QNAN = 0x7FC00000


def pack_row(state28, turn):
    """one reference-layout state and the side whose turn bit the row carries -> uint32 [8], the trajectory log's row"""
    row = P.planes(np.asarray(state28).reshape(1, 28))[0].copy()
    if int(turn):
        row[0] |= np.uint32(TURN_BIT)
    return row


def entry(board, mover, takes_part, kept_index, kept_states, v1_bits, v2_bits, terminal, filtered,
          after_bit=None, singleton_target=False, idle_lanes_log=False):
    """-> None (the lane writes nothing) or dict(rows uint32 [8], after uint32 [8], target uint32, v1 uint32).
    The three last arguments turn the model into the WRONG ones below."""
    mover = int(mover)
    if not takes_part and not idle_lanes_log:
        return None
    bit = 1 - mover if after_bit is None else after_bit(mover)
    out = dict(rows=pack_row(board, mover), after=pack_row(board, bit), target=np.uint32(QNAN), v1=np.uint32(QNAN))
    k = len(kept_index)
    if k == 0 or not takes_part:
        return out
    j = M.choose(np.asarray(kept_index, np.int64), np.asarray(v2_bits, np.uint32), mover)
    out["after"] = pack_row(np.asarray(kept_states).reshape(k, 28)[j], bit)
    out["v1"] = np.uint32(np.asarray(v1_bits, np.uint32)[j])
    searched = k >= (2 if filtered else 1)
    if searched:
        out["target"] = np.uint32(np.asarray(v2_bits, np.uint32)[j])
        if np.asarray(terminal, bool)[j]:              # a terminal candidate's V2 is its exact outcome, as its v1 is
            assert out["target"] == out["v1"] == M.bits(np.float32(1.0 if mover == 0 else 0.0).reshape(1))[0]
    elif singleton_target:
        out["target"] = out["v1"]
    return out


def entry_plain(board, mover, takes_part, kept_index, kept_states, v1_bits, v2_bits, terminal, filtered):
    """The header's sentences again, in plain Python: loops and ints, nothing shared with entry() but the reading of the layout."""
    if not takes_part:
        return None
    mover = int(mover)

    def row(s, turn):
        s = [int(x) for x in s]
        a, b = [0] * 26, [0] * 26                      # PLAYER1: 0 bar, 1..24 points, 25 off; PLAYER2: 25 bar, 0 off
        for i in range(24):
            if s[i] > 0:
                a[i + 1] = s[i]
            elif s[i] < 0:
                b[i + 1] = -s[i]
        a[0], b[25], a[25], b[0] = s[24], s[25], s[26], s[27]
        w = [0] * 8
        for pos in range(26):
            for k in range(4):
                w[k] |= ((a[pos] >> k) & 1) << pos
                w[4 + k] |= ((b[pos] >> k) & 1) << pos
        if turn:
            w[0] |= TURN_BIT
        return w

    opp = 1 - mover
    best = None
    for q in range(len(kept_index)):
        v = int(v2_bits[q])
        side = v if mover == 0 else -v                 # values in [0, 1]: their bit patterns order as they do
        if best is None or side > best[0] or (side == best[0] and int(kept_index[q]) < best[1]):
            best = (side, int(kept_index[q]), q)
    if best is None:
        return dict(rows=row(board, mover), after=row(board, opp), target=QNAN, v1=QNAN)
    q = best[2]
    was_searched = len(kept_index) >= 2 or not filtered
    return dict(rows=row(board, mover), after=row(kept_states[q], opp), target=int(v2_bits[q]) if was_searched else QNAN,
                v1=int(v1_bits[q]))


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(np.asarray(a[k], np.uint32), np.asarray(b[k], np.uint32)) for k in ("rows", "after", "target", "v1"))


# three deliberately wrong models: tests/test_search_log_model_cpu.py must tell each from entry()
WRONG = {
    "movers_bit_in_after": dict(after_bit=lambda mover: mover),
    "v1_as_singleton_target": dict(singleton_target=True),
    "idle_lanes_log": dict(idle_lanes_log=True),
}
