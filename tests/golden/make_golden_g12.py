#!/usr/bin/env python3
"""Fixture G12 from the UNMODIFIED reference (build container only: the compiled reference engine in oracle/_ref, built by
`oracle/Makefile ref`; nothing of it copied).

  g12_endgame_boards.npz   the end-game positions of tests/endgame_cases.py (every lane of cases()) with their mover and dice.  For each:
        the reference's evaluateTurnSequences (ordered sequences, afterstates) and legalMoves of the mover for the dice 1..6;
        `seq_dies`, the die of every move of every sequence (on a plain roll the sequences that play the first die first come first:
        their number is counted with the reference's own legalMoves on clones);
        `over`, per sequence: -1 where the sequence bears nothing off, else is_game_over of a clone on which the sequence was played move
        by move through tryMove (0 not over, 1 / 2 over and PLAYER1 / PLAYER2 won) -- the clone's position is asserted to be the
        afterstate that evaluateTurnSequences gave;
        the tryMove probes of endgame_cases.probes(), each on a clone of the lane's game: `probe_code` (0 success, else the index of the
        message in `messages`) and, for the probes that succeeded, the position they left (`probe_after`, in probe order); a refused
        probe is asserted to leave the clone as it was.

Bar counts are built through setGameBoard + tryMove hits (rule_cases.reference_game).  The archive is written with fixed time stamps, so
that a second run gives the same bytes; the script checks that.

    python tests/golden/make_golden_g12.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from endgame_cases import PROBE_KINDS, cases, probes  # noqa: E402
from make_golden_g10 import load_reference  # noqa: E402
from make_golden_g11 import save_npz  # noqa: E402
from rule_cases import reference_game  # noqa: E402

DIES = (1, 2, 3, 4, 5, 6)
MESSAGES = ("", "Invalid origin", "Origin out of range", "Destination out of range", "Cannot move in that direction.",
            "Move does not match dice.", "Invalid destination.", "Cannot bear off from jail")


def position(g):
    return g.getGameBoard() + [g.getJailedCount(0), g.getJailedCount(1), g.getBornOffCount(0), g.getBornOffCount(1)]


def build():
    rb = load_reference()
    p1, p2 = rb.Player("a", rb.PlayerType.PLAYER1), rb.Player("b", rb.PlayerType.PLAYER2)
    case_set = cases()
    st, mover, dice = case_set
    pr = probes(case_set)
    n = len(st)
    n_seq, seqs, seq_len, seq_dies, states, over, n_moves, moves = [], [], [], [], [], [], [], []
    probe_code, probe_after = [], []
    by_lane = {}
    for row in pr.tolist():
        by_lane.setdefault(row[0], []).append(row)
    for i in range(n):
        g = reference_game(rb, p1, p2, st[i])
        root = st[i].tolist()
        assert position(g) == root and position(g.clone()) == root
        pl, d1, d2 = int(mover[i]), int(dice[i, 0]), int(dice[i, 1])
        who = p1 if pl == 0 else p2
        q, a = g.evaluateTurnSequences(pl, d1, d2)
        a = np.asarray(a, dtype=np.int32).reshape(-1, 28)
        assert len(q) == len(a)
        first = len(q)
        if d1 != d2:
            first = 0
            for o, d in g.legalMoves(pl, d1):
                c = g.clone()
                assert c.tryMove(who, d1, o, d) == (True, "")
                first += max(1, len(c.legalMoves(pl, d2)))
        n_seq.append(len(q))
        for k, s in enumerate(q):
            row, dies = np.zeros((4, 2), dtype=np.int8), np.zeros(4, dtype=np.int8)
            if s:
                row[:len(s)] = s
                dies[:len(s)] = ([d1, d2] if k < first else [d2, d1])[:len(s)] if d1 != d2 else d1
            seqs.append(row); seq_len.append(len(s)); seq_dies.append(dies)
            if a[k, 26 + pl] == root[26 + pl]:
                over.append(-1)
                continue
            c = g.clone()
            for (o, d), die in zip(s, dies.tolist()):
                assert c.tryMove(who, die, o, d) == (True, ""), (i, k)
            assert position(c) == a[k].tolist(), (i, k)
            is_over, winner = c.is_game_over()
            assert (winner in (0, 1)) == is_over
            over.append(1 + winner if is_over else 0)
        states.append(a)
        for die in DIES:
            m = g.legalMoves(pl, die)
            n_moves.append(len(m))
            moves.extend(m)
        for _, kind, player, die, o, d in by_lane.get(i, []):
            c = g.clone()
            ok, msg = c.tryMove(p1 if player == 0 else p2, die, o, d)
            assert ok == (msg == ""), (i, kind, msg)
            probe_code.append(MESSAGES.index(msg))
            if ok:
                probe_after.append(position(c))
            else:
                assert position(c) == root, (i, PROBE_KINDS[kind])
        assert position(g) == root                            # everything above worked on clones
    return dict(boards=st.astype(np.int8), mover=mover.astype(np.int8), dice=dice.astype(np.int8),
                n_seq=np.array(n_seq, dtype=np.int32), seqs=np.array(seqs, dtype=np.int8).reshape(-1, 4, 2),
                seq_len=np.array(seq_len, dtype=np.int8), seq_dies=np.array(seq_dies, dtype=np.int8).reshape(-1, 4),
                states=np.concatenate(states).astype(np.int8), over=np.array(over, dtype=np.int8),
                dies=np.array(DIES, dtype=np.int8), n_moves=np.array(n_moves, dtype=np.int32).reshape(n, len(DIES)),
                moves=np.array(moves, dtype=np.int8).reshape(-1, 2),
                probes=pr.astype(np.int16), probe_code=np.array(probe_code, dtype=np.int8),
                probe_after=np.array(probe_after, dtype=np.int8).reshape(-1, 28),
                messages=np.array(MESSAGES))


def main():
    path = os.path.join(HERE, "g12_endgame_boards.npz")
    save_npz(path, **build())
    with open(path, "rb") as f:
        once = f.read()
    save_npz(path, **build())
    with open(path, "rb") as f:
        assert f.read() == once, "a second run gave other bytes"
    print("%s: %d bytes, the same on a second run" % (os.path.basename(path), len(once)))


if __name__ == "__main__":
    main()
