#!/usr/bin/env python3
"""Fixture G11 from the UNMODIFIED reference (build container only: the compiled reference engine in oracle/_ref, built by
`oracle/Makefile ref`; nothing of it copied).

  g11_bar_boards.npz   the bar-heavy positions of tests/rule_cases.py (every lane of cases(): both bars 0..15, closed and five-point
        boards, hand-built stuck and chain-hit boards) with their mover and dice.  For each: the reference's evaluateTurnSequences
        (ordered sequences, afterstates) and legalMoves of the mover for the dice 1..6.

The binding has no setter for the bar, but its public surface reaches every pair of bar counts: setGameBoard replaces the 24 points only
and leaves the bar counts alone, so repeated setGameBoard + tryMove hits build them.  PLAYER1's bar first, by hits of a PLAYER2 that has
nothing on the bar (bar1 + bar2 of them); then PLAYER2's, by bar2 entries of PLAYER1 that hit -- each takes one checker off PLAYER1's bar
again.  A last setGameBoard / setBorneOffPieces sets the position (rule_cases.reference_game).  getJailedCount is asserted to equal the
intended bars before a lane is recorded.

The archive is written with fixed time stamps, so that a second run gives the same bytes.

    python tests/golden/make_golden_g11.py
"""
import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden_g10 import load_reference  # noqa: E402
from rule_cases import cases, reference_game  # noqa: E402

DIES = (1, 2, 3, 4, 5, 6)


def save_npz(path, **arrays):
    """np.savez_compressed with fixed time stamps (numpy stamps every member with the time of the run)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rb = load_reference()
    p1, p2 = rb.Player("a", rb.PlayerType.PLAYER1), rb.Player("b", rb.PlayerType.PLAYER2)
    st, mover, dice = cases()
    n = len(st)
    n_seq, seqs, seq_len, states, n_moves, moves = [], [], [], [], [], []
    for i in range(n):
        g = reference_game(rb, p1, p2, st[i])
        assert g.getGameBoard() == st[i, :24].tolist()
        assert (g.getJailedCount(0), g.getJailedCount(1), g.getBornOffCount(0), g.getBornOffCount(1)) == tuple(st[i, 24:].tolist())
        pl, d1, d2 = int(mover[i]), int(dice[i, 0]), int(dice[i, 1])
        q, a = g.evaluateTurnSequences(pl, d1, d2)
        a = np.asarray(a, dtype=np.int32).reshape(-1, 28)
        assert len(q) == len(a)
        n_seq.append(len(q))
        for s in q:
            row = np.zeros((4, 2), dtype=np.int8)
            if s:
                row[:len(s)] = s
            seqs.append(row); seq_len.append(len(s))
        states.append(a)
        for die in DIES:
            m = g.legalMoves(pl, die)
            n_moves.append(len(m))
            moves.extend(m)
        assert (g.getJailedCount(0), g.getJailedCount(1)) == (int(st[i, 24]), int(st[i, 25]))     # enumeration works on clones
    save_npz(os.path.join(HERE, "g11_bar_boards.npz"), boards=st.astype(np.int8), mover=mover.astype(np.int8), dice=dice.astype(np.int8),
             n_seq=np.array(n_seq, dtype=np.int32), seqs=np.array(seqs, dtype=np.int8).reshape(-1, 4, 2),
             seq_len=np.array(seq_len, dtype=np.int8), states=np.concatenate(states).astype(np.int8),
             dies=np.array(DIES, dtype=np.int8), n_moves=np.array(n_moves, dtype=np.int32).reshape(n, len(DIES)),
             moves=np.array(moves, dtype=np.int8).reshape(-1, 2))


if __name__ == "__main__":
    main()
