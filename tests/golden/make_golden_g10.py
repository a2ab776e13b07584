#!/usr/bin/env python3
"""Fixture G10 from the UNMODIFIED reference (build container only: the compiled reference engine in oracle/_ref, built by
`oracle/Makefile ref`; nothing of it copied).

  g10_arbitrary_boards.npz   positions that play never reaches -- tests/helpers.random_boards(1500, 7, with_bar=False): random
        placement, heavy stacks, late bear-off boards -- with (player, die1, die2) drawn from RandomState(8), every fifth a double.
        For each: the reference's evaluateTurnSequences (ordered sequences, afterstates) and legalMoves for the dice 1, 4 and 6.
        The bar counts stay 0 here; make_golden_g11.py builds bar counts 0..15 through hits and records the bar-heavy boards.

    python tests/golden/make_golden_g10.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import random_boards  # noqa: E402

N_BOARDS, BOARD_SEED, DICE_SEED, DIES = 1500, 7, 8, (1, 4, 6)


def boards_and_dice():
    """The inputs, in the order the test draws them."""
    st = random_boards(N_BOARDS, BOARD_SEED, with_bar=False)
    rng = np.random.RandomState(DICE_SEED)
    dice = np.zeros((N_BOARDS, 3), dtype=np.int32)
    for i in range(N_BOARDS):
        pl, d1, d2 = int(rng.randint(2)), int(rng.randint(1, 7)), int(rng.randint(1, 7))
        dice[i] = pl, d1, d1 if i % 5 == 0 else d2
    return st, dice


def load_reference():
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = sorted(f for f in os.listdir(ref_dir) if f.startswith("backgammon_env") and f.endswith(".so"))
    spec = importlib.util.spec_from_file_location("backgammon_env", os.path.join(ref_dir, so[0]))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    return rb


def main():
    rb = load_reference()
    p1, p2 = rb.Player("a", rb.PlayerType.PLAYER1), rb.Player("b", rb.PlayerType.PLAYER2)
    st, dice = boards_and_dice()
    n_seq, seqs, seq_len, states, n_moves, moves = [], [], [], [], [], []
    for i in range(N_BOARDS):
        g = rb.Game(0)
        g.setPlayers(p1, p2)
        g.setGameBoard([int(v) for v in st[i, :24]])
        g.setBorneOffPieces(0, int(st[i, 26])); g.setBorneOffPieces(1, int(st[i, 27]))
        pl, d1, d2 = (int(x) for x in dice[i])
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
    np.savez_compressed(os.path.join(HERE, "g10_arbitrary_boards.npz"), boards=st.astype(np.int8), dice=dice.astype(np.int8),
                        n_seq=np.array(n_seq, dtype=np.int32), seqs=np.array(seqs, dtype=np.int8).reshape(-1, 4, 2),
                        seq_len=np.array(seq_len, dtype=np.int8), states=np.concatenate(states).astype(np.int8),
                        dies=np.array(DIES, dtype=np.int8), n_moves=np.array(n_moves, dtype=np.int32).reshape(N_BOARDS, len(DIES)),
                        moves=np.array(moves, dtype=np.int8).reshape(-1, 2))


if __name__ == "__main__":
    main()
