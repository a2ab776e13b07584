"""The exact model of the temperature-sampled step (include/bgamd.h, bgamd_env_step_sampled; csrc/bg_sample.h), the lane set its tests
play, and the census of near ties the comparison with the device leaves out (tests/test_sample_model_cpu.py, tests/test_gpu_sampled.py).
A helper module, not a conftest; nothing is read from outside tests/golden.

The rule, restated: a lane's candidates are its evaluated rows (eight 32-bit plane words, key, stored fp32 value v); a = v for mover
PLAYER1 and -v for PLAYER2; d = a - max(a) in fp32; u = (2 (C.x >> 9) + 1) 2^-24 with
    A = P(row[0..3]; seed)    B = P(row[4..7] ^ A; seed)    C = P((gid_lo, gid_hi, ply, 2); (B.x, B.y))        P = Philox4x32-10
and the score is s = d / T - log(-log(u)).  The largest score is played; on equal scores the smallest key."""
import math
import os

import numpy as np

import nets as N

STREAM_SAMPLE = 2
SEED = 20240603                    # VecGame's default seed: the env the GPU tests create draws the noise the model draws
TEMPERATURES = (2.0 ** -6, 0.05, 1.0, 1e-30)
LANE_COUNTS = (1, 63, 65, 257, 1000)

# ---- the near-tie margin ------------------------------------------------------------------------------------------------------------------
# The device forms s = q - L2 in fp32 with q = fl(d / T), L1 = logf(u), L2 = logf(-L1).  The model forms d and q in fp32 as well: one
# IEEE subtraction and one IEEE division of fp32 numbers give the same bits on any machine, so q carries NO error against the model, and
# u is an fp32 number by construction.  What differs from the model's fp64 score is
#   (1) L1: HIP's logf is OCML's log_f32 (no fast-math flag in the build), a library written to the OpenCL specification, whose
#       documented bound for log is E = 3 ulp: |dL1| <= E 2^-23 |L1|;
#   (2) L2 = logf(-L1): the argument's relative error E 2^-23 becomes an absolute error E 2^-23 of the logarithm, and the function
#       adds E ulp of its own result: |dL2| <= E 2^-23 (1 + |L2|), with |L2| <= log(24 log 2) = 2.82 below and <= 24 log 2 = 16.64
#       above (2^-24 <= u <= 1 - 2^-24), so |dL2| <= 17.64 E 2^-23;
#   (3) the final subtraction: half an ulp of s, <= 0.5 2^-23 |s|.
# One score is therefore within 2^-23 (17.64 E + 0.5 max(1, |s|)) of the model's, the difference of two within
# 2^-23 (35.28 E + max(1, |s_1|, |s_2|)) <= 2^-23 (35.28 E + 1) max(1, |s_1|, |s_2|).  With E = 3 that is 106.84; times 4 as margin:
C_TOL = 4 * (35.28 * 3 + 1)        # 427.36


def tolerance(s1, s2):
    m = max(1.0, abs(s1), abs(s2) if math.isfinite(s2) else 0.0)
    return C_TOL * 2.0 ** -23 * m


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------

def planes(states28):
    """[m, 28] reference-layout states -> uint32 [m, 8]: csrc/bg_board.h's bit planes, no turn bit.  Words 0..3 are PLAYER1's count bits
    0..3, words 4..7 PLAYER2's; bit i is position i: PLAYER1 0 = bar, 1..24 points, 25 = borne off; PLAYER2 25 = bar, 0 = borne off."""
    st = np.asarray(states28, np.int64).reshape(-1, 28)
    a, b = np.zeros((len(st), 26), np.int64), np.zeros((len(st), 26), np.int64)
    a[:, 1:25], b[:, 1:25] = np.maximum(st[:, :24], 0), np.maximum(-st[:, :24], 0)
    a[:, 0], b[:, 25], a[:, 25], b[:, 0] = st[:, 24], st[:, 25], st[:, 26], st[:, 27]
    sh = np.arange(26)
    out = np.zeros((len(st), 8), np.uint32)
    for k in range(4):
        out[:, k] = (((a >> k) & 1) << sh).sum(1)
        out[:, 4 + k] = (((b >> k) & 1) << sh).sum(1)
    return out


def uniform_int(seed, gid, ply, row, by_key=None):
    """k of u = k 2^-24 for one row (eight plane words), through oracle.philox.  by_key (a WRONG model, for the tests that must tell):
    the noise keyed by the row's key instead of its planes."""
    from oracle import oracle as O
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    r = [int(x) for x in row] if by_key is None else [int(by_key), 0, 0, 0, 0, 0, 0, 0]
    A = O.philox(r[0], r[1], r[2], r[3], k0, k1)
    B = O.philox(r[4] ^ A[0], r[5] ^ A[1], r[6] ^ A[2], r[7] ^ A[3], k0, k1)
    Cc = O.philox(gid & 0xFFFFFFFF, gid >> 32, ply, STREAM_SAMPLE, B[0], B[1])
    return 2 * (Cc[0] >> 9) + 1


def gumbel(k):
    """-log(-log(k 2^-24)) in fp64, k an int or an integer array"""
    return -np.log(-np.log(np.asarray(k, np.float64) * 2.0 ** -24))


def mover_side(values, mover, flip=True):
    v = np.asarray(values, np.float32)
    return -v if (int(mover) == 1 and flip) else v


def quotient(values, mover, T, flip=True, divide=True):
    """q = d / T of every row, in fp32 as the kernel forms it (-inf where it overflows).  flip / divide False: two WRONG models."""
    a = mover_side(values, mover, flip)
    d = (a - a.max()).astype(np.float32)
    if not divide:
        return d
    with np.errstate(over="ignore", under="ignore"):
        return (d / np.float32(T)).astype(np.float32)


def pick(s, rows, keys):
    """-> (winner's position, gap): the largest score, on equal scores the smallest key; gap = its score minus the best score of a
    DIFFERENT afterstate (inf when there is none)"""
    s, keys = np.asarray(s, np.float64), np.asarray(keys, np.int64)
    top = np.where(s == s.max())[0]
    w = int(top[np.argmin(keys[top])])
    other = (np.asarray(rows) != np.asarray(rows)[w]).any(1)
    gap = float(s[w] - s[other].max()) if other.any() else math.inf
    return w, gap


def lane(rows, keys, values, mover, seed, gid, ply, T, ks=None):
    """One lane of the sampled step.  rows uint32 [m, 8], keys [m], values float32 [m] -> dict: k (the integers of u), s (fp64 scores),
    winner (position in the lists), gap, near (gap under the margin: the device may pick the runner-up).  ks: the integers, when the
    caller has them already (they do not depend on T)."""
    rows = np.asarray(rows, np.uint32).reshape(-1, 8)
    if ks is None:
        ks = np.array([uniform_int(seed, gid, ply, r) for r in rows], np.int64)
    s = quotient(values, mover, T).astype(np.float64) + gumbel(ks)
    w, gap = pick(s, rows, keys)
    s2 = s[w] - gap
    return {"k": ks, "s": s, "winner": w, "gap": gap, "near": gap < tolerance(s[w], s2)}


# ---- Philox4x32-10 over arrays, for the 200 000 draws of the softmax test (checked against oracle.philox there) ---------------------------

def philox_np(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = (np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(k0, k1))
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c


def uniform_ints_np(seed, gid, plies, rows):
    """k of every (ply, row): int64 [len(plies), len(rows)]"""
    rows = np.asarray(rows, np.uint64).reshape(-1, 8)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    A = philox_np(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], k0, k1)
    B = philox_np(rows[:, 4] ^ A[0], rows[:, 5] ^ A[1], rows[:, 6] ^ A[2], rows[:, 7] ^ A[3], k0, k1)
    plies = np.asarray(plies, np.uint64)[:, None]
    Cc = philox_np(gid & 0xFFFFFFFF, gid >> 32, plies, STREAM_SAMPLE, B[0][None, :], B[1][None, :])
    return (2 * (Cc[0] >> np.uint64(9)) + 1).astype(np.int64)


# ---- the lane set -------------------------------------------------------------------------------------------------------------------------

_set = []


def lane_set():
    """1 000 lanes, fixture G10's arbitrary boards (bear-offs, heavy stacks, lanes without a move) and fixture G8's bar positions in turn,
    each with its mover and dice -> (boards int32 [1000, 28], mover int32 [1000], dice int32 [1000, 2]).  The tests' smaller envs take
    the first n lanes."""
    if not _set:
        g = np.load(os.path.join(N.GOLDEN, "g10_arbitrary_boards.npz"))
        r8, t8, d8 = N.fixture_pairs("g8_bar_candidate_values")[:3]
        st, tu, dice = np.empty((1000, 28), np.int32), np.empty(1000, np.int32), np.empty((1000, 2), np.int32)
        st[0::2], tu[0::2], dice[0::2] = g["boards"][:500], g["dice"][:500, 0], g["dice"][:500, 1:]
        st[1::2], tu[1::2], dice[1::2] = r8[:500], t8[:500], d8[:500]
        _set.extend((st, tu, dice))
    return tuple(_set)


_cands = {}


def candidates(i):
    """lane i's turn sequences from the oracle, in reference order -> (states int32 [C, 28], seq int8 [C, 4, 2], seq_len int32 [C])"""
    if i not in _cands:
        from oracle import oracle as O
        st, tu, dice = lane_set()
        seq, ln, cand = O.evaluate_turn_sequences(O.State.from28(st[i], int(tu[i])), int(tu[i]), int(dice[i, 0]), int(dice[i, 1]))
        _cands[i] = (np.ascontiguousarray(cand, np.int32).reshape(-1, 28), seq, ln)
    return _cands[i]


def twin_pair(i):
    """Does lane i hold one afterstate reached by two turn sequences that are NOT the same checker moves in another order (the expansion
    drops the larger key of two orders of the same moves; what remains is evaluated twice, under two keys)?"""
    cand, seq, ln = candidates(i)
    seen = {}
    for c, s, l in zip(cand, seq, ln):
        moves = tuple(sorted((int(s[k, 0]), int(s[k, 1])) for k in range(int(l))))
        if seen.setdefault(c.tobytes(), moves) != moves:
            return True
    return False


def oracle_values(w, i):
    """the oracle's float32 forward pass over lane i's candidates"""
    from oracle import oracle as O
    cand = candidates(i)[0]
    tu = lane_set()[1]
    return O.forward_f32(w, O.encode(cand, int(tu[i]))) if len(cand) else np.zeros(0, np.float32)
