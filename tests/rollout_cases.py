"""The host schedule of bgamd_env_rollout restated in plain Python (from include/bgamd.h and the rules of rollout_plan in
csrc/bg_rollout_plan.h), and the cases the edge tests run: the horizon table, the position sets and the fp64 reference of the calls that are
compared with it.  No device, no torch.  Shared by tests/test_rollout_cases_cpu.py, which states the conditions the GPU tests rest on,
and tests/test_gpu_rollout_edges.py."""
import functools
import os

import numpy as np

import outcome_ref as OR
import rollout_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 4242
ROLLOUT_LANES = 65536          # the default lane count's ceiling
ROLLOUT_RUN = 8                # turns per run when nothing limits it


# ---- the rules -------------------------------------------------------------------------------------------------------------------------

def run_length(M, rotate, plies=1):
    """Turns per run between two refill points (rollout_info()[3]).  A 2-ply turn is a run of its own.  M = 0: 8.  Else, with D the
    turns a seated trial has left at its start (a rotated trial starts at ply 1): 1 when D < 1, else the largest divisor of D not
    above 8, so that every trial's M-th turn ends a run."""
    if plies == 2:
        return 1
    if M == 0:
        return ROLLOUT_RUN
    D = M - (1 if rotate else 0)
    if D < 1:
        return 1
    return max(r for r in range(1, ROLLOUT_RUN + 1) if D % r == 0)


def default_lanes(N):
    """lanes = 0: min(65 536, N rounded up to 256)"""
    return min(ROLLOUT_LANES, -(-N // 256) * 256)


def first_dice(T):
    """int32 [T, 2]: rotation plays trial i's turn 0 with ordered pair i % 36, d1 = 1 + (i % 36) / 6, d2 = 1 + (i % 36) % 6"""
    k = np.arange(T) % 36
    return np.stack([1 + k // 6, 1 + k % 6], 1).astype(np.int32)


def fan_size(T):
    """fan entries per position under rotation: one per ordered pair that some trial uses"""
    return min(T, 36)


# ---- the horizons ----------------------------------------------------------------------------------------------------------------------

# (M, rotate): every run length 1..8; D < 1; D = 1 with and without rotation; a prime D > 8 (run length 1) without and with rotation;
# exactly two and three runs of 8 without and with rotation
HORIZONS = [(1, True), (1, False), (2, True), (3, True), (3, False), (4, False), (5, False), (6, True), (7, True), (7, False),
            (8, False), (9, True), (11, False), (12, True), (16, False), (17, True), (24, False), (25, True)]
# the horizons whose calls are also compared with the fp64 reference (tests/rollout_ref.py), on the live positions
REF_HORIZONS = [(1, True), (1, False), (2, True), (11, False)]
SWEEP_T, SWEEP_OFFSET = 37, 3          # rotation wraps once; trial ids start at 3 T


# ---- the positions ---------------------------------------------------------------------------------------------------------------------

def weights():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "tdgammonNEW100k.f32"), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _g10():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_arbitrary_boards.npz"))
    return g["boards"].astype(np.int32), g["dice"][:, 0].astype(np.int32)


def g10_picks():
    """six fixture boards spread over the file, side to move from the fixture"""
    st, tu = _g10()
    idx = 3 + np.arange(6) * (len(st) // 6)
    return st[idx], tu[idx]


def late_boards(n):
    """the first n fixture boards late in the game: both sides with eight to ten checkers off (five or more left: no roll ends the
    game at once) and none on a bar"""
    st, tu = _g10()
    ok = (st[:, 26] >= 8) & (st[:, 27] >= 8) & (st[:, 26] <= 10) & (st[:, 27] <= 10) & (st[:, 24] == 0) & (st[:, 25] == 0)
    idx = np.nonzero(ok)[0][:n]
    assert len(idx) == n
    return st[idx], tu[idx]


def bar_position():
    """PLAYER1 to move with a checker on its bar against six made points: every roll is a pass"""
    return OR._state(p1=[(24, 5), (23, 5), (22, 4)], p2=[(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 3)], bar1=1), 0


N_LIVE = 7                                             # start + six fixture boards: positions()[:N_LIVE]
KINDS = ("start",) + ("g10",) * 6 + ("forced",) * 10 + ("over",) * 2 + ("bar",)


def positions():
    """-> (states [20, 28], turn [20], kind [20]): the start position, six fixture boards, the ten forced positions (they end on their
    first turn; the last of them only for a roll holding a 1), two boards that are over, the bar position"""
    gst, gtu = g10_picks()
    fst, ftu, _, _ = OR.forced_positions()
    ost, _ = OR.over_boards()
    bst, btu = bar_position()
    st = np.concatenate([OR.START[None], gst, fst, ost, bst[None]]).astype(np.int32)
    tu = np.concatenate([[0], gtu, ftu, [0, 1], [btu]]).astype(np.int32)
    assert len(st) == len(KINDS)
    return st, tu, np.array(KINDS)


def skip_heavy():
    """-> (states [40, 28], turn [40], kind [40]): a batch for the seat loop.  Thirty positions are over before a lane plays a turn of
    them under rotation (the two boards that are over and the nine forced positions that end with any roll), interleaved three to one
    with ten live ones (nine late fixture boards and the forced position that ends only for a roll holding a 1)."""
    fst, ftu, _, _ = OR.forced_positions()
    ost, _ = OR.over_boards()
    lst, ltu = late_boards(9)
    skip = [(ost[k], k, "over") for k in range(2)] + [(fst[k], int(ftu[k]), "forced") for k in range(9)]
    live = [(lst[k], int(ltu[k]), "late") for k in range(9)] + [(fst[9], int(ftu[9]), "forced8")]
    rows = []
    for k in range(10):
        rows += [skip[(3 * k + q) % len(skip)] for q in range(3)] + [live[k]]
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows]))


def known_result(state, kind):
    """a position that is over, or a forced position that ends with any roll -> (value, turns, points) of every trial"""
    if kind == "over":
        pts = OR.points(state)
        return (1.0 if pts > 0 else 0.0), 0, pts
    fst, _, fpts, _ = OR.forced_positions()
    k = [q for q in range(9) if (fst[q] == state).all()]
    assert kind == "forced" and len(k) == 1
    pts = int(fpts[k[0]])
    return (1.0 if pts > 0 else 0.0), 1, pts


# ---- the fp64 reference of the sweep's calls ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sweep_reference(M, rotate):
    """rollout_ref.rollout of the sweep's call at horizon (M, rotate) on the live positions (computed once per process)"""
    st, tu, _ = positions()
    return R.rollout(weights(), st[:N_LIVE], tu[:N_LIVE], SWEEP_T, SEED, max_plies=M, rotate=rotate, position_offset=SWEEP_OFFSET)
