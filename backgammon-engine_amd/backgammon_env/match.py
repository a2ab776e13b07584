"""Match play on the cubeful rollouts (include/bgamd.h, bgamd_env_rollout_match): a match equity table and the score of each position.

    table = MatchTable.load("my_table.json")           # a published table the user brings; none is shipped
    table = MatchTable.janowski(7)                     # or the stated approximation
    r = env.rollout(st, turn, 1296, variance_reduction=True, cube=Cube(), match=Match(table, away1=3, away2=5))
    r["mwc"], r["mwc_stderr"], r["match_counts"]

No device and no torch in here: numpy only."""
import json
import math

import numpy as np

MAX_POINTS = 64                                        # the largest table of the C ABI
NORMAL, CRAWFORD, POST_CRAWFORD = 0, 1, 2


class MatchTable:
    """met [M, M]: met[a-1][b-1] = the chance that a side needing a points beats a side needing b; the 1-away row and column hold the
    Crawford-game values.  met_pc [M]: met_pc[k-1] = the post-Crawford chance of a trailer needing k against a leader needing 1
    (met_pc[0]: double match point).  Every entry in [0, 1]."""

    def __init__(self, met, met_pc):
        self.met = np.ascontiguousarray(np.asarray(met, dtype=np.float64))
        self.met_pc = np.ascontiguousarray(np.asarray(met_pc, dtype=np.float64).reshape(-1))
        M = self.met_pc.shape[0]
        if self.met.shape != (M, M) or not 1 <= M <= MAX_POINTS:
            raise ValueError("MatchTable: met must be [M, M] and met_pc [M], 1 <= M <= %d" % MAX_POINTS)
        for t in (self.met, self.met_pc):
            if not (np.isfinite(t).all() and (t >= 0.0).all() and (t <= 1.0).all()):
                raise ValueError("MatchTable: every entry is a chance in [0, 1]")

    @property
    def M(self):
        return self.met_pc.shape[0]

    @classmethod
    def load(cls, path):
        """A JSON file {"met": [[...], ...], "met_pc": [...]}, or a plain text file of numbers separated by blanks, commas or line
        ends ('#' starts a comment): the M x M entries of met row by row, then the M of met_pc -- M follows from their count."""
        with open(path) as f:
            text = f.read()
        if text.lstrip().startswith("{"):
            d = json.loads(text)
            return cls(d["met"], d["met_pc"])
        nums = [float(w) for line in text.splitlines() for w in line.split("#")[0].replace(",", " ").split()]
        M = (math.isqrt(4 * len(nums) + 1) - 1) // 2
        if M < 1 or M * M + M != len(nums):
            raise ValueError("MatchTable.load: %d numbers are no M x M table followed by M post-Crawford entries" % len(nums))
        return cls(np.array(nums[:M * M]).reshape(M, M), nums[M * M:])

    @classmethod
    def janowski(cls, M):
        """An APPROXIMATION, no published table: the chance of the side needing a against the side needing b is 0.5 + 0.85 D / (T + 6)
        with D = b - a and T = a + b, clamped to [0, 1] (Janowski's formula); the trailer's entry is 1.0 minus the leader's, so the
        table is complementary bit for bit.  Post-Crawford: met_pc[k-1] = 0.5 ** ceil(k / 2) (the free drop ignored)."""
        M = int(M)
        met = np.full((M, M), 0.5)
        for a in range(1, M + 1):
            for b in range(a + 1, M + 1):
                v = min(1.0, max(0.0, 0.5 + 0.85 * float(b - a) / float(a + b + 6)))
                met[a - 1, b - 1], met[b - 1, a - 1] = v, 1.0 - v
        return cls(met, [0.5 ** ((k + 1) // 2) for k in range(1, M + 1)])

    def after(self, a1, a2, state):
        """The MWC of the side needing a1 when the next game starts against a side needing a2 (include/bgamd.h, after)."""
        a1, a2 = int(a1), int(a2)
        if a1 <= 0:
            return 1.0
        if a2 <= 0:
            return 0.0
        if state != NORMAL and a2 == 1:
            return float(self.met_pc[a1 - 1])
        if state != NORMAL and a1 == 1:
            return 1.0 - float(self.met_pc[a2 - 1])
        return float(self.met[a1 - 1, a2 - 1])


class Match:
    """The match setting of VecGame.rollout(match=...): a MatchTable and, per position (scalars or one entry each), PLAYER1's and
    PLAYER2's points to go and the state -- 0 normal, 1 the Crawford game, 2 post-Crawford.  state=None derives it: 0 where no side is
    1-away; where one is, the score does not say whether this is the Crawford game, so the caller must (ValueError).
    window_share: where in the window between the point at which doubling stops losing and the opponent's take point the roller
    starts to double.  The default 0.5 is a rule of thumb and no measured optimum."""

    def __init__(self, table, away1, away2, state=None, window_share=0.5):
        if not isinstance(table, MatchTable):
            raise ValueError("Match: table is a MatchTable")
        self.table = table
        self.away1 = np.asarray(away1, dtype=np.int64)
        self.away2 = np.asarray(away2, dtype=np.int64)
        if state is None:
            if (np.minimum(self.away1, self.away2) <= 1).any():
                raise ValueError("Match: a side is 1-away; say whether this is the Crawford game (state=1) or after it (state=2)")
            state = 0
        self.state = np.asarray(state, dtype=np.int64)
        self.window_share = float(window_share)

    def per_position(self, P):
        """-> (away1, away2, state), each int32 [P]"""
        return tuple(np.ascontiguousarray(np.broadcast_to(x, (P,)).astype(np.int32)) for x in (self.away1, self.away2, self.state))
