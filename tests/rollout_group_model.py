"""The grouped rollout's two rules restated in plain Python (from include/bgamd.h: bgamd_env_rollout_grouped and
bgamd_env_rollout_paired_read), and the tables the GPU tests run.  No device, no torch.

  ids     trial i of position p rolls the dice of game id (group_offset + group[p]) * T + i; its result slot stays p * T + i
  paired  d_i = q_i(p) - q_i(r) in fp64; lane k of a 64-lane wave sums the trials k, k + 64, ... in order; the 64 partial sums go through
          the xor butterfly (masks 32, 16, ..., 1), lane 0's result; mean = sum / T; the squared deviations from it the same way;
          stderr = sqrt(sum / (T (T - 1))), 0 for T = 1.  A reference out of range or in another group: NaN, NaN.

Shared by tests/test_rollout_groups_cpu.py, which checks the model and states the conditions the GPU cases rest on, and
tests/test_gpu_rollout_groups.py."""
import math

import numpy as np

import rollout_cases as RC

WAVE = 64

# ---- the GPU tests' tables -----------------------------------------------------------------------------------------------------------

GROUPS = [3, 0, 3, 1, 0, 3, 5]                     # the main case: P = 7, groups out of order, apart from each other, with gaps
GROUP_OFFSET = 2
# rollout_cases.positions() of the main case: group 3 = start, a fixture board, a forced position; group 0 = two fixture boards;
# group 1 = a board that is over; group 5 = the bar position (every roll a pass)
PICKS = [0, 1, 2, 17, 3, 7, 19]
CASES = [(40, False, 0), (36, True, 0), (73, True, 4)]     # (T, rotate, M): 73 = one full 64-stride, a partial one, rotation wrapped twice
TWIN_GROUPS = [4, 4, 9]                            # one position three times: twice in group 4, once in group 9
TWIN_PICK = 2


def split_tables():
    """The main table as two calls that differ in group_offset: the positions whose group is below 3 with group_offset GROUP_OFFSET, the
    others with their groups counted from 3 and group_offset GROUP_OFFSET + 3.  -> [(position indices, groups, group_offset)] x 2"""
    lo = [p for p, g in enumerate(GROUPS) if g < 3]
    hi = [p for p, g in enumerate(GROUPS) if g >= 3]
    return [(lo, [GROUPS[p] for p in lo], GROUP_OFFSET), (hi, [GROUPS[p] - 3 for p in hi], GROUP_OFFSET + 3)]


def main_positions():
    st, tu, kind = RC.positions()
    return st[PICKS], tu[PICKS], kind[PICKS]


def twin_positions():
    st, tu, _ = RC.positions()
    k = [TWIN_PICK] * len(TWIN_GROUPS)
    return st[k], tu[k]


# ---- the id rule ---------------------------------------------------------------------------------------------------------------------

def trial_ids(groups, T, group_offset=0):
    """-> ids [P][T] (Python ints): the game id whose TURN-stream dice trial i of position p rolls"""
    return [[(group_offset + int(g)) * T + i for i in range(T)] for g in groups]


def slots(P, T):
    """-> [P][T]: where trial i of position p puts its result, whatever its group"""
    return [[p * T + i for i in range(T)] for p in range(P)]


def valid(groups, T, group_offset=0):
    """what bgamd_env_rollout_grouped accepts of a table (the other arguments being fine)"""
    return group_offset >= 0 and all(int(g) >= 0 for g in groups) and (max(int(g) for g in groups) + 1) * T < 2 ** 31


# ---- the paired statistic ------------------------------------------------------------------------------------------------------------

def wave_sum(vals):
    """vals[i], i < T, summed as a wave does: lane k adds vals[k], vals[k + 64], ... to 0.0 in order, then the xor butterfly"""
    s = [0.0] * WAVE
    for k in range(WAVE):
        for i in range(k, len(vals), WAVE):
            s[k] += vals[i]
    m = WAVE // 2
    while m >= 1:
        s = [s[k] + s[k ^ m] for k in range(WAVE)]
        m //= 2
    return s[0]


def paired(q, groups, p, r):
    """q [P][T] fp64 per-trial quantities -> (diff_mean, diff_stderr) of position p against reference r"""
    P, T = len(q), len(q[0])
    if not (0 <= r < P) or groups[r] != groups[p]:
        return math.nan, math.nan
    d = [float(q[p][i]) - float(q[r][i]) for i in range(T)]
    m = wave_sum(d) / float(T)
    ss = wave_sum([(x - m) * (x - m) for x in d])
    return m, (math.sqrt(ss / (float(T) * float(T - 1))) if T > 1 else 0.0)


def paired_fsum(q, groups, p, r):
    """the same numbers by exactly rounded sums"""
    P, T = len(q), len(q[0])
    if not (0 <= r < P) or groups[r] != groups[p]:
        return math.nan, math.nan
    d = [float(q[p][i]) - float(q[r][i]) for i in range(T)]
    m = math.fsum(d) / T
    return m, (math.sqrt(math.fsum((x - m) ** 2 for x in d) / (T * (T - 1))) if T > 1 else 0.0)


def unpaired_stderr(q, p, r):
    """sqrt(se_p^2 + se_r^2): what two independent rollouts would give for the difference"""
    def se2(x):
        T = len(x)
        m = math.fsum(x) / T
        return math.fsum((v - m) ** 2 for v in x) / (T * (T - 1))
    return math.sqrt(se2([float(v) for v in q[p]]) + se2([float(v) for v in q[r]]))


def mean_tolerance(T):
    """|model - exact| for diff_mean: at most T additions of numbers of size <= 3 (a difference of equities), each rounded to 2^-53
    relative of a partial sum <= 3 T -- far inside T 2^-52 once divided by T"""
    return T * 2.0 ** -52


def close(a, b, T, stderr=False):
    """the bounds of tests/test_rollout_groups_cpu.py and of the GPU tests: diff_mean within T 2^-52 absolute; diff_stderr within rtol
    1e-12 (the plain statistics' own, tests/test_gpu_rollout.py) plus atol T 2^-52 (a constant non-zero difference: the sum of squares
    is rounding noise around 0)"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    tol = mean_tolerance(T) + (1e-12 * abs(b) if stderr else 0.0)
    return abs(a - b) <= tol
