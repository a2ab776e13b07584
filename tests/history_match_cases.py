"""The match play entries of the history tests (tests/history_cases.py holds the rest and stays as it is): the probe whose results may
not depend on what the env did before, the steps that leave larger and other match state behind, and the read call of include/bgamd.h
that can be refused.  No device, no torch: the match tables are built by the caller's `Match` and `MatchTable` (backgammon_env.match).

bgamd_env_rollout_match_results is the one refusable read call of the header whose name does not end in _read (tests/history_cases.py
enumerates those): tests/test_history_match_cpu.py holds this table against the header with a pattern that takes _results in too, so a
further read call of either spelling has to be listed in one of the two places."""
import history_cases as H

# read call of include/bgamd.h -> (the runner's read that makes it, the probe whose call it reads)
REFUSABLE = {"bgamd_env_rollout_match_results": ("match", "ro_match")}
ALSO_READ = (("paired_mwc", "ro_match"),)
READS = ("rollout_info", "cube", "cube_info", "paired_cubeful", "match", "paired_mwc")
CUBE = dict(double_at=0.97, pass_at=0.0, too_good_at=0.97, max_cube=8)             # (a match ignores the first two: hardly a double, and all passed)
SOIL_CUBE = dict(double_at=1.0, pass_at=0.0, too_good_at=1.0, max_cube=64)
# the intervening calls of tests/history_cases.py after which the match reads MUST be refused: every rollout, played or refused
MUST_REFUSE = ("rollout", "refused_rollout")


def probe(Match, MatchTable):
    return H.E("ro_match", "rollout", READS, pos=("late", 4), trials=8, max_plies=6, variance_reduction=True, groups=(0, 0, 1, 1), cube=CUBE,
               match=Match(MatchTable.janowski(7), [5, 3, 2, 1], [5, 4, 6, 4], [0, 0, 0, 2], 0.3), lanes=64, **H.RO)


def soil(Match, MatchTable):
    """behind tests/history_cases.py's SOIL: a larger rollout under another, larger table (more positions, more trials, other scores,
    another window), and one under the table of double match point, which leaves the smallest tables uploaded"""
    return [H.E("big_ro_match", "rollout", READS, pos=("picks", 8), trials=36, max_plies=6, variance_reduction=True,
                groups=(0, 0, 0, 0, 1, 1, 1, 1), cube=SOIL_CUBE,
                match=Match(MatchTable.janowski(11), [9, 1, 4, 2, 11, 3, 1, 6], [9, 5, 1, 2, 2, 8, 1, 6], [0, 1, 2, 0, 0, 0, 1, 0], 0.9), **H.SRO),
            H.E("dmp_ro_match", "rollout", READS, pos=("picks", 2), trials=4, max_plies=3, variance_reduction=True, groups=(0, 0), cube=SOIL_CUBE,
                match=Match(MatchTable.janowski(1), [1, 1], [1, 1], [1, 2]), lanes=32, **H.SRO)]
