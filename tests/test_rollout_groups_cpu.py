"""The grouped rollout's rules and the conditions tests/test_gpu_rollout_groups.py rests on, checked without a device: the id rule of
tests/rollout_group_model.py against rollout_ref's, the paired statistic in the device's order against exactly rounded sums, three
wrong models that these cases must tell from the right one, the shape of the GPU tests' tables -- and that the new entry points are
declared in include/bgamd.h and listed in _capi.py."""
import importlib.util
import inspect
import math
import os
import random
import re

import numpy as np
import pytest

import rollout_group_model as GM
import rollout_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TABLES = [(GM.GROUPS, GM.GROUP_OFFSET), (GM.TWIN_GROUPS, 0)] + [(g, off) for _, g, off in GM.split_tables()]
TRIALS = sorted({T for T, _, _ in GM.CASES} | {1, 2, 63, 64, 65, 130, 1296})


# ---- the id rule -----------------------------------------------------------------------------------------------------------------------

def test_identity_groups_give_the_plain_rollouts_ids():
    # rollout_ref.rollout states the plain rule in its one line; the model with the identity table must be that line
    assert "j = (position_offset + p) * trials + i" in inspect.getsource(R.rollout)
    for P, T, off in ((1, 1, 0), (7, 36, 0), (7, 73, 2), (3, 1296, 11)):
        ids = GM.trial_ids(list(range(P)), T, off)
        assert ids == [[(off + p) * T + i for i in range(T)] for p in range(P)]
        assert GM.slots(P, T) == GM.trial_ids(list(range(P)), T, 0)       # (offset 0: the slot and the id are one number)


@pytest.mark.parametrize("groups,offset", TABLES)
def test_ids_are_shared_inside_a_group_and_nowhere_else(groups, offset):
    for T in TRIALS:
        ids = GM.trial_ids(groups, T, offset)
        for p in range(len(groups)):
            assert len(set(ids[p])) == T
            for r in range(len(groups)):
                if groups[p] == groups[r]:
                    assert ids[p] == ids[r]
                else:
                    assert not set(ids[p]) & set(ids[r])
        # a single-position plain call at position_offset = group_offset + group[p] has these ids: the GPU tests' yardstick
        for p, g in enumerate(groups):
            assert ids[p] == GM.trial_ids([0], T, offset + g)[0]
        slots = GM.slots(len(groups), T)
        assert sorted(s for row in slots for s in row) == list(range(len(groups) * T))


def test_a_split_over_group_offset_keeps_every_id():
    whole = GM.trial_ids(GM.GROUPS, 40, GM.GROUP_OFFSET)
    parts = GM.split_tables()
    assert sorted(p for idx, _, _ in parts for p in idx) == list(range(len(GM.GROUPS)))
    assert parts[0][2] != parts[1][2] and all(len(idx) >= 2 for idx, _, _ in parts)
    for idx, groups, off in parts:
        assert GM.valid(groups, 40, off)
        assert GM.trial_ids(groups, 40, off) == [whole[p] for p in idx]


def test_what_a_table_may_hold():
    assert GM.valid(GM.GROUPS, 73, GM.GROUP_OFFSET) and GM.valid([0], 1, 0)
    assert not GM.valid([0, -1], 8, 0) and not GM.valid([0, 1], 8, -1)
    T = 1 << 20
    assert GM.valid([2046], T, 0) and not GM.valid([2047], T, 0)          # (max group + 1) T < 2^31
    assert GM.valid([2 ** 31 - 2], 1, 0) and not GM.valid([2 ** 31 - 1], 1, 0)


# ---- the paired statistic ------------------------------------------------------------------------------------------------------------------

def _cases():
    """(name, q [P][T], groups): win values, net values, equities in points, and a constant non-zero difference"""
    rng = random.Random(20240603)
    out = []
    for T in TRIALS:
        base = [rng.random() for _ in range(T)]                            # the dice the group shares: its trials' luck
        wins = [[1.0 if base[i] + 0.2 * rng.random() > 0.5 + 0.05 * p else 0.0 for i in range(T)] for p in range(4)]
        nets = [[float(np.float32(min(1.0, max(0.0, base[i] + 0.1 * (rng.random() - 0.5) - 0.02 * p)))) for i in range(T)] for p in range(4)]
        pts = [[float(rng.choice((-3, -2, -1, -1, 1, 1, 2, 3))) if rng.random() < 0.8 else 2.0 * nets[p][i] - 1.0 for i in range(T)]
               for p in range(4)]
        const = [[base[i] + 0.25 * p for i in range(T)] for p in range(4)]
        for name, q in (("wins", wins), ("nets", nets), ("points", pts), ("constant", const)):
            out.append((f"{name}-{T}", q, [7, 2, 7, 7]))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,q,groups", CASES, ids=[c[0] for c in CASES])
def test_the_device_order_agrees_with_exact_sums(name, q, groups):
    T = len(q[0])
    for p in range(4):
        for r in range(-1, 5):
            m, se = GM.paired(q, groups, p, r)
            me, see = GM.paired_fsum(q, groups, p, r)
            if not (0 <= r < 4) or groups[r] != groups[p]:
                assert math.isnan(m) and math.isnan(se) and math.isnan(me) and math.isnan(see)
                continue
            assert abs(m - me) <= T * 2.0 ** -52, (p, r, m, me)
            assert abs(se - see) <= 1e-12 * abs(see) + T * 2.0 ** -52, (p, r, se, see)
            assert GM.close(m, me, T) and GM.close(se, see, T, stderr=True)
            if r == p:
                assert m == 0.0 and se == 0.0
            if T == 1:
                assert se == 0.0
    if name.startswith("constant"):                                        # the case the atol is for
        m, se = GM.paired(q, groups, 2, 0)
        assert abs(m - 0.5) <= T * 2.0 ** -52 and se <= T * 2.0 ** -52


def test_wave_sum_is_the_strided_order():
    # 130 values: lane 0 holds v0 + v64 + v128, lane 1 v1 + v65 + v129, lane 2 v2 + v66; values chosen so that the order shows
    v = [2.0 ** 60 if i == 0 else (-2.0 ** 60 if i == 64 else 1.0) for i in range(130)]
    assert GM.wave_sum(v) == 128.0                       # (v0 + v64 = 0 first: a left-to-right sum would lose the ones in between)
    s = 0.0
    for x in v:
        s += x
    assert s != 128.0
    assert GM.wave_sum([1.0] * 73) == 73.0 and GM.wave_sum([]) == 0.0


# ---- three wrong models --------------------------------------------------------------------------------------------------------------

def test_ids_by_position_are_told_apart():
    wrong = lambda groups, T, off: [[(off + p) * T + i for i in range(T)] for p in range(len(groups))]
    for groups, off in TABLES[:2]:
        T = 36
        ids = wrong(groups, T, off)
        pairs = [(p, r) for p in range(len(groups)) for r in range(p) if groups[p] == groups[r]]
        assert pairs and all(ids[p] != ids[r] for p, r in pairs)           # the check of the test above fails for every pair
        assert ids != GM.trial_ids(groups, T, off)


def test_the_unpaired_stderr_is_told_apart():
    n = 0
    for name, q, groups in CASES:
        T = len(q[0])
        if T < 36 or name.startswith("constant"):
            continue
        for p, r in ((0, 2), (2, 3), (3, 0)):
            _, see = GM.paired_fsum(q, groups, p, r)
            un = GM.unpaired_stderr(q, p, r)
            assert not GM.close(un, see, T, stderr=True), (name, p, r)
            if not name.startswith("points"):             # (the points cases draw every trial's points on their own: nothing shared)
                assert un > see                           # shared luck: the paired error is the smaller one
            n += 1
    assert n >= 12
    for name, q, groups in CASES:                         # and a constant difference has no paired error at all
        if name.startswith("constant") and len(q[0]) > 1:
            assert GM.unpaired_stderr(q, 2, 0) > 1e-3 > GM.paired(q, groups, 2, 0)[1]


def test_a_reference_from_another_group_is_told_apart():
    ungrouped = lambda q, p, r: GM.paired(q, [0] * len(q), p, r)           # a model that pairs whatever it is given
    for name, q, groups in CASES[:8]:
        for p, r in ((0, 1), (1, 0), (1, 3)):
            assert groups[p] != groups[r]
            m, se = GM.paired(q, groups, p, r)
            wm, wse = ungrouped(q, p, r)
            assert math.isnan(m) and math.isnan(se)
            assert not math.isnan(wm) and not GM.close(wm, m, len(q[0])) and not GM.close(wse, se, len(q[0]), stderr=True)


# ---- the conditions the GPU cases rest on -------------------------------------------------------------------------------------------

def test_the_gpu_tables():
    g = GM.GROUPS
    assert len(g) == 7 == len(GM.PICKS) and g == [3, 0, 3, 1, 0, 3, 5] and GM.GROUP_OFFSET == 2
    assert GM.CASES == [(40, False, 0), (36, True, 0), (73, True, 4)]
    # non-contiguous: a group's members do not stand together, and the groups do not come in order; sparse: numbers are left out
    members = {k: [p for p, x in enumerate(g) if x == k] for k in set(g)}
    assert any(m[-1] - m[0] >= len(m) for m in members.values()) and g != sorted(g)
    assert set(range(max(g) + 1)) - set(g)
    st, tu, kind = GM.main_positions()
    for k, m in members.items():
        if len(m) > 1:                                   # every shared group compares at least two different positions
            assert len({st[p].tobytes() + bytes([int(tu[p])]) for p in m}) >= 2, k
    assert len({st[p].tobytes() for p in range(7)}) == 7
    assert (kind == "over").sum() == 1 and len(members[g[int(np.flatnonzero(kind == "over")[0])]]) == 1
    assert "start" in kind and "bar" in kind and "forced" in kind and (kind == "g10").sum() == 3
    T73 = GM.CASES[2][0]
    assert T73 > 64 and T73 % 64 and T73 > 72             # more than one stride with a partial tail; the 36 pairs twice and one more
    assert all(7 * T > 3 * 64 for T, _, _ in GM.CASES)    # at 64 lanes every case has several times more trials than lanes
    tw, ttu = GM.twin_positions()
    assert GM.TWIN_GROUPS == [4, 4, 9] and (tw[0] == tw[1]).all() and (tw[0] == tw[2]).all() and len(set(ttu.tolist())) == 1
    assert kind[GM.PICKS.index(GM.TWIN_PICK)] == "g10"    # a live position: its trials depend on their dice
    for groups, off in TABLES:
        assert all(GM.valid(groups, T, off) for T in TRIALS)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    spec = importlib.util.spec_from_file_location("_bgamd_capi_listing", os.path.join(ROOT, "backgammon-engine_amd", "backgammon_env", "_capi.py"))
    capi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(capi)                         # (the listing only: nothing is loaded)
    listed = {name: args for name, _, args in capi.SYMBOLS}
    for name in ("bgamd_env_rollout_grouped", "bgamd_env_rollout_paired_read"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/bgamd.h"
        n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert name in listed, f"{name} is not listed in _capi.SYMBOLS"
        assert len(listed[name]) == n_args, (name, n_args, len(listed[name]))
    assert len(listed["bgamd_env_rollout_grouped"]) == len(listed["bgamd_env_rollout"]) + 1
