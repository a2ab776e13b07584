"""The learner's front end without a GPU: which library calls and which collectives DeviceTDLambdaLearner issues for a replay or a fit step,
for every combination of the facts that decide it (backgammon_env/learner.py: replay_route, _issue), against a restatement of the code
that decided it in four places before (tests/replay_route_ref.py).  The learner's OWN methods run -- replay_rows, replay_games, fit_step
and everything under them -- on an object built without __init__, with a recording stand-in for the library (bgamd_td_stream_schedule,
host code, goes to the real one) and for torch.distributed.  No process is started, no device is touched."""
import ctypes
import itertools

import pytest
import torch

import replay_route_ref as REF

LR, LAM, SCALE, SLOTS, MAX_GAMES = 0.1, 0.7, 0.5, 2, 64
# own steps -> lengths per lane: lock-step (the longest game), and streamed through two slots (the longer slot: 5 | 3 + 2)
LOCK = {0: [0, 0, 0, 0], 1: [1, 0, 1, 1], 5: [5, 3, 0, 1, 5, 2]}
STREAM = {0: [0, 0, 0], 1: [1, 0, 1], 5: [5, 3, 0, 2]}
ENTRIES = ("lock-step", "sub-rounds", "streamed", "game table", "fit step")
HAS_SPLIT_APPLY = ("lock-step", "sub-rounds", "streamed")


class _NoGroup(ValueError):
    """what torch.distributed raises for a collective without a process group"""


class _Dist:
    """torch.distributed as far as the learner uses it: a world size, and a MAX over the ranks that returns own + extra"""
    class ReduceOp:
        MAX, SUM = "MAX", "SUM"

    def __init__(self, events, world, group_up, extra):
        self.events, self.world, self.group_up, self.extra = events, world, group_up, extra

    def is_available(self):
        return True

    def is_initialized(self):
        return self.group_up

    def get_world_size(self, group=None):
        assert self.group_up
        return self.world

    def all_reduce(self, t, op=None, group=None):
        if not self.group_up:
            self.events.append(("raises",))
            raise _NoGroup("Default process group has not been initialized")
        assert group == "the group"                              # every collective goes to the group the caller named
        self.events.append(("all_reduce", op))
        if op == "MAX" and self.world > 1:
            t += self.extra


class _Lib:
    """libbgamd.so as far as a replay uses it: records every call's arguments that the dispatch decides.  bgamd_td_step marks the update
    buffer it is handed and bgamd_td_apply looks for the mark, so a zero_() in place of a step shows."""
    def __init__(self, events, real, learner):
        self.events, self.real, self.learner = events, real, learner

    @staticmethod
    def _upd(p):
        return ctypes.cast(p, ctypes.POINTER(ctypes.c_float))

    def bgamd_td_stream_schedule(self, h_len, n, k, *rest):
        self.events.append(("td_stream_schedule", n, k))
        return self.real.bgamd_td_stream_schedule(h_len, n, k, *rest)

    def bgamd_td_begin(self, h, rows, T, n, order, n_games, lengths, won, s):
        assert self.learner._keep is not None
        self.events.append(("td_begin", n_games))
        return 0

    def bgamd_td_begin_stream(self, h, rows, T, n, queue, qoff, k, lengths, won, s):
        assert self.learner._keep is not None
        self.events.append(("td_begin_stream", k))
        return 0

    def bgamd_td_begin_stream_games(self, h, rows, R, n, queue, qoff, k, n_table, lane, start, lengths, won, s):
        assert self.learner._keep is not None
        self.events.append(("td_begin_stream_games", k, n_table))
        return 0

    def bgamd_td_replay(self, h, n_steps, arr, alpha, lam, s):
        self.events.append(("td_replay", n_steps, list(arr), alpha, lam))
        return 0

    def bgamd_td_replay_allreduce(self, h, n_steps, arr, own, alpha, lam, s):
        self.events.append(("td_replay_allreduce", n_steps, list(arr), own, alpha, lam))
        return 0

    def bgamd_td_step(self, h, t, n_active, alpha, lam, upd, s):
        self.events.append(("td_step", t, n_active, alpha, lam, upd is not None))
        self._upd(upd)[0] = 1.0
        return 0

    def bgamd_td_apply(self, h, upd, s):
        self.events.append(("td_apply", self._upd(upd)[0] == 0.0))
        return 0

    def bgamd_td_stats(self, h, sq, cnt):
        assert self.learner._keep is not None                    # the buffers live until the statistics are read
        self.events.append(("td_stats",))
        return 0

    def bgamd_td_fit_step(self, h, rows, y, n, alpha, upd, s):
        self.events.append(("td_fit_step", n, alpha, upd is not None))
        if upd is not None:
            self._upd(upd)[0] = 1.0
        return 0

    def bgamd_td_fit_step_allreduce(self, h, rows, y, n, alpha, s):
        self.events.append(("td_fit_step_allreduce", n, alpha))
        return 0


def _learner(events, real, has_comm):
    """a DeviceTDLambdaLearner with no handle and no device: the attributes __init__ would set, tensors on the CPU, no stream"""
    from backgammon_env import _capi
    from backgammon_env.learner import DeviceTDLambdaLearner
    L = object.__new__(DeviceTDLambdaLearner)
    L._C, L._capi, L._h = ctypes, _capi, None
    L._lib = _Lib(events, real, L)
    L.device, L.max_games = torch.device("cpu"), MAX_GAMES
    L.learning_rate, L.lambda_decay, L._keep = LR, LAM, None
    L._s = lambda: None
    if has_comm:
        L._comm = (0, 1)
    return L


def _actual(entry, own, L, split_apply):
    """runs the entry on the learner"""
    kw = {"split_apply": True} if split_apply else {}
    if entry in ("lock-step", "sub-rounds"):
        ln = LOCK[own]
        rows = torch.zeros((max(ln + [1]), len(ln), 8), dtype=torch.int32)
        return L.replay_rows(rows, ln, [1] * len(ln), group="the group", batch_scale=SCALE, sub_round=2 if entry == "sub-rounds" else 0, **kw)
    ln = STREAM[own]
    rows = torch.zeros((max(ln + [1]), len(ln), 8), dtype=torch.int32)
    if entry == "streamed":
        return L.replay_rows(rows, ln, [1] * len(ln), group="the group", batch_scale=SCALE, slots=SLOTS, **kw)
    if entry == "game table":
        ln = [x for x in ln if x > 0]                            # a table holds finished games only; none at all: G = 0
        lane = [i for i, x in enumerate(STREAM[own]) if x > 0]
        return L.replay_games(rows, lane, [0] * len(ln), torch.tensor(ln, dtype=torch.int32), [1] * len(ln), slots=SLOTS, group="the group",
                              batch_scale=SCALE)
    return L.fit_step(torch.zeros((own, 8), dtype=torch.int32), torch.zeros(own), batch_scale=SCALE, group="the group")


def _expected(entry, own, parent, split_apply):
    """the same call on the restatement of the parent"""
    from backgammon_env.learner import stream_schedule
    alpha = float(LR) * float(SCALE)
    if entry in ("lock-step", "sub-rounds"):
        return parent.replay_rows(LOCK[own], 2 if entry == "sub-rounds" else 0, alpha, LAM, split_apply)
    if entry == "fit step":
        return parent.fit_step(own, alpha)
    ln = STREAM[own] if entry == "streamed" else [x for x in STREAM[own] if x > 0]
    _, _, n_steps, k = stream_schedule(torch.tensor(ln, dtype=torch.int32), SLOTS)     # the host restatement of the library's schedule
    if entry == "streamed":
        return parent.replay_stream(len(ln), SLOTS, sum(1 for x in ln if x > 0), k, n_steps, alpha, LAM, split_apply)
    return parent.replay_games(len(ln), SLOTS, k, n_steps, alpha, LAM)


def _cases():
    for entry, own, world, group_up, has_comm, force, torch_collective in itertools.product(
            ENTRIES, (0, 1, 5), (1, 2, 3), (False, True), (False, True), (False, True), (False, True)):
        for split_apply in ((False, True) if entry in HAS_SPLIT_APPLY else (False,)):
            for extra in ((0, 3) if world > 1 else (0,)):
                yield entry, own, world, group_up, has_comm, force, torch_collective, split_apply, extra


def _sweep(monkeypatch, bug=None):
    """every case on the learner and on the reference (with `bug` planted) -> [(case, the fields that differ)], the routes the learner took"""
    from backgammon_env import _capi
    from backgammon_env import learner as LM
    real = _capi.load()
    out, routes = [], {REF.LOCAL: 0, REF.LIBRARY: 0, REF.TORCH: 0}
    for case in _cases():
        entry, own, world, group_up, has_comm, force, torch_collective, split_apply, extra = case
        for name, on in (("BGAMD_FORCE_COLLECTIVE", force), ("BGAMD_TD_TORCH_COLLECTIVE", torch_collective)):
            if on:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        events = []
        monkeypatch.setattr(LM, "dist", _Dist(events, world, group_up, extra))
        L = _learner(events, real, has_comm)
        route, raised = L._route("the group", split_apply).kind, False
        try:
            _actual(entry, own, L, split_apply)
            assert L._keep is None
        except _NoGroup:
            raised = True
        got = REF.fields(route, raised, events)
        want = REF.run(REF.Parent(world, group_up, has_comm, force, torch_collective, extra, bug),
                       lambda p: _expected(entry, own, p, split_apply))
        out.append((case, REF.differing(got, want)))
        routes[route] += 1
        # the route the decision names is the one the calls show
        names = {e[0] for e in events}
        assert (route == REF.LOCAL) == bool(names & {"td_replay"} or ("td_fit_step", own, LR * SCALE, False) in events), case
        assert (route == REF.LIBRARY) == bool(names & {"td_replay_allreduce", "td_fit_step_allreduce"}), case
    return out, routes


def test_every_entry_issues_what_the_parent_issued(monkeypatch):
    """The product of entry (5) x own steps (0, 1, 5) x world (1, 2, 3) x process group up or not x communicator or not x each of
    BGAMD_FORCE_COLLECTIVE and BGAMD_TD_TORCH_COLLECTIVE unset or "1" x split_apply where the entry has it x, for a world of more than
    one, the other ranks' longest replay = own and own + 3: 1 920 cases -- 510 take LOCAL, 336 LIBRARY, 1 074 TORCH (asserted below).
    Every one matches the parent event for event, a collective reached without a process group included (both raise, at the same
    event).
    The counts by hand: an entry at one number of own steps sees 80 combinations of the other facts (world 1: 16; worlds 2 and 3: 16
    x 2 for the other ranks' maximum); 46 of them are distributed, 14 of those find a communicator that BGAMD_TD_TORCH_COLLECTIVE does not
    hold back.  Without split_apply (5 entries) that is 34 LOCAL | 14 LIBRARY | 32 TORCH, with it (3 entries) 0 | 14 | 66; times 3."""
    out, routes = _sweep(monkeypatch)
    bad = [(case, diff) for case, diff in out if diff]
    assert not bad, bad[:5]
    assert len(out) == 1920 and routes == {REF.LOCAL: 510, REF.LIBRARY: 336, REF.TORCH: 1074}, (len(out), routes)
    assert all(routes.values())


@pytest.mark.parametrize("bug, field, clean", [("stream_guard", "calls", ("route", "raises", "collectives")),
                                                ("max_world_only", "collectives", ("route", "raises", "calls")),
                                                ("library_if_comm", "route", ())])
def test_a_wrong_reference_is_caught_in_its_own_field(monkeypatch, bug, field, clean):
    """Three mistakes planted in the reference, one at a time: the sweep tells each from the learner, the first field that differs is
    the one the mistake is about, and the fields it does not touch stay equal in every case."""
    out, _ = _sweep(monkeypatch, bug)
    # (where there is no process group the first collective raises and cuts the run short, whatever came before it: such a case may
    #  differ in what it reached before that, which says nothing about the field)
    caught = [(case, diff) for case, diff in out if diff and case[3]]
    assert caught
    assert all(diff[0] == field for _, diff in caught), [c for c in caught if c[1][0] != field][:3]
    assert not any(f in diff for _, diff in caught for f in clean)
    if bug == "stream_guard":                                      # only the streamed entry, only where others run longer than this rank
        assert all(case[0] == "streamed" and case[1] > 0 and case[8] == 3 for case, _ in caught)
    if bug == "max_world_only":                                    # only a forced world of one, only replay_rows
        assert all(case[0] in HAS_SPLIT_APPLY and case[2] == 1 and case[5] for case, _ in caught)


def test_replay_route_truth_table():
    """replay_route on its own, against the three helpers it replaced, for every combination of its six facts"""
    from backgammon_env.learner import LIBRARY, LOCAL, TORCH, replay_route
    for world, group_up, has_comm, force, torch_collective, split_apply in itertools.product((1, 2, 3), *[(False, True)] * 5):
        if world > 1 and not group_up:
            continue                                               # (a world of more than one is read off a process group)
        p = REF.Parent(world, group_up, has_comm, force, torch_collective)
        d = p.distributed()
        kind = LOCAL if not d and not split_apply else LIBRARY if p.in_library(d) else TORCH
        assert replay_route(world, group_up, has_comm, force, torch_collective, split_apply) == (d, kind, world)
    assert (LOCAL, LIBRARY, TORCH) == (REF.LOCAL, REF.LIBRARY, REF.TORCH)
