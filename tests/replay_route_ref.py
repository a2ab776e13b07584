"""What DeviceTDLambdaLearner issued for a replay or a fit step BEFORE its dispatch was written once (backgammon_env/learner.py,
replay_route / _issue): a restatement of the four functions that each decided it for themselves -- _replay_order, _replay_stream,
replay_games and fit_step, with the _distributed / _in_library / _world helpers they shared -- written from their text as it stood, not
from the code that replaced them.  Plain Python, no torch, no library.  tests/test_replay_route_cpu.py drives the learner's own code
against it, call for call.

A run is a list of events, in the order issued:
    ("td_stream_schedule", n, slots asked for)             ("td_begin", n_games)
    ("td_begin_stream", k)                                 ("td_begin_stream_games", k, table entries)
    ("td_replay", n_steps, n_active array, alpha, lam)     ("td_replay_allreduce", steps, n_active array, own steps, alpha, lam)
    ("td_step", t, n_active, alpha, lam, update buffer passed)
    ("td_apply", the update it is handed was zeroed rather than written by a step)
    ("td_stats",)
    ("td_fit_step", n, alpha, update buffer passed)        ("td_fit_step_allreduce", n, alpha)
    ("all_reduce", "MAX" | "SUM")                          ("raises",)  -- a collective without a process group; nothing follows
The other ranks are one number: a MAX-reduce over a world of more than one returns own + `extra`.

`bug` plants one of three mistakes (the test must catch each, and each in a field of its own):
    "stream_guard"     the streamed torch loop calls bgamd_td_step only while t < n_steps      -> the library calls differ
    "max_world_only"   the torch route MAX-reduces the step count only for world > 1           -> the collectives differ
    "library_if_comm"  the library's route is taken whenever the learner has a communicator    -> the route differs"""

LOCAL, LIBRARY, TORCH = "local", "library", "torch"
BUGS = ("stream_guard", "max_world_only", "library_if_comm")


class _Raised(Exception):
    pass


class Parent:
    def __init__(self, world, group_up, has_comm, force, torch_collective, extra=0, bug=None):
        self.w = world if group_up else 1                    # _world: the group's size where a process group is up, else 1
        self.group_up, self.has_comm, self.force, self.torch_collective = group_up, has_comm, force, torch_collective
        self.extra, self.bug = extra, bug
        self.events, self.route = [], None

    # ---- the helpers as they stood
    def distributed(self):
        return self.w > 1 or (self.force and (self.group_up or self.has_comm))

    def in_library(self, distributed):
        if self.bug == "library_if_comm":
            return self.has_comm
        return distributed and self.has_comm and not self.torch_collective

    def all_reduce(self, op, value=None):
        if not self.group_up:
            self.events.append(("raises",))
            raise _Raised()
        self.events.append(("all_reduce", op))
        return value + self.extra if op == "MAX" and self.w > 1 else value

    def stats(self):
        self.events.append(("td_stats",))

    # ---- _replay_order
    def replay_order(self, n_games, n_steps, n_active, alpha, lam, split_apply):
        ev, distributed = self.events, self.distributed()
        ev.append(("td_begin", n_games))
        arr = list(n_active) + [0] * (max(n_steps, 1) - len(n_active))
        if not distributed and not split_apply:
            self.route = LOCAL
            ev.append(("td_replay", n_steps, arr, alpha, lam))
        elif self.in_library(distributed):
            self.route = LIBRARY
            ns = n_steps
            if self.w > 1:
                ns = self.all_reduce("MAX", ns)
            ev.append(("td_replay_allreduce", ns, arr, n_steps, alpha, lam))
        else:
            self.route = TORCH
            ns = n_steps
            if (self.w > 1) if self.bug == "max_world_only" else distributed:
                ns = self.all_reduce("MAX", ns)
            for t in range(ns):
                if t < n_steps:
                    ev.append(("td_step", t, n_active[t], alpha, lam, True))
                if distributed:
                    self.all_reduce("SUM")
                ev.append(("td_apply", not t < n_steps))
        self.stats()

    # ---- replay_rows without slots: the sub-rounds of the length-sorted order, each through _replay_order
    def replay_rows(self, lengths, sub_round, alpha, lam, split_apply):
        sl = sorted((x for x in lengths if x > 0), reverse=True)
        n_sub = max(1, -(-len(sl) // sub_round)) if sub_round > 0 else 1
        if self.distributed() and self.w > 1:
            n_sub = self.all_reduce("MAX", n_sub)
        for c in range(n_sub):
            s = sl[c::n_sub]
            n_steps = s[0] if s else 0
            self.replay_order(len(s), n_steps, [sum(1 for x in s if x > t) for t in range(n_steps)], alpha, lam, split_apply)

    # ---- _replay_stream: n lanes of which n_games have a length, the schedule's k slots and n_steps
    def replay_stream(self, n, slots_asked, n_games, k, n_steps, alpha, lam, split_apply):
        ev, distributed = self.events, self.distributed()
        ev.append(("td_stream_schedule", n, slots_asked))
        ev.append(("td_begin_stream", k))
        if not distributed and not split_apply:
            self.route = LOCAL
            ev.append(("td_replay", n_steps, [k] * n_steps or [0], alpha, lam))
        elif self.in_library(distributed):
            self.route = LIBRARY
            ns = n_steps
            if self.w > 1:
                ns = self.all_reduce("MAX", ns)
            own = n_steps if n_games else 0
            ev.append(("td_replay_allreduce", ns, [k] * own or [0], own, alpha, lam))
        else:
            self.route = TORCH
            ns = n_steps
            if (self.w > 1) if self.bug == "max_world_only" else distributed:
                ns = self.all_reduce("MAX", ns)
            for t in range(ns):
                step = (n_games and t < n_steps) if self.bug == "stream_guard" else n_games
                if step:
                    ev.append(("td_step", t, k, alpha, lam, True))
                if distributed:
                    self.all_reduce("SUM")
                ev.append(("td_apply", not step))
        self.stats()

    # ---- replay_games: a table of G games, the schedule's k slots and n_steps
    def replay_games(self, G, slots_asked, k, n_steps, alpha, lam):
        ev, distributed = self.events, self.distributed()
        ev.append(("td_stream_schedule", G, slots_asked))
        ev.append(("td_begin_stream_games", k, max(G, 1)))
        if not distributed:
            self.route = LOCAL
            ev.append(("td_replay", n_steps, [k] * n_steps or [0], alpha, lam))
        else:
            ns = n_steps
            if self.w > 1:
                ns = self.all_reduce("MAX", ns)
            if self.in_library(True):
                self.route = LIBRARY
                own = n_steps if G else 0
                ev.append(("td_replay_allreduce", ns, [k] * own or [0], own, alpha, lam))
            else:
                self.route = TORCH
                for t in range(ns):
                    step = G and t < n_steps
                    if step:
                        ev.append(("td_step", t, k, alpha, lam, True))
                    self.all_reduce("SUM")
                    ev.append(("td_apply", not step))
        self.stats()

    # ---- fit_step
    def fit_step(self, n, alpha):
        ev = self.events
        if not self.distributed():
            self.route = LOCAL
            ev.append(("td_fit_step", n, alpha, False))
        elif self.in_library(True):
            self.route = LIBRARY
            ev.append(("td_fit_step_allreduce", n, alpha))
        else:
            self.route = TORCH
            ev.append(("td_fit_step", n, alpha, True))
            self.all_reduce("SUM")
            ev.append(("td_apply", False))


def run(parent, call):
    """call(parent) -> {"route", "raises", "collectives", "calls", "events"}: the route of the LAST dispatch (every dispatch of a call
    takes the same one), whether a collective was reached without a process group, and the events whole and split in two."""
    raised = False
    try:
        call(parent)
    except _Raised:
        raised = True
    return fields(parent.route, raised, parent.events)


def fields(route, raised, events):
    return {"route": route, "raises": raised, "collectives": [e for e in events if e[0] == "all_reduce"],
            "calls": [e for e in events if e[0].startswith("td_")], "events": list(events)}


FIELDS = ("route", "raises", "collectives", "calls", "events")


def differing(a, b):
    """the fields in which two runs differ, in FIELDS' order"""
    return [f for f in FIELDS if a[f] != b[f]]
