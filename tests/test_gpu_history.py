"""No call's result depends on what the env did before (include/bgamd.h, "history rule"), on the MI355X.

The reference is the library itself on an env that has done nothing else, so every comparison is bit for bit, on every output tensor and
every info list.  tests/history_cases.py holds the program: the PROBES (one call each, with its reads), SOIL (the same features with other
arguments, larger and smaller, other boards, dice, seed and weights, every sticky setting set and cleared, refused calls), the reads that can
be refused and the calls put between a call and its reads.  tests/test_history_cases_cpu.py states why the comparison is not vacuous.
  fresh side   every probe on an env created for it: the constructor's seed, the probes' weights in both slots, boards and dice set;
  used side    one env through all of SOIL, brought back by documented calls only (load_weights on both slots, reseed, reset, reset_stats,
               settings cleared), then the probes in the listed order, in reverse, and each directly behind its own larger SOIL step;
               before a probe, scratch_info() says that the internal envs it will use exist and are larger than it needs.
A mismatch names the probe, the order, the field, the first differing element and the SOIL step run last; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import history_cases as H
import nets as NT
import search_lanes as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


def _tables():
    return {k: NT.table(k) for k in H.PROBE_NETS + H.SOIL_NETS}


def _np(x):
    if torch.is_tensor(x):
        return x.cpu().numpy()
    return np.asarray(x)


def _flat(prefix, d, out):
    for k, v in d.items():
        if isinstance(v, dict):
            _flat(prefix + k + ".", v, out)
        elif v is not None:
            out[prefix + k] = _np(v)


class Refused:
    def __init__(self, code):
        self.code = code

    def __repr__(self):
        return "Refused(%d)" % self.code


# ---- the reads ---------------------------------------------------------------------------------------------------------------------------

def _read_search_candidates(bg, env):
    names = ("states", "v1", "v2", "kept", "v3", "depth")
    return dict(zip(names, env.search_candidates()))


def _read_analysis(bg, env):
    out = {k: env._buf((env.n,), dt) for k, dt in env.ANALYSIS_FIELDS}
    out["best"] = env._buf((env.n, 28), torch.int32)
    out["summary"] = env._buf((12,), torch.float64)
    bg._capi.check(env._lib.bgamd_env_analysis_read(env._h, *[bg._ptr(out[k]) for k, _ in env.ANALYSIS_FIELDS], bg._ptr(out["best"]),
                                                    bg._ptr(out["summary"]), bg._stream()), "analysis_read")
    return out


def _read_vr(bg, env):
    P, T = env._rollout_shape
    out = {"vr_mean": env._buf((P,), torch.float64), "vr_stderr": env._buf((P,), torch.float64), "trial_luck": env._buf((P, T), torch.float64)}
    bg._capi.check(env._lib.bgamd_env_rollout_vr_read(env._h, bg._ptr(out["vr_mean"]), bg._ptr(out["vr_stderr"]), bg._ptr(out["trial_luck"]),
                                                      bg._stream()), "rollout_vr_read")
    return out


def _paired(which):
    def read(bg, env):
        P, _ = env._rollout_shape
        ref = [max(p - 1, 0) if p % 3 else p for p in range(P)]            # itself, or its neighbour: inside a group or across two
        dm, ds = env.rollout_paired(ref, which)
        return {"diff_mean": dm, "diff_stderr": ds}
    return read


def _read_unique_rows(bg, env):
    """the rows as a set: "the order of the rows inside an arena is the order in which the leaf stage's workgroups allocated them: no
    meaning" (include/bgamd.h, bgamd_env_unique_rows_read) -- sorted here by (game, key, state, value bits)"""
    info, st, val = (_np(x) for x in env.unique_rows())
    cols = np.concatenate([info, st.astype(np.int64), val.view(np.uint32).astype(np.int64)[:, None]], axis=1)
    order = np.lexsort(cols.T[::-1])
    return {"info": info[order], "states": st[order], "values": val[order]}


def _read_snapshot(bg, env):
    return {"snapshot": env.snapshot(), "states": env.states(), "turns": env.turns(), "flags": env.flags(), "dice": env.dice()}


def _read_progress(bg, env):
    ply, epi = env.progress()
    return {"ply": ply, "episode": epi}


def _read_stats(bg, env):
    s = env.stats()
    return {"stats": [s[k] for k in sorted(s)]}


READERS = {
    "last_choice": lambda bg, env: env.last_choice(),
    "unique_rows": _read_unique_rows,
    "choice_spread": lambda bg, env: env.choice_spread(),
    "snapshot": _read_snapshot,
    "progress": _read_progress,
    "stats": _read_stats,
    "sample_info": lambda bg, env: {"info": env.sample_info()},
    "search_candidates": _read_search_candidates,
    "search_info": lambda bg, env: {"info": env.search_info()},
    "search3_info": lambda bg, env: {"info": env.search3_info()},
    "analysis": _read_analysis,
    "rollout_info": lambda bg, env: {"info": env.rollout_info()},
    "outcomes": lambda bg, env: env.rollout_outcomes_read(per_trial=True),
    "vr": _read_vr,
    "cube": lambda bg, env: env.rollout_cube_read(per_trial=True),
    "cube_info": lambda bg, env: {"info": env.rollout_cube_info()},
    "paired_value": _paired("value"), "paired_vr": _paired("vr"), "paired_equity": _paired("equity"), "paired_cubeful": _paired("cubeful"),
}


def do_read(bg, env, read):
    """-> {field: array}, or Refused(code)"""
    try:
        out = {}
        _flat("", READERS[read](bg, env), out)
        return out
    except bg.BgamdError as e:
        return Refused(e.code)


def do_reads(bg, env, entry, out):
    for r in entry["reads"]:
        got = do_read(bg, env, r)
        assert not isinstance(got, Refused), (entry["name"], r, got)
        out.update({r + "." + k: v for k, v in got.items()})
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------

def _documented_state(bg, env):
    out = {}
    for r in ("snapshot", "progress"):
        _flat(r + ".", READERS[r](bg, env), out)
    h = (C.c_uint64 * 10)()
    env._lib.bgamd_env_stats(env._h, h)                                  # (the raw counters: a refused call may not raise an error bit either)
    out["stats"] = np.array(list(h))
    return out


def _set_lanes(env, sel):
    st, tu, dice = H.lanes(sel)
    assert len(st) == env.n
    env.set_states(st, tu)
    env.set_dice(dice)
    return st, tu, dice


def _played(env, sel):
    """the greedy move of every lane from its board and dice, the boards and dice put back: the move to analyse"""
    st, tu, dice = _set_lanes(env, sel)
    env.step_greedy(roll=False, auto_reset=False, no_flip=True)
    played = env.states()
    env.set_states(st, tu)
    env.set_dice(dice)
    return played


def _afterstate_rows(sel, roots):
    """the first `roots` live lanes of A (A1: its lane) that have a move, with their afterstates in reference order"""
    st, tu, _ = H.lanes(sel)
    idx = H.fixture_index(sel)
    pick = [g for g in range(len(st)) if (st[g] != H.OVER).any() and len(L.afterstates(int(idx[g])))][:roots]
    assert len(pick) == roots
    kids = [L.afterstates(int(idx[g])) for g in pick]
    return (st[pick], tu[pick], np.concatenate(kids).astype(np.int32), np.concatenate([np.full(len(k), q, np.int32) for q, k in enumerate(kids)]))


class Runner:
    """runs entries of tests/history_cases.py on one env"""

    def __init__(self, bg, n, tables, load=True):
        self.bg, self.tables = bg, tables
        self.env = bg.VecGame(n, seed=H.SEED)
        self.last = None                                                 # the entry run last
        self.keep = {}                                                   # tensors a sticky setting points to
        if load:
            self.load_probe_weights()

    def close(self):
        self.env.close()

    def load_probe_weights(self):
        for slot, name in enumerate(H.PROBE_NETS):
            self.env.load_weights(self.tables[name], slot)

    def restore(self, settings=False):
        """back to a new env's documented state, by documented calls only.  settings: also every sticky setting cleared -- once, behind
        SOIL; between two probes they are left as the probe before left them, which is cleared if the Python layer keeps its word"""
        env, lib, h = self.env, self.env._lib, self.env._h
        self.load_probe_weights()
        if settings:
            env.record_trajectory(None)
            env.record_ring(None)
            env.record_search_log(None)
            env.time_kernels(False)
            self.bg._capi.check(lib.bgamd_env_rollout_policy(h, 1, 0, 0.0), "rollout_policy")
            self.bg._capi.check(lib.bgamd_env_rollout_cube(h, 0, 0.0, 0.0, 0.0, 0, None, None), "rollout_cube")
            self.keep.clear()
        env.reseed(H.SEED)
        env.reset()
        env.reset_stats()

    def setting(self, what, on, kw):
        bg, env = self.bg, self.env
        lib, h, chk = env._lib, env._h, self.bg._capi.check
        if what == "time_kernels":
            env.time_kernels(on)
        elif what == "rollout_policy":
            p = H.SOIL_POLICY
            chk(lib.bgamd_env_rollout_policy(h, *((p["plies"], p["top_k"], p["margin"]) if on else (1, 0, 0.0))), what)
        elif what == "rollout_cube":
            if on:
                r = kw["rule"]
                value = torch.tensor(kw["value"], dtype=torch.int32, device=env.device)
                owner = torch.tensor(kw["owner"], dtype=torch.int32, device=env.device)
                self.keep["cube"] = (value, owner)
                flags = bg.CUBE_ON | (bg.CUBE_JACOBY if r.get("jacoby") else 0) | (bg.CUBE_HOLD_TURN0 if r.get("hold_turn0") else 0)
                chk(lib.bgamd_env_rollout_cube(h, flags, r["double_at"], r["pass_at"], r["too_good_at"], r["max_cube"], bg._ptr(value),
                                               bg._ptr(owner)), what)
            else:
                chk(lib.bgamd_env_rollout_cube(h, 0, 0.0, 0.0, 0.0, 0, None, None), what)
                self.keep.pop("cube", None)                              # the start tables are dropped: nothing may read them again
        else:
            raise KeyError(what)

    def call(self, e):
        """the entry's call (no reads) -> its own outputs, flat"""
        bg, env, op = self.bg, self.env, e["op"]
        kw = dict(e["kw"])
        for k in ("big", "refuse", "rewrites", "status", "log", "policy_in_force", "cube_in_force"):
            kw.pop(k, None)
        out = {}
        if op == "greedy":
            _set_lanes(env, kw.pop("lanes"))
            env.step_greedy(roll=False, auto_reset=False, **kw)
        elif op == "run_greedy":
            _set_lanes(env, kw.pop("lanes"))
            env.run_greedy(kw.pop("n_steps"), **kw)
        elif op == "random":
            _set_lanes(env, kw.pop("lanes"))
            env.step_random(**kw)
        elif op == "sampled":
            _set_lanes(env, kw.pop("lanes"))
            env.step_sampled(kw.pop("temperature"), roll=False, auto_reset=False, **kw)
        elif op == "run_sampled":
            _set_lanes(env, kw.pop("lanes"))
            env.run_sampled(kw.pop("n_steps"), kw.pop("temperature"), **kw)
        elif op == "search":
            _set_lanes(env, kw.pop("lanes"))
            env.step_search(roll=False, auto_reset=False, **kw)
        elif op == "analyze":
            sel = kw.pop("lanes")
            if kw.pop("played", None) == "start":                          # no lane's afterstate (the fixture boards are in mid-game): status 3
                _set_lanes(env, sel)
                played = torch.as_tensor(np.tile(H.OR.START, (env.n, 1))).to(env.device)
            else:
                played = _played(env, sel)
            bg._capi.check(env._lib.bgamd_env_analyze_moves(env._h, 0, kw["top_k"], bg._ptr(played), bg._stream()), "analyze_moves")
            torch.cuda.current_stream().synchronize()
        elif op == "preroll":
            st, tu = H.positions(*kw.pop("pos"))
            f, m = env.evaluate_preroll(st, tu, **kw)
            out.update(roll_values=_np(f), mean=_np(m))
        elif op == "rollout":
            st, tu = H.positions(*kw.pop("pos"))
            if "groups" in kw:
                kw["groups"] = list(kw["groups"])
            _flat("", env.rollout(st, tu, kw.pop("trials"), **kw), out)
        elif op == "evaluate":
            st, tu = H.positions(*kw.pop("pos"))
            rep = kw.pop("repeat", 1)
            out["values"] = _np(env.evaluate(np.tile(st, (rep, 1)), np.tile(tu, rep), precision=getattr(bg, kw.pop("precision")), **kw))
        elif op == "evaluate_incremental":
            rs, rt, kids, ri = _afterstate_rows(kw["lanes"], kw["roots"])
            out["values"] = _np(env.evaluate_incremental(rs, rt, kids, ri))
        elif op == "encode":
            out["x"] = _np(env.encode(*H.positions(*kw["pos"])))
        elif op == "encode_rows":
            st, tu = H.positions(*kw["pos"])
            rows = bg.pack_rows(st, tu)
            out.update(rows=_np(rows), x=_np(env.encode_rows(rows)))
        elif op == "enumerate":
            _set_lanes(env, kw["lanes"])
            out.update(zip(("offsets", "counts", "states", "seq", "seq_len"), (_np(x) for x in env.enumerate())))
        elif op in ("legal_moves", "try_move"):
            _, tu, dice = _set_lanes(env, kw["lanes"])
            n, pairs = env.legal_moves(tu, dice[:, 0])
            out.update(n=_np(n), pairs=_np(pairs))
            if op == "try_move":
                first = out["pairs"][:, 0, :].astype(np.int32) * (out["n"] > 0)[:, None]
                out["err"] = _np(env.try_move(tu, dice[:, 0], first[:, 0], first[:, 1]))
        elif op == "log_trajectory":
            env.reset()
            _set_lanes(env, kw["lanes"])
            log = env.record_trajectory(kw["max_plies"])
            for _ in range(kw["steps"]):
                env.step_greedy(auto_reset=False)
            out["log"] = _np(log)
            env.record_trajectory(None)
        elif op == "log_ring":
            env.reset()
            _set_lanes(env, kw["lanes"])
            rows, end = env.record_ring(kw["ring_steps"])
            for _ in range(kw["steps"]):
                env.step_greedy()
            out.update(rows=_np(rows), end=_np(end), step=np.array([env.trajectory_step()]))
            env.record_ring(None)
        elif op == "log_search":
            env.reset()
            _set_lanes(env, kw["lanes"])
            logs = env.record_search_log(kw["max_plies"])
            for _ in range(kw["steps"]):
                env.step_search(top_k=kw["top_k"], auto_reset=False)
            out.update(zip(("rows", "after", "target", "v1"), (_np(x) for x in logs)))
            env.record_search_log(None)
        elif op == "load":
            for slot, name in enumerate(kw["nets"]):
                if name:
                    env.load_weights(self.tables[name], slot)
        elif op == "reseed":
            env.reseed(kw["seed"])
        elif op == "setting":
            self.setting(kw["what"], kw["on"], kw)
        else:
            raise KeyError(op)
        return out

    def refused_reads(self, only=None):
        """every read of the refusal list: BGAMD_E_INVALID"""
        for call, (read, _) in H.REFUSABLE.items():
            if only and call[len("bgamd_env_"):] not in only:
                continue
            got = do_read(self.bg, self.env, read)
            assert isinstance(got, Refused) and got.code == H.E_INVALID, (call, "asked for out of turn", got)

    def run(self, e, standalone=False):
        """call + reads -> flat outputs.  A `refuse` entry: the code, and the documented state unchanged.  standalone: the sticky setting
        an entry runs under in SOIL's order is set for it here and cleared behind it."""
        bg, env, kw = self.bg, self.env, e["kw"]
        self.last = e["name"]
        if e["op"] == "refused_reads":
            self.refused_reads(kw.get("only"))
            return {}
        soil = H.by_name(H.SOIL)
        if standalone and kw.get("policy_in_force"):
            self.setting("rollout_policy", True, {})
        if standalone and kw.get("cube_in_force"):
            self.setting("rollout_cube", True, soil["cube_set"]["kw"])
        if kw.get("log") == "trajectory":
            env.record_trajectory(4)
        if kw.get("log") == "search":
            env.record_search_log(4)
        try:
            if "refuse" in kw:
                before = _documented_state(bg, env) if e["op"] not in ("greedy", "search") else None
                with pytest.raises(bg.BgamdError) as err:
                    self.call(e)
                assert err.value.code == kw["refuse"], (e["name"], err.value.code)
                if before is None:                                           # (a step's call sets boards and dice first: from there on)
                    _set_lanes(env, kw["lanes"])
                    before = _documented_state(bg, env)
                    with pytest.raises(bg.BgamdError):
                        self.call(e)
                after = _documented_state(bg, env)
                assert first_difference(before, after) is None, (e["name"], "a refused call changed", first_difference(before, after))
                return {}
            out = self.call(e)
            if kw.get("cube_in_force"):
                assert "cube" in e["reads"]
            do_reads(bg, env, e, out)
            if "status" in kw:                 # rows that are no afterstates: documented as status 3 and no code (2: the lane has no move at all)
                status = out["analysis.status"]
                assert np.isin(status, (2, kw["status"])).all() and (status == kw["status"]).sum() > env.n // 2, (e["name"], status)
            return out
        finally:
            if kw.get("log") == "trajectory":
                env.record_trajectory(None)
            if kw.get("log") == "search":
                env.record_search_log(None)
            if standalone and kw.get("policy_in_force"):
                self.setting("rollout_policy", False, {})
            if standalone and kw.get("cube_in_force"):
                self.setting("rollout_cube", False, {})


def first_difference(a, b):
    """-> None, or (field, first differing element, a's, b's) of two flat outputs"""
    if sorted(a) != sorted(b):
        return ("fields", sorted(set(a) ^ set(b)), None, None)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape:
            return (k, "dtype / shape", (x.dtype, x.shape), (y.dtype, y.shape))
        if x.tobytes() != y.tobytes():
            xb, yb = (np.frombuffer(v.tobytes(), np.uint8) for v in (x, y))
            i = int(np.flatnonzero(xb != yb)[0]) // max(x.dtype.itemsize, 1)
            return (k, i, x.reshape(-1)[i], y.reshape(-1)[i])
    return None


def same(fresh, used, probe, order, last):
    d = first_difference(fresh, used)
    assert d is None, "probe %s, order %s: field %s, first differing element %s: fresh %r, used %r (SOIL step run last: %s)" % (
        probe, order, d[0], d[1], d[2], d[3], last)


# ---- the fresh side, once ------------------------------------------------------------------------------------------------------------------

_fresh = {}


@pytest.fixture(scope="module")
def fresh(bg):
    """(lanes of the env, probe name) -> the probe's outputs on an env created for it"""
    tables = _tables()

    def get(n, e):
        key = (n, e["name"])
        if key not in _fresh:
            r = Runner(bg, n, tables)
            _fresh[key] = r.run(e)
            r.close()
        return _fresh[key]
    yield get
    _fresh.clear()


def _used(bg, n, soil, outputs=None):
    """a new env through all of `soil` -> its runner, not yet brought back"""
    r = Runner(bg, n, _tables(), load=False)
    for e in soil:
        out = r.run(e)
        if outputs is not None:
            outputs[e["name"]] = out
    return r


def _check_internal_envs(r, e, strict_rscratch):
    """the internal envs the probe will use exist and are larger than the lanes it asks for (the trial env is re-created at exactly the
    lanes of a rollout: after a larger rollout it is larger, otherwise it is some other rollout's)"""
    fam = H.families(e)
    scratch, rscratch, mid = r.env.scratch_info()
    if "scratch" in fam:
        assert scratch > fam["scratch"], (e["name"], scratch, fam)
    if "mid" in fam:
        assert mid > fam["mid"], (e["name"], mid, fam)
    if "rscratch" in fam:
        assert rscratch > fam["rscratch"] if strict_rscratch else rscratch > 0, (e["name"], rscratch, fam)


@pytest.mark.parametrize("n, order", [(H.N, "listed"), (H.N, "reverse"), (1, "listed"), (1, "reverse")])
def test_probes_on_a_used_env(bg, fresh, n, order):
    probes, soil = (H.PROBES, H.SOIL) if n == H.N else (H.PROBES_1, H.SOIL_1)
    soil_out = {}
    r = _used(bg, n, soil, soil_out)
    last = r.last
    # SOIL's own outputs are not the probes': stale data would show
    for p in probes:
        for s in H.partner(p["name"], soil):
            common = [k for k in soil_out[s["name"]] if k in fresh(n, p) and "stats" not in k]
            if s["op"] == p["op"] and common:
                assert any(first_difference({k: soil_out[s["name"]][k]}, {k: fresh(n, p)[k]}) for k in common), (p["name"], s["name"])
    r.restore(settings=True)
    for p in (probes if order == "listed" else probes[::-1]):
        r.restore()
        _check_internal_envs(r, p, False)
        same(fresh(n, p), r.run(p), p["name"], "%s, %d lanes" % (order, n), last)
    r.close()


@pytest.mark.parametrize("n", [H.N, 1])
def test_probes_directly_behind_their_larger_soil_step(bg, fresh, n):
    probes, soil = (H.PROBES, H.SOIL) if n == H.N else (H.PROBES_1, H.SOIL_1)
    r = Runner(bg, n, _tables(), load=False)
    for slot, name in enumerate(H.SOIL_NETS):
        r.env.load_weights(r.tables[name], slot)
    for p in probes:
        partners = H.partner(p["name"], soil)
        if not partners:
            continue
        for slot, name in enumerate(H.SOIL_NETS):
            r.env.load_weights(r.tables[name], slot)
        for s in partners:
            r.run(s, standalone=True)
        last = r.last
        r.restore(settings=True)
        _check_internal_envs(r, p, True)
        same(fresh(n, p), r.run(p), p["name"], "behind %s, %d lanes" % ("+".join(s["name"] for s in partners), n), last)
    r.close()


def test_2ply_rollout_on_envs_sized_once_by_a_larger_one(bg, fresh):
    """The 2-ply rollout sizes the search's scratch env once, for lanes x top_k x 21 virtual roots, and its trial env exactly.  Behind
    SOIL's 2-ply rollout (96 lanes, top_k 3 by the sticky policy: 96 * 3 * 21 = 6 048 -> 6 144 scratch lanes) the probe (64 lanes, top_k
    2: 64 * 2 * 21 = 2 688 -> 2 816) runs on the scratch env of 6 144 lanes as it stands and on a trial env re-created at 64."""
    r = Runner(bg, H.N, _tables(), load=False)
    for slot, name in enumerate(H.SOIL_NETS):
        r.env.load_weights(r.tables[name], slot)
    soil, p = H.by_name(H.SOIL)["big_ro_2ply"], H.by_name(H.PROBES)["ro_2ply"]
    assert (H.families(soil)["scratch"], H.families(soil)["rscratch"]) == (6144, 96)
    assert (H.families(p)["scratch"], H.families(p)["rscratch"]) == (2816, 64)
    r.run(soil, standalone=True)
    assert r.env.scratch_info() == [6144, 96, 0]
    r.restore(settings=True)
    same(fresh(H.N, p), r.run(p), "ro_2ply", "behind big_ro_2ply alone", "big_ro_2ply")
    assert r.env.scratch_info() == [6144, 64, 0]
    r.close()


def test_search3_and_2ply_rollouts_with_a_mid_env_of_256_lanes(bg, fresh, monkeypatch):
    """BGAMD_SEARCH3_CHUNK is read when an env's mid level is first sized: this run needs a used env of its own.  The mid env then has 256
    lanes whatever came before, and the probe's mid lanes take more than one piece of them."""
    monkeypatch.setenv("BGAMD_SEARCH3_CHUNK", "256")
    r = _used(bg, H.N, H.SOIL)
    last = r.last
    probes = H.by_name(H.PROBES)
    r.restore(settings=True)
    # (the 2-ply rollout never touches the mid env -- only the 3-ply step's deep level does: for it this run is the listed order once
    #  more on an env whose mid env happens to have 256 lanes, and the assertion on the mid env below says nothing about the rollout)
    for name in ("search3", "ro_2ply"):
        r.restore()
        assert r.env.scratch_info()[2] == 256 and r.env.scratch_info()[0] > H.families(probes[name])["scratch"]
        got = r.run(probes[name])
        same(fresh(H.N, probes[name]), got, name, "listed, mid env of 256 lanes", last)
        if name == "search3":
            assert got["search3_info.info"][3] * H.ROLLS > 256 and got["search3_info.info"][3] * H.ROLLS % 256      # a partial last piece
    r.close()


def test_a_reset_env_is_a_new_env(bg):
    """After SOIL: reseed(seed) + reset() + reset_stats().  Then snapshot, progress, stats, dice and 20 greedy steps with auto-reset are a
    new env's.  What the header documents as surviving bgamd_env_reset is named here: the weights ("bgamd_env_load_weights ... kept
    until the next load": both envs hold the same tables) and the sticky settings, which SOIL has cleared.  Nothing else is excluded."""
    tables = _tables()
    r = _used(bg, H.N, H.SOIL)
    last = r.last
    new = Runner(bg, H.N, tables, load=False)
    for slot, name in enumerate(H.SOIL_NETS):                               # (SOIL leaves its own tables loaded: the new env gets the same)
        new.env.load_weights(tables[name], slot)
    r.env.reseed(H.SEED)
    r.env.reset()
    r.env.reset_stats()

    def state(x, stepped):
        out = _documented_state(bg, x.env)
        if stepped:
            _flat("last_choice.", x.env.last_choice(), out)
        return out
    same(state(new, False), state(r, False), "state after reset", "reset", last)
    for step in range(20):
        for x in (new, r):
            x.env.step_greedy()
        same(state(new, True), state(r, True), "greedy step %d after reset" % step, "reset", last)
    for x in (new, r):
        assert x.env.stats()["error_flags"] == 0
        x.close()


@pytest.fixture(scope="module")
def soiled(bg):
    r = _used(bg, H.N, H.SOIL)
    r.restore(settings=True)
    yield r
    r.close()


@pytest.mark.parametrize("between", [x["name"] for x in H.INTERVENING])
def test_reads_after_unrelated_calls(bg, fresh, soiled, between):
    """Between a probe's call and a read: a call that is documented neither to answer that read anew nor to use what it reads as scratch.
    The read is then refused with BGAMD_E_INVALID, or returns exactly the bits it returned directly after its own call -- the fresh side's.
    search_info / search3_info count when first asked: they are also asked for the first time only after the other call."""
    r, last = soiled, "the whole of SOIL, then the pairs before this one"
    probes = H.by_name(H.PROBES)
    pairs = [q for q in H.read_pairs() if q[2]["name"] == between]
    assert pairs
    refused = 0
    for read, pname, x, lazy in pairs:
        p = probes[pname]
        want = {k[len(read) + 1:]: v for k, v in fresh(H.N, p).items() if k.startswith(read + ".")}
        assert want, (read, pname)
        r.restore()
        r.call(p)
        if not lazy:
            first = do_read(bg, r.env, read)
            assert not isinstance(first, Refused)
            same(want, first, pname, "read %s directly" % read, last)
        if "refuse" in x["kw"]:
            r.run(x)
        else:
            r.call(x)
        got = do_read(bg, r.env, read)
        what = "read %s after %s%s" % (read, x["name"], ", first asked for then" if lazy else "")
        if isinstance(got, Refused):
            assert got.code == H.E_INVALID, (pname, what, got)
            refused += 1
        else:
            assert (read, pname, x["name"]) not in H.MUST_REFUSE, (pname, what, "answered, but that call invalidates it")
            same(want, got, pname, what, last)
    assert refused >= len([m for m in H.MUST_REFUSE if m[2] == between])


# ---- the learner handle ----------------------------------------------------------------------------------------------------------------------
# The kernel route of bgamd_td_step is read from BGAMD_TD_* when a learner is created, so one handle has one route: one used learner per
# route of tests/learner_routes.py.  The delayed update's one-launch step takes a streamed replay through at least TD_DELAY_SLICES = 201
# workgroups (csrc/bg_td_plan.h, td_delay_g), more slots than the 160-game log of tests/test_gpu_learner_steps.py has games: the delayed
# replay streams that log four times side by side (640 games) through 512 slots; every other replay runs on the log itself.

def _learner_log(bg):
    import learner_ref as LR
    from test_gpu_learner_steps import _rows
    _, _, ln, p1 = LR.log()
    rows = _rows(bg, False)
    return rows, np.asarray(ln), np.asarray(p1), rows.repeat(1, 4, 1).contiguous(), np.tile(ln, 4), np.tile(p1, 4)


LEARNER_GAMES, DELAY_SLOTS = 640, 512


def _new_learner(monkeypatch, route):
    import learner_ref as LR
    from backgammon_env.learner import DeviceTDLambdaLearner
    from learner_routes import ROUTES, _VARS
    for k in _VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    return DeviceTDLambdaLearner(NT.table("ckpt"), max_games=LEARNER_GAMES, alpha=LR.ALPHA, lam=LR.LAM)


def _learner_call(bg, L, what):
    """one replay or fit step from the weights w0 -> its update (theta - w0 is theta itself, bit for bit: w0 is the same), the final theta,
    the replay's (sum of squared errors, updates), active_columns, written_columns, or fit_stats"""
    import learner_ref as LR
    rows, ln, p1, rows4, ln4, p14 = _learner_log(bg)
    L.set_weights(NT.table("ckpt"))
    out = {}
    if what == "lockstep":
        out["stats"] = L.replay_rows(rows, ln, p1, batch_scale=LR.BATCH_SCALE)
    elif what == "streamed":
        out["stats"] = L.replay_rows(rows, ln, p1, batch_scale=LR.BATCH_SCALE, slots=LR.SLOTS)
    elif what == "wide":                                             # (delayed while set_delay(1) holds and the route has the fused launch)
        out["stats"] = L.replay_rows(rows4, ln4, p14, batch_scale=48.0 / DELAY_SLOTS, slots=DELAY_SLOTS)
    elif what == "fit":
        y = np.random.RandomState(5).uniform(0.0, 1.0, 6 * rows.shape[1]).astype(np.float32)
        y[::37] = np.nan                                             # (skipped rows: counted by fit_stats)
        L.fit_step(rows[:6].reshape(-1, 8), y, batch_scale=0.05)
        out["fit_stats"] = L.fit_stats()
    else:
        raise KeyError(what)
    if what != "fit":
        out["columns"] = (L.active_columns(), L.written_columns())
    out = {k: np.asarray(v, np.float64) for k, v in out.items()}
    out["theta"] = _np(L.theta)
    return out


@pytest.mark.parametrize("route", ["valu", "direct_slice", "matrix_pipe", "direct_pipe", "direct_wide", "direct_wide_nt", "fused_g1",
                                   "fused_g16", "ordinary"])
def test_learner_handle_through_its_calls(bg, monkeypatch, route):
    """One learner per route through: a lock-step replay, a streamed one, a fit step, set_delay(1) with the wide streamed replay (delayed
    where the route has the one-launch step), then -- the delay still set, its buffers just used -- a lock-step and a 7-slot replay (they
    do not qualify: exact), set_delay(0) and the wide replay exactly, and the first three once more.  set_weights(w0) before each.  Every
    result -- final theta, the replay's statistics, active_columns, written_columns, fit_stats -- is, bit for bit, that of a learner
    created under the same route for that call alone."""
    from learner_routes import ROUTES
    assert route in ROUTES and len(ROUTES) == 9
    alone = {}

    def want(what, delay=0):
        if (what, delay) not in alone:
            A = _new_learner(monkeypatch, route)
            A.set_delay(delay)
            alone[what, delay] = _learner_call(bg, A, what)
            del A
        return alone[what, delay]

    U = _new_learner(monkeypatch, route)
    done = []
    for delay, what in ((0, "lockstep"), (0, "streamed"), (0, "fit"), (1, "wide"), (1, "lockstep"), (1, "streamed"), (1, "fit"), (1, "wide"),
                        (0, "wide"), (0, "lockstep"), (0, "streamed"), (0, "fit"), (1, "wide")):
        U.set_delay(delay)
        got = _learner_call(bg, U, what)
        done.append("%s (delay %d)" % (what, delay))
        d = first_difference(want(what, delay), got)
        assert d is None, "route %s, %s: field %s, first differing element %s: alone %r, used %r (the handle's calls so far: %s)" % (
            route, done[-1], d[0], d[1], d[2], d[3], ", ".join(done))
    # a replay that does not qualify is exact whatever the delay says; where the route has the one-launch step the delay is another result
    for what in ("lockstep", "streamed", "fit"):
        assert first_difference(want(what, 0), want(what, 1)) is None, (route, what)
    if route in ("valu", "ordinary"):                # (512 slots, two per workgroup: 256 workgroups; the other routes have no such launch)
        assert first_difference(want("wide", 0), want("wide", 1)) is not None, (route, "the wide replay was not delayed")
