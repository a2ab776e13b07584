"""The conditions tests/test_gpu_history.py rests on, without a device: the tables of tests/history_cases.py really leave the kept state
larger (and, somewhere, smaller) than every probe needs, every sticky setting is set and cleared, every read call of include/bgamd.h that
can be refused is asked for out of turn, and the sizes stay inside the budget."""
import os
import re

import numpy as np

import history_cases as H

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _sets():
    return (("65 lanes", H.PROBES, H.SOIL), ("1 lane", H.PROBES_1, H.SOIL_1))


def test_names_ops_and_families():
    for _, probes, soil in _sets():
        for entries in (probes, soil):
            names = [e["name"] for e in entries]
            assert len(set(names)) == len(names)
            for e in entries:
                fam = H.families(e)
                assert set(fam) <= set(H.FAMILIES), e["name"]
                assert all(fam[k] > 0 for k in fam if k in H.SIZED), (e["name"], fam)
    # every feature of the issue's list is a probe
    ops = {e["op"] for e in H.PROBES}
    assert ops >= {"greedy", "run_greedy", "random", "sampled", "run_sampled", "search", "analyze", "preroll", "rollout", "evaluate",
                   "evaluate_incremental", "encode", "encode_rows", "enumerate", "legal_moves", "try_move", "log_trajectory", "log_ring",
                   "log_search"}
    kinds = [e["kw"] for e in H.PROBES if e["op"] == "rollout"]
    assert len(kinds) == 5 and any(k.get("plies") == 2 for k in kinds) and any("cube" in k for k in kinds) and any("groups" in k for k in kinds)
    assert {r for e in H.PROBES for r in e["reads"] if r.startswith("paired_")} == {"paired_value", "paired_vr", "paired_equity", "paired_cubeful"}
    assert {e["kw"].get("precision") for e in H.PROBES if e["op"] == "evaluate"} == {"F32", "F16X2", "BF16"}
    assert all(f in {k for e in H.PROBES + H.SOIL for k in H.families(e)} for f in H.FAMILIES)


def test_every_probe_has_a_larger_soil_step_in_every_family_it_touches():
    for what, probes, soil in _sets():
        for p in probes:
            need = {k: v for k, v in H.families(p).items() if k in H.SIZED}
            partners = H.partner(p["name"], soil)
            assert partners or not need, (what, p["name"], "no SOIL step names it")
            for fam, size in need.items():
                # ... among the steps the targeted pairs run directly before it, and so in SOIL as a whole
                assert any(H.families(s).get(fam, 0) > size for s in partners), (what, p["name"], fam, size)


def test_soil_also_has_smaller_steps_so_that_growth_happens_between_probes():
    for fam in ("scratch", "mid", "rscratch", "search_buffers", "rollout_buffers"):
        # (an internal env that is kept has 256 lanes at least: a probe that needs no more cannot meet a smaller one)
        floor = {"search_buffers": 0, "rollout_buffers": 0, "rscratch": 0}.get(fam, 256)
        need = [H.families(p)[fam] for p in H.PROBES if H.families(p).get(fam, 0) > floor]
        sizes = [H.families(s)[fam] for s in H.SOIL if fam in H.families(s)]
        assert min(sizes) < min(need), (fam, min(sizes), min(need))
        first_small = min(k for k, s in enumerate(H.SOIL) if H.families(s).get(fam, 1 << 60) < min(need))
        assert any(H.families(s).get(fam, 0) > max(need) for s in H.SOIL[first_small + 1:]), fam      # it grows after the small one


def test_other_content():
    a, b = H.lanes("A"), H.lanes("B")
    assert not (a[0] == b[0]).all(axis=1).any() and H.live("A") == 60 and H.live("B") == 65 and H.live("A3") == 9 and H.live("B3") == 12
    assert (a[2][:, 0] != a[2][:, 1]).all() and (b[2][:, 0] == b[2][:, 1]).any()
    assert H.lanes("A1")[0].shape == (1, 28) and (H.lanes("B1")[2][:, 0] == H.lanes("B1")[2][:, 1]).all()
    assert H.SEED != H.OTHER_SEED and H.RO_SEED != H.RO_OTHER_SEED and not set(H.PROBE_NETS) & set(H.SOIL_NETS)
    bad = H.positions("bad", 8)[0]
    assert (np.abs(bad[:-1]) <= 15).all() and (np.abs(bad[-1]) > 15).sum() == 1
    loads = [e["kw"]["nets"] for e in H.SOIL if e["op"] == "load"]
    assert [n[0] for n in loads if n[0]] == [H.SOIL_NETS[0]] and [n[1] for n in loads if n[1]] == [H.SOIL_NETS[1]]


def test_every_setting_is_set_and_cleared():
    names = [e["name"] for e in H.SOIL]
    assert set(H.SETTINGS) == {"rollout_policy", "rollout_cube", "time_kernels", "reseed"}
    for what, (on, off) in H.SETTINGS.items():
        assert on in names and off in names and names.index(on) + 1 < names.index(off), what       # set, something run, cleared
    s = H.by_name(H.SOIL)
    # the logs: one entry each, whose op sets the log, steps under it and unsets it
    assert set(H.LOG_SETTINGS) == {"trajectory", "ring", "search_log"}
    for what, (entry, op) in H.LOG_SETTINGS.items():
        assert s[entry]["op"] == op and s[entry]["kw"]["steps"] > 0, what
    for what in ("rollout_policy", "rollout_cube", "time_kernels"):
        on, off = (s[n]["kw"] for n in H.SETTINGS[what])
        assert on["what"] == off["what"] == what and on["on"] and not off["on"]
        between = H.SOIL[names.index(H.SETTINGS[what][0]) + 1:names.index(H.SETTINGS[what][1])]
        assert between, what                                    # something runs while it is in force
    assert s["reseed_other"]["kw"]["seed"] == H.OTHER_SEED and s["reseed_back"]["kw"]["seed"] == H.SEED
    assert H.SOIL_POLICY["plies"] == 2
    assert any(e["kw"].get("policy_in_force") for e in H.SOIL) and any(e["kw"].get("cube_in_force") for e in H.SOIL)
    # the refused calls of the issue's list
    refused = {e["name"]: e["kw"]["refuse"] for e in H.SOIL if "refuse" in e["kw"]}
    assert refused == {"search_empty_slot": H.E_NOWEIGHTS, "preroll_bad_board": H.E_STATE, "rollout_bad_board": H.E_STATE,
                       "search_with_a_log": H.E_INVALID, "greedy_with_a_search_log": H.E_INVALID}
    assert names.index("search_empty_slot") < names.index("weights_slot1")
    assert names.index("big_ro_plain") < names.index("rollout_bad_board") and names.index("big_preroll") < names.index("preroll_bad_board")
    assert s["analyze_no_afterstates"]["kw"]["status"] == 3


def test_every_read_call_that_can_be_refused_is_in_the_refusal_list():
    hdr = open(os.path.join(ROOT, "include", "bgamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    reads = set(re.findall(r"\b(bgamd_env\w*(?:_read|_info|_last_choice|_choice_spread|_stats|_kernel_choice|_kernel_times))\s*\(", hdr))
    reads.discard("bgamd_env_reset_stats")
    assert reads == set(H.REFUSABLE) | set(H.NEVER_REFUSED), reads ^ (set(H.REFUSABLE) | set(H.NEVER_REFUSED))
    assert not set(H.REFUSABLE) & set(H.NEVER_REFUSED)
    probes = H.by_name(H.PROBES)
    for call, (read, probe) in H.REFUSABLE.items():
        assert read in probes[probe]["reads"], call
    pairs = H.read_pairs()
    for read, probe in list(H.REFUSABLE.values()) + list(H.ALSO_READ):
        mine = [x["name"] for r, p, x, _ in pairs if (r, p) == (read, probe)]
        assert len(set(mine)) >= 3, (read, mine)
    inter = {x["name"] for x in H.INTERVENING}
    assert {"preroll", "rollout", "analyze"} <= inter
    for lazy in H.LAZY:                                          # first asked for only after a pre-roll evaluation, a rollout and an analysis
        late = {x["name"] for r, _, x, first_late in pairs if r == lazy and first_late}
        assert {"preroll", "rollout", "analyze"} <= late, lazy
    for read, probe, x in H.MUST_REFUSE:
        assert any((r, p, e["name"]) == (read, probe, x) for r, p, e, _ in pairs)


def test_sizes_stay_inside_the_budget():
    B = H.BUDGET
    played_out = 0
    for e in H.PROBES + H.PROBES_1 + H.SOIL + H.SOIL_1 + H.INTERVENING:
        fam = H.families(e)
        assert fam.get("scratch", 0) <= B["scratch"] and fam.get("mid", 0) <= B["mid"], (e["name"], fam)
        if e["op"] == "rollout":
            kw = e["kw"]
            assert kw["pos"][1] <= B["positions"] and kw["trials"] <= B["trials"], e["name"]
            if kw["max_plies"] == 0:
                played_out += 1
            else:
                assert kw["max_plies"] <= B["max_plies"], e["name"]
        if e["op"] == "preroll":
            assert e["kw"]["pos"][1] <= B["positions"]
        if "lanes" in e["kw"] and isinstance(e["kw"]["lanes"], str):
            assert len(H.lanes(e["kw"]["lanes"])[0]) in (1, H.N)
    assert played_out == 2                                       # one probe, at 65 lanes and at 1
    # the sizes are those of the restated rules: spot values worked out by hand
    p = H.by_name(H.PROBES)
    assert H.families(p["search_k3"])["scratch"] == 4096 and H.families(p["analyze"])["scratch"] == 6912        # 65 * 3 * 21, 65 * 5 * 21
    assert H.families(p["ro_2ply"])["scratch"] == 2816 and H.families(p["ro_2ply"])["rscratch"] == 64           # 64 * 2 * 21
    assert H.families(p["ro_vr"])["scratch"] == 1536 and H.families(p["preroll"])["scratch"] == 256             # 64 * 21, 8 * 21
    assert H.families(p["search3"])["mid"] <= 512 and H.families(H.by_name(H.SOIL)["big_search3"])["mid"] == 768
    assert H.families(H.by_name(H.SOIL)["big_search"])["scratch"] == 16384
