"""The conditions tests/test_gpu_history_match.py rests on, without a device: the match's read call is listed, and together with
tests/history_cases.py's lists the listing covers every read call of include/bgamd.h under either spelling (_read, _results, ...);
the match's soil is larger than its probe and uses other tables; every intervening call of the history tests is asked."""
import os
import re

import history_cases as H
import history_match_cases as HM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _Match:                                              # (stand-ins: the package needs torch, the tables only their shapes here)
    def __init__(self, table, away1, away2, state, window_share=0.5):
        self.table, self.away1, self.away2, self.state, self.window_share = table, away1, away2, state, window_share


class _Table:
    @staticmethod
    def janowski(M):
        return M


def test_every_read_call_of_the_header_is_listed_here_or_in_the_history_cases():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgamd.h")).read(), flags=re.S)
    reads = set(re.findall(r"\b(bgamd_env\w*(?:_read|_results|_info|_last_choice|_choice_spread|_stats|_kernel_choice|_kernel_times))\s*\(", hdr))
    reads.discard("bgamd_env_reset_stats")
    listed = set(H.REFUSABLE) | set(H.NEVER_REFUSED) | set(HM.REFUSABLE)
    assert reads == listed, reads ^ listed
    assert set(HM.REFUSABLE) == {"bgamd_env_rollout_match_results"} and not set(HM.REFUSABLE) & (set(H.REFUSABLE) | set(H.NEVER_REFUSED))
    # (bgamd_env_rollout_match_thresholds reads the uploaded table, not a rollout: tests/test_gpu_rollout_match.py asks it out of turn)
    p = HM.probe(_Match, _Table)
    for call, (read, probe) in HM.REFUSABLE.items():
        assert probe == p["name"] and read in p["reads"], call
    assert all(read in p["reads"] for read, _ in HM.ALSO_READ)


def test_the_soil_is_larger_and_other_than_the_probe():
    p, soil = HM.probe(_Match, _Table), HM.soil(_Match, _Table)
    big, dmp = soil
    assert big["kw"]["pos"][1] > p["kw"]["pos"][1] and big["kw"]["trials"] > p["kw"]["trials"]
    assert big["kw"]["match"].table > p["kw"]["match"].table > dmp["kw"]["match"].table == 1           # the tables' sizes
    assert big["kw"]["match"].window_share != p["kw"]["match"].window_share and big["kw"]["seed"] != p["kw"]["seed"]
    assert {s for e in soil + [p] for s in e["kw"]["match"].state} == {0, 1, 2}
    for e in soil + [p]:
        m, n = e["kw"]["match"], e["kw"]["pos"][1]
        assert len(m.away1) == len(m.away2) == len(m.state) == n == len(e["kw"]["groups"])
        assert all(1 <= a <= m.table and 1 <= b <= m.table and ((min(a, b) == 1) == (s != 0)) for a, b, s in zip(m.away1, m.away2, m.state))
        assert e["kw"]["pos"][1] <= H.BUDGET["positions"] and e["kw"]["trials"] <= H.BUDGET["trials"] and e["kw"]["max_plies"] <= H.BUDGET["max_plies"]
        assert not e["kw"]["cube"].get("jacoby")


def test_every_intervening_call_is_asked_and_the_rollouts_must_refuse():
    names = [x["name"] for x in H.INTERVENING]
    assert set(HM.MUST_REFUSE) <= set(names) and set(HM.MUST_REFUSE) == {x["name"] for x in H.INTERVENING if x["op"] == "rollout"}
    assert len(names) >= 9
