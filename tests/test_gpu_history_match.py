"""Match play under the history rule on the MI355X (tests/test_gpu_history.py's method and runner, tests/history_match_cases.py's
entries): a rollout under a match on an env that has been through the whole of SOIL, and through larger rollouts under other match
tables and a set-and-cleared sticky match, returns bit for bit what an env created for it returns; its reads
(bgamd_env_rollout_match_results, the paired read's which = 4) are refused out of turn, and after every intervening call of the history
tests they are refused with BGAMD_E_INVALID or return exactly the bits they returned directly after their own call."""
import pytest

import history_cases as H
import history_match_cases as HM
import test_gpu_history as TH

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# the history tests' reads and the match's two, in a table of this file's own
READERS = dict(TH.READERS, match=lambda bg, env: env.rollout_match_read(per_trial=True), paired_mwc=TH._paired("mwc"))


def do_read(bg, env, read):
    """-> {field: array}, or TH.Refused(code): test_gpu_history.do_read on this file's table"""
    try:
        out = {}
        TH._flat("", READERS[read](bg, env), out)
        return out
    except bg.BgamdError as e:
        return TH.Refused(e.code)


def run(r, e):
    """Runner.run with the reads the runner does not know made here, directly behind its own"""
    out = r.run(dict(e, reads=tuple(x for x in e["reads"] if x in TH.READERS)))
    for read in (x for x in e["reads"] if x not in TH.READERS):
        got = do_read(r.bg, r.env, read)
        assert not isinstance(got, TH.Refused), (e["name"], read, got)
        out.update({read + "." + k: v for k, v in got.items()})
    return out


@pytest.fixture(scope="module")
def bg():
    import backgammon_env
    return backgammon_env


@pytest.fixture(scope="module")
def probe(bg):
    return HM.probe(bg.Match, bg.MatchTable)


@pytest.fixture(scope="module")
def fresh(bg, probe):
    r = TH.Runner(bg, H.N, TH._tables())
    out = run(r, probe)
    r.close()
    return out


def _refused(bg, env):
    for read in ("match", "paired_mwc"):
        got = do_read(bg, env, read)
        assert isinstance(got, TH.Refused) and got.code == H.E_INVALID, (read, "asked for out of turn", got)


@pytest.fixture(scope="module")
def soiled(bg, probe):
    """through SOIL, then the match's own soil: larger rollouts under other tables, a sticky match set in the C ABI with a rollout run
    under it and cleared, the reads asked for out of turn on the way"""
    r = TH._used(bg, H.N, H.SOIL)
    r.env._rollout_shape = getattr(r.env, "_rollout_shape", (1, 1))
    _refused(bg, r.env)                                                    # SOIL's last rollouts ran under no match
    for e in HM.soil(bg.Match, bg.MatchTable):
        run(r, e)
    one = torch.ones(8, dtype=torch.int32, device=r.env.device)
    two, zero = 2 * one, 0 * one                                           # (kept until the rollout's intake has read them)
    r.env._set_match(bg.MatchTable.janowski(3), 0.0, two, two, zero)        # sticky in the C ABI: the next cubeful rollout runs under it
    s = H.by_name(H.SOIL)
    r.setting("rollout_cube", True, s["cube_set"]["kw"])
    under = dict(s["big_ro_cube"], reads=HM.READS)
    run(r, under)
    assert r.env._lib.bgamd_env_rollout_match(r.env._h, 0, 0, None, None, 0.0, None, None, None) == 0
    r.run(s["big_ro_cube"])                                                # cleared: the same call under the cube alone
    _refused(bg, r.env)
    r.setting("rollout_cube", False, {})
    r.restore(settings=True)
    yield r
    r.close()


def test_reads_are_refused_out_of_turn(bg, probe):
    r = TH.Runner(bg, H.N, TH._tables())
    lib, h = r.env._lib, r.env._h
    assert lib.bgamd_env_rollout_match_results(h, None, None, None, None, None) == H.E_INVALID       # before any rollout
    r.run(H.by_name(H.PROBES)["ro_cube"])                                  # a cubeful rollout under no match
    _refused(bg, r.env)
    run(r, probe)
    r.run(H.by_name(H.SOIL)["rollout_bad_board"])                          # a rollout that failed
    _refused(bg, r.env)
    r.close()


def test_probe_on_a_used_env(bg, probe, fresh, soiled):
    for _ in range(2):                                                     # ... and once more behind itself
        soiled.restore()
        TH.same(fresh, run(soiled, probe), probe["name"], "behind SOIL and the match's soil", soiled.last)


@pytest.mark.parametrize("between", [x["name"] for x in H.INTERVENING])
def test_reads_after_unrelated_calls(bg, probe, fresh, soiled, between):
    r, last = soiled, "SOIL, the match's soil, then the pairs before this one"
    x = [e for e in H.INTERVENING if e["name"] == between][0]
    for read in [v[0] for v in HM.REFUSABLE.values()] + [v[0] for v in HM.ALSO_READ]:
        want = {k[len(read) + 1:]: v for k, v in fresh.items() if k.startswith(read + ".")}
        assert want, read
        r.restore()
        r.call(probe)
        first = do_read(bg, r.env, read)
        assert not isinstance(first, TH.Refused)
        TH.same(want, first, probe["name"], "read %s directly" % read, last)
        if "refuse" in x["kw"]:
            r.run(x)
        else:
            r.call(x)
        got = do_read(bg, r.env, read)
        what = "read %s after %s" % (read, between)
        if isinstance(got, TH.Refused):
            assert got.code == H.E_INVALID, (what, got)
        else:
            assert between not in HM.MUST_REFUSE, (what, "answered, but that call invalidates it")
            TH.same(want, got, probe["name"], what, last)
        if between in HM.MUST_REFUSE:
            assert isinstance(got, TH.Refused), what
