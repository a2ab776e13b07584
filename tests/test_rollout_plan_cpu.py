"""The rollout's plan (csrc/bg_rollout_plan.h) without a GPU: the header, compiled into tests/sanitize/rollout_plan_driver.cpp, against the
independent restatement of the entry point it replaced (tests/rollout_plan_ref.py), field by field over every edge of its rules; every
refusal and their precedence; three deliberately wrong references that the comparison must catch; the loop's verdicts on scripted
read-backs; and the same sweep once more through a driver built with AddressSanitizer + UBSan (its own program: nothing is preloaded)."""
import itertools
import os
import shutil
import subprocess

import pytest

import rollout_cases as RC
import rollout_plan_ref as R
import search_lanes as SL

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
ROT, S1, VR = R.ROTATE, R.SLOT1, R.VR
FLAGS8 = [a | b | c for a in (0, ROT) for b in (0, VR) for c in (0, S1)]
UNKNOWN = 1                                             # a flag of the greedy step, not of the rollout
TS = (1, 2, 35, 36, 37, 72, 1296)
PS = (1, 2, 7, 255, 256, 257, 1820, 65536)
MS = tuple(range(27))
LANES = (0, 1, 255, 256, 257, 768, 65536, 2 ** 30, 2 ** 30 + 1, -1)
BIG_OFFSET = 2 ** 63 - 1                                # offset T - L wraps for every T > 2 (and passes through 2^64 several times for T = 1296)
OFFSETS = (0, 3, -1, BIG_OFFSET)
POLICIES = ((1, 0), (1, 5), (2, 0), (2, 1), (2, 5), (2, 8), (2, 25))


def req(flags=0, P=3, offset=0, T=40, M=3, lanes=0, has_states=1, has_group=0, plies=1, top_k=0, cube=0, w0=1, w1=1):
    return (flags, P, offset, T, M, lanes, has_states, has_group, plies, top_k, cube, w0, w1)


def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "rollout_plan_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("rollout_plan") / "rollout_plan_driver")


def run(exe, args, lines_in, extra_env=None):
    r = subprocess.run([exe, *map(str, args)], env={**os.environ, **(extra_env or {})}, input="".join(lines_in), capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(lines_in)
    return lines


def plans(exe, requests, extra_env=None):
    return run(exe, ("plan", R.TURN_LIMIT), ["%d %d %d %d %d %d %d %d %d %d %d %d %d\n" % q for q in requests], extra_env)


def parse(line):
    w = line.split()
    return dict(zip(w[0::2], map(int, w[1::2])))


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

def trial_count_edges():
    """(P, T) that put N = P T at 65 535 / 65 536 / 65 537 and at every multiple of 256 below that with both neighbours (T = 1), and
    for every other T of the sweep the position counts on both sides of N = 65 536 and of N = 256"""
    out = [(256 * k + d, 1) for k in range(1, 257) for d in (-1, 0, 1)]
    for T in TS[1:]:
        out += [(max(1, edge // T + d), T) for edge in (256, 65536) for d in (-1, 0, 1, 2)]
    return sorted(set(out))


def search_edges():
    """(lanes, plies, top_k): for every policy the lane counts that put L k 21 (k = 8 for top_k 0) just below, at and above SEARCH_CHUNK,
    and two far from it"""
    out = []
    for plies, k in POLICIES:
        at = -(-SL.SEARCH_CHUNK // ((k or 8) * 21))       # the first L with L k 21 >= SEARCH_CHUNK
        out += [(lanes, plies, k) for lanes in (at - 13, at - 1, at, at + 1, 256, 65536)]
    return out


def requests():
    """Every request of the sweep, once.  Section by section (a full product of all twelve fields would be 10^9 requests; every rule
    reads a few of them, and each section is the full product of the fields one group of rules reads):
      a) T x P x M x lanes x the eight flag combinations: refusals by lanes, F, n_fan, L, fan_chunks, R, G, preroll_positions (P on
         both sides of L with and without rotation and the luck pass), every need;
      b) N around every edge of the default lane count x lanes 0 / 256 x flags x two horizons;
      c) position_offset x T x P x lanes: lane_offset, with its wrap;
      d) flags (with an unknown bit) x group table x cube x the weight slots' four states x states given or not;
      e) the policy x lanes around SEARCH_CHUNK x horizons x flags;
      f) the 2^31 / 2^30 bounds."""
    out = [req(f, P, 0, T, M, lanes) for T in TS for P in PS for M in MS for lanes in LANES for f in FLAGS8]
    out += [req(f, P, 0, T, M, lanes) for P, T in trial_count_edges() for lanes in (0, 256) for f in FLAGS8 for M in (0, 7)]
    out += [req(f, P, off, T, 5, lanes) for off in OFFSETS for T in TS for P in PS for lanes in LANES for f in (0, ROT | VR)]
    out += [req(f, 7, 3, 37, M, 0, hs, hg, 1, 0, cube, w0, w1) for f in FLAGS8 + [UNKNOWN, UNKNOWN | VR, 512 | ROT] for hs in (1, 0) for hg in (0, 1)
            for cube in (0, 1) for w0 in (0, 1) for w1 in (0, 1) for M in (0, 1, 12)]
    out += [req(f, P, 0, 37, M, lanes, 1, 0, plies, k) for lanes, plies, k in search_edges() for P in (2, 300) for M in (0, 1, 7) for f in FLAGS8]
    out += [req(f, P, 0, T, 0, lanes) for P, T in ((2 ** 31 - 1, 1), (2 ** 31, 1), (1, 2 ** 31 - 1), (1, 2 ** 31), (2 ** 16, 2 ** 15 - 1), (2 ** 16, 2 ** 15),
                                                    (2 ** 31 - 1, 2 ** 31 - 1), (46341, 46341), (46340, 46340)) for lanes in (0, 256, 2 ** 30, 2 ** 30 + 1)
            for f in (0, ROT | VR)]
    return out


@pytest.fixture(scope="module")
def sweep():
    return requests()


@pytest.fixture(scope="module")
def header_lines(driver, sweep):
    return plans(driver, sweep)


def test_plan_is_the_entry_point_it_replaced(sweep, header_lines):
    """Every field of every plan equals what the parent commit's bgamd_env_rollout_grouped decided inline, and every refused request
    gets the parent's code."""
    n_refused = 0
    for q, line in zip(sweep, header_lines):
        want = R.render(R.plan(q))
        if line != want:                                  # field by field: the fields that differ
            raise AssertionError((q, sorted(set(parse(line).items()) ^ set(parse(want).items())), line, want))
        n_refused += line != "rc 0" and line.startswith("rc ") and len(line.split()) == 2
    print("%d plans compared, %d of them refusals" % (len(sweep), n_refused))
    assert len(sweep) > 150000 and 0.05 < n_refused / len(sweep) < 0.5


def test_sweep_covers_the_rules(sweep):
    """what the issue names, counted on the accepted requests' reference plans"""
    ps = [R.plan(q) for q in sweep]
    ok = [p for p in ps if p["rc"] == 0]
    assert {p["R"] for p in ok} == set(range(1, 9)) and {p["G"] for p in ok} == {16 // r for r in range(1, 9)}
    for rot in (0, 1):
        D = {p["M"] - rot for p in ok if p["rotate"] == rot and p["M"] > 0 and not p["two_ply"]}
        assert {11, 13, 17, 19, 23} <= D and (rot == 0 or 0 in D) and set(range(1, 26)) <= D
    assert {p["N"] for p in ok} >= {65535, 65536, 65537} | {256 * k + d for k in range(1, 256) for d in (-1, 0, 1)}
    assert {p["F"] for p in ok} == {0, 1, 2, 35, 36}
    assert any(p["fan_chunks"] > 1 for p in ok) and any(p["fan_chunks"] == 1 for p in ok) and any(p["fan_eval"] for p in ok)
    assert any(p["lane_offset"] >= 2 ** 63 for p in ok) and any(0 < p["lane_offset"] < 2 ** 32 for p in ok)
    offs = [q for q in sweep if q[2] == BIG_OFFSET and R.refusal(q) == 0]
    assert any(q[2] * q[3] - R.plan(q)["L"] >= 2 ** 64 for q in offs)                     # the product wraps
    for k in (1, 5, 8, 25):
        two = [p for p, q in zip(ps, sweep) if p["rc"] == 0 and p["two_ply"] and (q[9] or 8) == k]
        assert any(p["L"] * k * 21 < SL.SEARCH_CHUNK for p in two) and any(p["L"] * k * 21 >= SL.SEARCH_CHUNK for p in two)
        assert {p["search_scratch_lanes"] == SL.SEARCH_CHUNK for p in two} == {False, True}
    vr = [p for p in ok if p["vr"]]
    assert any(p["rotate"] and p["P"] > p["L"] for p in vr) and any(p["rotate"] and p["P"] < p["L"] for p in vr)
    assert any(not p["rotate"] and p["P"] > p["L"] and p["preroll_positions"] == p["L"] for p in vr)
    assert {(p["grouped"], p["cube"], p["vr"]) for p in ok} == {(g, c, v) for g in (0, 1) for c in (0, 1) for v in (0, 1)} - {(0, 1, 0), (1, 1, 0)}
    assert {R.refusal(q) for q in sweep} == {R.OK, R.E_INVALID, R.E_NOWEIGHTS}


def test_reference_agrees_with_the_rules_the_gpu_tests_use(sweep):
    """rollout_cases.run_length / default_lanes / fan_size (tests/test_gpu_rollout*.py assert rollout_info against them) say what the
    restatement says, over the whole sweep"""
    n = 0
    for q in sweep:
        p = R.plan(q)
        if p["rc"]:
            continue
        assert p["R"] == RC.run_length(p["M"], bool(p["rotate"]), 2 if p["two_ply"] else 1), q
        assert q[5] > 0 or p["L"] == RC.default_lanes(p["N"]), q
        assert p["F"] == (RC.fan_size(p["T"]) if p["rotate"] else 0), q
        n += 1
    assert n > 100000
    assert R.CHUNK == SL.SEARCH_CHUNK and RC.ROLLOUT_LANES == 65536 and RC.ROLLOUT_RUN == 8


# ---- refusals --------------------------------------------------------------------------------------------------------------------

REFUSED = [("no states", dict(has_states=0), R.E_INVALID), ("P < 1", dict(P=0), R.E_INVALID), ("T < 1", dict(T=0), R.E_INVALID),
           ("M < 0", dict(M=-1), R.E_INVALID), ("lanes < 0", dict(lanes=-1), R.E_INVALID), ("offset < 0", dict(offset=-1), R.E_INVALID),
           ("unknown flag", dict(flags=UNKNOWN), R.E_INVALID), ("unknown flag beside known ones", dict(flags=512 | ROT | VR), R.E_INVALID),
           ("P >= 2^31", dict(P=2 ** 31, T=1), R.E_INVALID), ("T >= 2^31", dict(P=1, T=2 ** 31), R.E_INVALID),
           ("P T >= 2^31", dict(P=2 ** 16, T=2 ** 15), R.E_INVALID), ("lanes > 2^30", dict(lanes=2 ** 30 + 1), R.E_INVALID),
           ("cube without the luck pass", dict(cube=1), R.E_INVALID), ("cube, rotation, no luck pass", dict(cube=1, flags=ROT), R.E_INVALID),
           ("slot 0 empty", dict(w0=0), R.E_NOWEIGHTS), ("slot 1 empty", dict(flags=S1, w1=0), R.E_NOWEIGHTS),
           ("both empty", dict(w0=0, w1=0), R.E_NOWEIGHTS)]
ACCEPTED = [dict(), dict(P=2 ** 31 - 1, T=1), dict(P=1, T=2 ** 31 - 1), dict(P=2 ** 16, T=2 ** 15 - 1, lanes=2 ** 30), dict(cube=1, flags=VR),
            dict(w1=0), dict(flags=S1, w0=0), dict(M=0, lanes=0, offset=0), dict(flags=ROT | VR | S1, has_group=1)]


def test_refusals_and_their_precedence(driver):
    """every rule alone; an accepted neighbour of each; and of two broken rules the earlier one's code: the only pair with different
    codes is (anything, an empty weight slot), and the weights are looked at last"""
    lines = plans(driver, [req(**kw) for _, kw, _ in REFUSED])
    for (name, kw, code), line in zip(REFUSED, lines):
        assert line == "rc %d" % code == R.render(R.plan(req(**kw))), name
    for kw, line in zip(ACCEPTED, plans(driver, [req(**kw) for kw in ACCEPTED])):
        assert line.startswith("rc 0 ") and line == R.render(R.plan(req(**kw))), kw
    invalid = [(n, kw) for n, kw, code in REFUSED if code == R.E_INVALID]
    pairs = [(n, {**kw, "w0": 0, "w1": 0}) for n, kw in invalid]
    pairs += [(a + " + " + b, {**kb, **ka}) for (a, ka), (b, kb) in itertools.combinations(invalid, 2)]
    for (name, kw), line in zip(pairs, plans(driver, [req(**kw) for _, kw in pairs])):
        assert line == "rc %d" % R.E_INVALID, name
    # a bound of the third block broken with the cube rule: still refused, with the same code, and no overflow on the way (UBSan run below)
    assert plans(driver, [req(P=2 ** 31 - 1, T=2 ** 31 - 1, cube=1, w0=0)]) == ["rc %d" % R.E_INVALID]


# ---- the comparison can tell ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrong,fields", [(dict(divisor_descent=False), {"R"}), (dict(fan_by_trials=False), {"F", "n_fan"}),
                                          (dict(preroll_by_positions=False), {"preroll_positions"})])
def test_a_wrong_reference_fails_the_comparison(sweep, header_lines, wrong, fields):
    """R = min(D, 8) without the descent to a divisor, F = 36 whatever T, preroll_positions = L whatever P: each differs from the header
    somewhere in the sweep, in its own field."""
    differing = set()
    for q, line in zip(sweep, header_lines):
        want = R.render(R.plan(q, **wrong))
        if line != want:
            got, ref = parse(line), parse(want)
            differing |= {k for k in got if got[k] != ref[k]}
    assert fields <= differing, differing
    derived = {"R": {"G", "stall_turns"}, "F": {"fan", "fan_chunks"}, "preroll_positions": {"preroll_lanes"}}
    assert differing <= fields | set().union(*(derived.get(f, set()) for f in fields)), differing


# ---- the loop's verdicts ---------------------------------------------------------------------------------------------------------------

def verdicts(exe, T, M, plies, reads, extra_env=None):
    return [int(x) for x in run(exe, ("progress", R.TURN_LIMIT, T, M, plies), ["%d %d %d\n" % r for r in reads], extra_env)]


PROGRESS_RUNS = [(0, 1, 8, 2), (3, 2, 1, 16), (5, 1, 5, 3)]          # (M, plies) -> (R, G)


def progress_scripts(R_, G):
    """N = 40 trials.  The scripts, each a loop of its own: done reaches N exactly; passes it; either error word with done < N; done
    frozen (at 0 from the first read, and at 7 after progress) for the most read-backs that keep the stalled turns within the limit --
    exactly stall_limit turns when G R divides it -- and one more; progress by one resets the count."""
    step, limit = G * R_, R.TURN_LIMIT + 64
    k = limit // step                                     # read-backs of a frozen counter that go on
    assert k * step <= limit < (k + 1) * step and ((R_, G) == (5, 3) or k * step == limit)
    return [[(0, 0, 0), (12, 0, 0), (39, 0, 0), (40, 0, 0)], [(39, 0, 0), (41, 0, 0)], [(5, 8, 0)], [(5, 0, 2)], [(0, 16, 4)],
            [(0, 0, 0)] * (k + 1), [(7, 0, 0)] * (k + 2), [(3, 0, 0)] + [(3, 0, 0)] * (k - 1) + [(4, 0, 0)] + [(4, 0, 0)] * (k + 1),
            [(9, 0, 0)] * (k + 1) + [(40, 0, 0)]], k


@pytest.mark.parametrize("M,plies,R_,G", PROGRESS_RUNS)
def test_progress_verdicts(driver, M, plies, R_, G):
    p = R.plan(req(P=1, T=40, M=M, plies=plies))
    assert (p["R"], p["G"], p["N"], p["stall_turns"], p["stall_limit"]) == (R_, G, 40, R_ * G, 100064)
    scripts, k = progress_scripts(R_, G)
    for reads in scripts:
        got = verdicts(driver, 40, M, plies, reads)
        assert got == R.progress(40, R_, G, reads), reads[:4]
    # ... and the verdicts in numbers
    assert verdicts(driver, 40, M, plies, scripts[0]) == [0, 0, 0, 1] and verdicts(driver, 40, M, plies, scripts[1]) == [0, 1]
    assert [verdicts(driver, 40, M, plies, s) for s in scripts[2:5]] == [[1], [1], [1]]
    assert verdicts(driver, 40, M, plies, scripts[5]) == [0] * k + [2]                    # frozen from the start: the first read counts
    assert verdicts(driver, 40, M, plies, scripts[6]) == [0] * (k + 1) + [2]              # the read that shows progress does not
    assert verdicts(driver, 40, M, plies, scripts[7]) == [0] * (2 * k + 1) + [2]          # progress by one resets the count
    assert verdicts(driver, 40, M, plies, scripts[8]) == [0] * (k + 1) + [1]                # one read short of stalling, then every trial done


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------

def test_rollout_plan_under_asan_ubsan(tmp_path, sweep, header_lines):
    """The plan and the loop's verdicts compiled with the sanitizers and run as their own program over the same sweep and scripts: the
    same lines, and no report."""
    exe = build_driver(tmp_path / "rollout_plan_driver_san", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    assert plans(exe, sweep, SAN_ENV) == header_lines
    assert plans(exe, [req(P=2 ** 31 - 1, T=2 ** 31 - 1, cube=1, w0=0)], SAN_ENV) == ["rc %d" % R.E_INVALID]
    for M, plies, R_, G in PROGRESS_RUNS:
        for reads in progress_scripts(R_, G)[0]:
            assert verdicts(exe, 40, M, plies, reads, SAN_ENV) == R.progress(40, R_, G, reads)
