"""The search's plan (csrc/bg_search_plan.h) without a GPU: the header, compiled into tests/sanitize/search_plan_driver.cpp, against the
independent restatement of search_stages, search3_deep and the entry points it replaced (tests/search_plan_ref.py), field by field over
every edge of its rules; every refusal and their precedence; three deliberately wrong references that the comparison must catch; the
BGAMD_SEARCH3_CHUNK rule and the deep level's sizes; and the same sweep once more through a driver built with AddressSanitizer + UBSan
(its own program: nothing is preloaded)."""
import itertools
import os
import shutil
import subprocess

import pytest

import search_lanes as SL
import search_plan_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
KINDS = (R.STEP, R.FILTERED, R.THREE_PLY, R.MID, R.ANALYSIS)
STEP_BITS = (R.ROLL, R.AUTO_RESET, R.ONLY_P1, R.ONLY_P2, R.SLOT1)
ALL_FLAGS = [sum(c) for k in range(len(STEP_BITS) + 1) for c in itertools.combinations(STEP_BITS, k)]       # the 32 a step takes
UNKNOWN = 1 << 20                                       # no flag of include/bgamd.h
TOP_KS = (0, 1, 5, R.INT_MAX - 1, R.INT_MAX)
B = R.bits
NAN, NEG_NAN, INF, NEG_INF, NEG_ZERO, DENORMAL, NEG_DENORMAL = 0x7FC00000, 0xFFC00000, B(float("inf")), B(float("-inf")), 0x80000000, 1, 0x80000001
MARGINS = (0, NEG_ZERO, B(0.04), INF, DENORMAL, NAN, NEG_NAN, NEG_INF, NEG_DENORMAL, B(-1.0))       # the first five pass
SIZES = ((1, 64), (256, 256 * 40), (65536, 65536 * 40), (2 ** 20, 2 ** 20 * 40))                # (n, cap_rows)
CHUNK_TEXTS = ("", "0", "255", "256", "257", "512", "x", "-256", None, "65536", " 768", "1024x", "+256")


def req(kind=R.STEP, flags=0, top_k=5, margin=B(0.04), deep_k=2, deep_margin=B(0.02), reply_top_k=3, reply_margin=B(0.04), played=None,
        n=256, cap_rows=10240, logs=0, slog=0, w0=1, w1=1, h=(0, 0, 0)):
    return (kind, flags, top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin, int(kind == R.ANALYSIS if played is None else played),
            n, cap_rows, logs, slog, w0, w1, *h)


def build_driver(out, flags=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "backgammon-engine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sanitize", "search_plan_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("search_plan") / "search_plan_driver")


def run(exe, mode, lines_in, extra_env=None):
    r = subprocess.run([exe, mode], env={**os.environ, **(extra_env or {})}, input="".join(lines_in), capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(lines_in)
    return lines


def plans(exe, requests, extra_env=None):
    return run(exe, "plan", [" ".join(map(str, q)) + "\n" for q in requests], extra_env)


def chunks(exe, texts, extra_env=None):
    return [int(x) for x in run(exe, "chunk", ["unset\n" if t is None else "|%s|\n" % t for t in texts], extra_env)]


def deeps(exe, pairs, extra_env=None):
    return run(exe, "deep", ["%d %d\n" % p for p in pairs], extra_env)


def parse(line):
    w = line.split()
    return dict(zip(w[0::2], map(int, w[1::2])))


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

def list_totals():
    """List lengths T on both sides of the 1 024-row floor, of every multiple of 256 virtual lanes (T 21) from 256 x 470 to SEARCH_CHUNK,
    and of SEARCH_CHUNK itself in rows; and around two and three passes"""
    edges = {0, 1, 2, 1023, 1024, 1025, SL.SEARCH_CHUNK - 1, SL.SEARCH_CHUNK, SL.SEARCH_CHUNK + 1}
    for k in range(470, 513):
        edges |= {256 * k // 21, 256 * k // 21 + 1}
    for passes in (2, 3):
        edges |= {passes * SL.SEARCH_CHUNK // 21, passes * SL.SEARCH_CHUNK // 21 + 1}
    return sorted(edges)


def read_backs():
    """(kept in all, the longest list, searched in all): every total as the candidate list's length and as the searched list's"""
    return [(T, kmax, S) for T in list_totals() for kmax in (1, 7) for S in sorted({0, T // 2, T})]


def requests():
    """Every request of the sweep, once.  Section by section, each the full product of the fields one group of rules reads:
      a) kind x top_k x (n, cap_rows) x the read-back words: the select / fan-out / ending rule, k_lim, k_known, the read-back, every byte
         size, the pre-size with its floor, n_cand, n_searched, K, n_virtual, the grown rows, the scratch env's lanes, the passes;
      b) 2^30 lanes (the most an env has) at small top_k;
      c) kind x the 32 flag combinations and an unknown bit x trajectory / ring x search log x the weight slots' four states x played
         states given or not x top_k in {-1, 5} x a good and a NaN margin: every refusal and the logged rule;
      d) kind x each of the three margins over ten bit patterns x deep_k and reply_top_k in {-1, 0, 2}."""
    H = read_backs()
    out = [req(kind, 0, k, n=n, cap_rows=cap, h=h) for kind in KINDS for k in TOP_KS for n, cap in SIZES for h in H]
    out += [req(kind, R.SLOT1, k, n=2 ** 30, cap_rows=2 ** 34, h=h) for kind in KINDS for k in (0, 1, 5) for h in H[::7]]
    out += [req(kind, f, k, m, played=pl, logs=logs, slog=slog, w0=w0, w1=w1, h=(700, 4, 650))
            for kind in KINDS for f in ALL_FLAGS + [UNKNOWN, UNKNOWN | R.SLOT1] for logs in (0, 1) for slog in (0, 1) for w0 in (0, 1)
            for w1 in (0, 1) for pl in (0, 1) for k in (-1, 5) for m in (B(0.04), NAN)]
    for kind in KINDS:
        for dk, rk in itertools.product((-1, 0, 2), repeat=2):
            for m in MARGINS:
                out += [req(kind, 0, 5, m, dk, B(0.02), rk, B(0.04), h=(700, 4, 650)), req(kind, 0, 5, B(0.04), dk, m, rk, B(0.04), h=(700, 4, 650)),
                        req(kind, 0, 5, B(0.04), dk, B(0.02), rk, m, h=(700, 4, 650))]
    return list(dict.fromkeys(out))


@pytest.fixture(scope="module")
def sweep():
    return requests()


@pytest.fixture(scope="module")
def header_lines(driver, sweep):
    return plans(driver, sweep)


def test_plan_is_the_code_it_replaced(sweep, header_lines):
    """Every field of every plan equals what the parent commit's search_stages and entry points decided inline, and every refused
    request gets the parent's code."""
    n_refused = 0
    for q, line in zip(sweep, header_lines):
        want = R.render(R.plan(q))
        if line != want:                                  # field by field: the fields that differ
            raise AssertionError((q, sorted(set(parse(line).items()) ^ set(parse(want).items())), line, want))
        n_refused += len(line.split()) == 2
    print("%d plans compared, %d of them refusals" % (len(sweep), n_refused))
    assert len(sweep) > 60000 and 0.1 < n_refused / len(sweep) < 0.4


def test_sweep_covers_the_rules(sweep):
    """what the issue names, counted on the reference alone"""
    ps = [R.plan(q) for q in sweep]
    ok = [p for p in ps if p["rc"] == 0]
    refused = sum(p["rc"] != 0 for p in ps)
    assert 0.1 < refused / len(ps) < 0.4
    assert {p["rc"] for p in ps} == {R.OK, R.E_INVALID, R.E_NOWEIGHTS}
    assert {p["kind"] for p in ok} == set(KINDS) and {p["ending"] for p in ok} == {R.END_PLAIN, R.END_FILTERED, R.END_MID, R.END_ANALYSIS}
    assert {p["select"] for p in ok} == {R.SEL_PLAIN, R.SEL_MARGIN, R.SEL_ANALYSIS} and {p["fanout"] for p in ok} == {R.FAN_PLAIN, R.FAN_MAPPED}
    for kind in KINDS:
        mine = [p for p in ok if p["kind"] == kind]
        assert {p["top_k"] for p in mine} >= set(TOP_KS)
        assert {p["read_back"] for p in mine} == ({0, 1} if kind in (R.STEP, R.ANALYSIS) else {1})
        assert {p["per_game_bytes"] for p in mine} >= {8, 1028, 2 ** 32 + 4}
        # the floor, every multiple of 256 below SEARCH_CHUNK with both sides, SEARCH_CHUNK itself, one pass and several
        read = [p for p in mine if p["read_back"]]
        assert {p["cand_rows"] for p in read} >= {0, 1024, 1025} and any(p["n_cand"] == 1023 and p["cand_rows"] == 1024 for p in read)
        assert {p["scratch_lanes"] for p in read} >= {0, 256} | {256 * k for k in range(471, 513)}
        assert {p["passes"] for p in read} >= {0, 1, 2, 3, 4}
        for edge in (SL.SEARCH_CHUNK,):
            assert any(p["n_virtual"] < edge <= p["n_virtual"] + 21 for p in read) and any(edge <= p["n_virtual"] < edge + 21 for p in read)
    assert {(p["kind"], p["logged"]) for p in ok} >= {(R.STEP, 1), (R.FILTERED, 1), (R.STEP, 0), (R.FILTERED, 0)}
    assert not any(p["logged"] for p in ok if p["kind"] in (R.THREE_PLY, R.MID, R.ANALYSIS))
    assert {(p["kind"], p["min_searched"]) for p in ok} == {(R.STEP, 1), (R.ANALYSIS, 1), (R.FILTERED, 2), (R.THREE_PLY, 2), (R.MID, 2)}
    assert {p["flags"] for p in ok if p["kind"] == R.STEP} == set(ALL_FLAGS) | {UNKNOWN, UNKNOWN | R.SLOT1}      # (a step takes any bit)
    assert {p["flags"] for p in ok if p["kind"] == R.ANALYSIS} == {f for f in ALL_FLAGS if not f & (R.ROLL | R.AUTO_RESET)}
    assert {p["margin"] for p in ok if p["kind"] == R.FILTERED} == set(MARGINS[:5])
    assert {p["deep_margin"] for p in ok if p["deep"]} == set(MARGINS[:5]) | {B(0.02)} and {p["reply_margin"] for p in ok if p["deep"]} == set(MARGINS[:5])
    assert {p["deep_k_lim"] for p in ok if p["deep"]} == {2, 0xFFFFFFFF} and {p["reply_top_k"] for p in ok if p["deep"]} == {0, 2, 3}
    # the analysis' bound with the played candidate beside top_k = INT_MAX: 2^31 per lane, which the replaced code could not form
    assert any(p["kind"] == R.ANALYSIS and p["top_k"] == R.INT_MAX and p["n_cand"] == 2 ** 31 * 256 for p in ok)
    assert any(p["kind"] == R.ANALYSIS and p["cand_presize"] == 1024 and p["n_cand"] == 2 for p in ok)             # one lane, top_k 1


def test_reference_agrees_with_the_rule_the_gpu_tests_use(sweep):
    assert R.CHUNK == SL.SEARCH_CHUNK
    for q in sweep[::97]:
        p = R.plan(q)
        if p["rc"] == 0 and p["n_virtual"]:
            assert p["scratch_lanes"] == min(SL.SEARCH_CHUNK, -(-p["n_virtual"] // 256) * 256)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

# in the order the code looks at them: the entry point's own checks, the trajectory / ring, logged + auto-reset, the weights
REFUSED = [("step: top_k < 0", dict(kind=R.STEP, top_k=-1), R.E_INVALID),
           ("filtered: top_k < 0", dict(kind=R.FILTERED, top_k=-1), R.E_INVALID),
           ("filtered: negative margin", dict(kind=R.FILTERED, margin=B(-1e-30)), R.E_INVALID),
           ("filtered: NaN margin", dict(kind=R.FILTERED, margin=NAN), R.E_INVALID),
           ("3-ply: top_k < 0", dict(kind=R.THREE_PLY, top_k=-1), R.E_INVALID),
           ("3-ply: deep_k < 0", dict(kind=R.THREE_PLY, deep_k=-1), R.E_INVALID),
           ("3-ply: reply_top_k < 0", dict(kind=R.THREE_PLY, reply_top_k=-1), R.E_INVALID),
           ("3-ply: negative margin", dict(kind=R.THREE_PLY, margin=NEG_DENORMAL), R.E_INVALID),
           ("3-ply: NaN margin", dict(kind=R.THREE_PLY, margin=NEG_NAN), R.E_INVALID),
           ("3-ply: negative deep margin", dict(kind=R.THREE_PLY, deep_margin=NEG_INF), R.E_INVALID),
           ("3-ply: NaN deep margin", dict(kind=R.THREE_PLY, deep_margin=NAN), R.E_INVALID),
           ("3-ply: negative reply margin", dict(kind=R.THREE_PLY, reply_margin=B(-0.5)), R.E_INVALID),
           ("3-ply: NaN reply margin", dict(kind=R.THREE_PLY, reply_margin=NAN), R.E_INVALID),
           ("3-ply: a search log is set", dict(kind=R.THREE_PLY, slog=1), R.E_INVALID),
           ("analysis: no played states", dict(kind=R.ANALYSIS, played=0), R.E_INVALID),
           ("analysis: top_k < 0", dict(kind=R.ANALYSIS, top_k=-1), R.E_INVALID),
           ("analysis: auto-reset", dict(kind=R.ANALYSIS, flags=R.AUTO_RESET), R.E_INVALID),
           ("analysis: roll", dict(kind=R.ANALYSIS, flags=R.ROLL | R.SLOT1), R.E_INVALID),
           ("analysis: unknown flag", dict(kind=R.ANALYSIS, flags=UNKNOWN), R.E_INVALID)]
for _k, _name in ((R.STEP, "step"), (R.FILTERED, "filtered"), (R.THREE_PLY, "3-ply"), (R.MID, "mid"), (R.ANALYSIS, "analysis")):
    REFUSED.append((_name + ": trajectory or ring", dict(kind=_k, logs=1), R.E_INVALID))
    if _k in (R.STEP, R.FILTERED, R.MID):
        REFUSED.append((_name + ": logged with auto-reset", dict(kind=_k, slog=1, flags=R.AUTO_RESET), R.E_INVALID))
    REFUSED += [(_name + ": slot 0 empty", dict(kind=_k, w0=0), R.E_NOWEIGHTS), (_name + ": slot 1 empty", dict(kind=_k, flags=R.SLOT1, w1=0), R.E_NOWEIGHTS)]
ACCEPTED = [dict(kind=R.STEP, top_k=0), dict(kind=R.STEP, top_k=R.INT_MAX), dict(kind=R.FILTERED, top_k=0, margin=0), dict(kind=R.FILTERED, margin=NEG_ZERO),
            dict(kind=R.FILTERED, margin=INF), dict(kind=R.FILTERED, margin=DENORMAL), dict(kind=R.THREE_PLY, top_k=0, deep_k=0, reply_top_k=0),
            dict(kind=R.THREE_PLY, margin=NEG_ZERO, deep_margin=INF, reply_margin=DENORMAL), dict(kind=R.THREE_PLY, flags=R.AUTO_RESET | R.ROLL),
            dict(kind=R.ANALYSIS, top_k=0), dict(kind=R.ANALYSIS, top_k=R.INT_MAX), dict(kind=R.ANALYSIS, flags=R.ONLY_P1 | R.ONLY_P2 | R.SLOT1),
            dict(kind=R.ANALYSIS, slog=1), dict(kind=R.ANALYSIS, margin=NAN), dict(kind=R.STEP, margin=NAN, deep_k=-1, reply_top_k=-1),
            dict(kind=R.STEP, slog=1), dict(kind=R.FILTERED, slog=1, flags=R.ROLL), dict(kind=R.STEP, flags=R.AUTO_RESET), dict(kind=R.STEP, w1=0),
            dict(kind=R.FILTERED, flags=R.SLOT1, w0=0), dict(kind=R.MID, flags=R.SLOT1, w0=0), dict(kind=R.STEP, flags=UNKNOWN)]


def test_refusals_and_their_precedence(driver):
    """every rule alone; an accepted neighbour of each; and of two broken rules of one kind the earlier one's code: the only pairs with
    different codes are (anything, an empty weight slot), and the weights are looked at last"""
    lines = plans(driver, [req(**kw) for _, kw, _ in REFUSED])
    for (name, kw, code), line in zip(REFUSED, lines):
        assert line == "rc %d" % code == R.render(R.plan(req(**kw))), name
    for kw, line in zip(ACCEPTED, plans(driver, [req(**kw) for kw in ACCEPTED])):
        assert line.startswith("rc 0 ") and line == R.render(R.plan(req(**kw))), kw
    pairs = [(a + " + " + b, {**kb, **ka}, ca) for (a, ka, ca), (b, kb, cb) in itertools.combinations(REFUSED, 2) if ka["kind"] == kb["kind"]]
    pairs += [(a + " + both slots empty", {**ka, "w0": 0, "w1": 0}, ca) for a, ka, ca in REFUSED]
    assert len(pairs) > 150 and any(ca != cb for (_, _, ca), (_, _, cb) in itertools.combinations(REFUSED, 2))
    for (name, kw, code), line in zip(pairs, plans(driver, [req(**kw) for _, kw, _ in pairs])):
        assert line == "rc %d" % code == R.render(R.plan(req(**kw))), name


# ---- the comparison can tell ----------------------------------------------------------------------------------------------------------

SIZED = {"n_cand", "n_searched", "n_virtual", "cand_rows", "scratch_lanes", "passes"}


@pytest.mark.parametrize("wrong,fields,derived", [
    (dict(mid_skips_singletons=True), {"skip_singletons"}, {"read_searched", "fanout"} | SIZED),
    (dict(floor_at_zero=True), {"cand_rows"}, {"cand_presize"}),
    (dict(analysis_plus_one=False), {"cand_presize"}, SIZED)])
def test_a_wrong_reference_fails_the_comparison(sweep, header_lines, wrong, fields, derived):
    """Singletons skipped in the mid env too, the 1 024-row floor applied to an empty list, the analysis' played candidate left out of
    its bound: each differs from the header somewhere in the sweep, in its own field (and in what is computed from that field)."""
    differing, kinds = set(), set()
    for q, line in zip(sweep, header_lines):
        want = R.render(R.plan(q, **wrong))
        if line != want:
            got, ref = parse(line), parse(want)
            differing |= {k for k in got if got[k] != ref[k]}
            kinds.add(q[0])
    assert fields <= differing <= fields | derived, differing
    assert "mid_skips_singletons" not in wrong or kinds == {R.MID}
    assert "analysis_plus_one" not in wrong or kinds == {R.ANALYSIS}


# ---- the chunk hook and the deep level ---------------------------------------------------------------------------------------------------

def deep_cases():
    """n_deep that put n_deep 21 on both sides of SEARCH3_CHUNK, of a 256 and a 512 override and of their multiples, and none at all"""
    ns = {0, 1, 2, 12, 13, 24, 25, 36, 37, 48, 49, 3120, 3121, 3122, 6241, 6242, 9362, 9363, 100000}
    return [(n, c) for n in sorted(ns) for c in (R.CHUNK3, 256, 512, 768)]


def test_chunk_hook_and_deep_level(driver):
    got = chunks(driver, CHUNK_TEXTS)
    assert got == [R.chunk(t) for t in CHUNK_TEXTS]
    assert dict(zip(CHUNK_TEXTS, got)) == {"": 65536, "0": 65536, "255": 65536, "256": 256, "257": 65536, "512": 512, "x": 65536, "-256": 65536,
                                           None: 65536, "65536": 65536, " 768": 768, "1024x": 1024, "+256": 256}
    cases = deep_cases()
    want = [R.deep(n, c) for n, c in cases]
    assert deeps(driver, cases) == ["none %(none)d n_mid %(n_mid)d mid_lanes %(mid_lanes)d chunks %(chunks)d" % d for d in want]
    assert {d["none"] for d in want} == {0, 1} and {d["chunks"] for d in want} >= {0, 1, 2, 3, 4}
    for chunk in (R.CHUNK3, 256, 512):
        mine = [d for (n, c), d in zip(cases, want) if c == chunk and not d["none"]]
        assert any(d["n_mid"] < chunk and d["mid_lanes"] <= chunk for d in mine) and any(d["n_mid"] > chunk and d["mid_lanes"] == chunk for d in mine)
        assert any(chunk - 21 < d["n_mid"] < chunk for d in mine) and any(chunk < d["n_mid"] <= chunk + 21 for d in mine)


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------

def test_search_plan_under_asan_ubsan(tmp_path, sweep, header_lines):
    """The plan, the sizes, the chunk rule and the deep level compiled with the sanitizers and run as their own program over the same
    sweep: the same lines, and no report -- the analysis with top_k = INT_MAX among them."""
    exe = build_driver(tmp_path / "search_plan_driver_san", ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    assert plans(exe, sweep, SAN_ENV) == header_lines
    int_max = req(R.ANALYSIS, 0, R.INT_MAX, n=65536, cap_rows=65536 * 40)
    line, = plans(exe, [int_max], SAN_ENV)
    assert parse(line)["cand_presize"] == 65536 * 2 ** 31 == R.plan(int_max)["cand_presize"]
    assert chunks(exe, CHUNK_TEXTS + ("99999999999999999999999", "-99999999999999999999999"), SAN_ENV)[:len(CHUNK_TEXTS)] == [R.chunk(t) for t in CHUNK_TEXTS]
    cases = deep_cases()
    assert deeps(exe, cases, SAN_ENV) == ["none %(none)d n_mid %(n_mid)d mid_lanes %(mid_lanes)d chunks %(chunks)d" % R.deep(n, c) for n, c in cases]
