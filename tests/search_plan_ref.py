"""An independent restatement of what a search call decides on the host, for tests/test_search_plan_cpu.py to hold
csrc/bg_search_plan.h against.  Written from the text of search_stages, search3_deep and the five entry points (bgamd_env_step_search,
_step_search_filtered, _step_search3, bgamd_env_analyze_moves, and the mid env's call inside search3_deep) as they stood in the commit
before the header existed -- their argument checks in their order, the four nullable pointers d_played / margin / deep / mid and the
combinations of them every stage tested, the locals n_cand, n_searched, K, n_virtual, the sizes passed to grow_candidates, scratch_env
and the alloc groups -- not from the header.  No device, no numpy: plain integers, margins as float32 bit patterns.

A request is the tuple (kind, flags, top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin, has_played, n, cap_rows, logs,
slog, w0, w1, kept_total, kept_max, searched_total) as the driver reads it; the last three are the words the call reads back.

The ONE defined deviation of the header from that code: it formed the candidate bound as (long long)(top_k + (d_played ? 1 : 0)), the addition in int,
so an analysis with top_k = INT_MAX was undefined behaviour there.  Here, as in the header, the sum is the mathematical one.

One deviation of the CALLERS, which no request can show: a turn of a 2-ply rollout's trial env called search_stages directly, without
bgamd_env_step_search_filtered's checks of top_k and margin; it is now a FILTERED request and passes them again.  bgamd_env_rollout_policy
has refused a negative top_k and a negative or NaN margin before, so no such turn exists.  A mid env's search (MID) is checked as little
as it was: search3_deep passed reply_top_k and reply_margin on as its step had checked them."""
import struct

STEP, FILTERED, THREE_PLY, MID, ANALYSIS = range(5)      # what the pointers said: none; margin; margin + deep; margin + mid; d_played
ROLL, AUTO_RESET, ONLY_P1, ONLY_P2, SLOT1 = 1, 2, 16, 32, 64        # include/bgamd.h
OK, E_INVALID, E_NOWEIGHTS = 0, -1, -6
INT_MAX = 2 ** 31 - 1
ROLLS = 21
CHUNK = 131072                                          # the search's scratch env: at most this many lanes
CHUNK3 = 65536                                          # the mid env: at most this many lanes
SEL_PLAIN, SEL_MARGIN, SEL_ANALYSIS = range(3)
FAN_PLAIN, FAN_MAPPED = range(2)
END_PLAIN, END_FILTERED, END_MID, END_ANALYSIS = range(4)
FIELDS = ("rc", "kind", "flags", "slot", "top_k", "k_lim", "margin", "select", "match_played", "pass_replies", "skip_singletons",
          "read_back", "read_searched", "k_known", "fanout", "ending", "logged", "min_searched", "deep", "deep_k_lim", "deep_margin",
          "reply_top_k", "reply_margin", "apply", "per_game_bytes", "per_row_bytes", "ana_word_bytes", "ana_state_bytes",
          "deep_game_bytes", "cand_presize", "n_cand", "n_searched", "K", "n_virtual", "cand_rows", "scratch_lanes", "passes")


def bits(x):
    """float -> its float32 bit pattern"""
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def bad_margin(b):
    """!(margin >= 0.0f): negative or NaN (-0.0 compares equal to 0 and passes)"""
    return not f32(b) >= 0.0


def refusal(q):
    """the code of a request that is refused before anything is issued, or OK: the entry point's own checks, then search_stages'"""
    kind, flags, top_k, margin, deep_k, deep_margin, reply_top_k, reply_margin, has_played, n, cap_rows, logs, slog, w0, w1 = q[:15]
    if kind == STEP and top_k < 0:
        return E_INVALID
    if kind == FILTERED and (top_k < 0 or bad_margin(margin)):
        return E_INVALID
    if kind == THREE_PLY:
        if top_k < 0 or deep_k < 0 or reply_top_k < 0 or bad_margin(margin) or bad_margin(deep_margin) or bad_margin(reply_margin):
            return E_INVALID
        if slog:
            return E_INVALID
    if kind == ANALYSIS and (not has_played or top_k < 0 or flags & ~(ONLY_P1 | ONLY_P2 | SLOT1)):
        return E_INVALID
    # (MID: search3_deep called search_stages with the reply_top_k and reply_margin its step had checked: no check of its own)
    if logs:
        return E_INVALID
    logged = slog and kind != ANALYSIS                  # env->slog.rows && !d_played
    if logged and flags & AUTO_RESET:
        return E_INVALID
    if not (w1 if flags & SLOT1 else w0):
        return E_NOWEIGHTS
    return OK


def floor_rows(need, floor_at_zero=False):
    """grow_candidates: at least 1 024 rows once there is one"""
    if floor_at_zero:                                   # (a deliberately wrong reference)
        return 1024 if need < 1024 else need
    return 1024 if 0 < need < 1024 else need


def scratch_lanes(n_virtual):
    return min(CHUNK, 256 * -(-n_virtual // 256))


def plan(q, mid_skips_singletons=False, floor_at_zero=False, analysis_plus_one=True):
    """-> {field: int} of an accepted request, {"rc": code} of a refused one.  The three keywords switch on the deliberately wrong
    references of test_a_wrong_reference_fails_the_comparison."""
    rc = refusal(q)
    if rc:
        return {"rc": rc}
    kind, flags, top_k, margin_bits, deep_k, deep_margin, reply_top_k, reply_margin, has_played, n, cap_rows, logs, slog, w0, w1, h0, h1, h2 = q
    d_played, margin, deep, mid = kind == ANALYSIS, kind in (FILTERED, THREE_PLY, MID), kind == THREE_PLY, kind == MID
    logged = bool(slog) and not d_played
    # bound on the kept candidates (top_k = 0: read back); the analysis keeps the played one beside the top_k
    n_cand = n * (top_k + (1 if d_played and analysis_plus_one else 0)) if top_k > 0 and not margin else 0
    presize = floor_rows(n_cand, floor_at_zero) if n_cand > 0 or floor_at_zero else 0
    K, n_searched = top_k, 0
    singletons_skipped = margin and (not mid or mid_skips_singletons)
    read_back = margin or top_k == 0
    cand_rows = presize
    if read_back:
        n_cand, n_searched = h0, (h2 if singletons_skipped else 0)
        if top_k == 0:
            K = h1
        cand_rows = floor_rows(n_cand, floor_at_zero)
    n_virtual = (n_searched if singletons_skipped else n_cand) * ROLLS
    lanes = scratch_lanes(n_virtual) if n_virtual > 0 else 0
    if d_played:
        ending = END_ANALYSIS
    elif mid:
        ending = END_MID
    else:
        ending = END_FILTERED if margin else END_PLAIN
    applies = ending in (END_PLAIN, END_FILTERED)
    return dict(rc=0, kind=kind, flags=flags, slot=int(bool(flags & SLOT1)), top_k=top_k, k_lim=top_k if top_k > 0 else 0xFFFFFFFF,
                margin=margin_bits if margin else 0, select=SEL_ANALYSIS if d_played else SEL_MARGIN if margin else SEL_PLAIN,
                match_played=int(d_played), pass_replies=int(mid), skip_singletons=int(singletons_skipped), read_back=int(read_back),
                read_searched=int(read_back and singletons_skipped), k_known=int(top_k != 0),      # (`int K = top_k; if (top_k == 0) K = h[1]`)
                fanout=FAN_MAPPED if singletons_skipped else FAN_PLAIN, ending=ending, logged=int(logged and applies),
                min_searched=2 if margin else 1, deep=int(deep), deep_k_lim=(deep_k if deep_k > 0 else 0xFFFFFFFF) if deep else 0,
                deep_margin=deep_margin if deep else 0, reply_top_k=reply_top_k if deep else 0, reply_margin=reply_margin if deep else 0,
                apply=int(applies), per_game_bytes=(n + 1) * 4, per_row_bytes=cap_rows * 4, ana_word_bytes=n * 4 if d_played else 0,
                ana_state_bytes=n * 32 if d_played else 0, deep_game_bytes=(n + 1) * 4 if deep else 0, cand_presize=presize,
                n_cand=n_cand, n_searched=n_searched, K=K, n_virtual=n_virtual, cand_rows=cand_rows, scratch_lanes=lanes,
                passes=-(-n_virtual // lanes) if lanes else 0)


def render(d):
    """a plan as the driver prints it"""
    return "rc %d" % d["rc"] if d["rc"] else " ".join("%s %d" % (k, d[k]) for k in FIELDS)


def chunk(text):
    """BGAMD_SEARCH3_CHUNK as search3_deep read it (text None: unset): atoll's value when it is at least 256 and a multiple of 256"""
    t = (text or "").lstrip(" \t\n\v\f\r")
    sign, digits = 1, ""
    if t[:1] in ("+", "-"):
        sign, t = (-1 if t[0] == "-" else 1), t[1:]
    for c in t:
        if not c.isdigit():
            break
        digits += c
    c = sign * int(digits or "0")
    return c if c >= 256 and c % 256 == 0 else CHUNK3


def deep(n_deep, chunk_lanes):
    """search3_deep after its read-back: (none, n_mid, mid lanes, chunks on a mid env of exactly that many lanes)"""
    if n_deep == 0:
        return dict(none=1, n_mid=0, mid_lanes=0, chunks=0)
    n_mid = n_deep * ROLLS
    want = 256 * -(-n_mid // 256) if n_mid < chunk_lanes else chunk_lanes
    return dict(none=0, n_mid=n_mid, mid_lanes=want, chunks=len(range(0, n_mid, want)))
