// bg_search_plan.h -- host-only part of the 2-ply search and what is built on it (bgamd_env_step_search, _step_search_filtered,
// _step_search3 and its mid env, bgamd_env_analyze_moves; include/bgamd.h): whether a call is refused and with which code, which select,
// fan-out and reduce launches it issues, whether it reads its list lengths back, how its buffers and its scratch envs are sized.  Plain
// C++ (no HIP), like bg_rollout_plan.h: bgamd.hip's SearchCall issues what a SearchPlan names, tests/test_search_plan_cpu.py holds it
// against an independent restatement without a GPU and runs it under AddressSanitizer + UBSan (tests/sanitize/search_plan_driver.cpp).
// The kernels: bg_search.h, bg_filter.h, bg_analysis.h, bg_search3.h, bg_search_log.h.
//
// This is the ONE place where the search's host rules and their constants live.
#pragma once
#include <cstdint>
#include <cstdlib>
#include "../../include/bgamd.h"         // the flags and the error codes

namespace bg {

constexpr int SEARCH_ROLLS = 21;         // opponent rolls per candidate: one virtual lane each (= SRCH_ROLLS, bg_search_order.h)

// ---- what the 2-ply search, the pre-roll evaluation and the rollouts share ----
// Virtual lanes per scoring pass: the search's scratch env has at most this many lanes (a 131 072-lane env: ~3.4 GB).  Every virtual
// lane is scored on its own, so no result depends on it.
constexpr long long SEARCH_CHUNK = 131072;
// the lanes env->scratch needs for n_virtual virtual lanes: rounded up to 256, at most SEARCH_CHUNK
inline long long search_lanes(long long n_virtual) { return n_virtual < SEARCH_CHUNK ? ((n_virtual + 255) / 256) * 256 : SEARCH_CHUNK; }

// Mid lanes per chunk: the 3-ply step's mid env has at most this many lanes (~1.8 GB at 65 536, its search buffers included).  A chunk
// costs ~1.5 ms beside its scoring passes (its launches and its one synchronisation): at 16 384 lanes per chunk a 16 384-lane step took
// 74 ms, at 65 536 it takes 49 ms (profiles/search3.txt).  Every mid lane is searched on its own, so no result depends on it.
constexpr long long SEARCH3_CHUNK = 65536;
// ... and the test hook BGAMD_SEARCH3_CHUNK (text: its value, NULL when unset): at least 256 and a multiple of 256, anything else is ignored
inline long long search3_chunk(const char *text)
{
    const long long c = text ? std::strtoll(text, nullptr, 10) : 0;
    return c >= 256 && c % 256 == 0 ? c : SEARCH3_CHUNK;
}

// The candidate buffers hold at least this many rows once they hold one: a small env's first steps do not re-create them list by list.
constexpr long long SEARCH_MIN_CAND_ROWS = 1024;
inline long long candidate_rows(long long need) { return need > 0 && need < SEARCH_MIN_CAND_ROWS ? SEARCH_MIN_CAND_ROWS : need; }

// What a call is.  STEP: bgamd_env_step_search.  FILTERED: bgamd_env_step_search_filtered, and a turn of a 2-ply rollout's trial env.
// THREE_PLY: bgamd_env_step_search3's root level.  MID: the search of that step's mid env, a chunk of mid lanes at a time.
// ANALYSIS: bgamd_env_analyze_moves.
enum class SearchKind { STEP, FILTERED, THREE_PLY, MID, ANALYSIS };

// the arguments of a call that decide anything, and what the env has been set to
struct SearchRequest {
    SearchKind kind;
    int flags;
    int top_k;
    float margin;                        // every kind but STEP and ANALYSIS
    int deep_k; float deep_margin;       // THREE_PLY
    int reply_top_k; float reply_margin; // THREE_PLY: top_k and margin of its MID searches
    bool has_played;                     // ANALYSIS: d_played28 given
    long long n, cap_rows;               // the env's lanes and the rows its arenas hold
    bool logs_steps;                     // a trajectory or ring log is set
    bool has_search_log;                 // bgamd_env_set_search_log
    bool has_weights[2];                 // the env's two weight slots
};

enum class SearchSelect { PLAIN, MARGIN, ANALYSIS };    // srch_select_kernel, flt_select_kernel, ana_select_kernel
enum class SearchFanout { PLAIN, MAPPED };              // srch_fanout_kernel over the candidate list, flt_fanout_kernel over the searched list
enum class SearchEnding { PLAIN, FILTERED, MID, ANALYSIS };

struct SearchPlan {
    int rc;                              // BGAMD_OK, or the code the call returns before anything is issued: nothing below is set then
    SearchKind kind;
    int flags, slot;                     // as given, and the weight slot
    int top_k;
    uint32_t k_lim;                      // candidates a lane keeps at most (top_k = 0: no limit)
    float margin;                        // select == MARGIN
    SearchSelect select;
    bool match_played;                   // ANALYSIS: the played row is matched first and forced into the kept set
    bool pass_replies;                   // MID: a mid lane without rows keeps its pass reply, and the pass replies are emitted
    bool skip_singletons;                // no virtual root for a lane that keeps one candidate: the searched list is scanned and mapped
    // The list's length is not known before the launches (the margin rule, or every distinct afterstate): it is read back, with the
    // searched list's when singletons are skipped -- the call's one synchronisation.  k_known (top_k != 0): K is top_k, else the longest list read back
    bool read_back, read_searched, k_known;
    SearchFanout fanout;
    SearchEnding ending;
    bool logged;                         // the step writes its ply into the search log ...
    uint32_t min_searched;               // ... a lane counts as searched from this many kept candidates on (also bgamd_env_search_info)
    bool deep;                           // THREE_PLY: the deep level runs between the reduce and the apply
    uint32_t deep_k_lim; float deep_margin; int reply_top_k; float reply_margin;     // deep
    bool apply;                          // the greedy step's apply launch ends the call, and the env remembers the step
    // bytes of a buffer of each group: per game (n + 1 words), per arena row, the analysis' per-lane words and afterstates, the deep
    // level's per-game words (0: the kind has no such group)
    long long per_game_bytes, per_row_bytes, ana_word_bytes, ana_state_bytes, deep_game_bytes;
    long long cand_presize;              // candidate rows the buffers hold before anything is launched (0: sized after the read-back)
    long long n;
};

inline SearchPlan search_plan(const SearchRequest &q)
{
    SearchPlan p{};
    const bool analysis = q.kind == SearchKind::ANALYSIS, three = q.kind == SearchKind::THREE_PLY, mid = q.kind == SearchKind::MID;
    const bool by_margin = !analysis && q.kind != SearchKind::STEP;
    p.rc = BGAMD_E_INVALID;
    // the entry point's own checks (a NaN margin fails its comparison).  MID has no entry point: the 3-ply step that issues it has
    // checked reply_top_k and reply_margin, and nothing is checked again
    if (!mid && (q.top_k < 0 || (by_margin && !(q.margin >= 0.0f)))) return p;
    if (three && (q.deep_k < 0 || q.reply_top_k < 0 || !(q.deep_margin >= 0.0f) || !(q.reply_margin >= 0.0f))) return p;
    if (three && q.has_search_log) return p;             // 3-ply targets are not logged: refused, not written half-right
    if (analysis && (!q.has_played || (q.flags & ~(BGAMD_ONLY_P1 | BGAMD_ONLY_P2 | BGAMD_WEIGHTS_SLOT1)))) return p;
    // a search step logs nothing into a trajectory or a ring: refused rather than a hole in a log.  Its own log is written by the search
    // step alone -- the analysis applies nothing and ignores it -- and with auto-reset a lane's next game would write over its last one.
    if (q.logs_steps) return p;
    const bool logged = q.has_search_log && !analysis;
    if (logged && (q.flags & BGAMD_AUTO_RESET)) return p;
    const int slot = (q.flags & BGAMD_WEIGHTS_SLOT1) ? 1 : 0;
    if (!q.has_weights[slot]) { p.rc = BGAMD_E_NOWEIGHTS; return p; }
    p.rc = BGAMD_OK;

    p.kind = q.kind; p.flags = q.flags; p.slot = slot; p.top_k = q.top_k; p.n = q.n;
    p.k_lim = q.top_k > 0 ? (uint32_t)q.top_k : 0xFFFFFFFFu;
    p.select = analysis ? SearchSelect::ANALYSIS : by_margin ? SearchSelect::MARGIN : SearchSelect::PLAIN;
    p.margin = by_margin ? q.margin : 0.0f;
    p.match_played = analysis;
    p.pass_replies = mid;
    p.skip_singletons = by_margin && !mid;               // (the mid env searches every kept reply: its searched list is its candidate list)
    p.read_back = by_margin || q.top_k == 0;
    p.read_searched = p.read_back && p.skip_singletons;
    p.k_known = q.top_k != 0;
    p.fanout = p.skip_singletons ? SearchFanout::MAPPED : SearchFanout::PLAIN;
    p.ending = analysis ? SearchEnding::ANALYSIS : mid ? SearchEnding::MID : by_margin ? SearchEnding::FILTERED : SearchEnding::PLAIN;
    p.apply = !analysis && !mid;
    p.logged = logged && p.apply;
    p.min_searched = by_margin ? 2u : 1u;
    p.deep = three;
    if (three) {
        p.deep_k_lim = q.deep_k > 0 ? (uint32_t)q.deep_k : 0xFFFFFFFFu;
        p.deep_margin = q.deep_margin; p.reply_top_k = q.reply_top_k; p.reply_margin = q.reply_margin;
    }
    p.per_game_bytes = (q.n + 1) * 4;
    p.per_row_bytes = q.cap_rows * 4;
    if (analysis) { p.ana_word_bytes = q.n * 4; p.ana_state_bytes = q.n * 32; }
    if (three) p.deep_game_bytes = (q.n + 1) * 4;
    // bound on the kept candidates when it is known here; the analysis keeps the played one beside the top_k (in long long: top_k may be INT_MAX)
    p.cand_presize = p.read_back ? 0 : candidate_rows(q.n * ((long long)q.top_k + (analysis ? 1 : 0)));
    return p;
}

// What is known after the read-back of (candidates kept in all, the longest kept list, candidates of the lanes that kept two or more) --
// or, for a plan that reads nothing back, before the first launch (the three arguments are not looked at then).  The call asks once its
// candidate buffers hold cand_presize rows, so n_cand is a row count that fits device memory and n_cand x 21 is far from overflowing.
struct SearchSized {
    long long n_cand, n_searched;        // rows of the candidate list (no read-back: its bound), and of the searched list
    int K;                               // the longest kept list, at most (bgamd_env_search_read's row stride)
    long long n_virtual;                 // virtual lanes: one per (searched candidate, opponent roll)
    long long cand_rows;                 // the candidate buffers hold at least this many rows
    long long scratch_lanes;             // lanes env->scratch has at least (0: nothing is scored, the scratch env is not touched)
    long long passes;                    // scoring passes on a scratch env of exactly that many lanes (a larger one at hand: fewer)
};

inline SearchSized search_sized(const SearchPlan &p, long long kept_total, long long kept_max, long long searched_total)
{
    SearchSized z{};
    z.n_cand = p.read_back ? kept_total : p.n * ((long long)p.top_k + (p.match_played ? 1 : 0));
    z.n_searched = p.read_searched ? searched_total : 0;
    z.K = p.k_known ? p.top_k : (int)kept_max;
    z.n_virtual = (p.skip_singletons ? z.n_searched : z.n_cand) * SEARCH_ROLLS;
    z.cand_rows = candidate_rows(z.n_cand);
    z.scratch_lanes = z.n_virtual > 0 ? search_lanes(z.n_virtual) : 0;
    z.passes = z.n_virtual > 0 ? (z.n_virtual + z.scratch_lanes - 1) / z.scratch_lanes : 0;
    return z;
}

// The 3-ply step's deep level, once the deep list's length n_deep has been read back; chunk: search3_chunk of the env's first such step
struct DeepPlan {
    bool none;                           // no lane is searched deeper: the filtered step's choices stand, nothing below is set
    long long n_mid;                     // mid lanes: one per (deep candidate, opponent roll)
    long long mid_lanes;                 // lanes env->mid has at least: n_mid rounded up to 256, at most the chunk
    long long chunks;                    // searches of a mid env of exactly that many lanes (a larger one at hand: fewer)
};

inline DeepPlan deep_plan(long long n_deep, long long chunk)
{
    DeepPlan d{};
    d.none = n_deep == 0;
    if (d.none) return d;
    d.n_mid = n_deep * SEARCH_ROLLS;
    d.mid_lanes = d.n_mid < chunk ? ((d.n_mid + 255) / 256) * 256 : chunk;
    d.chunks = (d.n_mid + d.mid_lanes - 1) / d.mid_lanes;
    return d;
}

}  // namespace bg
