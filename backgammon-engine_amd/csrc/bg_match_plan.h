// bg_match_plan.h -- host-only part of match play on the cubeful rollouts (bgamd_env_rollout_match, include/bgamd.h; the rule is restated
// in bg_match.h): whether a setting is refused and why, the threshold table that is computed once per setting and uploaded beside the
// match equity table, whether a rollout call is refused under a match, and the sizes of the new buffers.  Plain C++ (no HIP), like
// bg_rollout_plan.h: bgamd.hip issues what it names, tests/test_match_model_cpu.py holds the table against tests/match_model.py bit
// for bit without a GPU and runs it under AddressSanitizer + UBSan (tests/sanitize/match_plan_driver.cpp).
//
// Every fp64 operation below is rounded on its own: no contraction into a fused multiply-add, so that a Python float model is exact.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/bgamd.h"         // the flags and the error codes

#if defined(__clang__)
#define BG_MATCH_EXACT
#define BG_MATCH_EXACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define BG_MATCH_EXACT __attribute__((optimize("fp-contract=off")))
#define BG_MATCH_EXACT_BODY
#else
#define BG_MATCH_EXACT
#define BG_MATCH_EXACT_BODY
#endif

namespace bg {
namespace match {

constexpr int MAX_POINTS = 64;                         // the largest table: M x M
enum { NORMAL = 0, CRAWFORD = 1, POST_CRAWFORD = 2 };  // state[p]

// cube levels of the threshold table: the cubes 2^l < M, the only ones that are alive for a roller needing at most M (ceil(log2 M))
inline int levels(int M)
{
    int l = 0;
    while ((1ll << l) < M) ++l;
    return l;
}

// why a setting is refused, in the order the rules are looked at (every one returns BGAMD_E_INVALID)
enum Refusal { SET_OK = 0, SET_FLAGS = 1, SET_SIZE = 2, SET_NO_TABLE = 3, SET_ENTRY = 4, SET_WINDOW = 5 };

inline Refusal check_setting(int match_flags, long long M, const double *met, const double *met_pc, double window_share)
{
    if (match_flags & ~BGAMD_MATCH_ON) return SET_FLAGS;
    if (M < 1 || M > MAX_POINTS) return SET_SIZE;
    if (!met || !met_pc) return SET_NO_TABLE;
    auto in01 = [](double x) { return x >= 0.0 && x <= 1.0; };     // (false for a NaN; an infinity is outside)
    for (long long i = 0; i < M * M; ++i) if (!in01(met[i])) return SET_ENTRY;
    for (long long i = 0; i < M; ++i) if (!in01(met_pc[i])) return SET_ENTRY;
    if (!in01(window_share)) return SET_WINDOW;
    return SET_OK;
}

// why a rollout call is refused while a match is set (BGAMD_E_INVALID before anything is played).  The last already follows from the cube.
enum CallRefusal { CALL_OK = 0, CALL_NO_CUBE = 1, CALL_JACOBY = 2, CALL_NO_VR = 3 };

inline CallRefusal check_call(bool match_on, int cube_flags, int rollout_flags)
{
    if (!match_on) return CALL_OK;
    if (!(cube_flags & BGAMD_CUBE_ON)) return CALL_NO_CUBE;
    if (cube_flags & BGAMD_CUBE_JACOBY) return CALL_JACOBY;
    if (!(rollout_flags & BGAMD_ROLLOUT_VR)) return CALL_NO_VR;
    return CALL_OK;
}

// after(a1, a2, state): the MWC of the side that needs a1 when the next game starts against a side that needs a2 (include/bgamd.h)
inline double after(long long a1, long long a2, int state, int M, const double *met, const double *met_pc)
{
    if (a1 <= 0) return 1.0;
    if (a2 <= 0) return 0.0;
    if (state != NORMAL && a2 == 1) return met_pc[a1 - 1];
    if (state != NORMAL && a1 == 1) return 1.0 - met_pc[a2 - 1];
    return met[(a1 - 1) * M + (a2 - 1)];
}

// {double_at, pass_at} of a roller that needs a against a side that needs b, cube c, state NORMAL or POST_CRAWFORD.  The roller reads the
// table from its own row, whichever seat it has.  A denominator <= 0 or a result that is not finite: no decision, {+inf, +inf}.
BG_MATCH_EXACT inline void thresholds(int state, long long c, int a, int b, int M, const double *met, const double *met_pc, double window_share,
                                      double out[2])
{
    BG_MATCH_EXACT_BODY
    const double inf = std::numeric_limits<double>::infinity();
    const double W1 = after(a - c, b, state, M, met, met_pc), L1 = after(a, b - c, state, M, met, met_pc);
    const double W2 = after(a - 2 * c, b, state, M, met, met_pc), L2 = after(a, b - 2 * c, state, M, met, met_pc);
    out[0] = out[1] = inf;
    const double d1 = W2 - L2;
    const double n2 = L1 - L2;
    const double g2 = W2 - W1;
    const double d2 = n2 + g2;
    if (!(d1 > 0.0) || !(d2 > 0.0)) return;
    const double n1 = W1 - L2;
    const double pass_at = n1 / d1;
    const double open = n2 / d2;
    const double span = pass_at - open;
    const double part = window_share * span;
    const double double_at = open + part;
    if (!std::isfinite(pass_at) || !std::isfinite(open) || !std::isfinite(double_at)) return;
    out[0] = double_at; out[1] = pass_at;
}

// What is uploaded for a setting, one block of doubles: met [M][M] | met_pc [M] | thr [2][levels][M][M][2], thr's first index 0 for
// NORMAL and 1 for POST_CRAWFORD.  The offsets are in doubles; thr starts at an even one (16-byte loads).
struct Layout {
    int M, levels;
    long long met, met_pc, thr, doubles;
};
inline Layout layout(int M)
{
    Layout l{M, levels(M), 0, (long long)M * M, 0, 0};
    l.thr = (l.met_pc + M + 1) & ~1ll;
    l.doubles = l.thr + 2ll * l.levels * M * M * 2;
    return l;
}
inline long long thr_index(const Layout &l, int state, int level, int a, int b)      // in entries of two doubles
{
    return ((((long long)(state == NORMAL ? 0 : 1) * l.levels + level) * l.M + (a - 1)) * l.M + (b - 1));
}

// the block of an accepted setting
inline std::vector<double> build(int M, const double *met, const double *met_pc, double window_share)
{
    const Layout l = layout(M);
    std::vector<double> blob((size_t)l.doubles, 0.0);
    for (long long i = 0; i < (long long)M * M; ++i) blob[(size_t)(l.met + i)] = met[i];
    for (long long i = 0; i < M; ++i) blob[(size_t)(l.met_pc + i)] = met_pc[i];
    for (int s = 0; s < 2; ++s)
        for (int lv = 0; lv < l.levels; ++lv)
            for (int a = 1; a <= M; ++a)
                for (int b = 1; b <= M; ++b)
                    thresholds(s ? POST_CRAWFORD : NORMAL, 1ll << lv, a, b, M, met, met_pc, window_share,
                               &blob[(size_t)(l.thr + 2 * thr_index(l, s ? POST_CRAWFORD : NORMAL, lv, a, b))]);
    return blob;
}

// elements of the env's new buffers for a call of P positions and N trials under a match: the packed (away1, away2, state) words, the
// per-trial MWC
struct Needs { long long words, trials; };
inline Needs needs(bool match_on, long long P, long long N) { return match_on ? Needs{P, N} : Needs{0, 0}; }

}  // namespace match
}  // namespace bg
