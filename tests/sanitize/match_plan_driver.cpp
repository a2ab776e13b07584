// Driver for the host-only plan of match play (csrc/bg_match_plan.h), built by tests/test_match_model_cpu.py, plain and with
// g++ -fsanitize=address,undefined.  A program of its own: nothing is preloaded.  Doubles go in and out as C hex floats.
//   match_plan_driver table     stdin: "M window_share", then M M + M doubles (met row by row, met_pc)
//                               -> "layout M levels met met_pc thr doubles", then per entry "state cube a b double_at pass_at", in the
//                                  uploaded block's order, read from the block that build() returns
//   match_plan_driver setting   lines "flags M has_tables window_share k v": a table of 0.5s whose entry k (>= 0; met, then met_pc) is v
//                               -> per line the refusal (0 = accepted)
//   match_plan_driver call      lines "match_on cube_flags rollout_flags" -> per line the refusal of the rollout call
//   match_plan_driver sizes     lines "M P N match_on" -> per line "levels doubles words trials"
#include <cstdio>
#include <cstring>
#include <vector>
#include "bg_match_plan.h"

namespace m = bg::match;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "table")) {
        int M = 0;
        double ws = 0.0;
        if (std::scanf("%d %la", &M, &ws) != 2 || M < 1 || M > m::MAX_POINTS) return 3;
        std::vector<double> met((size_t)M * M), pc((size_t)M);
        for (double &x : met) if (std::scanf("%la", &x) != 1) return 3;
        for (double &x : pc) if (std::scanf("%la", &x) != 1) return 3;
        if (m::check_setting(BGAMD_MATCH_ON, M, met.data(), pc.data(), ws) != m::SET_OK) return 4;
        const m::Layout l = m::layout(M);
        const std::vector<double> blob = m::build(M, met.data(), pc.data(), ws);
        if ((long long)blob.size() != l.doubles) return 5;
        std::printf("layout %d %d %lld %lld %lld %lld\n", l.M, l.levels, l.met, l.met_pc, l.thr, l.doubles);
        for (long long i = 0; i < (long long)M * M; ++i) if (blob[(size_t)(l.met + i)] != met[(size_t)i]) return 6;
        for (long long i = 0; i < M; ++i) if (blob[(size_t)(l.met_pc + i)] != pc[(size_t)i]) return 6;
        for (int s = 0; s < 2; ++s)
            for (int lv = 0; lv < l.levels; ++lv)
                for (int a = 1; a <= M; ++a)
                    for (int b = 1; b <= M; ++b) {
                        const int state = s ? m::POST_CRAWFORD : m::NORMAL;
                        const double *e = &blob[(size_t)(l.thr + 2 * m::thr_index(l, state, lv, a, b))];
                        std::printf("%d %lld %d %d %a %a\n", state, 1ll << lv, a, b, e[0], e[1]);
                    }
        return 0;
    }
    if (!strcmp(argv[1], "setting")) {
        int flags = 0, has = 0;
        long long M = 0, k = 0;
        double ws = 0.0, v = 0.0;
        while (std::scanf("%d %lld %d %la %lld %la", &flags, &M, &has, &ws, &k, &v) == 6) {
            const long long n = M >= 1 && M <= m::MAX_POINTS ? M : 1;
            std::vector<double> t((size_t)(n * n + n), 0.5);
            if (k >= 0 && k < (long long)t.size()) t[(size_t)k] = v;
            std::printf("%d\n", (int)m::check_setting(flags, M, has ? t.data() : nullptr, has ? t.data() + n * n : nullptr, ws));
        }
        return 0;
    }
    if (!strcmp(argv[1], "call")) {
        int on = 0, cube = 0, flags = 0;
        while (std::scanf("%d %d %d", &on, &cube, &flags) == 3) std::printf("%d\n", (int)m::check_call(on != 0, cube, flags));
        return 0;
    }
    if (!strcmp(argv[1], "sizes")) {
        int M = 0, on = 0;
        long long P = 0, N = 0;
        while (std::scanf("%d %lld %lld %d", &M, &P, &N, &on) == 4) {
            const m::Layout l = m::layout(M);
            const m::Needs nd = m::needs(on != 0, P, N);
            std::printf("%d %lld %lld %lld\n", l.levels, l.doubles, nd.words, nd.trials);
        }
        return 0;
    }
    return 2;
}
