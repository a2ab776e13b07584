// Driver for the search's host-only plan (csrc/bg_search_plan.h), built by tests/test_search_plan_cpu.py, plain and with
// g++ -fsanitize=address,undefined.  A program of its own: nothing is preloaded.
//   search_plan_driver plan      lines "kind flags top_k margin deep_k deep_margin reply_top_k reply_margin has_played n cap_rows logs slog
//                                w0 w1 kept_total kept_max searched_total" on stdin, the margins as float32 bit patterns (NaN, -0.0, +inf
//                                and denormals arrive unchanged) -> per line "rc <code>" of a refused request, else every field of the
//                                plan and of search_sized for the three read-back words as "name value" pairs
//   search_plan_driver chunk     lines on stdin, each a text of BGAMD_SEARCH3_CHUNK between two '|' (nothing else on the line: unset)
//                                -> per line search3_chunk
//   search_plan_driver deep      lines "n_deep chunk" on stdin -> per line "none .. n_mid .. mid_lanes .. chunks .."
#include <cstdio>
#include <cstring>
#include <string>
#include "bg_search_plan.h"

static float from_bits(unsigned b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static unsigned to_bits(float f)
{
    unsigned b;
    std::memcpy(&b, &f, 4);
    return b;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "chunk")) {
        char line[256];
        while (std::fgets(line, sizeof line, stdin)) {
            const char *a = std::strchr(line, '|'), *b = a ? std::strrchr(line, '|') : nullptr;
            if (!a || a == b) {
                std::printf("%lld\n", bg::search3_chunk(nullptr));
                continue;
            }
            const std::string text(a + 1, b);
            std::printf("%lld\n", bg::search3_chunk(text.c_str()));
        }
        return 0;
    }
    if (!strcmp(argv[1], "deep")) {
        long long n_deep = 0, chunk = 0;
        while (std::scanf("%lld %lld", &n_deep, &chunk) == 2) {
            const bg::DeepPlan d = bg::deep_plan(n_deep, chunk);
            std::printf("none %d n_mid %lld mid_lanes %lld chunks %lld\n", d.none ? 1 : 0, d.n_mid, d.mid_lanes, d.chunks);
        }
        return 0;
    }
    if (strcmp(argv[1], "plan")) return 2;
    bg::SearchRequest q{};
    int kind = 0, has_played = 0, logs = 0, slog = 0, w0 = 0, w1 = 0;
    unsigned margin = 0, deep_margin = 0, reply_margin = 0;
    long long kept_total = 0, kept_max = 0, searched_total = 0;
    while (std::scanf("%d %d %d %u %d %u %d %u %d %lld %lld %d %d %d %d %lld %lld %lld", &kind, &q.flags, &q.top_k, &margin, &q.deep_k, &deep_margin,
                      &q.reply_top_k, &reply_margin, &has_played, &q.n, &q.cap_rows, &logs, &slog, &w0, &w1, &kept_total, &kept_max,
                      &searched_total) == 18) {
        if (kind < 0 || kind > 4) return 2;
        q.kind = (bg::SearchKind)kind;
        q.margin = from_bits(margin); q.deep_margin = from_bits(deep_margin); q.reply_margin = from_bits(reply_margin);
        q.has_played = has_played != 0; q.logs_steps = logs != 0; q.has_search_log = slog != 0;
        q.has_weights[0] = w0 != 0; q.has_weights[1] = w1 != 0;
        const bg::SearchPlan p = bg::search_plan(q);
        if (p.rc) {
            std::printf("rc %d\n", p.rc);
            continue;
        }
        const bg::SearchSized z = bg::search_sized(p, kept_total, kept_max, searched_total);
        std::printf("rc 0 kind %d flags %d slot %d top_k %d k_lim %u margin %u select %d match_played %d pass_replies %d skip_singletons %d "
                    "read_back %d read_searched %d k_known %d fanout %d ending %d logged %d min_searched %u deep %d deep_k_lim %u deep_margin %u "
                    "reply_top_k %d reply_margin %u apply %d per_game_bytes %lld per_row_bytes %lld ana_word_bytes %lld ana_state_bytes %lld "
                    "deep_game_bytes %lld cand_presize %lld n_cand %lld n_searched %lld K %d n_virtual %lld cand_rows %lld scratch_lanes %lld "
                    "passes %lld\n",
                    (int)p.kind, p.flags, p.slot, p.top_k, p.k_lim, to_bits(p.margin), (int)p.select, p.match_played ? 1 : 0, p.pass_replies ? 1 : 0,
                    p.skip_singletons ? 1 : 0, p.read_back ? 1 : 0, p.read_searched ? 1 : 0, p.k_known ? 1 : 0, (int)p.fanout, (int)p.ending,
                    p.logged ? 1 : 0, p.min_searched, p.deep ? 1 : 0, p.deep_k_lim, to_bits(p.deep_margin), p.reply_top_k, to_bits(p.reply_margin),
                    p.apply ? 1 : 0, p.per_game_bytes, p.per_row_bytes, p.ana_word_bytes, p.ana_state_bytes, p.deep_game_bytes, p.cand_presize,
                    z.n_cand, z.n_searched, z.K, z.n_virtual, z.cand_rows, z.scratch_lanes, z.passes);
    }
    return 0;
}
