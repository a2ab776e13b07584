// Driver for the rollout's host-only plan (csrc/bg_rollout_plan.h), built by tests/test_rollout_plan_cpu.py, plain and with
// g++ -fsanitize=address,undefined.  A program of its own: nothing is preloaded.
//   rollout_plan_driver plan <turn_limit>       lines "flags P offset T M lanes has_states has_group plies top_k cube w0 w1" on stdin
//                                               -> per line "rc <code>" of a refused request, else every field as "name value" pairs
//   rollout_plan_driver progress <turn_limit> <T> <M> <plies>
//                                               the plan of one position with T trials; lines "done ro_err env_err" on stdin, the
//                                               read-backs of one loop in order -> per line the verdict (0 go on, 1 finished, 2 stalled)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bg_rollout_plan.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long long turn_limit = atoll(argv[2]);
    if (!strcmp(argv[1], "progress")) {
        if (argc != 6) return 2;
        const bg::RolloutRequest q{0, 1, 0, atoll(argv[3]), atoll(argv[4]), 0, true, false, atoi(argv[5]), 0, false, {true, true}};
        const bg::RolloutPlan p = bg::rollout_plan(q, turn_limit);
        if (p.rc) return 3;
        bg::RolloutProgress progress(p);
        unsigned long long done = 0, ro_err = 0, env_err = 0;
        while (std::scanf("%llu %llu %llu", &done, &ro_err, &env_err) == 3) std::printf("%d\n", (int)progress.read(done, ro_err, env_err));
        return 0;
    }
    if (strcmp(argv[1], "plan")) return 2;
    bg::RolloutRequest q{};
    int has_states = 0, has_group = 0, cube = 0, w0 = 0, w1 = 0;
    while (std::scanf("%d %lld %lld %lld %lld %lld %d %d %d %d %d %d %d", &q.flags, &q.n_positions, &q.position_offset, &q.trials, &q.max_plies,
                      &q.lanes, &has_states, &has_group, &q.ro_plies, &q.ro_top_k, &cube, &w0, &w1) == 13) {
        q.has_states = has_states != 0; q.has_group = has_group != 0; q.cube_on = cube != 0;
        q.has_weights[0] = w0 != 0; q.has_weights[1] = w1 != 0;
        const bg::RolloutPlan p = bg::rollout_plan(q, turn_limit);
        if (p.rc) {
            std::printf("rc %d\n", p.rc);
            continue;
        }
        const bg::RolloutNeeds &n = p.needs;
        std::printf("rc 0 P %lld T %lld N %lld M %lld rotate %d vr %d cube %d grouped %d two_ply %d slot %d run_flags %d F %lld n_fan %lld L %lld "
                    "fan_chunks %lld fan_eval %d lane_offset %llu R %d G %d truncates %d search_scratch_lanes %lld preroll_positions %lld "
                    "preroll_lanes %lld pos %lld fan %lld trials %lld lanes %lld vtrials %lld vlanes %lld vpos %lld group %lld ctrials %lld "
                    "cstart %lld stall_turns %lld stall_limit %lld\n",
                    p.P, p.T, p.N, p.M, p.rotate ? 1 : 0, p.vr ? 1 : 0, p.cube ? 1 : 0, p.grouped ? 1 : 0, p.two_ply ? 1 : 0, p.slot, p.run_flags,
                    p.F, p.n_fan, p.L, p.fan_chunks, p.fan_eval ? 1 : 0, p.lane_offset, p.R, p.G, p.truncates ? 1 : 0, p.search_scratch_lanes,
                    p.preroll_positions, p.preroll_lanes, n.pos, n.fan, n.trials, n.lanes, n.vtrials, n.vlanes, n.vpos, n.group, n.ctrials,
                    n.cstart, p.stall_turns, p.stall_limit);
    }
    return 0;
}
