// Driver for the env's host-only step plan (csrc/bg_step_plan.h), built by tests/test_step_plan_cpu.py, plain and with
// g++ -fsanitize=address,undefined.  The tuning comes from the environment through the header's own parser, as in env_create.
//   step_plan_driver <experimental>     lines "n n_cu cap_rows precision wm_ok" on stdin -> per line the tuning of an n-lane env and
//                                       its plan | the grids of the callers outside a run, as "name value" pairs on one line
#include <cstdio>
#include <cstdlib>
#include "bg_step_plan.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const bool experimental = atoi(argv[1]) != 0;
    long long n = 0, cap_rows = 0;
    int n_cu = 0, precision = 0, wm_ok = 0;
    while (std::scanf("%lld %d %lld %d %d", &n, &n_cu, &cap_rows, &precision, &wm_ok) == 5) {
        const bg::StepTuning u = bg::step_tuning_from_env(getenv, experimental, n);
        const bg::StepPlan p = bg::step_plan(u, n, n_cu, cap_rows, precision, wm_ok != 0);
        std::printf("mfma_delta %d d16 %d list_shards %d split_arena %d expand_merged %d expand_parts %d expand_dbl_npb %d expand_dbl_pct %d "
                    "root_in_boundary %d overlap %d root_f32_mfma %d root_resident %d | ",
                    u.mfma_delta, u.d16, u.list_shards, u.split_arena, u.expand_merged, u.expand_parts, u.expand_dbl_npb, u.expand_dbl_pct,
                    u.root_in_boundary, u.overlap, u.root_f32_mfma, u.root_resident);
        std::printf("incremental %d delta_mfma %d b_base %lld xall_nd %lld xall_nl %lld shards %d ply2_grid %lld leaf_grid %lld delta_grid %lld "
                    "eval_grid %lld d16_grid %lld root %d root_grid %lld root_may_run_in_boundary %d fused_with_more %d sample_score_grid %lld "
                    "sample_pick_grid %lld rnd_count_grid %lld choice0 %d choice1_own %d choice1_ready %d forked_own_2nd %d forked_ready_2nd %d "
                    "forked_own_1st %d own_launch_first %d own_launch_ready %d | ",
                    p.incremental ? 1 : 0, p.mfma_delta ? 1 : 0, p.b_base, p.xall_nd, p.xall_nl, p.shards, p.ply2_grid, p.leaf_grid, p.delta_grid,
                    p.eval.lds, p.eval.d16, (int)p.root, p.root_grid, p.root_in_boundary ? 1 : 0, p.fused_with_more ? 1 : 0, p.sample_score_grid,
                    p.sample_pick_grid, p.rnd_count_grid, p.choice_eval, bg::step_choice_root(p, false), bg::step_choice_root(p, true),
                    bg::step_choice_forked(p, false, true), bg::step_choice_forked(p, true, true), bg::step_choice_forked(p, false, false),
                    bg::own_root_launch(p, false) ? 1 : 0, bg::own_root_launch(p, true) ? 1 : 0);
        // callers outside a run: bgamd_evaluate_incremental over n roots and n rows, bgamd_evaluate over n rows, the random step
        const bg::RootPass r = bg::root_pass_kind(u, false);
        std::printf("inc_root %d inc_root_grid %lld inc_delta_grid %lld imm_eval_grid %lld imm_d16_grid %lld random_count_grid %lld\n", (int)r,
                    bg::root_pass_grid(r, n, n_cu), bg::delta_grid(n, n_cu), bg::eval_grids(n, n_cu).lds, bg::eval_grids(n, n_cu).d16,
                    bg::rnd_count_grid(n * 64, n_cu));
    }
    return 0;
}
