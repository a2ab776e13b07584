// bg_outcome.h -- a finished game in points: single game, gammon, backgammon (bgamd_outcomes, bgamd_env_outcomes, and the rollout's
// per-trial points, include/bgamd.h).  Included by bgamd.hip inside its anonymous namespace, before the rollout's kernels.
//
// The reference knows wins only (over(), cppsrc/game.cpp:388-407), so the standard rules apply: the loser who has borne off a checker
// loses 1 point; one who has not loses 3 with a checker on the bar or in the winner's home board, else 2.
#pragma once

constexpr uint32_t OUT_P2_DEEP = 0x03F80000u;        // PLAYER2's planes: points 19..24 (PLAYER1's home) and 25 (PLAYER2's bar)
constexpr uint32_t OUT_P1_DEEP = 0x0000007Fu;        // PLAYER1's planes: 0 (PLAYER1's bar) and points 1..6 (PLAYER2's home)

// the result from PLAYER1's side: 0 = not over, +1 / +2 / +3 = PLAYER1 won a single game / gammon / backgammon, -1 / -2 / -3 = PLAYER2
// did.  The winner is over_code's (PLAYER1 first: 15 off on both sides is PLAYER1's single game).  Only the LOSER's planes are read
// past that: its off bit (PLAYER2: bit 0, PLAYER1: bit 25) and its bar | the winner's home.
__device__ __forceinline__ int outcome_points(const uint32_t (&p)[8])
{
    const int oc = over_code(p);
    if (!oc) return 0;
    const uint32_t loser = oc == 1 ? (p[4] | p[5] | p[6] | p[7]) : (p[0] | p[1] | p[2] | p[3]);
    const uint32_t off = oc == 1 ? 1u : (1u << 25);
    const uint32_t deep = oc == 1 ? OUT_P2_DEEP : OUT_P1_DEEP;
    const int pts = (loser & off) ? 1 : ((loser & deep) ? 3 : 2);
    return oc == 1 ? pts : -pts;
}

// The kernels of this feature are templates (LAST is unused): a template's code is emitted behind the non-template kernels, so the kernels
// of the greedy step keep the order and distances they had in the code object (where the step's code lies costs ~1 %).
// thread per state: int32[28] -> points (a count outside -15 .. 15, or a bar / off count outside 0 .. 15: BGAMD_OUTCOME_BAD)
template <int LAST>
__global__ __launch_bounds__(256) void outcomes_kernel(const int32_t *__restrict__ st, long long n, int32_t *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t s[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) s[k] = st[i * 28 + k];
    uint32_t p[8];
    int bad = 0;
    planes_from_state28(s, p, &bad);
    out[i] = bad ? BGAMD_OUTCOME_BAD : outcome_points(p);
}

// thread per lane: the points of the lane's current board (a lane still playing, or auto-reset to the start position: 0)
template <int LAST>
__global__ __launch_bounds__(256) void env_outcomes_kernel(EnvView e, int32_t *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    out[g] = outcome_points(p);
}
