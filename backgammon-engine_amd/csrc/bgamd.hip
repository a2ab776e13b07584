// bgamd.hip -- kernels of the env step + the C ABI declared in include/bgamd.h (gfx950 only): the env handle here, the learner's
// (bgamd_td) in bg_learner_host.h, included at the end.
//
// Data layout in HBM (one env = n_games lanes on one device):
//   planes   uint32[8][n]   bit-plane boards, SoA: a 64-lane wave reads 256 contiguous bytes per plane
//   meta     uint32[n]      bit0 turn | bits4-6 die1 | bits8-10 die2 | bit12 finished
//   ply, episode uint32[n]  Philox counter words (game_id = lane_offset + lane + episode*lane_stride)
//   arena    uint4[2*cap]   candidate afterstates, 32 B rows, reference order inside a lane's segment
//   values   float[cap]     value-net output per row
// Greedy step: roots -> stage<PLY2> -> stage<PLY3> -> stage<LEAF> (bg_staged_kernels.h) -> eval (bg_eval.h) -> apply.
// Random step: rnd_tasks -> rnd_count -> rnd_select (bg_random_kernels.h).  emit_kernel serves the ordered enumerate API.
// What a greedy step launches and how big -- the kernel variants, the grids, the row arenas, the BGAMD_* switches and their defaults --
// is decided once per run by step_plan (bg_step_plan.h, plain C++, checked without a GPU); GreedyRun::step issues what the plan names.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include <queue>
#include <algorithm>
#include <initializer_list>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is resolved at run time (rccl_api, bg_learner_host.h), libbgamd.so does not link it

#include "../../include/bgamd.h"
#include "bg_board.h"
#include "bg_eval.h"
#include "bg_root_resident.h"
// Kernels that lost their same-box A/B (DESIGN.md §4 / NOTEBOOK.md) compile only with -DBGAMD_EXPERIMENTAL (the library
// __graft_entry__.build_experimental() makes; the tests marked gpu_experimental run against it): the K-compacted MFMA delta kernel
// (BGAMD_MFMA_DELTA=1), the dense f16 x 2 kernel with register-resident weights (BGAMD_F16X2_RESIDENT=1), the LDS-staged / f32-MFMA root
// passes (BGAMD_ROOT_RESIDENT=0, BGAMD_ROOT_F32=1), the learner's unfused matrix-pipe forward (BGAMD_TD_FUSED=0).  In the default build
// those switches are ignored and bgamd_build_flags() says so.
#ifdef BGAMD_EXPERIMENTAL
#include "bg_eval_mfma.h"
#include "bg_eval_dense16.h"
constexpr bool EXPERIMENTAL_BUILD = true;
#else
constexpr bool EXPERIMENTAL_BUILD = false;
#endif
#include "bg_learner.h"
#include "bg_fit.h"
#include "bg_schedule.h"
#include "bg_step_plan.h"
#include "bg_search_plan.h"
#include "bg_rollout_plan.h"
#include "bg_movegen.h"
#include "bg_staged.h"
#include "bg_search3.h"
#include "bg_cube.h"
#include "bg_match.h"
#include "bg_match_plan.h"

using namespace bg;

namespace {

// Env counters, one 128-byte line each (BG_STAT_STRIDE=1: packed, as up to round 2).  Atomics queue up at the memory side per LINE: the
// boundary launch's three statistics from 256 workgroups were 768 atomics on one line -- 4 us of its 18 (same-box A/B, round 3:
// boundary 0.0182 -> 0.0139 ms).  Further copies of the statistics per group of workgroups (8, 16) measured nothing on top.
#ifndef BG_STAT_STRIDE
#define BG_STAT_STRIDE 16
#endif
enum { C_ARENA_TOP = 0, C_STEPS = BG_STAT_STRIDE, C_FINISHED = 2 * BG_STAT_STRIDE, C_P1WINS = 3 * BG_STAT_STRIDE, C_CAND_RAW = 4 * BG_STAT_STRIDE,
       C_ROWS_EVAL = 5 * BG_STAT_STRIDE, C_ERR = 6 * BG_STAT_STRIDE, C_FNODES = 7 * BG_STAT_STRIDE, C_DNODES = 8 * BG_STAT_STRIDE,
       C_KSTEPS = 9 * BG_STAT_STRIDE, C_COUNT = 10 * BG_STAT_STRIDE };
enum { ERRF_ARENA = 1, ERRF_STATE = 2, ERRF_DELTA = 4 };
constexpr uint32_t META_FINISHED = 1u << 12;

struct EnvView {
    long long n;
    unsigned long long seed, lane_offset, lane_stride;
    long long cap;
    uint32_t *planes, *meta, *ply, *episode, *flags;
    uint32_t *cand_off, *cand_cnt;
    int32_t *chosen;
    uint32_t *chosen_seq;
    float *chosen_val;
    uint4 *rows;
    uint32_t *seqs;
    float *values;
    unsigned long long *counters;
    uint4 *traj;               // optional [max_plies][n][2]: pre-move row of every turn (train.py:105-106)
    long long traj_plies;
    // ring log of continuous self-play (bgamd_env_set_trajectory_ring): traj is [traj_ring][n][2] indexed by the ENV STEP (mod traj_ring),
    // not by the lane's ply -- a lane's column holds game after game -- and endrec[slot][lane] says whether the game whose turn was
    // logged in that slot ended with it: 0, or logged turns of the game | winner << 15.  log_slot / end_slot: the slots the roots /
    // the apply of THIS launch write (set by the host per launch).
    unsigned short *endrec;
    long long traj_ring, log_slot, end_slot;
};

__device__ __forceinline__ uint32_t meta_pack(int turn, int d1, int d2, bool fin)
{
    return (uint32_t)turn | ((uint32_t)d1 << 4) | ((uint32_t)d2 << 8) | (fin ? META_FINISHED : 0u);
}

__device__ __forceinline__ void load_planes(const EnvView &e, long long g, uint32_t (&p)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = e.planes[(long long)k * e.n + g];
}
__device__ __forceinline__ void store_planes(const EnvView &e, long long g, const uint32_t (&p)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) e.planes[(long long)k * e.n + g] = p[k];
}

__device__ __forceinline__ unsigned long long wave_sum_u32(uint32_t v)
{
    unsigned long long s = v;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)s, m, 64), hi = __shfl_xor((uint32_t)(s >> 32), m, 64);
        s += ((unsigned long long)hi << 32) | lo;
    }
    return s;
}

// Terminal check (game.cpp:388-407), auto-reset / turn flip (train.py:113-120), write-back.
// fwd (optional, [3]): the lane's meta / ply / episode as they stand after this call (p is updated in place) -- for a
// caller that goes on with the lane's next turn in the same kernel instead of reading the state back
__device__ __forceinline__ void finish_turn(const EnvView &e, long long g, uint32_t (&p)[8], int turn, int d1, int d2,
                                            uint32_t ply, uint32_t epi, int flags, bool live, uint32_t *fwd = nullptr)
{
    uint32_t oflags = 0;
    bool fin = false;
    const int oc = live ? over_code(p) : 0;
    if (e.endrec && g < e.n)                               // ring log: did the game whose turn sits in this step's slot end with it?
        e.endrec[e.end_slot * e.n + g] = oc ? (unsigned short)((ply + 1u > 0x7FFFu ? 0x7FFFu : ply + 1u) | ((uint32_t)(oc - 1) << 15)) : (unsigned short)0;
    if (oc) {
        oflags = 1u | ((uint32_t)(oc - 1) << 1);
        if (flags & BGAMD_AUTO_RESET) {
            epi += 1; ply = 0;
            constexpr StartPlanes sp = start_planes();
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = sp.p[k];
            const unsigned long long gid = e.lane_offset + (unsigned long long)g + (unsigned long long)epi * e.lane_stride;
            turn = opening_turn(e.seed, gid);
        } else if (!(flags & BGAMD_NO_FLIP)) {
            fin = true; oflags |= 4u;
        }
    } else if (live && !(flags & BGAMD_NO_FLIP)) {
        turn ^= 1; ply += 1;
    }
    if (live) {
        store_planes(e, g, p);
        e.meta[g] = meta_pack(turn, d1, d2, fin);
        e.ply[g] = ply; e.episode[g] = epi; e.flags[g] = oflags;
        if (fwd) { fwd[0] = meta_pack(turn, d1, d2, fin); fwd[1] = ply; fwd[2] = epi; }
    }
    // counters: wave sums -> one LDS word each -> ONE global atomic per block and counter (same-address global
    // atomics retire at ~10 ns each: a per-wave atomic from 1 024 waves costs more than the kernel itself)
    __shared__ unsigned int s_stat[3];
    if (threadIdx.x < 3) s_stat[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long nsteps = wave_sum_u32(live ? 1u : 0u);
    const unsigned long long nfin = wave_sum_u32(oc ? 1u : 0u);
    const unsigned long long nw1 = wave_sum_u32(oc == 1 ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) {
        if (nsteps) atomicAdd(&s_stat[0], (unsigned int)nsteps);
        if (nfin) atomicAdd(&s_stat[1], (unsigned int)nfin);
        if (nw1) atomicAdd(&s_stat[2], (unsigned int)nw1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_stat[0]) atomicAdd(&e.counters[C_STEPS], (unsigned long long)s_stat[0]);
        if (s_stat[1]) atomicAdd(&e.counters[C_FINISHED], (unsigned long long)s_stat[1]);
        if (s_stat[2]) atomicAdd(&e.counters[C_P1WINS], (unsigned long long)s_stat[2]);
    }
}

struct LaneCtx {
    uint32_t p[8];
    uint32_t meta, ply, epi;
    int turn, d1, d2;
    U4 x;
    bool live;
};

// lane_derive: everything lane_begin does after its loads (c.p, c.meta, c.ply, c.epi are in place)
__device__ __forceinline__ void lane_derive(const EnvView &e, long long g, int flags, LaneCtx &c)
{
    c.live = g < e.n;
    const long long gg = c.live ? g : 0;
    if (c.meta & META_FINISHED) c.live = false;
    c.turn = c.meta & 1;
    // head-to-head play (train.py:262-277): only the lanes whose side is to move take part in this call
    if (((flags & BGAMD_ONLY_P1) && c.turn != 0) || ((flags & BGAMD_ONLY_P2) && c.turn != 1)) c.live = false;
    const unsigned long long gid = e.lane_offset + (unsigned long long)gg + (unsigned long long)c.epi * e.lane_stride;
    c.x = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), c.ply, STREAM_TURN, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
    if (flags & BGAMD_ROLL) { c.d1 = die_from_u32(c.x.x); c.d2 = die_from_u32(c.x.y); }
    else { c.d1 = (c.meta >> 4) & 7; c.d2 = (c.meta >> 8) & 7; }
    if (c.d1 < 1 || c.d1 > 6 || c.d2 < 1 || c.d2 > 6) { c.d1 = 1; c.d2 = 1; }   // Game::last_dice default {1,1}
}

__device__ __forceinline__ void lane_begin(const EnvView &e, long long g, int flags, LaneCtx &c)
{
    const long long gg = g < e.n ? g : 0;
    load_planes(e, gg, c.p);
    c.meta = e.meta[gg]; c.ply = e.ply[gg]; c.epi = e.episode[gg];
    lane_derive(e, g, flags, c);
}

__device__ __forceinline__ void split_sides(const uint32_t (&p)[8], int turn, Side &own, Side &opp)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        own.b[k] = turn ? p[4 + k] : p[k];
        opp.b[k] = turn ? p[k] : p[4 + k];
    }
}
__device__ __forceinline__ void join_sides(const Side &own, const Side &opp, int turn, uint32_t (&p)[8])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] = turn ? opp.b[k] : own.b[k];
        p[4 + k] = turn ? own.b[k] : opp.b[k];
    }
}

// ---- random-policy step: everything in one kernel ----------------------------------------------
__global__ __launch_bounds__(64) void step_random_kernel(EnvView e, int flags, const uint32_t *__restrict__ choice)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    LaneCtx c;
    lane_begin(e, g, flags, c);
    Side own, opp;
    split_sides(c.p, c.turn, own, opp);
    uint32_t C = 0;
    if (c.live) {
        CountVisitor cv;
        walk_sequences(own, opp, c.turn, c.d1, c.d2, cv);
        C = cv.n;
    }
    int32_t chosen = -1;
    uint32_t cseq = 0;
    if (C > 0) {
        const uint32_t u = choice ? choice[g] : c.x.z;
        const uint32_t k = (uint32_t)(((unsigned long long)u * C) >> 32);
        SelectVisitor sv(k);
        walk_sequences(own, opp, c.turn, c.d1, c.d2, sv);
        join_sides(sv.own, sv.opp, c.turn, c.p);
        chosen = (int32_t)k; cseq = sv.seq | (c.turn ? (1u << 29) : 0u);   // bit 29: mover moves down (unpack_seq)
    }
    if (c.live) { e.chosen[g] = chosen; e.chosen_seq[g] = cseq; e.cand_cnt[g] = C; e.chosen_val[g] = 0.0f; }
    const unsigned long long tot = wave_sum_u32(C);
    if (threadIdx.x == 0 && tot) atomicAdd(&e.counters[C_CAND_RAW], tot);
    finish_turn(e, g, c.p, c.turn, c.d1, c.d2, c.ply, c.epi, flags, c.live);
}

// ---- emit: count pass, wave-level bump allocation, emit pass ---------------------------------
__global__ __launch_bounds__(64) void emit_kernel(EnvView e, int flags, int with_seq, const int32_t *__restrict__ ov_player,
                                                  const int32_t *__restrict__ ov_dice)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    const int lane = threadIdx.x;
    LaneCtx c;
    lane_begin(e, g, flags, c);
    if (g < e.n) {       // explicit (player, d1, d2) of legalTurnSequences / evaluateTurnSequences
        if (ov_player) c.turn = ov_player[g] == 1 ? 1 : 0;
        if (ov_dice) {
            const int a = ov_dice[2 * g], b = ov_dice[2 * g + 1];
            if (a >= 1 && a <= 6 && b >= 1 && b <= 6) { c.d1 = a; c.d2 = b; } else c.live = false;
        }
    }
    Side own, opp;
    split_sides(c.p, c.turn, own, opp);
    uint32_t C = 0;
    if (c.live) {
        CountVisitor cv;
        walk_sequences(own, opp, c.turn, c.d1, c.d2, cv);
        C = cv.n;
    }
    // inclusive scan over the wave
    uint32_t incl = C;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 0 && total) {
        base = atomicAdd(&e.counters[C_ARENA_TOP], (unsigned long long)total);
        atomicAdd(&e.counters[C_CAND_RAW], (unsigned long long)total);
    }
    base = ((unsigned long long)__shfl((uint32_t)(base >> 32), 0, 64) << 32) | __shfl((uint32_t)base, 0, 64);
    const bool overflow = base + total > (unsigned long long)e.cap;
    if (overflow) {
        if (lane == 0) atomicOr(&e.counters[C_ERR], (unsigned long long)ERRF_ARENA);
        C = 0;
    }
    const unsigned long long my_off = overflow ? 0ull : base + incl - C;
    if (C > 0) {
        EmitVisitor ev(e.rows + 2 * my_off, with_seq ? e.seqs + my_off : nullptr, c.turn);
        walk_sequences(own, opp, c.turn, c.d1, c.d2, ev);
    }
    if (g < e.n) {
        e.cand_off[g] = (uint32_t)my_off;
        e.cand_cnt[g] = C;
        if ((flags & BGAMD_ROLL) && c.live) e.meta[g] = meta_pack(c.turn, c.d1, c.d2, false);
    }
}

// ---- small state kernels ---------------------------------------------------------------------------
// mask == nullptr: every lane restarts at episode 0.  Otherwise only the lanes with mask != 0 restart, as the NEXT
// episode of that lane (what the auto-reset of a finished game does)
__global__ void reset_kernel(EnvView e, const int32_t *__restrict__ mask, uint32_t episode)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    if (mask && mask[g] == 0) return;
    constexpr StartPlanes sp = start_planes();
    uint32_t p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = sp.p[k];
    store_planes(e, g, p);
    const uint32_t epi = mask ? e.episode[g] + 1u : episode;
    const unsigned long long gid = e.lane_offset + (unsigned long long)g + (unsigned long long)epi * e.lane_stride;
    e.meta[g] = meta_pack(opening_turn(e.seed, gid), 1, 1, false);
    e.ply[g] = 0; e.episode[g] = epi; e.flags[g] = 0;
    e.cand_off[g] = 0; e.cand_cnt[g] = 0; e.chosen[g] = -1; e.chosen_seq[g] = 0; e.chosen_val[g] = 0.0f;
}

__global__ void set_states_kernel(EnvView e, const int32_t *__restrict__ st, const int32_t *__restrict__ turn)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    if (st) {
        uint32_t p[8];
        int bad = 0;
        int32_t s[28];
#pragma unroll
        for (int i = 0; i < 28; ++i) s[i] = st[g * 28 + i];
        planes_from_state28(s, p, &bad);
        if (bad) atomicOr(&e.counters[C_ERR], (unsigned long long)ERRF_STATE);
        store_planes(e, g, p);
    }
    const uint32_t m = e.meta[g];
    const int t = turn ? (turn[g] & 1) : (int)(m & 1);
    e.meta[g] = (m & ~(1u | META_FINISHED)) | (uint32_t)t;
}

__global__ void get_states_kernel(EnvView e, int32_t *__restrict__ st, int32_t *__restrict__ turn)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    if (st) {
        int32_t s[28];
        state28_from_planes(p, s);
#pragma unroll
        for (int i = 0; i < 28; ++i) st[g * 28 + i] = s[i];
    }
    if (turn) turn[g] = (int32_t)(e.meta[g] & 1);
}

__global__ void get_flags_kernel(EnvView e, int32_t *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    const int oc = over_code(p);          // is_game_over on the CURRENT board (game.cpp:388-407)
    out[g] = (oc ? (1 | ((oc - 1) << 1)) : 0) | ((e.meta[g] & META_FINISHED) ? 4 : 0) | (int32_t)((e.flags[g] & 3u) << 4);
}

__global__ void snapshot_kernel(EnvView e, int32_t *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    int32_t s[28];
    state28_from_planes(p, s);
    int32_t *o = out + g * 32;
#pragma unroll
    for (int i = 0; i < 28; ++i) o[i] = s[i];
    const uint32_t m = e.meta[g];
    const int oc = over_code(p);
    o[28] = (int32_t)(m & 1); o[29] = (int32_t)((m >> 4) & 7); o[30] = (int32_t)((m >> 8) & 7);
    o[31] = (oc ? (1 | ((oc - 1) << 1)) : 0) | ((m & META_FINISHED) ? 4 : 0) | (int32_t)((e.flags[g] & 3u) << 4);
}

__global__ void dice_kernel(EnvView e, const int32_t *__restrict__ in, int32_t *__restrict__ out, int roll)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t m = e.meta[g];
    if (in || roll) {
        int d1, d2;
        if (roll) {
            const unsigned long long gid = e.lane_offset + (unsigned long long)g + (unsigned long long)e.episode[g] * e.lane_stride;
            const U4 x = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), e.ply[g], STREAM_TURN, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
            d1 = die_from_u32(x.x); d2 = die_from_u32(x.y);
            if (roll == 2) e.ply[g] += 1;      // scalar Game::rollDice: every call draws fresh dice
        } else { d1 = in[2 * g] & 7; d2 = in[2 * g + 1] & 7; }
        m = (m & ~0x770u) | ((uint32_t)d1 << 4) | ((uint32_t)d2 << 8);
        e.meta[g] = m;
    }
    if (out) { out[2 * g] = (m >> 4) & 7; out[2 * g + 1] = (m >> 8) & 7; }
}

__global__ void cand_info_kernel(EnvView e, int64_t *__restrict__ offs, int32_t *__restrict__ cnts)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    if (offs) offs[g] = (int64_t)e.cand_off[g];
    if (cnts) cnts[g] = (int32_t)e.cand_cnt[g];
}

__device__ __forceinline__ void unpack_seq(uint32_t q, int8_t *out8, int32_t *len_out)
{
    const int len = (q >> 20) & 7, dA = (q >> 23) & 7, dB = (q >> 26) & 7;
    // direction is recovered from the move itself: the mover's sign is not stored, so the
    // caller passes it through bit 29 (1 = PLAYER2 moves down)
    const int down = (q >> 29) & 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int o = -1, d = -1;
        if (k < len) {
            o = (q >> (5 * k)) & 31;
            const int die = (k & 1) ? dB : dA;
            d = down ? o - die : o + die;
            d = d < 0 ? 0 : (d > 25 ? 25 : d);
        }
        out8[2 * k] = (int8_t)o; out8[2 * k + 1] = (int8_t)d;
    }
    if (len_out) *len_out = len;
}

__global__ void rows_read_kernel(const uint4 *__restrict__ rows, const uint32_t *__restrict__ seqs, long long first,
                                 long long n, int32_t *__restrict__ st, int8_t *__restrict__ seq, int32_t *__restrict__ len)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = first + i;
    const uint4 u0 = rows[2 * r], u1 = rows[2 * r + 1];
    const uint32_t p[8] = {u0.x & ~TURN_BIT, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    if (st) {
        int32_t s[28];
        state28_from_planes(p, s);
#pragma unroll
        for (int k = 0; k < 28; ++k) st[i * 28 + k] = s[k];
    }
    if (seq) {
        const uint32_t q = seqs[r] | ((u0.x & TURN_BIT) ? (1u << 29) : 0u);
        unpack_seq(q, seq + i * 8, len ? len + i : nullptr);
    }
}

// (b_base > 0: four arenas -- the logical rows are the rows of arena 0, then those of arena 1, ...; tops = the step's counters)
__global__ void rows_values_kernel(const uint4 *__restrict__ rows, const float *__restrict__ values, long long first, long long n,
                                   int32_t *__restrict__ st, float *__restrict__ val, const unsigned long long *__restrict__ tops, long long b_base)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long r = first + i;
#ifdef BG_EVAL_WGCLOCK                                         // (diagnostic build, tools/eval_wg_clock.py: physical rows)
    b_base = 0;
#endif
    if (b_base > 0) {
        long long k = 0, rest = r;
        for (; k < N_ARENAS; ++k) {
            long long c = (long long)tops[arena_counter((int)k)];
            if (c > b_base) c = b_base;
            if (rest < c) break;
            rest -= c;
        }
        if (k == N_ARENAS) {                                    // past the rows the step produced (every arena clamped, the last one too):
            if (st)                                             // zeros, never a read beyond the arenas
                for (int j = 0; j < 28; ++j) st[i * 28 + j] = 0;
            if (val) val[i] = 0.0f;
            return;
        }
        r = k * b_base + rest;
    }
    if (st) {
        const uint4 u0 = rows[2 * r], u1 = rows[2 * r + 1];
        const uint32_t p[8] = {u0.x & ~TURN_BIT, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        int32_t s[28];
        state28_from_planes(p, s);
#pragma unroll
        for (int k = 0; k < 28; ++k) st[i * 28 + k] = s[k];
    }
    if (val) val[i] = values[r];
}

__global__ void last_choice_kernel(EnvView e, int32_t *chosen, int32_t *count, int8_t *seq, int32_t *len, float *val)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    if (chosen) chosen[g] = e.chosen[g];
    if (count) count[g] = (int32_t)e.cand_cnt[g];
    if (val) val[g] = e.chosen_val[g];
    if (seq) {
        // the mover of the last step: turn was flipped unless the game ended / NO_FLIP; the packed
        // sequence carries the direction in bit 29, set by the step kernels' callers below
        unpack_seq(e.chosen_seq[g], seq + g * 8, len ? len + g : nullptr);
    }
}

__global__ void pack_rows_kernel(const int32_t *__restrict__ st, const int32_t *__restrict__ turn, long long n,
                                 uint4 *__restrict__ rows, unsigned long long *err)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t s[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) s[k] = st[i * 28 + k];
    uint32_t p[8];
    int bad = 0;
    planes_from_state28(s, p, &bad);
    if (bad && err) atomicOr(err, (unsigned long long)ERRF_STATE);
    const int t = turn ? (turn[i] & 1) : 0;
    rows[2 * i] = make_uint4(p[0] | (t ? TURN_BIT : 0u), p[1], p[2], p[3]);
    rows[2 * i + 1] = make_uint4(p[4], p[5], p[6], p[7]);
}

// rows of the stateless incremental operator: afterstate i belongs to root root_index[i] and carries that root's turn bit
__global__ void pack_child_rows_kernel(const int32_t *__restrict__ st, const int32_t *__restrict__ root_index, long long n,
                                       long long n_roots, const uint4 *__restrict__ root_rows, uint4 *__restrict__ rows,
                                       uint2 *__restrict__ info, unsigned long long *err)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t s[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) s[k] = st[i * 28 + k];
    uint32_t p[8];
    int bad = 0;
    planes_from_state28(s, p, &bad);
    long long r = root_index[i];
    if (r < 0 || r >= n_roots) { bad = 1; r = 0; }
    if (bad && err) atomicOr(err, (unsigned long long)ERRF_STATE);
    const uint32_t tb = root_rows[2 * r].x & TURN_BIT;
    rows[2 * i] = make_uint4(p[0] | tb, p[1], p[2], p[3]);
    rows[2 * i + 1] = make_uint4(p[4], p[5], p[6], p[7]);
    info[i] = make_uint2((uint32_t)r, (uint32_t)(i & 0x00FFFFFF) | (tb ? 0x80000000u : 0u));
}

__global__ void encode_states_kernel(const int32_t *__restrict__ st, const int32_t *__restrict__ turn, long long n,
                                     float *__restrict__ out)
{
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    int32_t s[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) s[k] = st[row * 28 + k];
    uint32_t p[8];
    planes_from_state28(s, p, nullptr);
    const Side sd[2] = {{{p[0], p[1], p[2], p[3]}}, {{p[4], p[5], p[6], p[7]}}};
    float *x = out + row * N_IN;
    for (int i = 0; i < 24; ++i) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = count_at(sd[q], i + 1);
            x[8 * i + 4 * q + 0] = c >= 1 ? 1.0f : 0.0f;
            x[8 * i + 4 * q + 1] = c >= 2 ? 1.0f : 0.0f;
            x[8 * i + 4 * q + 2] = c >= 3 ? 1.0f : 0.0f;
            x[8 * i + 4 * q + 3] = c >= 4 ? 0.5f * (float)(c - 3) : 0.0f;
        }
    }
    const int t = turn ? (turn[row] & 1) : 0;
    x[192] = t == 0 ? 1.0f : 0.0f;
    x[193] = t == 0 ? 0.0f : 1.0f;
    x[194] = 0.5f * (float)count_at(sd[0], 0);
    x[195] = 0.5f * (float)count_at(sd[1], 25);
    x[196] = (float)count_at(sd[0], 25) / 15.0f;
    x[197] = (float)count_at(sd[1], 0) / 15.0f;
}

// Game::tryMove with the reference's check order (game.cpp:583-662); err codes 1..7
__global__ void try_move_kernel(EnvView e, const int32_t *__restrict__ player, const int32_t *__restrict__ dice,
                                const int32_t *__restrict__ origin, const int32_t *__restrict__ dest, int32_t *__restrict__ err)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    const int pl = player[g] == 1 ? 1 : 0, d = dice[g], o = origin[g], t = dest[g];
    Side own, opp;
    split_sides(p, pl, own, opp);
    const uint32_t barbit = pl ? (1u << 25) : 1u;
    const uint32_t own_any = any_of(own);
    int code = 0;
    // isValidOrigin (game.cpp:416-457)
    bool vo;
    if (own_any & barbit) vo = (o == (pl ? 25 : 0));
    else vo = (o >= 1 && o <= 24) && ((own_any >> o) & 1u);
    if (!vo) code = 1;
    else if (o < 0 || o > 25) code = 2;
    else if (t < 0 || t > 25) code = 3;
    else {
        const int diff = o - t;
        if (t != 0 && t != 25) {
            const int adiff = diff < 0 ? -diff : diff;
            if ((pl ? -diff : diff) > 0) code = 4;            // diff * (-multi) < 0
            else if (d != adiff) code = 5;
            else if ((ge2_of(opp) >> t) & 1u) code = 6;       // t in 1..24 here
            else {
                dec_at(own, 1u << o);                          // bar or point: same plane arithmetic
                const uint32_t md = 1u << t;
                const uint32_t hm = md & opp.b[0] & ~ge2_of(opp);
                opp.b[0] ^= hm;
                inc_at(opp, hm ? (pl ? 1u : (1u << 25)) : 0u);
                inc_at(own, md);
            }
        } else {
            // bear-off branch (game.cpp:636-648): only "origin on the board" is re-checked;
            // the checker leaves the origin and the MOVER's freed counter grows, whatever t is
            if (o == 0 || o == 25) code = 7;
            else { dec_at(own, 1u << o); inc_at(own, pl ? 1u : (1u << 25)); }
        }
    }
    if (code == 0) {
        join_sides(own, opp, pl, p);
        store_planes(e, g, p);
    }
    err[g] = code;
}

__global__ void legal_moves_kernel(EnvView e, const int32_t *__restrict__ player, const int32_t *__restrict__ die,
                                   int32_t *__restrict__ n_out, int8_t *__restrict__ pairs)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.n) return;
    uint32_t p[8];
    load_planes(e, g, p);
    const int pl = player[g] == 1 ? 1 : 0, d = die[g];
    Side own, opp;
    split_sides(p, pl, own, opp);
    uint32_t m = (d >= 1 && d <= 6) ? legal_origins(own, opp, pl, d) : 0u;
    int n = 0;
    while (m) {
        const int o = __ffs(m) - 1; m &= m - 1;
        int t = pl ? o - d : o + d;
        t = t < 0 ? 0 : (t > 25 ? 25 : t);
        pairs[(g * 26 + n) * 2] = (int8_t)o; pairs[(g * 26 + n) * 2 + 1] = (int8_t)t;
        ++n;
    }
    n_out[g] = n;
}

#include "bg_staged_kernels.h"
#include "bg_random_kernels.h"
#include "bg_search.h"
#include "bg_outcome.h"
#include "bg_rollout.h"
#include "bg_vr.h"
#include "bg_health.h"
#include "bg_analysis.h"
#include "bg_filter.h"

}  // namespace

// ================================================================================================
//                                           C ABI
// ================================================================================================
static thread_local std::string g_hip_err;

#define HIPCHK(call)                                                                   \
    do {                                                                               \
        hipError_t _e = (call);                                                        \
        if (_e != hipSuccess) {                                                        \
            g_hip_err = std::string(#call) + ": " + hipGetErrorString(_e);             \
            return BGAMD_E_HIP;                                                        \
        }                                                                              \
    } while (0)

// every entry point that takes an env (or a learner) first makes its device current: one process may drive envs on
// several devices, and the caller's current device need not be the env's
#define ENV_GUARD(env)                                   \
    do {                                                 \
        if (!(env)) return BGAMD_E_INVALID;              \
        HIPCHK(hipSetDevice((env)->device));             \
    } while (0)

// Device memory has ONE owner per handle (bgamd_env::mem, bgamd_td::mem; bg_devmem.h): a new buffer is a pointer member and one
// allocation call on it, and destroy frees what was handed out.  This backend holds the file's only spellings of the four HIP calls.
#include "bg_devmem.h"
namespace {
struct HipMemBackend {
    static int done(hipError_t e, const char *call, const char *name)
    {
        if (e != hipSuccess) g_hip_err = std::string(call) + "(" + name + "): " + hipGetErrorString(e);
        return e == hipSuccess ? BGAMD_OK : BGAMD_E_HIP;
    }
    int alloc(void **p, size_t bytes, const char *name) { return done(hipMalloc(p, bytes), "hipMalloc", name); }
    int alloc_pinned(void **p, size_t bytes, const char *name) { return done(hipHostMalloc(p, bytes), "hipHostMalloc", name); }
    void free(void *p) { hipFree(p); }
    void free_pinned(void *p) { hipHostFree(p); }
};
using DevMem = DevMemOwner<HipMemBackend>;

// The value net's device tables: per weight slot (head-to-head: one per side) the raw weights and every layout of W1 a kernel reads,
// and the two count LUTs.  An env that borrows another's tables (scratch_env) takes them by assigning the struct; it never owned them.
struct NetTables {
    float *d_w[2] = {nullptr, nullptr};    // raw weights 25601
    float4 *d_wl[2] = {nullptr, nullptr};  // fp32 MFMA layout [99][64]
    float4 *d_wt[2] = {nullptr, nullptr};  // W1^T [198][132] for the incremental evaluator
    uint4 *d_wm[2] = {nullptr, nullptr};   // W1^T as f16 hi | lo dwords [198][4][32] for the MFMA delta kernel (bg_eval_mfma.h)
    uint4 *d_wl3[2] = {nullptr, nullptr};  // bf16 hi | mid | lo split, bf16 MFMA layout x 3 (root term, rounds 1-4; -DBG_ROOT_F16X2=0)
    uint4 *d_wr2[2] = {nullptr, nullptr};  // f16 hi | lo split in the same layout (the root pass, bg_root_resident.h)
    uint4 *d_wl16[2] = {nullptr, nullptr}; // bf16 MFMA layout [13][4][64] x 8 bf16
    uint4 *d_wlx2[2] = {nullptr, nullptr}; // f16 hi | lo split, same layout twice
    uint4 *d_wd16[2] = {nullptr, nullptr}; // the same split with -log2(e) and b1 folded in: the register-resident dense kernel (bg_eval_dense16.h)
    uint2 *d_lut = nullptr;                // count -> 4 bf16 features
    uint2 *d_lut16 = nullptr;              // count -> 4 f16 features
    bool wm_ok[2] = {false, false};        // the slot's d_wm fits f16 (else the VALU delta kernel evaluates that slot)
    bool has_weights[2] = {false, false};
    const float *b1(int slot) const { return d_w[slot] + N_HID * N_IN; }      // the fp32 tail of the raw weights: b1 [N_HID], W2 [N_HID], b2 [1]
    const float *w2(int slot) const { return b1(slot) + N_HID; }
    const float *b2(int slot) const { return w2(slot) + N_HID; }
    const uint4 *root_w(int slot) const { return ROOT_F16X2 ? d_wr2[slot] : d_wl3[slot]; }    // the root pass's W1 planes and LUT (bg_root_resident.h)
    const uint2 *root_lut() const { return ROOT_F16X2 ? d_lut16 : d_lut; }
};
// Fresh tables for an env that has its own: the list of (pointer, bytes), all or none.  A new table is its member above and its line
// here: one left out is never allocated and stays null, which its first kernel trips over at once.  d_wm and d_wd16 are members in both
// builds but listed, and so allocated, in the experimental build only: its kernels are their only readers.
static int net_tables_alloc(DevMem &mem, NetTables &t)
{
#define BOTH(member, bytes) BG_BUF(t.member[0], bytes), BG_BUF(t.member[1], bytes)
    return mem.alloc_group({
        BOTH(d_w, N_PARAMS * 4),            BOTH(d_wl, EVAL_LDS_BYTES),         BOTH(d_wt, DELTA_W_FLOATS * 4),
        BOTH(d_wl3, 3 * EVAL16_W_BYTES),    BOTH(d_wr2, 2 * EVAL16_W_BYTES),    BOTH(d_wl16, EVAL16_W_BYTES),
        BOTH(d_wlx2, EVAL16X2_W_BYTES),     BG_BUF(t.d_lut16, EVAL16_LUT_BYTES), BG_BUF(t.d_lut, EVAL16_LUT_BYTES),
#ifdef BGAMD_EXPERIMENTAL
        BOTH(d_wm, MD_W_BYTES),             BOTH(d_wd16, EVAL16X2_W_BYTES),
#endif
    });
#undef BOTH
}

// What the env remembers of its last search step: the read and info calls (bgamd_env_search_read / _info, bgamd_env_search3_read /
// _info) test it.  One assignment clears the record when a search call of any kind begins, one fills it when a step has succeeded: an
// analysis, a failed step and a mid env's searches leave every read refusing.
struct SearchResult {
    int k = -1;                            // K of the step (-1: none yet, or the last call failed or was no step)
    uint32_t min_searched = 1;             // the least kept count of a searched lane (bgamd_env_search_info)
    hipStream_t stream = nullptr;          // the step's stream: the info calls count on it
    bool deep = false;                     // it was a 3-ply step (bgamd_env_search3_read / _info)
    bool info_read = false, info3_read = false;            // the host copies below have been read
    int64_t info[4] = {0, 0, 0, 0};
    int64_t info3[6] = {0, 0, 0, 0, 0, 0};
};

// 2-ply search (bgamd_env_step_search, bg_search.h)
struct SearchState {
    uint32_t *cnt = nullptr, *off = nullptr, *fill = nullptr, *kept = nullptr, *koff = nullptr, *max = nullptr;  // per game (+1)
    uint32_t *grp = nullptr;               // [cap_rows] row indices grouped by game
    int32_t *rank = nullptr;               // [cap_rows]
    uint4 *c_rows = nullptr;               // candidates [c_cap][2]
    uint32_t *c_key = nullptr;
    float *c_v1 = nullptr, *c_v2 = nullptr, *c_rval = nullptr;     // c_rval [c_cap][21]
    long long c_cap = 0;
    // the filtered step (bg_filter.h): skept [n] = kept of the searched lanes (kept >= 2, else 0), soff [n + 1] its scan, vmap [c_cap] the
    // searched candidates' places in the candidate list; bgamd_env_search_info: d_info [4]
    uint32_t *skept = nullptr, *soff = nullptr, *vmap = nullptr;
    unsigned long long *d_info = nullptr;
    // the 3-ply step (bg_search3.h), allocated by the first one: dkept [n] = |L2| of the lanes searched deeper (else 0), doff [n + 1] its
    // scan; per candidate [d_cap] c_d3 (rank in L2 or -1), c_v3, dmap (the deep list), r3 [d_cap][21] the mid roots' values; d_info3 [6],
    // d_l3 the count of level-3 roots
    uint32_t *dkept = nullptr, *doff = nullptr, *dmap = nullptr;
    int32_t *c_d3 = nullptr;
    float *c_v3 = nullptr, *r3 = nullptr;
    unsigned long long *d_info3 = nullptr, *d_l3 = nullptr;
    long long d_cap = 0;
    float *pass_v1 = nullptr;              // a MID env's: [n] the value srch_collect_kernel forms per lane, the pass reply's v1
    SearchResult last;
};

// a search of the 3-ply step's mid env (SearchKind::MID): the mid lanes are mid roots v0 .. of r3; roots counts the level-3 virtual roots
struct Search3Mid {
    s3::DeepList deep;
    float *r3;
    long long v0;
    unsigned long long *roots;
};

// search log (bgamd_env_set_search_log, bg_search_log.h): the caller's buffers, [plies][n] each; rows NULL = no log
struct SearchLog {
    uint4 *rows = nullptr, *after = nullptr;
    float *target = nullptr, *v1 = nullptr;
    long long plies = 0;
};

// move analysis (bgamd_env_analyze_moves, bg_analysis.h): the per-lane results of the last one and its summary
struct AnalysisState {
    AnaView v{};
    double *summary = nullptr;             // [ANA_SUMMARY]
    bool ready = false;                    // an analysis has run and nothing has failed since (bgamd_env_analysis_read)
};

// What the env remembers of its last rollout call: the read calls (bgamd_env_rollout_*_read) test it.  One assignment clears `ok` when a
// call begins, one fills the record when it has succeeded; info / cube_info keep the numbers of the last call that did (with the cube).
struct RolloutResult {
    bool ok = false;                       // the last call succeeded; false: none yet, or it failed -- every read refuses, and only the infos below mean anything
    bool vr = false, cube = false, grouped = false;    // it had BGAMD_ROLLOUT_VR / the cube on / a group table (false: RolloutState::group is not read)
    long long P = 0, T = 0;
    cube::Rule cube_rule{};                // cube: the rule it was played under
    int64_t info[4] = {0, 0, 0, 0};        // bgamd_env_rollout_info
    int64_t cube_info[2] = {0, 0};         // bgamd_env_rollout_cube_info
    bool match = false;                    // it ran under a match (bgamd_env_rollout_match) whose tables are still the uploaded ones
};

// Monte Carlo rollouts (bgamd_env_rollout, bg_rollout.h), and what the luck-adjusted ones add (bg_vr.h)
struct RolloutState {
    uint4 *pos = nullptr, *fan = nullptr, *trows = nullptr;        // [cap_pos], [cap_fan], [cap_lanes]
    float *fval = nullptr, *tval = nullptr, *tv = nullptr;         // [cap_fan], [cap_trials], [cap_lanes]
    uint32_t *tturns = nullptr, *lane = nullptr, *tids = nullptr;  // [cap_trials], [cap_lanes], [cap_lanes]
    long long cap_pos = 0, cap_fan = 0, cap_trials = 0, cap_lanes = 0;
    unsigned long long *host = nullptr;    // pinned, [2][4] (done, truncated, rollout error bits, env error bits) of the last two reads
    hipEvent_t ev[2] = {nullptr, nullptr}; // ... and the event behind each of the two
    double *tluck = nullptr, *m0 = nullptr;                        // tluck [P T] luck totals, m0 [P] / f0 [P][21]: turn 0 (rotation)
    float *vf = nullptr, *f0 = nullptr;                            // vf [L][21]: the trial lanes' f of the turn at hand
    long long cap_vtrials = 0, cap_vlanes = 0, cap_vpos = 0;
    int32_t *group = nullptr;              // [cap_group] the group table of the last bgamd_env_rollout_grouped (bgamd_env_rollout_paired_read)
    long long cap_group = 0;
    // the doubling cube (bgamd_env_rollout_cube, bg_cube.h): ctrial [cap_ctrials] the trials' records, ceq [cap_ctrials] their cubeful
    // equities (left by the reduce launch that ends a cubeful rollout: bgamd_env_rollout_paired_read's which = 3), cstart [2 cap_cstart]
    // the env's copy of the start tables, cctr [2] the lane-turn counters
    cube::Trial *ctrial = nullptr;
    double *ceq = nullptr;
    uint32_t *cstart = nullptr;
    unsigned long long *cctr = nullptr;
    long long cap_ctrials = 0, cap_cstart = 0;
    // match play (bgamd_env_rollout_match, bg_match.h): mwords [cap_mwords] the positions' packed (away1, away2, state), cmwc [cap_mtrials]
    // the trials' MWC (left by the reduce launch that ends a rollout under a match: bgamd_env_rollout_paired_read's which = 4)
    uint32_t *mwords = nullptr;
    double *cmwc = nullptr;
    long long cap_mwords = 0, cap_mtrials = 0;
    RolloutResult last;
};
static_assert(cube::LANE_FINISHED == META_FINISHED && cube::LANE_NONE == RO_NONE && cube::WORD_TRUNC == RO_TRUNC &&
              cube::WORD_PTS_SHIFT == RO_PTS_SHIFT && cube::ROLLS == SRCH_ROLLS && ROLLOUT_ROLLS == SRCH_ROLLS && SEARCH_ROLLS == SRCH_ROLLS,
              "bg_cube.h, bg_rollout_plan.h and bg_search_plan.h restate these");

// pre-roll evaluation (bgamd_env_evaluate_preroll, bg_vr.h)
struct PrerollState {
    uint4 *rows = nullptr;                 // [cap] the positions
    float *f = nullptr;                    // [cap][21]
    long long cap = 0;
};

enum { A_INTAKE = RO_CTRS, A_WORDS = RO_CTRS + 2 };      // bgamd_env::a_ctr
}  // namespace

struct bgamd_env {
    int device = 0;
    DevMem mem;                            // owns every block of device (and pinned) memory the members below point at
    EnvView v{};
    StagedView sv{};
    RandomView rv{};
    NetTables net;                         // the value net's device tables (a scratch env: its parent's, see scratch_env)
    StepTuning tune;                       // the switches of the greedy step's dispatch (bg_step_plan.h), read at create
    int n_cu = 256;
    hipStream_t side = nullptr;            // second stream: the root pass of the value net runs beside the doubles plies
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;   //   (fork after roots_kernel, join before the incremental kernel)

    unsigned long long *tops_base = nullptr;   // [2][T_COUNT]; sv.tops points at the set of the last step
    // ring log of continuous self-play (bgamd_env_set_trajectory_ring): greedy steps log by env step; traj_step counts the steps logged
    uint4 *ring_rows = nullptr;
    unsigned short *ring_end = nullptr;
    long long ring_steps = 0;
    long long traj_step = 0;
    int32_t *d_scalar = nullptr;           // device staging of the scalar (host-argument) surface: args at [0..63], results behind
    void *d_tmp = nullptr;                 // ... and of its enumerate call (states | seq | len), grown on demand
    long long tmp_bytes = 0;
    int choice[4] = {0, 0, 0, 0};           // kernels of the last greedy step (bgamd_env_kernel_choice)
    // kernel timing
    unsigned timing = 0;                   // bit k: bracket kernel group k with HIP events
    unsigned timing_stride = 1;            // ... on every timing_stride-th launch of the group (an event pair costs ~4 us)
    unsigned timing_seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<hipEvent_t> ev;            // pairs
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    double t_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // The analysis features run the greedy step's kernels on internal envs (scratch_env): `scratch` holds the virtual roots the 2-ply search
    // and the pre-roll evaluation score, `rscratch` plays the rollout's trials.  Such an env has no tables of its own: its `net` is its parent's.
    bgamd_env *scratch = nullptr, *rscratch = nullptr;
    // the 3-ply step's mid env (bg_search3.h): one lane per (deep candidate, opponent roll), searched with `scratch` lent to it.  Created by
    // the first 3-ply step, with at most mid_chunk lanes (search3_chunk, bg_search_plan.h, of the test hook BGAMD_SEARCH3_CHUNK read then)
    bgamd_env *mid = nullptr;
    long long mid_chunk = 0;
    // [A_WORDS]: the rollout's counters (RoView::ctr), then the word that takes the bad-state bit of intake_positions -- one allocation, a
    // whole number of 16-byte units, so that the rollout's one fill launch clears both.  48 bytes, allocated with every env (env_allocate).
    unsigned long long *a_ctr = nullptr;
    SearchState srch;
    SearchLog slog;                        // set: search steps log into it, every other step is refused (bgamd_env_set_search_log)
    int ro_plies = 1, ro_top_k = 0;        // bgamd_env_rollout_policy: who plays the trials' turns (1 = the greedy step)
    float ro_margin = 0.0f;
    // bgamd_env_rollout_cube: the sticky cube setting (flags 0 = off) and the caller's start tables, read by the next rollout's intake
    int cube_flags = 0;
    cube::Rule cube_rule{0.70, 0.78, 1.0, 64u, 0, 0};
    const int32_t *cube_value = nullptr, *cube_owner = nullptr;
    // bgamd_env_rollout_match: the sticky match setting (flags 0 = off), the uploaded block (bg_match_plan.h, Layout) and the caller's
    // score tables, read by the next rollout's intake
    int match_flags = 0;
    double *match_blob[2] = {nullptr, nullptr};        // two blocks of the largest layout each: a setting is written into the one not in
    int match_cur = 0;                                 // force (match_cur) and put in force only once it is whole
    match::Table match_tab{};
    const int32_t *match_away1 = nullptr, *match_away2 = nullptr, *match_state = nullptr;
    AnalysisState ana;
    RolloutState ro;
    PrerollState pre;
    uint32_t *spread = nullptr;            // [5][n] per-lane words of bgamd_env_choice_spread (bg_health.h, SpreadView)
    bool greedy_stepped = false;           // a greedy step has been issued on this env: the arenas hold its rows
    // the sampled step (bg_sample.h), allocated by the first one: smp_words = [2] counters | [n] per-lane maxima, smp_score [cap_rows]
    unsigned long long *smp_words = nullptr;
    float *smp_score = nullptr;
    bool sampled = false;                  // a sampled step has been issued: bgamd_env_sample_info has something to read
    hipStream_t smp_stream = nullptr;      // ... on this stream
};

namespace {
#include "bg_sample.h"
#include "bg_search_log.h"
#include "bg_rollout_groups.h"

// The order of the kernels in the code object, which decides ~1 % of the greedy step.  Plain kernels are emitted in the order
// of their definitions, the kernel templates behind them in the order in which this file first names an instance -- and this list, ahead
// of every host function, is that first naming.  A new kernel is a template and its entry goes at the END of the list; nothing else about
// the layout of this file matters to the code object.  tests/test_kernel_order_cpu.py holds the outcome.
#define K(...) (const void *)&__VA_ARGS__
#define K_FUSED(G, DELAY) K(td_step_fused_kernel<true, G, DELAY>), K(td_step_fused_kernel<false, G, DELAY>)
#define K_FUSED_ALL(DELAY) K_FUSED(1, DELAY), K_FUSED(2, DELAY), K_FUSED(4, DELAY), K_FUSED(8, DELAY), K_FUSED(16, DELAY)
[[maybe_unused]] const void *const KERNEL_ORDER[] = {
    K(eval_rows_f32_kernel<false>),
#ifdef BGAMD_EXPERIMENTAL
    K(eval_rows_f32_kernel<true>),
#endif
    K(boundary_kernel<true>),
#ifdef BGAMD_EXPERIMENTAL
    K(eval_rows_d16_kernel<2>), K(expand_kernel<MODE_LEAF>),
#endif
    K(boundary_kernel<false>),
    K(ana_match_kernel<64>), K(ana_select_kernel<64>), K(ana_reduce_kernel<SRCH_NT>), K(ana_summary_kernel<ANA_SUM_NT>), K(ana_read_kernel<SRCH_NT>),
    K(pre_fanout_kernel<true>), K(pre_fanout_kernel<false>),
    K(ro_outcome_reduce_kernel<0>), K(outcomes_kernel<0>), K(env_outcomes_kernel<0>),
    K(td_forward_kernel<2, false>), K(td_forward_kernel<4, false>),
    K_FUSED_ALL(false),
    K(td_trace_pipe_kernel<true>), K(td_trace_pipe_kernel<false>),
    K(td_trace_wide_kernel<true, true>), K(td_trace_wide_kernel<false, true>), K(td_trace_wide_kernel<false, false>),
    K(td_trace_kernel<true>), K(td_trace_kernel<false>),
    K_FUSED_ALL(true),
    K(flt_select_kernel<64>), K(flt_vmap_kernel<SRCH_NT>), K(flt_fanout_kernel<SRCH_NT>), K(flt_reduce_kernel<SRCH_NT>), K(flt_info_kernel<1024>),
    K(sample_score_kernel<SRCH_NT>), K(sample_pick_kernel<SRCH_NT>),
    K(srch_log_kernel<SRCH_NT>),
    K(ro_group_intake_kernel<128>), K(ro_pair_reduce_kernel<64>),
};
#undef K_FUSED_ALL
#undef K_FUSED
#undef K

inline dim3 grid1(long long n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

int flush_events(bgamd_env *env)
{
    for (size_t i = 0; i < env->ev_used; ++i) {
        HIPCHK(hipEventSynchronize(env->ev[2 * i + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, env->ev[2 * i], env->ev[2 * i + 1]));
        env->t_ms[env->ev_kind[i]] += ms;
        env->t_n[env->ev_kind[i]] += 1;
    }
    env->ev_used = 0;
    return BGAMD_OK;
}

struct KTimer {
    bgamd_env *env; hipStream_t s; size_t slot; bool on;
    KTimer(bgamd_env *e, hipStream_t st, int kind) : env(e), s(st), slot(0), on((e->timing >> kind) & 1u)
    {
        if (on && e->timing_stride > 1) on = (e->timing_seen[kind]++ % e->timing_stride) == 0;
        if (!on) return;
        if (env->ev_used * 2 + 2 > env->ev.size()) {
            if (env->ev.size() >= 2 * 8192) { flush_events(env); }
            else {
                hipEvent_t x[2] = {nullptr, nullptr};
                if (hipEventCreate(&x[0]) != hipSuccess || hipEventCreate(&x[1]) != hipSuccess) {
                    if (x[0]) hipEventDestroy(x[0]);
                    on = false;                          // no event pair: this launch goes untimed
                    return;
                }
                env->ev.push_back(x[0]); env->ev.push_back(x[1]);
                env->ev_kind.push_back(0);
            }
        }
        if (env->ev_used * 2 + 2 > env->ev.size()) { on = false; return; }
        slot = env->ev_used;
        if (hipEventRecord(env->ev[2 * slot], s) != hipSuccess) { on = false; return; }
        env->ev_used++;
        env->ev_kind[slot] = kind;
    }
    // a pair whose second record failed would poison flush_events: record it on the null stream as a last resort
    ~KTimer() { if (on && hipEventRecord(env->ev[2 * slot + 1], s) != hipSuccess) hipEventRecord(env->ev[2 * slot + 1], nullptr); }
};
}  // namespace

extern "C" {

int bgamd_version(void) { return 200; }

#ifndef BGAMD_SRC_HASH
#define BGAMD_SRC_HASH "unknown"
#endif
// the marker lets the build script read the digest out of the file without loading it
const char *bgamd_source_hash(void) { static const char tag[] = "BGAMD_SRC_HASH=" BGAMD_SRC_HASH; return tag + 15; }

const char *bgamd_error_string(int code)
{
    switch (code) {
    case BGAMD_OK: return "ok";
    case BGAMD_E_INVALID: return "invalid argument";
    case BGAMD_E_HIP: return "HIP runtime error";
    case BGAMD_E_NODEVICE: return "no usable gfx950 device";
    case BGAMD_E_ARENA: return "candidate arena overflow";
    case BGAMD_E_STATE: return "state with |count| > 15";
    case BGAMD_E_NOWEIGHTS: return "weights not loaded";
    case BGAMD_E_DELTA: return "incremental value net: a row differs from its root in more features than a legal turn changes";
    case BGAMD_E_WEIGHTS: return "weights refused: a value is not finite or an fc1 weight is outside the f16 hi + lo range (|w| >= 65504)";
    default: return "unknown error";
    }
}
const char *bgamd_last_hip_error(void) { return g_hip_err.c_str(); }

int bgamd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int env_allocate(bgamd_env *env, int64_t n_games, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride,
                        int64_t arena_rows, bool borrows_weights);

static int env_create(bgamd_env **out, int64_t n_games, int device, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride,
                      int64_t arena_rows, bool borrows_weights);

int bgamd_env_create(bgamd_env **out, int64_t n_games, int device, uint64_t seed, uint64_t lane_offset,
                     uint64_t lane_stride, int64_t arena_rows)
{
    return env_create(out, n_games, device, seed, lane_offset, lane_stride, arena_rows, false);
}

// borrows_weights: a scratch env (scratch_env) -- no weight tables of its own, the parent's are assigned to it before every use
static int env_create(bgamd_env **out, int64_t n_games, int device, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride,
                      int64_t arena_rows, bool borrows_weights)
{
    if (!out || n_games <= 0 || n_games > (1ll << 30)) return BGAMD_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BGAMD_E_NODEVICE;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BGAMD_E_NODEVICE;
    bgamd_env *env = new bgamd_env();
    env->device = device;
    env->n_cu = prop.multiProcessorCount;
    // the one way out after a failure: the env goes, with whatever it had allocated, and the text of the failure (a copy) stays
    auto fail = [env](int rc, std::string why) { bgamd_env_destroy(env); g_hip_err = why; return rc; };
    int rc = env_allocate(env, n_games, seed, lane_offset, lane_stride, arena_rows, borrows_weights);
    if (rc == BGAMD_OK) rc = bgamd_env_reset(env, nullptr);
    if (rc != BGAMD_OK) return fail(rc, g_hip_err);
    env->tune = step_tuning_from_env(getenv, EXPERIMENTAL_BUILD, n_games);
    if (hipStreamCreateWithFlags(&env->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&env->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&env->ev_join, hipEventDisableTiming) != hipSuccess)
        return fail(BGAMD_E_HIP, "side stream / events");
    *out = env;
    return BGAMD_OK;
}

static int env_allocate(bgamd_env *env, int64_t n_games, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride,
                        int64_t arena_rows, bool borrows_weights)
{
    EnvView &v = env->v;
    v.n = n_games; v.seed = seed; v.lane_offset = lane_offset; v.lane_stride = lane_stride ? lane_stride : (uint64_t)n_games;
    long long cap = arena_rows > 0 ? arena_rows : n_games * 256;
    if (cap < 65536) cap = 65536;
    if (cap > (1ll << 31) - 64) cap = (1ll << 31) - 64;
    v.cap = cap;
    const size_t n = (size_t)n_games, rows = (size_t)cap;
    if (int rc = env->mem.alloc_group({BG_BUF(v.planes, n * 8 * 4), BG_BUF(v.meta, n * 4), BG_BUF(v.ply, n * 4), BG_BUF(v.episode, n * 4),             // per lane
                                  BG_BUF(v.flags, n * 4), BG_BUF(v.cand_off, n * 4), BG_BUF(v.cand_cnt, n * 4), BG_BUF(v.chosen, n * 4),
                                  BG_BUF(v.chosen_seq, n * 4), BG_BUF(v.chosen_val, n * 4),
                                  BG_BUF(v.rows, rows * 32), BG_BUF(v.seqs, rows * 4), BG_BUF(v.values, rows * 4),                                 // per arena row
                                  BG_BUF(v.counters, C_COUNT * 8), BG_BUF(env->a_ctr, A_WORDS * 8)})) return rc;
    if (!borrows_weights)
        if (int rc = net_tables_alloc(env->mem, env->net)) return rc;
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_f16x2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, EVAL16X2_LDS_TOTAL));
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, EVAL16_LDS_TOTAL));
    {   // staged greedy step (bg_staged.h): node lists, per-workgroup staging, unique arena
        StagedView &sv = env->sv;
        const long long ng = n_games;
        sv.cap_d1 = ng * 15 < 4096 ? 4096 : ng * 15;
        sv.cap_d2 = ng * 64 < 4096 ? 4096 : ng * 64;
        sv.cap_f = ng * 256 < 16384 ? 16384 : ng * 256;
        sv.cap_f2 = sv.cap_f;
        sv.cap_rows = cap;
        sv.b_base = 0;
        sv.shards = 1;
        RandomView &rv = env->rv;                    // bounded random-policy step (bg_random_kernels.h): own task list and counter -- a step
        rv.cap = sv.cap_f;                           // boundary of a multi-step run reads the tasks while the next roots write sv.f
        if (int rc = env->mem.alloc_group({BG_BUF(sv.d1, (size_t)sv.cap_d1 * sizeof(Node)), BG_BUF(sv.d2, (size_t)sv.cap_d2 * sizeof(Node)),
                                      BG_BUF(sv.f, (size_t)sv.cap_f * sizeof(Node)), BG_BUF(sv.f2, (size_t)sv.cap_f2 * sizeof(Node)),
                                      BG_BUF(sv.u_rows, rows * 32), BG_BUF(sv.u_info, rows * sizeof(uint2)),
                                      BG_BUF(sv.best, n * 8), BG_BUF(sv.root_rows, n * 32), BG_BUF(sv.root_hidden, n * N_HID * 4),
                                      BG_BUF(sv.tops, 2 * T_COUNT * 8),         // two sets: consecutive steps of a run alternate
                                      BG_BUF(rv.tasks, (size_t)rv.cap * sizeof(Node)), BG_BUF(rv.top, 8),
                                      BG_BUF(rv.task_count, (size_t)rv.cap * 4), BG_BUF(rv.task_off, n * 4), BG_BUF(rv.task_n, n * 4),
                                      BG_BUF(env->spread, n * 5 * 4)})) return rc;
        env->tops_base = sv.tops;
        // an overflowing step (flagged, raised by stats) leaves holes in the arena: they must name a valid game
        HIPCHK(hipMemset(sv.u_rows, 0, rows * 32));
        HIPCHK(hipMemset(sv.u_info, 0, rows * sizeof(uint2)));
        HIPCHK(hipMemset(sv.tops, 0, 2 * T_COUNT * 8));
        HIPCHK(hipMemset(rv.top, 0, 8));
    }
    HIPCHK(hipMemset(v.counters, 0, C_COUNT * 8));
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_f32_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, EVAL_LDS_TOTAL));
#ifdef BGAMD_EXPERIMENTAL
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_f32_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, EVAL_LDS_TOTAL));
#endif
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_delta_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DELTA_LDS_TOTAL));
    HIPCHK(hipFuncSetAttribute((const void *)boundary_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, BROOT_LDS_BYTES));
#ifdef BGAMD_EXPERIMENTAL
    HIPCHK(hipFuncSetAttribute((const void *)eval_rows_mdelta_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MD_LDS_TOTAL));
    HIPCHK(hipFuncSetAttribute((const void *)root_hidden_bf16x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ROOT3_LDS_TOTAL));
#endif
    return BGAMD_OK;
}

int bgamd_env_destroy(bgamd_env *env)
{
    ENV_GUARD(env);
    hipDeviceSynchronize();
    if (env->scratch) bgamd_env_destroy(env->scratch);            // (on this device too; each frees what its own owner handed out)
    if (env->rscratch) bgamd_env_destroy(env->rscratch);
    if (env->mid) bgamd_env_destroy(env->mid);
    env->mem.release_all();
    for (hipEvent_t e : env->ev) hipEventDestroy(e);
    for (hipEvent_t e : {env->ev_fork, env->ev_join, env->ro.ev[0], env->ro.ev[1]}) if (e) hipEventDestroy(e);
    if (env->side) hipStreamDestroy(env->side);
    delete env;
    return BGAMD_OK;
}

int64_t bgamd_env_num_games(const bgamd_env *env) { return env ? env->v.n : 0; }

int bgamd_env_reset(bgamd_env *env, void *stream)
{
    ENV_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(reset_kernel, grid1(env->v.n, 256), dim3(256), 0, s, env->v, (const int32_t *)nullptr, 0u);
    HIPCHK(hipMemsetAsync(env->v.counters, 0, C_COUNT * 8, s));
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_reset_episode(bgamd_env *env, uint32_t episode, void *stream)
{
    ENV_GUARD(env);
    hipLaunchKernelGGL(reset_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, (const int32_t *)nullptr, episode);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_reseed(bgamd_env *env, uint64_t seed, uint64_t lane_offset, uint64_t lane_stride, void *stream)
{
    ENV_GUARD(env);
    env->v.seed = seed;
    env->v.lane_offset = lane_offset;
    env->v.lane_stride = lane_stride ? lane_stride : (uint64_t)env->v.n;
    return bgamd_env_reset_episode(env, 0u, stream);
}

int bgamd_env_reset_lanes(bgamd_env *env, const int32_t *d_mask, void *stream)
{
    if (!env || !d_mask) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(reset_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, d_mask, 0u);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_set_states(bgamd_env *env, const int32_t *d_states28, const int32_t *d_turn, void *stream)
{
    if (!env || (!d_states28 && !d_turn)) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(set_states_kernel, grid1(env->v.n, 128), dim3(128), 0, (hipStream_t)stream, env->v, d_states28, d_turn);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_get_states(bgamd_env *env, int32_t *d_states28, int32_t *d_turn, void *stream)
{
    ENV_GUARD(env);
    hipLaunchKernelGGL(get_states_kernel, grid1(env->v.n, 128), dim3(128), 0, (hipStream_t)stream, env->v, d_states28, d_turn);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_get_flags(bgamd_env *env, int32_t *d_flags, void *stream)
{
    if (!env || !d_flags) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(get_flags_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, d_flags);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_snapshot(bgamd_env *env, int32_t *d_out, void *stream)
{
    if (!env || !d_out) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(snapshot_kernel, grid1(env->v.n, 128), dim3(128), 0, (hipStream_t)stream, env->v, d_out);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// ---- scalar surface with host arguments (one-lane envs) ----
static int launch_emit(bgamd_env *env, int flags, int with_seq, const int32_t *ov_player, const int32_t *ov_dice, hipStream_t s);
static int check_err_flags(bgamd_env *env, unsigned long long f);
static int scalar_guard(bgamd_env *env)
{
    if (!env || env->v.n != 1) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    return env->d_scalar ? BGAMD_OK : env->mem.alloc(BG_BUF(env->d_scalar, 1024 * 4));
}

int bgamd_game_snapshot(bgamd_env *env, int32_t h_out[32])
{
    int rc = scalar_guard(env);
    if (rc || !h_out) return rc ? rc : BGAMD_E_INVALID;
    hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(64), 0, nullptr, env->v, env->d_scalar + 64);
    HIPCHK(hipMemcpy(h_out, env->d_scalar + 64, 32 * 4, hipMemcpyDeviceToHost));
    return BGAMD_OK;
}

int bgamd_game_set_state(bgamd_env *env, const int32_t *h_state28, int turn)
{
    int rc = scalar_guard(env);
    if (rc || (!h_state28 && turn < 0)) return rc ? rc : BGAMD_E_INVALID;
    int32_t h[29];
    if (h_state28) memcpy(h, h_state28, 28 * 4);
    h[28] = turn;
    HIPCHK(hipMemcpy(env->d_scalar, h, 29 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(set_states_kernel, dim3(1), dim3(64), 0, nullptr, env->v, h_state28 ? (const int32_t *)env->d_scalar : nullptr,
                       turn >= 0 ? (const int32_t *)(env->d_scalar + 28) : nullptr);
    HIPCHK(hipDeviceSynchronize());
    return BGAMD_OK;
}

int bgamd_game_set_dice(bgamd_env *env, int d1, int d2)
{
    int rc = scalar_guard(env);
    if (rc) return rc;
    const int32_t h[2] = {d1, d2};
    HIPCHK(hipMemcpy(env->d_scalar, h, 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dice_kernel, dim3(1), dim3(64), 0, nullptr, env->v, (const int32_t *)env->d_scalar, (int32_t *)nullptr, 0);
    HIPCHK(hipDeviceSynchronize());
    return BGAMD_OK;
}

int bgamd_game_roll(bgamd_env *env, int32_t h_dice[2])
{
    int rc = scalar_guard(env);
    if (rc || !h_dice) return rc ? rc : BGAMD_E_INVALID;
    hipLaunchKernelGGL(dice_kernel, dim3(1), dim3(64), 0, nullptr, env->v, (const int32_t *)nullptr, env->d_scalar + 64, 2);
    HIPCHK(hipMemcpy(h_dice, env->d_scalar + 64, 8, hipMemcpyDeviceToHost));
    return BGAMD_OK;
}

int bgamd_game_legal_moves(bgamd_env *env, int player, int die, int8_t *h_pairs)
{
    int rc = scalar_guard(env);
    if (rc || !h_pairs) return rc ? rc : BGAMD_E_INVALID;
    const int32_t h[2] = {player, die};
    HIPCHK(hipMemcpy(env->d_scalar, h, 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(legal_moves_kernel, dim3(1), dim3(64), 0, nullptr, env->v, (const int32_t *)env->d_scalar, (const int32_t *)(env->d_scalar + 1),
                       env->d_scalar + 64, (int8_t *)(env->d_scalar + 80));
    int32_t out[1 + 13];
    HIPCHK(hipMemcpy(out, env->d_scalar + 64, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_pairs, env->d_scalar + 80, 52, hipMemcpyDeviceToHost));
    return out[0];
}

int bgamd_game_try_move(bgamd_env *env, int player, int dice, int origin, int dest)
{
    int rc = scalar_guard(env);
    if (rc) return rc;
    const int32_t h[4] = {player, dice, origin, dest};
    HIPCHK(hipMemcpy(env->d_scalar, h, 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(try_move_kernel, dim3(1), dim3(64), 0, nullptr, env->v, (const int32_t *)env->d_scalar, (const int32_t *)(env->d_scalar + 1),
                       (const int32_t *)(env->d_scalar + 2), (const int32_t *)(env->d_scalar + 3), env->d_scalar + 64);
    int32_t code = 0;
    HIPCHK(hipMemcpy(&code, env->d_scalar + 64, 4, hipMemcpyDeviceToHost));
    return code;
}

int64_t bgamd_game_enumerate(bgamd_env *env, int player, int d1, int d2, int32_t *h_states28, int8_t *h_seq, int32_t *h_len, int64_t cap)
{
    int rc = scalar_guard(env);
    if (rc || cap < 0) return rc ? rc : BGAMD_E_INVALID;
    const int32_t h[3] = {player, d1, d2};
    HIPCHK(hipMemcpy(env->d_scalar, h, 12, hipMemcpyHostToDevice));
    rc = launch_emit(env, 0, 1, (const int32_t *)env->d_scalar, (const int32_t *)(env->d_scalar + 1), nullptr);
    if (rc) return rc;
    unsigned long long hc[C_COUNT];
    HIPCHK(hipMemcpy(hc, env->v.counters, sizeof hc, hipMemcpyDeviceToHost));
    rc = check_err_flags(env, hc[C_ERR]);
    if (rc) return rc;
    const long long C = (long long)hc[C_ARENA_TOP];
    const long long m = C < cap ? C : cap;
    if (m > 0 && (h_states28 || h_seq || h_len)) {
        if ((rc = env->mem.grow(m * (28 * 4 + 8 + 4), env->tmp_bytes, {BG_BUF(env->d_tmp, 1)}))) return rc;
        int32_t *d_st = (int32_t *)env->d_tmp;
        int32_t *d_len = d_st + (size_t)m * 28;
        int8_t *d_seq = (int8_t *)(d_len + m);
        hipLaunchKernelGGL(rows_read_kernel, grid1(m, 128), dim3(128), 0, nullptr, env->v.rows, env->v.seqs, 0ll, m, d_st, d_seq, d_len);
        if (h_states28) HIPCHK(hipMemcpy(h_states28, d_st, (size_t)m * 28 * 4, hipMemcpyDeviceToHost));
        if (h_len) HIPCHK(hipMemcpy(h_len, d_len, (size_t)m * 4, hipMemcpyDeviceToHost));
        if (h_seq) HIPCHK(hipMemcpy(h_seq, d_seq, (size_t)m * 8, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipGetLastError());
    return (int64_t)C;
}

int bgamd_env_set_dice(bgamd_env *env, const int32_t *d_dice, void *stream)
{
    if (!env || !d_dice) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(dice_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, d_dice, (int32_t *)nullptr, 0);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}
int bgamd_env_get_dice(bgamd_env *env, int32_t *d_dice, void *stream)
{
    if (!env || !d_dice) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(dice_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, (const int32_t *)nullptr, d_dice, 0);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}
int bgamd_env_roll(bgamd_env *env, int advance_ply, void *stream)
{
    ENV_GUARD(env);
    hipLaunchKernelGGL(dice_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, (const int32_t *)nullptr, (int32_t *)nullptr, advance_ply ? 2 : 1);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

static int launch_emit(bgamd_env *env, int flags, int with_seq, const int32_t *ov_player, const int32_t *ov_dice, hipStream_t s)
{
    HIPCHK(hipMemsetAsync(&env->v.counters[C_ARENA_TOP], 0, 8, s));
    {
        KTimer t(env, s, 0);
        hipLaunchKernelGGL(emit_kernel, grid1(env->v.n, 64), dim3(64), 0, s, env->v, flags, with_seq, ov_player, ov_dice);
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_enumerate(bgamd_env *env, const int32_t *d_player, const int32_t *d_dice, void *stream)
{
    ENV_GUARD(env);
    return launch_emit(env, 0, 1, d_player, d_dice, (hipStream_t)stream);
}

static int check_err_flags(bgamd_env *env, unsigned long long f)
{
    (void)env;
    if (f & ERRF_ARENA) return BGAMD_E_ARENA;
    if (f & ERRF_STATE) return BGAMD_E_STATE;
    if (f & ERRF_DELTA) return BGAMD_E_DELTA;
    return BGAMD_OK;
}

int64_t bgamd_env_candidates_info(bgamd_env *env, int64_t *d_offsets, int32_t *d_counts, void *stream)
{
    ENV_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cand_info_kernel, grid1(env->v.n, 256), dim3(256), 0, s, env->v, d_offsets, d_counts);
    unsigned long long h[C_COUNT];
    HIPCHK(hipMemcpyAsync(h, env->v.counters, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int rc = check_err_flags(env, h[C_ERR]);
    if (rc) return rc;
    return (int64_t)h[C_ARENA_TOP];
}

int bgamd_env_candidates_read(bgamd_env *env, int64_t first, int64_t n_rows, int32_t *d_states28, int8_t *d_seq,
                              int32_t *d_seq_len, void *stream)
{
    if (!env || first < 0 || n_rows < 0 || first + n_rows > env->v.cap) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    if (n_rows == 0) return BGAMD_OK;
    hipLaunchKernelGGL(rows_read_kernel, grid1(n_rows, 128), dim3(128), 0, (hipStream_t)stream, env->v.rows, env->v.seqs,
                       (long long)first, (long long)n_rows, d_states28, d_seq, d_seq_len);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_step_random(bgamd_env *env, int flags, const uint32_t *d_choice_u32, void *stream)
{
    ENV_GUARD(env);
    if (env->slog.rows) return BGAMD_E_INVALID;                      // a search log is set: no step but the search's (no hole in a log)
    hipStream_t s = (hipStream_t)stream;
    const long long n = env->v.n;
    HIPCHK(hipMemsetAsync(env->rv.top, 0, 8, s));
    {
        KTimer t(env, s, 3);
        hipLaunchKernelGGL(rnd_tasks_kernel, grid1(n, 256), dim3(256), 0, s, env->v, env->rv, flags, -1.0f);
        hipLaunchKernelGGL(rnd_count_kernel, dim3((unsigned)rnd_count_grid(n * 64, env->n_cu)), dim3(256), 0, s, env->v, env->rv);
        hipLaunchKernelGGL(rnd_select_kernel, grid1(n, 256), dim3(256), 0, s, env->v, env->rv, flags, d_choice_u32);
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// the whole-tree walk (one lane per game, count pass + select pass); kept as the reference implementation of
// the bounded kernels above -- tests compare the two
int bgamd_env_step_random_walk(bgamd_env *env, int flags, const uint32_t *d_choice_u32, void *stream)
{
    ENV_GUARD(env);
    if (env->slog.rows) return BGAMD_E_INVALID;                      // (as bgamd_env_step_random)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(step_random_kernel, grid1(env->v.n, 64), dim3(64), 0, s, env->v, flags, d_choice_u32);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_load_weights(bgamd_env *env, const float *h_weights) { return bgamd_env_load_weights_slot(env, 0, h_weights); }

// host only: do the 25 601 floats survive the value net's weight layouts?  (b1, W2, b2 stay fp32: they must be finite; W1 must fit the
// f16 hi + lo planes of the root pass, bg_root_resident.h)
int bgamd_weights_check(const float *h_weights)
{
    if (!h_weights) return BGAMD_E_INVALID;
    for (int i = N_HID * N_IN; i < N_PARAMS; ++i)
        if (!(h_weights[i] - h_weights[i] == 0.0f)) return BGAMD_E_WEIGHTS;
    std::vector<uint16_t> planes((size_t)3 * K16_STEPS * 4 * 64 * 8);
    return relayout_w1_f16x2_root(h_weights, planes.data()) < 0 ? BGAMD_E_WEIGHTS : BGAMD_OK;
}

int bgamd_env_load_weights_slot(bgamd_env *env, int slot, const float *h_weights)
{
    if (!env || !h_weights || slot < 0 || slot > 1) return BGAMD_E_INVALID;
    if (int rc = bgamd_weights_check(h_weights)) return rc;      // before anything of the slot is overwritten
    HIPCHK(hipSetDevice(env->device));
    std::vector<float> wl((size_t)K_STEPS * 64 * 4);
    relayout_w1_f32(h_weights, wl.data());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(env->net.d_w[slot], h_weights, N_PARAMS * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(env->net.d_wl[slot], wl.data(), EVAL_LDS_BYTES, hipMemcpyHostToDevice));
    std::vector<float> wt((size_t)DELTA_W_FLOATS);
    relayout_w1_delta(h_weights, wt.data());
    HIPCHK(hipMemcpy(env->net.d_wt[slot], wt.data(), DELTA_W_FLOATS * 4, hipMemcpyHostToDevice));
#ifdef BGAMD_EXPERIMENTAL
    std::vector<uint32_t> wmd((size_t)MD_W_DWORDS);
    env->net.wm_ok[slot] = relayout_w1_mdelta(h_weights, wmd.data()) >= 0;
    HIPCHK(hipMemcpy(env->net.d_wm[slot], wmd.data(), MD_W_BYTES, hipMemcpyHostToDevice));
#endif
    std::vector<uint16_t> wl3((size_t)3 * K16_STEPS * 4 * 64 * 8);
    relayout_w1_bf16x3(h_weights, wl3.data());
    HIPCHK(hipMemcpy(env->net.d_wl3[slot], wl3.data(), 3 * EVAL16_W_BYTES, hipMemcpyHostToDevice));
    relayout_w1_f16x2_root(h_weights, wl3.data());
    HIPCHK(hipMemcpy(env->net.d_wr2[slot], wl3.data(), 2 * EVAL16_W_BYTES, hipMemcpyHostToDevice));
    std::vector<uint16_t> wl16((size_t)K16_STEPS * 4 * 64 * 8);
    relayout_w1_bf16(h_weights, wl16.data());
    uint32_t lut[32];
    make_count_lut(lut);
    HIPCHK(hipMemcpy(env->net.d_wl16[slot], wl16.data(), EVAL16_W_BYTES, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(env->net.d_lut, lut, EVAL16_LUT_BYTES, hipMemcpyHostToDevice));
    std::vector<uint16_t> wx2((size_t)2 * K16_STEPS * 4 * 64 * 8);
    relayout_w1_f16x2(h_weights, wx2.data());
    make_count_lut_f16(lut);
    HIPCHK(hipMemcpy(env->net.d_wlx2[slot], wx2.data(), EVAL16X2_W_BYTES, hipMemcpyHostToDevice));
#ifdef BGAMD_EXPERIMENTAL
    relayout_w1_d16(h_weights, wx2.data());
    HIPCHK(hipMemcpy(env->net.d_wd16[slot], wx2.data(), EVAL16X2_W_BYTES, hipMemcpyHostToDevice));
#endif
    HIPCHK(hipMemcpy(env->net.d_lut16, lut, EVAL16_LUT_BYTES, hipMemcpyHostToDevice));
    env->net.has_weights[slot] = true;
    return BGAMD_OK;
}

// The dense evaluators over n_rows_imm rows, or over *n_rows_ptr (<= n_rows_imm) of them.  g: eval_grids of the rows expected -- of
// n_rows_imm, or, when the count is on the device, of a greedy step's worth of the env's lanes (StepPlan::eval)
static int launch_eval(bgamd_env *env, int slot, int precision, const EvalGrids &g, const unsigned long long *n_rows_ptr, long long n_rows_imm,
                       const uint4 *rows, float *values, const uint2 *info, unsigned long long *best, hipStream_t s)
{
    if (!env->net.has_weights[slot]) return BGAMD_E_NOWEIGHTS;
    if (precision != BGAMD_F32 && precision != BGAMD_BF16 && precision != BGAMD_F16X2 && precision != BGAMD_F32_DENSE)
        return BGAMD_E_INVALID;
    const NetTables &t = env->net;
    const float *b1 = t.b1(slot), *w2 = t.w2(slot), *b2 = t.b2(slot);
    unsigned long long *rows_ctr = n_rows_ptr ? &env->v.counters[C_ROWS_EVAL] : nullptr, *ksteps = n_rows_ptr ? &env->v.counters[C_KSTEPS] : nullptr;
    const dim3 egrid((unsigned)g.lds);
    KTimer timer(env, s, 1);
#ifdef BGAMD_EXPERIMENTAL
    if (precision == BGAMD_F16X2 && env->tune.d16)
        hipLaunchKernelGGL(eval_rows_d16_kernel<2>, dim3((unsigned)g.d16), dim3(D16_THREADS), D16_LDS_BYTES, s, rows, n_rows_ptr, n_rows_imm, rows_ctr,
                           (const uint4 *)t.d_wd16[slot], (const uint2 *)t.d_lut16, w2, b2, values, info, best, ksteps, (unsigned long long *)nullptr, 0);
    else
#endif
    if (precision == BGAMD_F16X2)
        hipLaunchKernelGGL(eval_rows_f16x2_kernel, egrid, dim3(EVAL_THREADS), EVAL16X2_LDS_TOTAL, s, rows, n_rows_ptr, n_rows_imm, rows_ctr,
                           (const uint4 *)t.d_wlx2[slot], (const uint2 *)t.d_lut16, b1, w2, b2, values, info, best);
    else if (precision == BGAMD_BF16)
        hipLaunchKernelGGL(eval_rows_bf16_kernel, egrid, dim3(EVAL_THREADS), EVAL16_LDS_TOTAL, s, rows, n_rows_ptr, n_rows_imm, rows_ctr,
                           (const uint4 *)t.d_wl16[slot], (const uint2 *)t.d_lut, b1, w2, b2, values, info, best);
    else
        hipLaunchKernelGGL(eval_rows_f32_kernel<false>, egrid, dim3(EVAL_THREADS), EVAL_LDS_TOTAL, s, rows, n_rows_ptr, n_rows_imm, rows_ctr,
                           (const float4 *)t.d_wl[slot], b1, w2, b2, values, info, best, ksteps);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// The incremental value net's root pass: hidden[n][N_HID] = W1 x + b1 of the n root rows, by the kernel `kind` names on `grid` workgroups
// (root_pass_kind, root_pass_grid: bg_step_plan.h)
static void launch_root_pass(bgamd_env *env, int slot, [[maybe_unused]] RootPass kind, long long grid, const uint4 *rows, long long n, float *hidden, hipStream_t s)
{
    const NetTables &t = env->net;
#ifdef BGAMD_EXPERIMENTAL
    if (kind == RootPass::F32_CHAIN)
        hipLaunchKernelGGL(eval_rows_f32_kernel<true>, dim3((unsigned)grid), dim3(EVAL_THREADS), EVAL_LDS_TOTAL, s, rows,
                           (const unsigned long long *)nullptr, n, (unsigned long long *)nullptr, (const float4 *)t.d_wl[slot], t.b1(slot),
                           t.w2(slot), t.b2(slot), hidden, (const uint2 *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr);
    else if (kind == RootPass::LDS_STAGED)
        hipLaunchKernelGGL(root_hidden_bf16x3_kernel, dim3((unsigned)grid), dim3(ROOT3_THREADS), ROOT3_LDS_TOTAL, s, rows, n,
                           (const uint4 *)t.d_wl3[slot], (const uint2 *)t.d_lut, t.b1(slot), hidden);
    else
#endif
    hipLaunchKernelGGL(root_hidden_resident_kernel, dim3((unsigned)grid), dim3(ROOTR_THREADS), ROOTR_LDS_BYTES, s, rows, n,
                       t.root_w(slot), t.root_lut(), t.b1(slot), hidden);
}

// The incremental value net over the rows of sv on `grid` workgroups (delta_grid, bg_step_plan.h).  A greedy step: *n_rows_ptr rows, in
// arenas of sv.b_base rows when that is set, and zero_words, the counter set to clear for the next roots (or NULL).  A caller with its
// own rows: n_rows_ptr NULL, n_rows_imm rows from 0, no counters.  mfma: eval_rows_mdelta_kernel (experimental build; one arena).
static void launch_delta(bgamd_env *env, int slot, [[maybe_unused]] bool mfma, long long grid, const StagedView &sv, const unsigned long long *n_rows_ptr,
                         long long n_rows_imm, float *values, unsigned long long *zero_words, hipStream_t s)
{
    const NetTables &t = env->net;
    unsigned long long *rows_ctr = n_rows_ptr ? &env->v.counters[C_ROWS_EVAL] : nullptr, *ksteps = n_rows_ptr ? &env->v.counters[C_KSTEPS] : nullptr;
    const int n_zero = n_rows_ptr ? (int)T_COUNT : 0;
#ifdef BGAMD_EXPERIMENTAL
    if (mfma)
        hipLaunchKernelGGL(eval_rows_mdelta_kernel, dim3((unsigned)grid), dim3(MD_THREADS), MD_LDS_TOTAL, s, (const uint4 *)sv.u_rows, n_rows_ptr, n_rows_imm,
                           rows_ctr, (const uint4 *)t.d_wm[slot], t.w2(slot), t.b2(slot), (const uint4 *)sv.root_rows, (const float *)sv.root_hidden, values,
                           (const uint2 *)sv.u_info, sv.best, ksteps, zero_words, n_zero, &env->v.counters[C_ERR], (unsigned long long)ERRF_DELTA);
    else
#endif
    hipLaunchKernelGGL(eval_rows_delta_kernel, dim3((unsigned)grid), dim3(DELTA_THREADS), DELTA_LDS_TOTAL, s, (const uint4 *)sv.u_rows, n_rows_ptr, n_rows_imm,
                       rows_ctr, (const float4 *)t.d_wt[slot], t.w2(slot), t.b2(slot), (const uint4 *)sv.root_rows, (const float *)sv.root_hidden, values,
                       (const uint2 *)sv.u_info, sv.best, ksteps, zero_words, n_zero, &env->v.counters[C_ERR], (unsigned long long)ERRF_DELTA,
                       sv.b_base > 0 ? (const unsigned long long *)&sv.tops[T_UB] : (const unsigned long long *)nullptr,
                       (long long)sv.b_base);                     // (the counters of arenas 1, 2, 3 follow one another from T_UB)
}

}  // extern "C"

// The sampled step's two passes (bg_sample.h) on s, between the value net and the apply
static void launch_sample_passes(bgamd_env *env, const EnvView &ev, const unsigned long long *tops, long long b_base, float temperature,
                                 const StepPlan &p, hipStream_t s)
{
    const long long n = ev.n, cap_rows = env->sv.cap_rows;
    const SampleView sm{env->smp_words + 2, env->smp_words, env->smp_score};
    hipMemsetAsync(sm.pick, 0, (size_t)n * 8, s);
    hipLaunchKernelGGL(sample_score_kernel<SRCH_NT>, dim3((unsigned)p.sample_score_grid), dim3(SRCH_NT), 0, s, ev, tops, b_base, cap_rows,
                       (const uint4 *)env->sv.u_rows, (const uint2 *)env->sv.u_info, (const float *)env->v.values,
                       (const unsigned long long *)env->sv.best, temperature, sm);
    hipLaunchKernelGGL(sample_pick_kernel<SRCH_NT>, dim3((unsigned)p.sample_pick_grid), dim3(SRCH_NT), 0, s, n, tops, b_base, cap_rows,
                       (const uint2 *)env->sv.u_info, (const float *)env->v.values, env->sv.best, sm);
}

namespace {
// The streams one greedy step is issued on: everything on `gen`, except the root pass of the incremental value net, which
// goes to `root` (the env's side stream when it overlaps the doubles plies, else the same stream).
// (A CU-partitioned variant -- move generation of one sub-batch on 64-128 masked CUs beside the value net of another on the
// rest -- was built on this and measured 2.2-4x SLOWER: the "latency-bound" stage kernels need every CU's wave slots,
// their time scales with 1/CUs.  profiles/r02_cu_partition_group_run.txt)
struct StepStreams {
    hipStream_t gen, root;
};

// State of a run of greedy steps on one env (what bgamd_env_run_greedy kept in locals)
struct GreedyRun {
    bgamd_env *env;
    int flags, slot, precision, parity = 0;
    float epsilon;
    float temperature = 0.0f;              // > 0: the sampled step (set after init() by bgamd_env_run_sampled, which passes epsilon 0)
    StepPlan plan;                         // what a step of this run launches, and how big (bg_step_plan.h)
    StagedView sv;
    EnvView ev;                            // the env's view as this run's launches take it (ring log: the slots of the step at hand)
    long long cur_step = 0;                // ring log: the env step being played
    bool root_ready = false;               // the boundary launch of the step before has already run this step's root pass
    bool first_of_run = true;              // no step since begin() (read by the BG_ABL_STEP timing ablation only)

    int init(bgamd_env *e, int fl, float eps, int prec)
    {
        env = e; flags = fl; epsilon = eps; precision = prec;
        slot = (fl & BGAMD_WEIGHTS_SLOT1) ? 1 : 0;
        if (!env->net.has_weights[slot]) return BGAMD_E_NOWEIGHTS;
        if (prec != BGAMD_F32 && prec != BGAMD_BF16 && prec != BGAMD_F16X2 && prec != BGAMD_F32_DENSE) return BGAMD_E_INVALID;
        plan = step_plan(env->tune, env->v.n, env->n_cu, env->sv.cap_rows, prec, env->net.wm_ok[slot]);
        sv = env->sv;
        sv.tops = env->tops_base;
        sv.b_base = plan.b_base;
        sv.shards = plan.shards;
        parity = 0;
        root_ready = false;
        ev = env->v;
        if (env->ring_rows) {
            // the ring log's contract (include/bgamd.h): every lane takes part in every logged step and restarts itself -- a game is the
            // `length` contiguous slots that end at its end record.  Anything else would make the game table point at other games' rows.
            if (!(fl & BGAMD_AUTO_RESET) || (fl & (BGAMD_ONLY_P1 | BGAMD_ONLY_P2))) return BGAMD_E_INVALID;
            ev.traj = env->ring_rows; ev.traj_plies = env->ring_steps; ev.traj_ring = env->ring_steps; ev.endrec = env->ring_end;
        }
        return BGAMD_OK;
    }
    // ring log: the roots about to be launched log env step traj_step (the step they begin)
    void next_log_slot()
    {
        if (!ev.traj_ring) return;
        cur_step = env->traj_step++;
        ev.log_slot = cur_step % ev.traj_ring;
    }
    // two sets of list counters: step t uses set t & 1.  Inside a run the apply of step t and the roots of step t+1
    // share one launch (boundary_kernel); the value-net kernel of step t clears the set those roots allocate from.
    int begin(hipStream_t s)
    {
        HIPCHK(hipMemsetAsync(env->tops_base, 0, 2 * T_COUNT * 8, s));
        KTimer t(env, s, 4);
        next_log_slot();
        hipLaunchKernelGGL(roots_kernel, grid1(env->v.n, LANE_NT), dim3(LANE_NT), 0, s, ev, sv, flags);
        first_of_run = true;
        return BGAMD_OK;
    }
    // The lanes of e as they stand, scored and not moved (the 2-ply search, the pre-roll evaluation): one greedy step's roots, expansion
    // and incremental value net with the weights of fl's slot on stream s, no apply launch -- e->sv.best and root_hidden are the caller's
    int score(bgamd_env *e, int fl, hipStream_t s)
    {
        int rc;
        if ((rc = init(e, fl, 0.0f, BGAMD_F32)) || (rc = begin(s))) return rc;
        return step(StepStreams{s, s}, false, true);
    }
    int step(const StepStreams &ss, bool more, bool score_only = false)
    {
        const long long n = env->v.n;
        hipStream_t s = ss.gen;
        const StepPlan &p = plan;
        const bool own_root_launch = bg::own_root_launch(p, root_ready);
        env->choice[0] = p.choice_eval;
        env->choice[1] = step_choice_root(p, root_ready);
        env->choice[2] = step_choice_forked(p, root_ready, ss.root != s) | (env->tune.expand_merged ? 2 : 0);
        if (own_root_launch) {
            // The value net's root pass (one dense W1 x + b1 per GAME) needs only the root rows the roots just wrote.
            // It runs on a second stream beside the doubles plies -- small latency-bound launches that leave
            // most of the chip idle -- and is joined before the incremental kernel.
            hipStream_t s2 = ss.root;
            if (s2 != s) {
                HIPCHK(hipEventRecord(env->ev_fork, s));
                HIPCHK(hipStreamWaitEvent(s2, env->ev_fork, 0));
            }
#if defined(BG_ABL_STEP) && (BG_ABL_STEP & 1)            // ablation (timing only: the values go stale): no root pass after a run's first step
            if (first_of_run)
#endif
            {
                KTimer t(env, s2, 6);
                launch_root_pass(env, slot, p.root, p.root_grid, (const uint4 *)sv.root_rows, n, sv.root_hidden, s2);
            }
            if (s2 != s) HIPCHK(hipEventRecord(env->ev_join, s2));
        }
        StagedView sv_next = sv;
        sv_next.tops = env->tops_base + (parity ^ 1) * T_COUNT;
#ifdef BGAMD_EXPERIMENTAL
        if (!env->tune.expand_merged) {                        // rounds 1-4's two launches (bit-identity reference)
            {
                KTimer t(env, s, 4);
                hipLaunchKernelGGL(doubles_kernel, dim3((unsigned)p.ply2_grid), dim3(expand_threads(MODE_PLY2)), 0, s, ev, sv);
            }
            {
                KTimer t(env, s, 5);
                hipLaunchKernelGGL(expand_kernel<MODE_LEAF>, dim3((unsigned)p.leaf_grid), dim3(expand_threads(MODE_LEAF)), 0, s, ev, sv);
            }
        } else
#endif
        {
            // one launch: the doubles turns' plies 2, 3 and leaf stage on the first workgroups, the non-doubles leaf stage on the others
            // (two 512-thread workgroups per CU are resident: one of each kind per CU at the default share)
            KTimer t(env, s, 5);
            hipLaunchKernelGGL(expand_all_kernel, dim3((unsigned)(p.xall_nd + p.xall_nl)), dim3(XALL_NT), 0, s, ev, sv, (unsigned)p.xall_nd,
                               (unsigned)env->tune.expand_dbl_npb, (unsigned)env->tune.expand_parts, more ? sv_next.tops : (unsigned long long *)nullptr,
                               (int)T_COUNT);
        }
        // inside a run the apply of this step and the roots of the next share a launch (StepPlan::fused_with_more)
        const bool fused = more && p.fused_with_more;
        if (p.incremental) {
            if (own_root_launch && ss.root != s) HIPCHK(hipStreamWaitEvent(s, env->ev_join, 0));
            KTimer t(env, s, 1);
            launch_delta(env, slot, p.mfma_delta, p.delta_grid, sv, &sv.tops[T_U], sv.cap_rows, env->v.values,
                         fused ? sv_next.tops : (unsigned long long *)nullptr, s);
        } else {
            const int rc = launch_eval(env, slot, precision, p.eval, &sv.tops[T_U], sv.cap_rows, sv.u_rows, env->v.values, sv.u_info, sv.best, s);
            if (rc) return rc;
        }
        // sampled step: sv.best[g] becomes the pack of the row drawn with probability ~ exp(value / T) (never for a scoring pass)
        if (temperature > 0.0f && !score_only) launch_sample_passes(env, ev, sv.tops, sv.b_base, temperature, p, s);
        ExploreView xv{env->rv.tasks, env->rv.task_count, env->rv.task_off, env->rv.task_n};
        if (epsilon > 0.0f) {                              // exploring lanes pick through their counted tasks (bounded work)
            KTimer t(env, s, 3);
            HIPCHK(hipMemsetAsync(env->rv.top, 0, 8, s));
            hipLaunchKernelGGL(rnd_tasks_kernel, grid1(n, 256), dim3(256), 0, s, ev, env->rv, flags & ~BGAMD_ROLL, epsilon);
            hipLaunchKernelGGL(rnd_count_kernel, dim3((unsigned)p.rnd_count_grid), dim3(256), 0, s, ev, env->rv);
        }
        if (!score_only) {
            KTimer t(env, s, 2);
            ev.end_slot = ev.traj_ring ? cur_step % ev.traj_ring : 0;      // the apply half closes the step the last roots began
            if (fused) {
                next_log_slot();                                           // ... and the roots half begins the next one
                root_ready = p.root_in_boundary;
                if (root_ready)
                    hipLaunchKernelGGL(boundary_kernel<true>, grid1(n, BROOT_GPW), dim3(LANE_NT), BROOT_LDS_BYTES, s, ev, sv, sv_next, xv, flags, epsilon,
                                       env->net.root_w(slot), env->net.root_lut(), env->net.b1(slot));
                else
                    hipLaunchKernelGGL(boundary_kernel<false>, grid1(n, LANE_NT), dim3(LANE_NT), 0, s, ev, sv, sv_next, xv, flags, epsilon,
                                       (const uint4 *)nullptr, (const uint2 *)nullptr, (const float *)nullptr);
            } else {
                root_ready = false;
                hipLaunchKernelGGL(apply_kernel, grid1(n, LANE_NT), dim3(LANE_NT), 0, s, ev, sv, xv, flags, epsilon);
            }
        }
        env->sv.tops = sv.tops;                                // the set whose T_U describes the last evaluated rows
        env->sv.b_base = sv.b_base;
        first_of_run = false;
        if (fused) { parity ^= 1; sv = sv_next; }
        else if (more) {                                       // dense value-net modes: plain per-step sequence
            HIPCHK(hipMemsetAsync(sv.tops, 0, T_COUNT * 8, s));
            KTimer t(env, s, 4);
            next_log_slot();
            hipLaunchKernelGGL(roots_kernel, grid1(n, LANE_NT), dim3(LANE_NT), 0, s, ev, sv, flags);
        }
        return BGAMD_OK;
    }
};

// One scoring pass over the virtual lanes 0 .. n_virtual, a scratch env's worth at a time (env->scratch: ready, see scratch_env).
// seed(lanes, v0) launches the kernel that makes the virtual lanes from v0 on the lanes of that env; they are scored as a greedy step
// scores its roots, and srch_collect_kernel writes out[v] of every virtual lane v that has a score: out is [n_virtual / 21][21].
template <class Seed>
int score_virtual_lanes(bgamd_env *env, int slot, long long n_virtual, const Seed &seed, float *out, hipStream_t s)
{
    bgamd_env *sc = env->scratch;
    for (long long v0 = 0; v0 < n_virtual; v0 += sc->v.n) {
        seed(sc->v, v0);
        GreedyRun sr;
        if (int rc = sr.score(sc, slot ? BGAMD_WEIGHTS_SLOT1 : 0, s)) return rc;
        hipLaunchKernelGGL(srch_collect_kernel, grid1(sc->v.n, SRCH_NT), dim3(SRCH_NT), 0, s, sc->v, (const unsigned long long *)sc->sv.best,
                           (const float *)sc->sv.root_hidden, env->net.w2(slot), env->net.b2(slot), v0, out);
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// n_steps >= 1 steps of an initialised run on s: the first roots, the steps, the launch error check
int run_steps(GreedyRun &run, int64_t n_steps, hipStream_t s)
{
    bgamd_env *env = run.env;
    const StepStreams ss{s, (run.plan.incremental && env->tune.overlap) ? env->side : s};
    int rc = run.begin(s);
    if (rc) return rc;
    for (int64_t step = 0; step < n_steps; ++step) {
        rc = run.step(ss, step + 1 < n_steps);
        if (rc) return rc;
        env->greedy_stepped = true;
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

}  // namespace

extern "C" {

int bgamd_env_run_greedy(bgamd_env *env, int flags, float epsilon, int precision, int64_t n_steps, void *stream)
{
    if (!env || n_steps < 0) return BGAMD_E_INVALID;
    if (env->slog.rows) return BGAMD_E_INVALID;                      // a search log is set: no step but the search's (no hole in a log)
    HIPCHK(hipSetDevice(env->device));
    GreedyRun run;
    if (int rc = run.init(env, flags, epsilon, precision)) return rc;
    return n_steps == 0 ? BGAMD_OK : run_steps(run, n_steps, (hipStream_t)stream);
}

int bgamd_env_step_greedy(bgamd_env *env, int flags, float epsilon, int precision, void *stream)
{
    return bgamd_env_run_greedy(env, flags, epsilon, precision, 1, stream);
}

int bgamd_env_run_sampled(bgamd_env *env, int flags, float temperature, int precision, int64_t n_steps, void *stream)
{
    if (!env || n_steps < 0 || !(temperature >= 0.0f) || __builtin_isinf(temperature)) return BGAMD_E_INVALID;      // (NaN fails the >=)
    if (env->slog.rows) return BGAMD_E_INVALID;                      // (as bgamd_env_run_greedy)
    if (temperature == 0.0f) return bgamd_env_run_greedy(env, flags, 0.0f, precision, n_steps, stream);
    HIPCHK(hipSetDevice(env->device));
    GreedyRun run;
    int rc = run.init(env, flags, 0.0f, precision);
    if (rc) return rc;
    run.temperature = temperature;
    if (n_steps == 0) return BGAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!env->smp_words && (rc = env->mem.alloc_group({BG_BUF(env->smp_words, (size_t)(env->v.n + 2) * 8),
                                                       BG_BUF(env->smp_score, (size_t)env->sv.cap_rows * 4)}))) return rc;
    HIPCHK(hipMemsetAsync(env->smp_words, 0, 2 * 8, s));            // the two counters: sums over the steps of this call
    env->sampled = true;
    env->smp_stream = s;
    return run_steps(run, n_steps, s);
}

int bgamd_env_step_sampled(bgamd_env *env, int flags, float temperature, int precision, void *stream)
{
    return bgamd_env_run_sampled(env, flags, temperature, precision, 1, stream);
}

int bgamd_env_sample_info(bgamd_env *env, int64_t h_out[2])
{
    if (!env || !h_out || !env->sampled) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, env->smp_words, 2 * 8, hipMemcpyDeviceToHost, env->smp_stream));
    HIPCHK(hipStreamSynchronize(env->smp_stream));
    h_out[0] = (int64_t)h[0]; h_out[1] = (int64_t)h[1];
    return BGAMD_OK;
}

// ---- what the 2-ply search, the pre-roll evaluation and the rollouts share --------------------------------------------------------
// (SEARCH_CHUNK, the virtual lanes per scoring pass, and search_lanes: bg_search_plan.h)

// *which (env->scratch or env->rscratch) ready to use: an env on env's device with want_lanes lanes -- exactly that many (exact), else
// at least that many -- created, or after a wait for s re-created, when the one at hand does not do.  Leaves env's device current and
// the scratch env's weight tables those of env as they are now: a reload since the last call is seen.
static int scratch_env(bgamd_env *env, bgamd_env **which, long long want_lanes, bool exact, uint64_t lane_stride, hipStream_t s)
{
    bgamd_env *&sc = *which;
    if (sc && (exact ? sc->v.n != want_lanes : sc->v.n < want_lanes)) {
        HIPCHK(hipStreamSynchronize(s));
        bgamd_env_destroy(sc);
        sc = nullptr;
    }
    if (!sc) {
        const int rc = env_create(&sc, want_lanes, env->device, 0, 0, lane_stride, 0, true);
        if (rc) return rc;
        HIPCHK(hipDeviceSynchronize());                // (its reset ran on the null stream)
    }
    HIPCHK(hipSetDevice(env->device));
    sc->net = env->net;
    return BGAMD_OK;
}

// Caller-provided positions [n][28] (+ turn) as rows; a bad state is refused before anything is done with them (synchronises).
// PRECONDITION: the caller has cleared env->a_ctr[A_INTAKE] on s.  The clear is not done here because the rollout clears its own
// counters with the same fill (see bgamd_env::a_ctr) and then one more buffer before the pack: doing it here would add a launch to
// the rollout or reorder its launches.  The bad-state word is read into a pageable local; the synchronise below covers that copy.
// h_word: the whole word as read, for a caller that had another kernel flag something in it before this call (the grouped rollout).
static int intake_positions(bgamd_env *env, const int32_t *d_states28, const int32_t *d_turn, long long n, uint4 *rows, hipStream_t s,
                            unsigned long long *h_word = nullptr)
{
    unsigned long long h = 0;
    hipLaunchKernelGGL(pack_rows_kernel, grid1(n, 128), dim3(128), 0, s, d_states28, d_turn, n, rows, &env->a_ctr[A_INTAKE]);
    HIPCHK(hipMemcpyAsync(&h, &env->a_ctr[A_INTAKE], 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_word) *h_word = h;
    return (h & ERRF_STATE) ? BGAMD_E_STATE : BGAMD_OK;
}

// ---- 2-ply expectimax (bg_search.h), its filtered and 3-ply steps (bg_filter.h, bg_search3.h), the move analysis (bg_analysis.h) ------
namespace {
// the request of a search of env: the call's kind and first arguments, and what the env has been set to
SearchRequest search_request(const bgamd_env *env, SearchKind kind, int flags, int top_k, float margin = 0.0f)
{
    SearchRequest q{};
    q.kind = kind; q.flags = flags; q.top_k = top_k; q.margin = margin;
    q.n = env->v.n; q.cap_rows = env->sv.cap_rows;
    q.logs_steps = env->v.traj || env->ring_rows;
    q.has_search_log = env->slog.rows != nullptr;
    q.has_weights[0] = env->net.has_weights[0]; q.has_weights[1] = env->net.has_weights[1];
    return q;
}

// `inner` (a rollout's trial env, a 3-ply step's mid env) searched with owner's scratch env lent to it for the virtual roots: everything is
// stream-ordered, and a second env of up to SEARCH_CHUNK lanes would buy nothing.  No device is made current: owner's call has done that.
int search_lent(bgamd_env *owner, bgamd_env *inner, SearchKind kind, int flags, int top_k, float margin, const Search3Mid *mid, hipStream_t s);

// One search call after search_plan has decided it (bg_search_plan.h, plain C++, checked without a GPU: refusal, the select / fan-out /
// reduce rule, the read-back, the sizes): what the call kept in locals, and its stages in their order.  The step kinds end with the
// greedy step's own apply (terminal check, flip / auto-reset, counters, last_choice); the analysis and a mid env's search apply nothing.
struct SearchCall {
    bgamd_env *env;
    const SearchPlan &p;
    hipStream_t s;
    const int32_t *d_played;               // ANALYSIS: the played afterstates [n][28]
    const Search3Mid *mid;                 // MID: the mid roots this env's lanes are, and where their values go
    SearchState &se;                       // env->srch
    AnalysisState &an;                     // env->ana
    long long n;                           // env->v.n
    SearchSized z{};                       // known from list_lengths() on
    const uint2 *info = nullptr;           // the scored rows (from select() on)
    const uint4 *rows = nullptr;

    SearchCall(bgamd_env *e, const SearchPlan &plan, hipStream_t stream, const int32_t *played, const Search3Mid *m)
        : env(e), p(plan), s(stream), d_played(played), mid(m), se(e->srch), an(e->ana), n(e->v.n) {}

    int run()
    {
        se.last = SearchResult{};                          // until this call has succeeded as a step, every read refuses
        if (p.ending == SearchEnding::ANALYSIS) an.ready = false;
        int rc;
        if ((rc = buffers()) || (rc = score_roots()) || (rc = select()) || (rc = list_lengths()) || (rc = emit()) || (rc = score_replies()))
            return rc;
        switch (p.ending) {
        case SearchEnding::ANALYSIS: return end_analysis();
        case SearchEnding::MID: return end_mid();
        default: return end_step();
        }
    }
    int grow_candidates(long long rows_needed)
    {
        return env->mem.grow(rows_needed, se.c_cap, {BG_BUF(se.c_rows, 32), BG_BUF(se.c_key, 4), BG_BUF(se.c_v1, 4), BG_BUF(se.c_v2, 4),
                                                     BG_BUF(se.c_rval, 4 * SRCH_ROLLS), BG_BUF(se.vmap, 4)});
    }
    int buffers()
    {
        DevMem &mem = env->mem;
        int rc;
        if (p.ending == SearchEnding::ANALYSIS && !an.summary) {           // all or none: summary != NULL says that every buffer is there
            AnaView &v = an.v;
            const long long w = p.ana_word_bytes;
            if ((rc = mem.alloc_group({BG_BUF(v.status, w), BG_BUF(v.distinct, w), BG_BUF(v.rank1, w), BG_BUF(v.rank2, w), BG_BUF(v.v1_played, w),
                    BG_BUF(v.v1_best, w), BG_BUF(v.v2_played, w), BG_BUF(v.v2_best, w), BG_BUF(v.error, w), BG_BUF(v.best, p.ana_state_bytes),
                    BG_BUF(v.ppos, w), BG_BUF(v.pslot, w), BG_BUF(an.summary, ANA_SUMMARY * 8)}))) return rc;
        }
        if (!se.cnt) {                                     // all or none: cnt != NULL says that every buffer is there
            const long long per_game = p.per_game_bytes, per_row = p.per_row_bytes;
            if ((rc = mem.alloc_group({BG_BUF(se.cnt, per_game), BG_BUF(se.off, per_game), BG_BUF(se.fill, per_game), BG_BUF(se.kept, per_game),
                                       BG_BUF(se.koff, per_game), BG_BUF(se.skept, per_game), BG_BUF(se.soff, per_game),
                                       BG_BUF(se.max, 8), BG_BUF(se.d_info, 4 * 8), BG_BUF(se.grp, per_row), BG_BUF(se.rank, per_row)})))
                return rc;
        }
        return grow_candidates(p.cand_presize);            // (0: the list's length is read back first)
    }
    // stage A: the greedy step's roots, expansion and incremental value net, no apply
    int score_roots()
    {
        GreedyRun run;
        return run.score(env, p.flags, s);
    }
    // stage B: group by game, select
    int select()
    {
        const unsigned long long *tops = env->sv.tops;
        const long long bb = env->sv.b_base, cap_rows = env->sv.cap_rows;
        info = env->sv.u_info;
        rows = env->sv.u_rows;
        const dim3 rgrid((unsigned)(env->n_cu * 8));
        HIPCHK(hipMemsetAsync(se.cnt, 0, (size_t)n * 4, s));
        HIPCHK(hipMemsetAsync(se.fill, 0, (size_t)n * 4, s));
        hipLaunchKernelGGL(srch_count_kernel, rgrid, dim3(SRCH_NT), 0, s, tops, bb, cap_rows, info, se.cnt);
        hipLaunchKernelGGL(srch_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)se.cnt, se.off, n, (uint32_t *)nullptr);
        hipLaunchKernelGGL(srch_scatter_kernel, rgrid, dim3(SRCH_NT), 0, s, tops, bb, cap_rows, info, (const uint32_t *)se.off, se.fill, se.grp);
        if (p.match_played)
            hipLaunchKernelGGL(ana_match_kernel<64>, dim3((unsigned)n), dim3(64), 0, s, env->v, p.flags, d_played, (const uint32_t *)se.cnt,
                               (const uint32_t *)se.off, (const uint32_t *)se.grp, rows, info, an.v);
        switch (p.select) {
        case SearchSelect::ANALYSIS:
            hipLaunchKernelGGL(ana_select_kernel<64>, dim3((unsigned)n), dim3(64), 0, s, n, (const uint32_t *)se.cnt, (const uint32_t *)se.off,
                               (const uint32_t *)se.grp, rows, info, (const float *)env->v.values, p.k_lim, se.rank, se.kept, an.v);
            break;
        case SearchSelect::MARGIN:
            hipLaunchKernelGGL(flt_select_kernel<64>, dim3((unsigned)n), dim3(64), 0, s, n, (const uint32_t *)se.cnt, (const uint32_t *)se.off,
                               (const uint32_t *)se.grp, rows, info, (const float *)env->v.values, p.k_lim, p.margin, se.rank, se.kept, se.skept);
            break;
        case SearchSelect::PLAIN:
            hipLaunchKernelGGL(srch_select_kernel, dim3((unsigned)n), dim3(64), 0, s, n, (const uint32_t *)se.cnt, (const uint32_t *)se.off,
                               (const uint32_t *)se.grp, rows, info, (const float *)env->v.values, p.k_lim, se.rank, se.kept);
            break;
        }
        if (p.pass_replies)                                // a mid lane without rows keeps its pass reply
            s3::reply_fix(s, n, mid->v0, mid->deep, (const uint32_t *)se.cnt, se.kept);
        return BGAMD_OK;
    }
    // ... list the kept candidates (and the searched ones), and size what follows: read back, or known from the plan
    int list_lengths()
    {
        hipLaunchKernelGGL(srch_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)se.kept, se.koff, n, se.max);
        if (p.skip_singletons)
            hipLaunchKernelGGL(srch_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)se.skept, se.soff, n, (uint32_t *)nullptr);
        uint32_t h[3] = {0, 0, 0};
        if (p.read_back) {                                 // (the one synchronisation)
            HIPCHK(hipMemcpyAsync(&h[0], se.koff + n, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(&h[1], se.max, 4, hipMemcpyDeviceToHost, s));
            if (p.read_searched) HIPCHK(hipMemcpyAsync(&h[2], se.soff + n, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        z = search_sized(p, h[0], h[1], h[2]);
        int rc;
        if (p.read_back && (rc = grow_candidates(z.cand_rows))) return rc;
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    int emit()
    {
        hipLaunchKernelGGL(srch_emit_kernel, dim3((unsigned)n), dim3(64), 0, s, (const uint32_t *)se.cnt, (const uint32_t *)se.off,
                           (const uint32_t *)se.grp, rows, info, (const float *)env->v.values, (const int32_t *)se.rank,
                           (const uint32_t *)se.koff, se.c_rows, se.c_key, se.c_v1);
        if (p.pass_replies && z.n_cand > 0) {              // the pass replies: v1 as srch_collect_kernel forms the value of a lane without a move
            int rc;
            if (!se.pass_v1 && (rc = env->mem.alloc(BG_BUF(se.pass_v1, (size_t)n * 4)))) return rc;
            hipLaunchKernelGGL(srch_collect_kernel, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, env->v, (const unsigned long long *)env->sv.best,
                               (const float *)env->sv.root_hidden, env->net.w2(p.slot), env->net.b2(p.slot), 0ll, se.pass_v1);
            s3::pass_emit(s, n, mid->v0, mid->deep, (const uint32_t *)se.cnt, (const uint32_t *)se.koff, (const float *)se.pass_v1, se.c_rows,
                          se.c_key, se.c_v1);
        }
        return BGAMD_OK;
    }
    // stage C: one virtual lane per (searched candidate, opponent roll), scored on the scratch env
    int score_replies()
    {
        if (z.n_virtual == 0) return BGAMD_OK;
        const bool mapped = p.fanout == SearchFanout::MAPPED;
        if (mapped)
            hipLaunchKernelGGL(flt_vmap_kernel<SRCH_NT>, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, (const uint32_t *)se.kept,
                               (const uint32_t *)se.koff, (const uint32_t *)se.soff, se.vmap);
        if (const int rc = scratch_env(env, &env->scratch, z.scratch_lanes, false, 0, s)) return rc;
        const auto fanout = [&](const EnvView &lanes, long long v0) {
            if (mapped)
                hipLaunchKernelGGL(flt_fanout_kernel<SRCH_NT>, grid1(lanes.n, SRCH_NT), dim3(SRCH_NT), 0, s, lanes, v0, (const uint32_t *)(se.soff + n),
                                   (const uint32_t *)se.vmap, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key);
            else
                hipLaunchKernelGGL(srch_fanout_kernel, grid1(lanes.n, SRCH_NT), dim3(SRCH_NT), 0, s, lanes, v0, (const uint32_t *)(se.koff + n),
                                   (const uint4 *)se.c_rows, (const uint32_t *)se.c_key);
        };
        return score_virtual_lanes(env, p.slot, z.n_virtual, fanout, se.c_rval, s);
    }
    unsigned long long *scratch_err() const { return env->scratch ? &env->scratch->v.counters[C_ERR] : (unsigned long long *)nullptr; }
    // stage D of the analysis: V2, the best and the played candidate's place, the summary
    int end_analysis()
    {
        hipLaunchKernelGGL(ana_reduce_kernel<SRCH_NT>, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, (const uint32_t *)se.kept,
                           (const uint32_t *)se.koff, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key, (const float *)se.c_v1,
                           (const float *)se.c_rval, se.c_v2, an.v, &env->v.counters[C_ERR], scratch_err());
        hipLaunchKernelGGL(ana_summary_kernel<ANA_SUM_NT>, dim3(1), dim3(ANA_SUM_NT), 0, s, env->v, an.v, an.summary);
        HIPCHK(hipGetLastError());
        an.ready = true;
        return BGAMD_OK;
    }
    // stage D of a mid env: the best searched reply of every mid lane into the 3-ply step's r3
    int end_mid()
    {
        s3::r3_reduce(s, n, mid->v0, mid->deep, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint32_t *)se.c_key,
                      (const float *)se.c_v1, (const float *)se.c_rval, se.c_v2, mid->r3, mid->roots, &env->v.counters[C_ERR], scratch_err());
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    // stage D of a step: V2 and the choice, the log, the 3-ply step's deep level, the apply -- and the env remembers the step
    int end_step()
    {
        if (p.ending == SearchEnding::FILTERED)
            hipLaunchKernelGGL(flt_reduce_kernel<SRCH_NT>, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, (const uint32_t *)se.kept,
                               (const uint32_t *)se.koff, (const uint32_t *)se.soff, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key,
                               (const float *)se.c_v1, (const float *)se.c_rval, se.c_v2, env->sv.best, &env->v.counters[C_ERR], scratch_err());
        else
            hipLaunchKernelGGL(srch_reduce_kernel, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, (const uint32_t *)se.kept,
                               (const uint32_t *)se.koff, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key, (const float *)se.c_v1,
                               (const float *)se.c_rval, se.c_v2, env->sv.best, &env->v.counters[C_ERR], scratch_err());
        if (p.logged)
            hipLaunchKernelGGL(srch_log_kernel<SRCH_NT>, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, env->v, p.flags, (const uint4 *)env->sv.root_rows,
                               (const unsigned long long *)env->sv.best, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint4 *)se.c_rows,
                               (const uint32_t *)se.c_key, (const float *)se.c_v1, (const float *)se.c_v2, p.min_searched, env->slog);
        int rc;
        if (p.deep && (rc = deep_level())) return rc;
        const ExploreView xv{env->rv.tasks, env->rv.task_count, env->rv.task_off, env->rv.task_n};
        hipLaunchKernelGGL(apply_kernel, grid1(n, LANE_NT), dim3(LANE_NT), 0, s, env->v, env->sv, xv, p.flags, 0.0f);
        HIPCHK(hipGetLastError());
        se.last = SearchResult{z.K, p.min_searched, s, p.deep};
        return BGAMD_OK;
    }
    // The 3-ply step's deep level (bg_search3.h): env holds a filtered step's kept lists, V2 and best[g].  Selects the deep set of every
    // searched lane, searches its (candidate, opponent roll) mid lanes on env->mid a chunk at a time -- env->scratch lent to it -- and
    // leaves best[g] of the lanes searched deeper as their V3 choice.  Synchronises s once for the deep list's length and once per chunk.
    int deep_level()
    {
        int rc;
        if (!se.dkept) {                                   // all or none: dkept != NULL says that every buffer is there
            const long long per_game = p.deep_game_bytes;
            if ((rc = env->mem.alloc_group({BG_BUF(se.dkept, per_game), BG_BUF(se.doff, per_game), BG_BUF(se.d_info3, 6 * 8), BG_BUF(se.d_l3, 8)})))
                return rc;
        }
        if ((rc = env->mem.grow(se.c_cap, se.d_cap, {BG_BUF(se.c_d3, 4), BG_BUF(se.c_v3, 4), BG_BUF(se.dmap, 4), BG_BUF(se.r3, 4 * SRCH_ROLLS)})))
            return rc;
        HIPCHK(hipMemsetAsync(se.d_l3, 0, 8, s));
        s3::deep_select(s, n, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key,
                        (const float *)se.c_v2, p.deep_k_lim, p.deep_margin, se.c_d3, se.dkept);
        hipLaunchKernelGGL(srch_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)se.dkept, se.doff, n, (uint32_t *)nullptr);
        uint32_t n_deep = 0;
        HIPCHK(hipMemcpyAsync(&n_deep, se.doff + n, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        if (n_deep && !env->mid_chunk) env->mid_chunk = search3_chunk(getenv("BGAMD_SEARCH3_CHUNK"));
        const DeepPlan d = deep_plan(n_deep, env->mid_chunk);
        if (d.none) return BGAMD_OK;                       // no lane is searched deeper: the filtered step's choices stand
        s3::deep_map(s, n, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint32_t *)se.dkept, (const uint32_t *)se.doff,
                     (const int32_t *)se.c_d3, se.dmap);
        if ((rc = scratch_env(env, &env->mid, d.mid_lanes, false, 0, s))) return rc;
        bgamd_env *me = env->mid;
        for (long long v0 = 0; v0 < d.n_mid; v0 += me->v.n) {
            hipLaunchKernelGGL(flt_fanout_kernel<SRCH_NT>, grid1(me->v.n, SRCH_NT), dim3(SRCH_NT), 0, s, me->v, v0, (const uint32_t *)(se.doff + n),
                               (const uint32_t *)se.dmap, (const uint4 *)se.c_rows, (const uint32_t *)se.c_key);
            const Search3Mid out{{se.doff + n, se.dmap, se.c_rows, se.c_key}, se.r3, v0, se.d_l3};
            if ((rc = search_lent(env, me, SearchKind::MID, p.slot ? BGAMD_WEIGHTS_SLOT1 : 0, p.reply_top_k, p.reply_margin, &out, s))) return rc;
        }
        s3::v3_reduce(s, n, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint32_t *)se.dkept, (const uint32_t *)se.doff,
                      (const uint4 *)se.c_rows, (const uint32_t *)se.c_key, (const float *)se.c_v1, (const int32_t *)se.c_d3, (const float *)se.r3,
                      se.c_v3, env->sv.best, &env->v.counters[C_ERR], &me->v.counters[C_ERR]);
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
};

int search_lent(bgamd_env *owner, bgamd_env *inner, SearchKind kind, int flags, int top_k, float margin, const Search3Mid *mid, hipStream_t s)
{
    const SearchPlan p = search_plan(search_request(inner, kind, flags, top_k, margin));
    if (p.rc) return p.rc;
    inner->scratch = owner->scratch;
    const int rc = SearchCall(inner, p, s, nullptr, mid).run();
    owner->scratch = inner->scratch;                       // (re-created if it had to grow)
    inner->scratch = nullptr;
    return rc;
}

// a search entry point's call on the caller's env: refused with the plan's code, or run
int search_entry(bgamd_env *env, const SearchRequest &q, const int32_t *d_played, void *stream)
{
    const SearchPlan p = search_plan(q);
    if (p.rc) return p.rc;
    HIPCHK(hipSetDevice(env->device));
    return SearchCall(env, p, (hipStream_t)stream, d_played, nullptr).run();
}
}  // namespace

int bgamd_env_step_search3(bgamd_env *env, int flags, int top_k, float margin, int deep_k, float deep_margin, int reply_top_k,
                           float reply_margin, void *stream)
{
    if (!env) return BGAMD_E_INVALID;
    SearchRequest q = search_request(env, SearchKind::THREE_PLY, flags, top_k, margin);
    q.deep_k = deep_k; q.deep_margin = deep_margin; q.reply_top_k = reply_top_k; q.reply_margin = reply_margin;
    return search_entry(env, q, nullptr, stream);
}

int bgamd_env_search3_read(bgamd_env *env, float *d_v3, int32_t *d_depth, void *stream)
{
    ENV_GUARD(env);
    const SearchState &se = env->srch;
    if (se.last.k < 0 || !se.last.deep) return BGAMD_E_INVALID;
    const long long n = env->v.n, K = se.last.k;
    if (K > 0 && (d_v3 || d_depth))
        s3::read((hipStream_t)stream, n, (int)K, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint32_t *)se.dkept,
                 (const int32_t *)se.c_d3, (const float *)se.c_v3, d_v3, d_depth);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// taken when asked for, on the stream of the step it describes, as bgamd_env_search_info
int bgamd_env_search3_info(bgamd_env *env, int64_t h_out[6])
{
    ENV_GUARD(env);
    SearchState &se = env->srch;
    if (!h_out || se.last.k < 0 || !se.last.deep) return BGAMD_E_INVALID;
    if (!se.last.info3_read) {
        unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
        s3::info(se.last.stream, (long long)env->v.n, (const uint32_t *)se.kept, (const uint32_t *)se.koff, (const uint32_t *)se.dkept,
                 (const uint32_t *)se.c_key, (const int32_t *)se.c_d3, (const unsigned long long *)se.d_l3, se.d_info3);
        HIPCHK(hipMemcpyAsync(h, se.d_info3, 6 * 8, hipMemcpyDeviceToHost, se.last.stream));
        HIPCHK(hipStreamSynchronize(se.last.stream));
        for (int q = 0; q < 6; ++q) se.last.info3[q] = (int64_t)h[q];
        se.last.info3_read = true;
    }
    for (int q = 0; q < 6; ++q) h_out[q] = se.last.info3[q];
    return BGAMD_OK;
}

int bgamd_env_step_search(bgamd_env *env, int flags, int top_k, void *stream)
{
    if (!env) return BGAMD_E_INVALID;
    return search_entry(env, search_request(env, SearchKind::STEP, flags, top_k), nullptr, stream);
}

int bgamd_env_step_search_filtered(bgamd_env *env, int flags, int top_k, float margin, void *stream)
{
    if (!env) return BGAMD_E_INVALID;
    return search_entry(env, search_request(env, SearchKind::FILTERED, flags, top_k, margin), nullptr, stream);
}

// The counts are taken when they are asked for, on the stream of the step they describe: a search step launches nothing for them.
int bgamd_env_search_info(bgamd_env *env, int64_t h_out[4])
{
    ENV_GUARD(env);
    SearchState &se = env->srch;
    if (!h_out || se.last.k < 0) return BGAMD_E_INVALID;
    if (!se.last.info_read) {
        unsigned long long h[4] = {0, 0, 0, 0};
        hipLaunchKernelGGL(flt_info_kernel<1024>, dim3(1), dim3(1024), 0, se.last.stream, (long long)env->v.n, (const uint32_t *)se.kept,
                           (const uint32_t *)se.koff, (const uint32_t *)se.c_key, se.last.min_searched, se.d_info);
        HIPCHK(hipMemcpyAsync(h, se.d_info, 4 * 8, hipMemcpyDeviceToHost, se.last.stream));
        HIPCHK(hipStreamSynchronize(se.last.stream));
        for (int q = 0; q < 4; ++q) se.last.info[q] = (int64_t)h[q];
        se.last.info_read = true;
    }
    for (int q = 0; q < 4; ++q) h_out[q] = se.last.info[q];
    return BGAMD_OK;
}

// ---- move analysis (bg_analysis.h) -------------------------------------------------------------------------------------------------
int bgamd_env_analyze_moves(bgamd_env *env, int flags, int top_k, const int32_t *d_played28, void *stream)
{
    if (!env) return BGAMD_E_INVALID;
    SearchRequest q = search_request(env, SearchKind::ANALYSIS, flags, top_k);
    q.has_played = d_played28 != nullptr;
    return search_entry(env, q, d_played28, stream);
}

int bgamd_env_analysis_read(bgamd_env *env, int32_t *d_status, int32_t *d_distinct, int32_t *d_rank1, int32_t *d_rank2,
                            float *d_v1_played, float *d_v1_best, float *d_v2_played, float *d_v2_best, float *d_error,
                            int32_t *d_best28, double *d_summary, void *stream)
{
    ENV_GUARD(env);
    const AnalysisState &an = env->ana;
    if (!an.ready) return BGAMD_E_INVALID;
    const long long n = env->v.n;
    const AnaView out{d_status, d_distinct, d_rank1, d_rank2, d_v1_played, d_v1_best, d_v2_played, d_v2_best, d_error, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(ana_read_kernel<SRCH_NT>, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, (hipStream_t)stream, n, an.v,
                       (const double *)an.summary, out, d_best28, d_summary);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_search_read(bgamd_env *env, int32_t *d_states28, float *d_v1, float *d_v2, int32_t *d_kept, void *stream)
{
    ENV_GUARD(env);
    const SearchState &se = env->srch;
    if (se.last.k < 0) return BGAMD_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n = env->v.n, K = se.last.k;
    if (d_kept) hipLaunchKernelGGL(srch_kept_kernel, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, (const uint32_t *)se.kept, d_kept);
    if (K > 0 && (d_states28 || d_v1 || d_v2))
        hipLaunchKernelGGL(srch_read_kernel, grid1(n * K, SRCH_NT), dim3(SRCH_NT), 0, s, n, (int)K, (const uint32_t *)se.kept,
                           (const uint32_t *)se.koff, (const uint4 *)se.c_rows, (const float *)se.c_v1, (const float *)se.c_v2,
                           d_states28, d_v1, d_v2);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// ---- pre-roll evaluation (bg_vr.h) ---------------------------------------------------------------------------------------
// f of n positions x 21 rolls: the positions are rows[n] (src NULL) or the lanes of the env src (n = its lane count); every (position,
// roll) is a virtual lane of the search's scratch env.  Writes f[q][r] of every position that is neither over nor a finished lane.
static int preroll_pass(bgamd_env *env, int slot, long long n, const uint4 *rows, const EnvView *src, float *f, hipStream_t s)
{
    const auto fanout = [&](const EnvView &lanes, long long v0) {
        if (src)
            hipLaunchKernelGGL(pre_fanout_kernel<true>, grid1(lanes.n, SRCH_NT), dim3(SRCH_NT), 0, s, lanes, v0, n, (const uint4 *)nullptr, *src);
        else
            hipLaunchKernelGGL(pre_fanout_kernel<false>, grid1(lanes.n, SRCH_NT), dim3(SRCH_NT), 0, s, lanes, v0, n, rows, lanes);
    };
    return score_virtual_lanes(env, slot, n * SRCH_ROLLS, fanout, f, s);
}

// the search's scratch env with `lanes` lanes (search_lanes of positions x 21 rolls), its error bits cleared: what preroll_pass scores on,
// preroll_errors reads
static int preroll_begin(bgamd_env *env, long long lanes, hipStream_t s)
{
    if (int rc = scratch_env(env, &env->scratch, lanes, false, 0, s)) return rc;
    HIPCHK(hipMemsetAsync(&env->scratch->v.counters[C_ERR], 0, 8, s));
    return BGAMD_OK;
}

// the error bits the scratch env's greedy kernels raised since it was cleared -> host (synchronises), cleared again
static int preroll_errors(bgamd_env *env, hipStream_t s)
{
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, &env->scratch->v.counters[C_ERR], 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemsetAsync(&env->scratch->v.counters[C_ERR], 0, 8, s));
    HIPCHK(hipStreamSynchronize(s));
    return check_err_flags(env->scratch, h);
}

int bgamd_env_evaluate_preroll(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, int64_t n,
                               float *d_roll_values, double *d_mean, void *stream)
{
    if (!env || !d_states28 || n < 1 || n >= (1ll << 31) / SRCH_ROLLS || (flags & ~BGAMD_WEIGHTS_SLOT1)) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    const int slot = (flags & BGAMD_WEIGHTS_SLOT1) ? 1 : 0;
    if (!env->net.has_weights[slot]) return BGAMD_E_NOWEIGHTS;
    hipStream_t s = (hipStream_t)stream;
    PrerollState &pre = env->pre;
    int rc;
    if ((rc = env->mem.grow(n, pre.cap, {BG_BUF(pre.rows, 32), BG_BUF(pre.f, 4 * SRCH_ROLLS)}))) return rc;

    HIPCHK(hipMemsetAsync(&env->a_ctr[A_INTAKE], 0, 8, s));
    if ((rc = intake_positions(env, d_states28, d_turn, n, pre.rows, s))) return rc;

    if ((rc = preroll_begin(env, search_lanes(n * SRCH_ROLLS), s)) || (rc = preroll_pass(env, slot, n, pre.rows, nullptr, pre.f, s))) return rc;
    hipLaunchKernelGGL(pre_reduce_kernel, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, (long long)n, (const uint4 *)pre.rows, pre.f,
                       d_roll_values, d_mean);
    HIPCHK(hipGetLastError());
    return preroll_errors(env, s);
}

// ---- Monte Carlo rollouts (bg_rollout.h) -----------------------------------------------------------------------------------
namespace {
// One call of bgamd_env_rollout_grouped after rollout_plan has decided it (bg_rollout_plan.h, plain C++, checked without a GPU: refusal,
// lanes, run length, read-back period, buffer sizes): what the call kept in locals, and its schedule in the entry point's order
struct RolloutCall {
    bgamd_env *env;
    const RolloutPlan &p;
    hipStream_t s;
    RolloutState &ro;                      // env->ro
    bgamd_env *sc = nullptr;               // the trial env: env->rscratch, exactly p.L lanes
    RoView r{};
    long long steps = 0;                   // env steps issued on the trial env (bgamd_env_rollout_info [1])
    bool match = false;                    // a match is set (bg_match.h): its init and turn kernels stand in for the cube's

    // the scratch env (exactly L lanes) and the buffers of this call: one pass over the plan's needs (a need of 0 grows nothing)
    int buffers()
    {
        DevMem &mem = env->mem;
        const RolloutNeeds &n = p.needs;
        int rc;
        if ((rc = scratch_env(env, &env->rscratch, p.L, true, 1, s))) return rc;
        sc = env->rscratch;
        if ((rc = mem.grow(n.pos, ro.cap_pos, {BG_BUF(ro.pos, 32)})) ||
            (rc = mem.grow(n.fan, ro.cap_fan, {BG_BUF(ro.fan, 32), BG_BUF(ro.fval, 4)})) ||
            (rc = mem.grow(n.trials, ro.cap_trials, {BG_BUF(ro.tval, 4), BG_BUF(ro.tturns, 4)})) ||
            (rc = mem.grow(n.lanes, ro.cap_lanes, {BG_BUF(ro.lane, 4), BG_BUF(ro.trows, 32), BG_BUF(ro.tids, 4), BG_BUF(ro.tv, 4)})) ||
            (rc = mem.grow(n.vtrials, ro.cap_vtrials, {BG_BUF(ro.tluck, 8)})) ||
            (rc = mem.grow(n.vlanes, ro.cap_vlanes, {BG_BUF(ro.vf, 4 * SRCH_ROLLS)})) ||
            (rc = mem.grow(n.vpos, ro.cap_vpos, {BG_BUF(ro.f0, 4 * SRCH_ROLLS), BG_BUF(ro.m0, 8)})) ||
            (rc = mem.grow(n.group, ro.cap_group, {BG_BUF(ro.group, 4)})) ||
            (rc = mem.grow(n.ctrials, ro.cap_ctrials, {BG_BUF(ro.ctrial, sizeof(cube::Trial)), BG_BUF(ro.ceq, 8)})) ||
            (rc = mem.grow(n.cstart, ro.cap_cstart, {BG_BUF(ro.cstart, 2 * 4)})))
            return rc;
        const match::Needs mn = match::needs(match, p.P, p.N);
        if ((rc = mem.grow(mn.words, ro.cap_mwords, {BG_BUF(ro.mwords, 4)})) || (rc = mem.grow(mn.trials, ro.cap_mtrials, {BG_BUF(ro.cmwc, 8)})))
            return rc;
        if (p.cube && !ro.cctr && (rc = mem.alloc(BG_BUF(ro.cctr, cube::CTR_WORDS * 8)))) return rc;
        if (!ro.host && (rc = mem.alloc_pinned(BG_BUF(ro.host, 8 * 8)))) return rc;        // the pinned words and the two events: first use
        for (hipEvent_t &e : ro.ev) if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return BGAMD_OK;
    }
    // the positions as rows; a bad state is refused before anything is played
    int intake(const int32_t *d_states28, const int32_t *d_turn, const int32_t *d_group)
    {
        HIPCHK(hipMemsetAsync(env->a_ctr, 0, A_WORDS * 8, s));
        HIPCHK(hipMemsetAsync(sc->v.counters, 0, C_COUNT * 8, s));
        // ... and, in the same pass, a bad group table: the env's copy is written, checked, and read by nothing before the synchronise
        unsigned long long intake = 0;
        if (p.grouped) hipLaunchKernelGGL(ro_group_intake_kernel<128>, grid1(p.P, 128), dim3(128), 0, s, d_group, p.P, p.T, ro.group, &env->a_ctr[A_INTAKE]);
        if (p.cube) cube::intake(s, p.P, env->cube_value, env->cube_owner, ro.cstart, &env->a_ctr[A_INTAKE], (unsigned long long)ERRF_RO_CUBE);
        if (match) match::intake(s, p.P, env->match_tab.M, env->match_away1, env->match_away2, env->match_state, ro.mwords, &env->a_ctr[A_INTAKE],
                                 match::ERRF_RO_MATCH);
        const int rc = intake_positions(env, d_states28, d_turn, p.P, ro.pos, s, &intake);
        if (intake & (ERRF_RO_GROUP | ERRF_RO_CUBE | match::ERRF_RO_MATCH)) return BGAMD_E_INVALID;
        return rc;
    }
    // trial jl = p T + i of the call plays game id base + jl (base = position_offset T): episode jl + L - g of lane g, stride 1.
    // Grouped: game id (group_offset + group[p]) T + i, episode group[p] T + i + L - g (ro_refill_kernel); the slot stays jl.
    int seat(uint64_t seed)
    {
        sc->v.seed = seed; sc->v.lane_stride = 1; sc->v.lane_offset = p.lane_offset;
        r = RoView{p.N, p.T, p.M, p.rotate ? 1 : 0, p.F, ro.pos, ro.fan, ro.fval, ro.lane, ro.tval, ro.tturns, ro.trows, ro.tids, env->a_ctr,
                   p.grouped ? (const int32_t *)ro.group : nullptr};
        // plies = 2: the search's virtual roots are scored on THIS env's scratch env, lent to the trial env for the step (search_turn), sized once
        return p.two_ply ? scratch_env(env, &env->scratch, p.search_scratch_lanes, false, 0, s) : BGAMD_OK;
    }
    int search_turn()
    {
        return search_lent(env, sc, SearchKind::FILTERED, p.run_flags, env->ro_top_k, env->ro_margin, nullptr, s);
    }
    // rotation: the first turn of every (position, ordered pair) as one greedy step with injected dice, L virtual lanes at a time
    int fan()
    {
        for (long long c = 0; c < p.fan_chunks; ++c) {
            const long long v0 = c * p.L;
            hipLaunchKernelGGL(ro_fan_seed_kernel, grid1(p.L, RO_NT), dim3(RO_NT), 0, s, sc->v, v0, p.n_fan, r);
            if (const int rc = p.two_ply ? search_turn() : bgamd_env_step_greedy(sc, p.run_flags, 0.0f, BGAMD_F32, s)) return rc;
            hipLaunchKernelGGL(ro_fan_collect_kernel, grid1(p.L, RO_NT), dim3(RO_NT), 0, s, sc->v, v0, p.n_fan, ro.fan);
            ++steps;
        }
        return p.fan_eval ? launch_eval(sc, p.slot, BGAMD_F32, eval_grids(p.n_fan, sc->n_cu), nullptr, p.n_fan, ro.fan, ro.fval, nullptr, nullptr, s)
                          : BGAMD_OK;
    }
    // luck adjustment: the pre-roll evaluation on the search's scratch env -- of the P positions once (rotation: turn 0's luck), then
    // of the trial lanes before every turn (vr_turn); every trial's luck total starts at 0 or at its turn-0 luck
    int luck_init()
    {
        if (!p.vr) return BGAMD_OK;
        if (const int rc = preroll_begin(env, p.preroll_lanes, s)) return rc;
        if (p.rotate) {
            if (const int rc = preroll_pass(env, p.slot, p.P, ro.pos, nullptr, ro.f0, s)) return rc;
            hipLaunchKernelGGL(pre_reduce_kernel, grid1(p.P, SRCH_NT), dim3(SRCH_NT), 0, s, (long long)p.P, (const uint4 *)ro.pos, ro.f0,
                               (float *)nullptr, ro.m0);
        }
        hipLaunchKernelGGL(ro_vr_init_kernel, dim3((unsigned)(sc->n_cu * 4)), dim3(RO_NT), 0, s, r, (const float *)ro.f0,
                           (const double *)ro.m0, ro.tluck);
        // the cube: every trial's record at its start, with the decision before a rotated turn 0 on the position's own mean
        if (p.cube) {
            HIPCHK(hipMemsetAsync(ro.cctr, 0, cube::CTR_WORDS * 8, s));
            if (match) match::init(s, p.N, p.T, p.rotate ? 1 : 0, ro.pos, ro.cstart, p.P, ro.m0, env->cube_rule, env->match_tab, ro.mwords, ro.ctrial);
            else cube::init(s, p.N, p.T, p.rotate ? 1 : 0, ro.pos, ro.cstart, p.P, ro.m0, env->cube_rule, ro.ctrial);
        }
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    // (the roots of the turn at hand are in place: the board, side to move and dice of every live trial lane)
    int vr_turn()
    {
        if (const int e = preroll_pass(env, p.slot, p.L, nullptr, &sc->v, ro.vf, s)) return e;
        hipLaunchKernelGGL(ro_vr_luck_kernel, grid1(p.L, RO_NT), dim3(RO_NT), 0, s, sc->v, (const uint32_t *)ro.lane, (const float *)ro.vf, ro.tluck);
        if (match) match::turn(s, p.L, p.T, sc->v.meta, sc->v.ply, ro.lane, ro.vf, env->cube_rule, env->match_tab, ro.mwords, ro.ctrial, ro.cctr);
        else if (p.cube) cube::turn(s, p.L, sc->v.meta, sc->v.ply, ro.lane, ro.vf, env->cube_rule, ro.ctrial, ro.cctr);
        return BGAMD_OK;
    }
    int refill()
    {
        hipLaunchKernelGGL(ro_refill_kernel, grid1(p.L, RO_NT), dim3(RO_NT), 0, s, sc->v, r);
        if (p.truncates) {                             // truncated trials: the dense fp32 evaluator of bgamd_evaluate_slot
            const EvalGrids grids = eval_grids(sc->v.n * EST_ROWS, sc->n_cu);        // (the truncated rows are counted on the device: sized as a step's)
            if (const int e = launch_eval(sc, p.slot, BGAMD_F32, grids, &r.ctr[RO_NTRUNC], p.L, ro.trows, ro.tv, nullptr, nullptr, s)) return e;
            hipLaunchKernelGGL(ro_trunc_scatter_kernel, dim3((unsigned)sc->n_cu), dim3(RO_NT), 0, s, r, (const float *)ro.tv);
            HIPCHK(hipMemsetAsync(&r.ctr[RO_NTRUNC], 0, 8, s));
        }
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    // (trials done, truncated now, the rollout's error bits, the trial env's error bits) -> dst[0 .. 3], asynchronously
    int read_back(unsigned long long *dst)
    {
        HIPCHK(hipMemcpyAsync(dst, &r.ctr[RO_DONE], 3 * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(dst + 3, &sc->v.counters[C_ERR], 8, hipMemcpyDeviceToHost, s));
        return BGAMD_OK;
    }
    // G runs of R turns with a refill after each, then a read-back into pinned memory; the host waits for the read before the last
    // one, so the device always has a group queued
    int turns()
    {
        const StepStreams ss{s, sc->tune.overlap ? sc->side : s};
        RolloutProgress progress(p);
        for (int k = 0;; ++k) {
            const int b = k & 1;
            int e;
            if ((e = read_back(ro.host + 4 * b))) return e;
            HIPCHK(hipEventRecord(ro.ev[b], s));
            if (k > 0) {
                HIPCHK(hipEventSynchronize(ro.ev[b ^ 1]));
                const unsigned long long *hp = ro.host + 4 * (b ^ 1);
                const RolloutProgress::Verdict v = progress.read(hp[0], hp[2], hp[3]);
                if (v != RolloutProgress::GO_ON) return v == RolloutProgress::FINISHED ? BGAMD_OK : BGAMD_E_INVALID;
            }
            for (int gi = 0; gi < p.G; ++gi) {
                if (p.two_ply) {
                    // the turn's dice go into the lanes first (the TURN-stream dice of the lane's game id and ply, what BGAMD_ROLL draws):
                    // the luck pass reads them, and the search step plays them as set dice -- with and without the luck pass
                    hipLaunchKernelGGL(dice_kernel, grid1(p.L, 256), dim3(256), 0, s, sc->v, (const int32_t *)nullptr, (int32_t *)nullptr, 1);
                    if ((p.vr && (e = vr_turn())) || (e = search_turn()) || (e = refill())) return e;
                    steps += 1;
                    continue;
                }
                GreedyRun run;
                if ((e = run.init(sc, BGAMD_ROLL | p.run_flags, 0.0f, BGAMD_F32)) || (e = run.begin(s))) return e;
                for (int t = 0; t < p.R; ++t)
                    if ((p.vr && (e = vr_turn())) || (e = run.step(ss, t + 1 < p.R))) return e;
                steps += p.R;
                if ((e = refill())) return e;
            }
        }
    }
    // every lane empty, the first refill, then the loop; the stream is drained whichever way the loop ended
    int play()
    {
        HIPCHK(hipMemsetAsync(ro.lane, 0xFF, (size_t)p.L * 4, s));
        if (const int rc = refill()) return rc;
        const int rc = turns();
        hipStreamSynchronize(s);
        return rc;
    }
    // the errors of the whole call, the reductions into the caller's outputs, and the record the read calls test
    int finish(double *d_mean, double *d_stderr, int64_t *d_turns, int32_t *d_truncated, float *d_trial_value, int32_t *d_trial_turns)
    {
        unsigned long long *h = ro.host;
        int rc;
        if ((rc = read_back(h))) return rc;
        HIPCHK(hipMemcpyAsync(h + 4, &sc->v.counters[C_STEPS], 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if ((rc = check_err_flags(sc, h[3]))) return rc;
        if (h[2] & (ERRF_RO_LONG | ERRF_RO_PLY) || h[0] != (unsigned long long)p.N) return BGAMD_E_INVALID;
        if (p.vr && (rc = preroll_errors(env, s))) return rc;
        hipLaunchKernelGGL(ro_reduce_kernel, dim3((unsigned)p.P), dim3(64), 0, s, (long long)p.T, (const float *)ro.tval,
                           (const uint32_t *)ro.tturns, d_mean, d_stderr, d_turns, d_truncated, d_trial_value, d_trial_turns);
        // the cube: every trial's cubeful equity into the env's buffer (the paired read's which = 3); the two lane-turn counters
        unsigned long long h_cube[cube::CTR_WORDS] = {0ull, 0ull};
        if (p.cube) {
            cube::reduce(s, p.P, p.T, ro.tval, ro.tturns, ro.ctrial, env->cube_rule, ro.ceq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            HIPCHK(hipMemcpyAsync(h_cube, ro.cctr, sizeof h_cube, hipMemcpyDeviceToHost, s));
        }
        // a match: every trial's MWC into the env's buffer (the paired read's which = 4)
        if (match) match::reduce(s, p.P, p.T, ro.tval, ro.tturns, ro.ctrial, env->match_tab, ro.mwords, ro.cmwc, nullptr, nullptr, nullptr, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        RolloutResult done{true, p.vr, p.cube, p.grouped, p.P, p.T, env->cube_rule, {p.L, steps, (int64_t)h[4], p.R},
                           {(int64_t)h_cube[cube::CTR_TURNS], (int64_t)h_cube[cube::CTR_AFTER_DROP]}};
        if (!p.cube) for (int k = 0; k < 2; ++k) done.cube_info[k] = ro.last.cube_info[k];     // (still those of the last call that had the cube)
        done.match = match;
        ro.last = done;
        return BGAMD_OK;
    }
};
}  // namespace

int bgamd_env_rollout(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, int64_t n_positions,
                      int64_t position_offset, int64_t trials, int64_t max_plies, uint64_t seed, int64_t lanes,
                      double *d_mean, double *d_stderr, int64_t *d_turns, int32_t *d_truncated,
                      float *d_trial_value, int32_t *d_trial_turns, void *stream)
{
    return bgamd_env_rollout_grouped(env, flags, d_states28, d_turn, nullptr, n_positions, position_offset, trials, max_plies, seed, lanes,
                                     d_mean, d_stderr, d_turns, d_truncated, d_trial_value, d_trial_turns, stream);
}

// d_group NULL: every position its own group, position p's being p -- bgamd_env_rollout with position_offset = group_offset: no group
// table is copied or read, the launches are those of that call.
int bgamd_env_rollout_grouped(bgamd_env *env, int flags, const int32_t *d_states28, const int32_t *d_turn, const int32_t *d_group,
                              int64_t n_positions, int64_t position_offset /* group_offset */, int64_t trials, int64_t max_plies,
                              uint64_t seed, int64_t lanes, double *d_mean, double *d_stderr, int64_t *d_turns, int32_t *d_truncated,
                              float *d_trial_value, int32_t *d_trial_turns, void *stream)
{
    if (!env) return BGAMD_E_INVALID;
    env->ro.last.ok = false;                           // the read calls refuse until a call has succeeded again
    const RolloutPlan plan = rollout_plan(RolloutRequest{flags, n_positions, position_offset, trials, max_plies, lanes, d_states28 != nullptr,
                                                         d_group != nullptr, env->ro_plies, env->ro_top_k, (env->cube_flags & BGAMD_CUBE_ON) != 0,
                                                         {env->net.has_weights[0], env->net.has_weights[1]}}, RO_TURN_LIMIT);
    if (plan.rc) return plan.rc;
    const bool match_on = (env->match_flags & BGAMD_MATCH_ON) != 0;
    if (match::check_call(match_on, env->cube_flags, flags) != match::CALL_OK) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    RolloutCall call{env, plan, (hipStream_t)stream, env->ro};
    call.match = match_on;
    int rc;
    if ((rc = call.buffers()) || (rc = call.intake(d_states28, d_turn, d_group)) || (rc = call.seat(seed)) ||
        (rc = call.fan()) || (rc = call.luck_init()) || (rc = call.play()))        // turn 0 (the rotation fan, the luck and cube records), then the trials
        return rc;
    return call.finish(d_mean, d_stderr, d_turns, d_truncated, d_trial_value, d_trial_turns);
}

int bgamd_env_rollout_paired_read(bgamd_env *env, const int32_t *d_ref, int which, double *d_diff_mean, double *d_diff_stderr, void *stream)
{
    ENV_GUARD(env);
    const RolloutState &ro = env->ro;
    const RolloutResult &last = ro.last;
    if (!last.ok || !d_ref || which < 0 || which > 4) return BGAMD_E_INVALID;
    if (which == 1 && !last.vr) return BGAMD_E_INVALID;
    const int32_t *group = last.grouped ? (const int32_t *)ro.group : (const int32_t *)nullptr;
    if (which == 3) {                                  // the cubeful equity: the buffer the cubeful rollout's reduce launch left (bg_cube.h)
        if (!last.cube) return BGAMD_E_INVALID;
        cube::paired((hipStream_t)stream, last.P, last.T, d_ref, group, ro.ceq, d_diff_mean, d_diff_stderr);
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    if (which == 4) {                                  // the MWC: the buffer the reduce launch of a rollout under a match left (bg_match.h)
        if (!last.match) return BGAMD_E_INVALID;
        cube::paired((hipStream_t)stream, last.P, last.T, d_ref, group, ro.cmwc, d_diff_mean, d_diff_stderr);
        HIPCHK(hipGetLastError());
        return BGAMD_OK;
    }
    hipLaunchKernelGGL(ro_pair_reduce_kernel<64>, dim3((unsigned)last.P), dim3(64), 0, (hipStream_t)stream, (long long)last.P,
                       (long long)last.T, which, d_ref, group, (const float *)ro.tval, (const uint32_t *)ro.tturns, (const double *)ro.tluck,
                       d_diff_mean, d_diff_stderr);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_rollout_policy(bgamd_env *env, int plies, int top_k, float margin)
{
    if (!env || (plies != 1 && plies != 2) || top_k < 0 || !(margin >= 0.0f)) return BGAMD_E_INVALID;
    env->ro_plies = plies; env->ro_top_k = top_k; env->ro_margin = margin;
    return BGAMD_OK;
}

// ---- the doubling cube on the rollout's trials (bg_cube.h) -----------------------------------------------------------------------------
int bgamd_env_rollout_cube(bgamd_env *env, int cube_flags, double double_at, double pass_at, double too_good_at, int64_t max_cube,
                           const int32_t *d_cube_value, const int32_t *d_cube_owner)
{
    if (!env || (cube_flags & ~(BGAMD_CUBE_ON | BGAMD_CUBE_JACOBY | BGAMD_CUBE_HOLD_TURN0))) return BGAMD_E_INVALID;
    if (!(cube_flags & BGAMD_CUBE_ON)) {               // off (another flag alone is nothing): the rollouts launch what they did before
        if (cube_flags) return BGAMD_E_INVALID;
        env->cube_flags = 0; env->cube_value = nullptr; env->cube_owner = nullptr;
        return BGAMD_OK;
    }
    auto in01 = [](double x) { return x >= 0.0 && x <= 1.0; };     // (false for a NaN)
    if (!in01(double_at) || !in01(pass_at) || !in01(too_good_at) || double_at > too_good_at) return BGAMD_E_INVALID;
    if (max_cube < 1 || max_cube > (1ll << 30) || (max_cube & (max_cube - 1))) return BGAMD_E_INVALID;
    env->cube_flags = cube_flags;
    env->cube_rule = cube::Rule{double_at, pass_at, too_good_at, (uint32_t)max_cube, (cube_flags & BGAMD_CUBE_JACOBY) ? 1 : 0,
                                (cube_flags & BGAMD_CUBE_HOLD_TURN0) ? 1 : 0};
    env->cube_value = d_cube_value; env->cube_owner = d_cube_owner;
    return BGAMD_OK;
}

int bgamd_env_rollout_cube_read(bgamd_env *env, double *d_cubeful, double *d_cubeful_stderr, int64_t *d_counts, double *d_trial_cubeful,
                                int32_t *d_trial_cube, int32_t *d_trial_dropped, void *stream)
{
    ENV_GUARD(env);
    const RolloutState &ro = env->ro;
    if (!ro.last.ok || !ro.last.cube) return BGAMD_E_INVALID;
    cube::reduce((hipStream_t)stream, ro.last.P, ro.last.T, ro.tval, ro.tturns, ro.ctrial, ro.last.cube_rule, ro.ceq, d_cubeful, d_cubeful_stderr,
                 d_counts, d_trial_cubeful, d_trial_cube, d_trial_dropped);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_rollout_cube_info(bgamd_env *env, int64_t h_out[2])
{
    if (!env || !h_out) return BGAMD_E_INVALID;
    h_out[0] = env->ro.last.cube_info[0]; h_out[1] = env->ro.last.cube_info[1];
    return BGAMD_OK;
}

// ---- match play on the cubeful rollouts (bg_match.h, bg_match_plan.h) ------------------------------------------------------------------
int bgamd_env_rollout_match(bgamd_env *env, int match_flags, int64_t M, const double *h_met, const double *h_met_pc, double window_share,
                            const int32_t *d_away1, const int32_t *d_away2, const int32_t *d_state)
{
    if (!env || (match_flags & ~BGAMD_MATCH_ON)) return BGAMD_E_INVALID;
    if (!(match_flags & BGAMD_MATCH_ON)) {             // off: the rollouts launch what they did before
        env->match_flags = 0; env->match_away1 = env->match_away2 = env->match_state = nullptr;
        return BGAMD_OK;
    }
    if (match::check_setting(match_flags, M, h_met, h_met_pc, window_share) != match::SET_OK || !d_away1 || !d_away2 || !d_state)
        return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    const match::Layout l = match::layout((int)M);
    const std::vector<double> blob = match::build((int)M, h_met, h_met_pc, window_share);
    // Everything that can fail comes first and touches nothing in force: the two blocks (first use), the wait for stream-ordered readers,
    // the copy into the block that is NOT in force.  Only then is the setting changed, in plain assignments.
    if (!env->match_blob[0]) {
        const size_t bytes = (size_t)match::layout(match::MAX_POINTS).doubles * 8;
        if (const int rc = env->mem.alloc_group({BG_BUF(env->match_blob[0], bytes), BG_BUF(env->match_blob[1], bytes)})) return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    double *dst = env->match_blob[env->match_cur ^ 1];
    HIPCHK(hipMemcpy(dst, blob.data(), (size_t)l.doubles * 8, hipMemcpyHostToDevice));
    env->match_cur ^= 1;
    env->match_tab = match::Table{dst + l.met, dst + l.met_pc, reinterpret_cast<const double2 *>(dst + l.thr), l.M, l.levels};
    env->ro.last.match = false;                        // (a rollout that ran under the old tables can no longer be read as a match)
    env->match_flags = match_flags;
    env->match_away1 = d_away1; env->match_away2 = d_away2; env->match_state = d_state;
    return BGAMD_OK;
}

int bgamd_env_rollout_match_results(bgamd_env *env, double *d_mwc, double *d_mwc_stderr, int64_t *d_counts, double *d_trial_mwc, void *stream)
{
    ENV_GUARD(env);
    const RolloutState &ro = env->ro;
    if (!ro.last.ok || !ro.last.match) return BGAMD_E_INVALID;
    match::reduce((hipStream_t)stream, ro.last.P, ro.last.T, ro.tval, ro.tturns, ro.ctrial, env->match_tab, ro.mwords, ro.cmwc, d_mwc, d_mwc_stderr,
                  d_counts, d_trial_mwc);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_rollout_match_thresholds(bgamd_env *env, int state, int64_t cube, int a, int b, double h_out[2])
{
    if (!env || !h_out || !env->match_tab.thr) return BGAMD_E_INVALID;
    const match::Table &t = env->match_tab;
    if ((state != match::NORMAL && state != match::POST_CRAWFORD) || cube < 1 || (cube & (cube - 1)) || a < 1 || a > t.M || b < 1 || b > t.M)
        return BGAMD_E_INVALID;
    int level = 0;
    while ((1ll << level) < cube) ++level;
    if (level >= t.levels) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    const match::Layout l = match::layout(t.M);
    HIPCHK(hipMemcpy(h_out, t.thr + match::thr_index(l, state, level, a, b), 16, hipMemcpyDeviceToHost));
    return BGAMD_OK;
}

int bgamd_env_rollout_info(bgamd_env *env, int64_t h_out[4])
{
    if (!env || !h_out) return BGAMD_E_INVALID;
    for (int k = 0; k < 4; ++k) h_out[k] = env->ro.last.info[k];
    return BGAMD_OK;
}

int bgamd_env_rollout_vr_read(bgamd_env *env, double *d_vr_mean, double *d_vr_stderr, double *d_trial_luck, void *stream)
{
    ENV_GUARD(env);
    if (!env->ro.last.ok || !env->ro.last.vr) return BGAMD_E_INVALID;
    hipLaunchKernelGGL(ro_vr_reduce_kernel, dim3((unsigned)env->ro.last.P), dim3(64), 0, (hipStream_t)stream, (long long)env->ro.last.T,
                       (const float *)env->ro.tval, (const double *)env->ro.tluck, d_vr_mean, d_vr_stderr, d_trial_luck);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_rollout_outcomes_read(bgamd_env *env, int64_t *d_counts, double *d_equity, double *d_equity_stderr,
                                    int8_t *d_trial_points, void *stream)
{
    ENV_GUARD(env);
    if (!env->ro.last.ok) return BGAMD_E_INVALID;
    hipLaunchKernelGGL((ro_outcome_reduce_kernel<0>), dim3((unsigned)env->ro.last.P), dim3(64), 0, (hipStream_t)stream, (long long)env->ro.last.T,
                       (const float *)env->ro.tval, (const uint32_t *)env->ro.tturns, d_counts, d_equity, d_equity_stderr, d_trial_points);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// ---- points of finished games (bg_outcome.h) ---------------------------------------------------------------------------------
int bgamd_outcomes(const int32_t *d_states28, int64_t n, int32_t *d_points, void *stream)
{
    if (!d_states28 || !d_points || n < 1) return BGAMD_E_INVALID;
    hipLaunchKernelGGL((outcomes_kernel<0>), grid1(n, 256), dim3(256), 0, (hipStream_t)stream, d_states28, (long long)n, d_points);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_outcomes(bgamd_env *env, int32_t *d_points, void *stream)
{
    ENV_GUARD(env);
    if (!d_points) return BGAMD_E_INVALID;
    hipLaunchKernelGGL((env_outcomes_kernel<0>), grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, d_points);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_last_choice(bgamd_env *env, int32_t *d_chosen, int32_t *d_count, int8_t *d_seq, int32_t *d_seq_len,
                          float *d_value, void *stream)
{
    ENV_GUARD(env);
    hipLaunchKernelGGL(last_choice_kernel, grid1(env->v.n, 256), dim3(256), 0, (hipStream_t)stream, env->v, d_chosen, d_count,
                       d_seq, d_seq_len, d_value);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_stats(bgamd_env *env, uint64_t h_out[10])
{
    if (!env || !h_out) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long h[C_COUNT];
    HIPCHK(hipMemcpy(h, env->v.counters, sizeof h, hipMemcpyDeviceToHost));
    h_out[0] = h[C_STEPS]; h_out[1] = h[C_FINISHED]; h_out[2] = h[C_P1WINS];
    h_out[3] = h[C_CAND_RAW]; h_out[4] = h[C_ROWS_EVAL]; h_out[5] = h[C_ERR];
    h_out[6] = h[C_FNODES]; h_out[7] = h[C_DNODES]; h_out[8] = h[C_KSTEPS]; h_out[9] = 0;
    return check_err_flags(env, h[C_ERR]);
}

int bgamd_env_reset_stats(bgamd_env *env, void *stream)
{
    ENV_GUARD(env);
    HIPCHK(hipMemsetAsync(env->v.counters, 0, C_COUNT * 8, (hipStream_t)stream));
    return BGAMD_OK;
}

int bgamd_env_try_move(bgamd_env *env, const int32_t *d_player, const int32_t *d_dice, const int32_t *d_origin,
                       const int32_t *d_dest, int32_t *d_err, void *stream)
{
    if (!env || !d_player || !d_dice || !d_origin || !d_dest || !d_err) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(try_move_kernel, grid1(env->v.n, 128), dim3(128), 0, (hipStream_t)stream, env->v, d_player, d_dice,
                       d_origin, d_dest, d_err);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_legal_moves(bgamd_env *env, const int32_t *d_player, const int32_t *d_die, int32_t *d_n, int8_t *d_pairs,
                          void *stream)
{
    if (!env || !d_player || !d_die || !d_n || !d_pairs) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    hipLaunchKernelGGL(legal_moves_kernel, grid1(env->v.n, 128), dim3(128), 0, (hipStream_t)stream, env->v, d_player, d_die,
                       d_n, d_pairs);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int64_t bgamd_env_unique_rows_info(bgamd_env *env, void *d_info, int64_t cap, void *stream)
{
    ENV_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    const long long bb = env->sv.b_base;                   // four arenas: the rows of the first, then those of the second, ...
    const int na = bb > 0 ? N_ARENAS : 1;
    unsigned long long cnt[N_ARENAS] = {0, 0, 0, 0};
    for (int k = 0; k < na; ++k) HIPCHK(hipMemcpyAsync(&cnt[k], &env->sv.tops[arena_counter(k)], 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const long long cap_a = bb > 0 ? bb : env->sv.cap_rows;
    long long total = 0, done = 0;
    for (int k = 0; k < na; ++k) {
        if ((long long)cnt[k] > cap_a) cnt[k] = (unsigned long long)cap_a;
        total += (long long)cnt[k];
        const long long m = (long long)cnt[k] < cap - done ? (long long)cnt[k] : cap - done;
        if (d_info && m > 0)
            HIPCHK(hipMemcpyAsync((uint2 *)d_info + done, env->sv.u_info + (long long)k * bb, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
        done += m > 0 ? m : 0;
    }
    return (int64_t)total;
}

int bgamd_env_unique_rows_read(bgamd_env *env, int64_t first, int64_t n_rows, int32_t *d_states28, float *d_values, void *stream)
{
    if (!env || first < 0 || n_rows < 0 || first + n_rows > env->sv.cap_rows) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    if (n_rows == 0 || (!d_states28 && !d_values)) return BGAMD_OK;
    hipLaunchKernelGGL(rows_values_kernel, grid1(n_rows, 128), dim3(128), 0, (hipStream_t)stream, (const uint4 *)env->sv.u_rows,
                       (const float *)env->v.values, (long long)first, (long long)n_rows, d_states28, d_values,
                       (const unsigned long long *)env->sv.tops, (long long)env->sv.b_base);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_choice_spread(bgamd_env *env, int32_t *d_count, float *d_best, float *d_worst, int32_t *d_tied, int64_t *d_summary,
                            void *stream)
{
    ENV_GUARD(env);
    if (!env->greedy_stepped) return BGAMD_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n = env->v.n;
    const SpreadView sp{env->spread, env->spread + n, env->spread + 2 * n, env->spread + 3 * n, env->spread + 4 * n};
    HIPCHK(hipMemsetAsync(env->spread, 0, (size_t)n * 5 * 4, s));
    HIPCHK(hipMemsetAsync(sp.lo, 0xFF, (size_t)n * 4, s));
    if (d_summary) HIPCHK(hipMemsetAsync(d_summary, 0, 4 * 8, s));
    // the walk of bgamd_env_unique_rows_read: the last step's counters, the arenas one after the other (bg_search.h)
    const unsigned long long *tops = env->sv.tops;
    const long long bb = env->sv.b_base, cap_rows = env->sv.cap_rows;
    long long rblocks = (cap_rows + SRCH_NT - 1) / SRCH_NT;
    const long long lim = 8ll * env->n_cu;
    const dim3 rgrid((unsigned)(rblocks < 1 ? 1 : (rblocks > lim ? lim : rblocks)));
    hipLaunchKernelGGL(spread_reduce_kernel, rgrid, dim3(SRCH_NT), 0, s, tops, bb, cap_rows, (const uint4 *)env->sv.u_rows,
                       (const uint2 *)env->sv.u_info, (const float *)env->v.values, n, sp);
    hipLaunchKernelGGL(spread_tied_kernel, rgrid, dim3(SRCH_NT), 0, s, tops, bb, cap_rows, (const uint4 *)env->sv.u_rows,
                       (const uint2 *)env->sv.u_info, (const float *)env->v.values, n, sp);
    hipLaunchKernelGGL(spread_finish_kernel, grid1(n, SRCH_NT), dim3(SRCH_NT), 0, s, n, sp, d_count, d_best, d_worst, d_tied,
                       (unsigned long long *)d_summary);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

static_assert(sizeof(bgamd_net_health_t) == sizeof(HealthOut) && offsetof(bgamd_net_health_t, max_abs) == offsetof(HealthOut, max_abs) &&
              offsetof(bgamd_net_health_t, fits_f16_split) == offsetof(HealthOut, fits_f16_split) &&
              offsetof(bgamd_net_health_t, unit_saturated) == offsetof(HealthOut, unit_saturated), "bgamd_net_health_t and its device image");

int bgamd_net_health(const float *d_theta, const void *d_rows, int64_t n_rows, float threshold, bgamd_net_health_t *d_out, void *stream)
{
    // (unit_saturated is int32: a count per unit must fit)
    if (!d_theta || !d_out || !(threshold > 0.0f) || n_rows < 0 || n_rows > 0x7FFFFFFFll || (n_rows > 0 && !d_rows)) return BGAMD_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HealthOut *out = reinterpret_cast<HealthOut *>(d_out);
    hipLaunchKernelGGL(health_weights_kernel, dim3(1), dim3(HEALTH_W_THREADS), 0, s, d_theta, (long long)n_rows, out);
    if (n_rows > 0) {
        // the device's CU count and the kernel's LDS opt-in: looked up once per device (the stores race only with equal values)
        static std::atomic<int> cu_of[64];
        int dev = 0, n_cu = 0;
        HIPCHK(hipGetDevice(&dev));
        if (dev >= 0 && dev < 64) n_cu = cu_of[dev].load(std::memory_order_acquire);
        if (n_cu <= 0) {
            HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
            HIPCHK(hipFuncSetAttribute((const void *)health_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HEALTH_LDS_TOTAL));
            if (n_cu <= 0) n_cu = 256;
            if (dev >= 0 && dev < 64) cu_of[dev].store(n_cu, std::memory_order_release);
        }
        long long blocks = ((n_rows + 31) / 32 + HEALTH_THREADS / 64 - 1) / (HEALTH_THREADS / 64);
        blocks = blocks > n_cu ? n_cu : blocks;
        hipLaunchKernelGGL(health_rows_kernel, dim3((unsigned)blocks), dim3(HEALTH_THREADS), HEALTH_LDS_TOTAL, s, d_theta, (const uint4 *)d_rows,
                           (long long)n_rows, threshold, out);
        hipLaunchKernelGGL(health_finish_kernel, dim3(1), dim3(N_HID), 0, s, out);
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_set_trajectory(bgamd_env *env, void *d_rows, int64_t max_plies)
{
    if (!env || (d_rows && max_plies <= 0)) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    env->v.traj = (uint4 *)d_rows;
    env->v.traj_plies = d_rows ? max_plies : 0;
    return BGAMD_OK;
}

int bgamd_env_set_trajectory_ring(bgamd_env *env, void *d_rows, int64_t ring_steps, uint16_t *d_end)
{
    if (!env || (d_rows && (ring_steps <= 0 || !d_end))) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    env->ring_rows = (uint4 *)d_rows;
    env->ring_end = d_rows ? (unsigned short *)d_end : nullptr;
    env->ring_steps = d_rows ? ring_steps : 0;
    env->traj_step = 0;
    return BGAMD_OK;
}

int64_t bgamd_env_trajectory_step(const bgamd_env *env) { return env ? env->traj_step : 0; }

int bgamd_env_set_search_log(bgamd_env *env, void *d_rows, void *d_after, float *d_target, float *d_v1, int64_t max_plies)
{
    if (!env || (d_rows && max_plies <= 0)) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    env->slog = SearchLog{};
    if (d_rows) env->slog = SearchLog{(uint4 *)d_rows, (uint4 *)d_after, d_target, d_v1, (long long)max_plies};
    return BGAMD_OK;
}

int bgamd_env_get_progress(bgamd_env *env, int32_t *d_ply, int32_t *d_episode, void *stream)
{
    ENV_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    if (d_ply) HIPCHK(hipMemcpyAsync(d_ply, env->v.ply, (size_t)env->v.n * 4, hipMemcpyDeviceToDevice, s));
    if (d_episode) HIPCHK(hipMemcpyAsync(d_episode, env->v.episode, (size_t)env->v.n * 4, hipMemcpyDeviceToDevice, s));
    return BGAMD_OK;
}

int bgamd_encode_rows(const void *d_rows, int64_t n, float *d_out198, void *stream)
{
    if (!d_rows || !d_out198 || n < 0) return BGAMD_E_INVALID;
    if (n == 0) return BGAMD_OK;
    hipLaunchKernelGGL(encode_rows_kernel, grid1(n, 128), dim3(128), 0, (hipStream_t)stream, (const uint4 *)d_rows, (long long)n,
                       d_out198);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_encode(const int32_t *d_states28, const int32_t *d_turn, int64_t n, float *d_out198, void *stream)
{
    if (!d_states28 || !d_out198 || n < 0) return BGAMD_E_INVALID;
    if (n == 0) return BGAMD_OK;
    hipLaunchKernelGGL(encode_states_kernel, grid1(n, 128), dim3(128), 0, (hipStream_t)stream, d_states28, d_turn, (long long)n,
                       d_out198);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_evaluate(bgamd_env *env, const int32_t *d_states28, const int32_t *d_turn, int64_t n, int precision,
                   float *d_values, void *stream)
{
    return bgamd_evaluate_slot(env, 0, d_states28, d_turn, n, precision, d_values, stream);
}

int bgamd_evaluate_slot(bgamd_env *env, int slot, const int32_t *d_states28, const int32_t *d_turn, int64_t n, int precision,
                        float *d_values, void *stream)
{
    if (!env || slot < 0 || slot > 1 || !d_states28 || !d_values || n < 0 || n > env->v.cap) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    if (!env->net.has_weights[slot]) return BGAMD_E_NOWEIGHTS;
    if (n == 0) return BGAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    // the candidate arena doubles as scratch for caller-provided states
    hipLaunchKernelGGL(pack_rows_kernel, grid1(n, 128), dim3(128), 0, s, d_states28, d_turn, (long long)n, env->v.rows,
                       &env->v.counters[C_ERR]);
    return launch_eval(env, slot, precision, eval_grids((long long)n, env->n_cu), nullptr, (long long)n, env->v.rows, d_values, nullptr, nullptr, s);
}

int bgamd_evaluate_incremental(bgamd_env *env, int slot, const int32_t *d_root_states28, const int32_t *d_root_turn,
                               int64_t n_roots, const int32_t *d_states28, const int32_t *d_root_index, int64_t n,
                               float *d_values, void *stream)
{
    if (!env || slot < 0 || slot > 1 || !d_root_states28 || !d_root_turn || !d_states28 || !d_root_index || !d_values ||
        n_roots <= 0 || n_roots > env->v.n || n < 0 || n > env->sv.cap_rows)
        return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(env->device));
    if (!env->net.has_weights[slot]) return BGAMD_E_NOWEIGHTS;
    if (n == 0) return BGAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    StagedView &sv = env->sv;
    // the env's root / afterstate arenas double as scratch, as the candidate arena does for bgamd_evaluate; the rows are written
    // linearly from 0: a later unique_rows_read must not remap them through the arena counters of an earlier greedy step
    sv.b_base = 0;
    hipLaunchKernelGGL(pack_rows_kernel, grid1(n_roots, 128), dim3(128), 0, s, d_root_states28, d_root_turn, (long long)n_roots,
                       sv.root_rows, &env->v.counters[C_ERR]);
    hipLaunchKernelGGL(pack_child_rows_kernel, grid1(n, 128), dim3(128), 0, s, d_states28, d_root_index, (long long)n,
                       (long long)n_roots, (const uint4 *)sv.root_rows, sv.u_rows, sv.u_info, &env->v.counters[C_ERR]);
    HIPCHK(hipMemsetAsync(sv.best, 0, (size_t)n_roots * 8, s));
    const RootPass root = root_pass_kind(env->tune, false);
    launch_root_pass(env, slot, root, root_pass_grid(root, (long long)n_roots, env->n_cu), (const uint4 *)sv.root_rows, (long long)n_roots, sv.root_hidden, s);
    KTimer t(env, s, 1);
    launch_delta(env, slot, env->tune.mfma_delta && env->net.wm_ok[slot], delta_grid((long long)n, env->n_cu), sv, nullptr, (long long)n, d_values, nullptr, s);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_env_time_kernels(bgamd_env *env, int enable)
{
    ENV_GUARD(env);
    if (!enable && env->timing) flush_events(env);
    env->timing = enable == 1 ? 0xFFu : ((unsigned)enable >> 8) & 0xFFu;   // 1 = every group, (mask << 8) = chosen groups
    env->timing_stride = ((unsigned)enable >> 20) & 0xFFu;                 // (stride << 20): every stride-th launch only
    if (env->timing_stride == 0) env->timing_stride = 1;
    for (unsigned &c : env->timing_seen) c = 0;
    if (env->timing)                                      // events are created here, not inside somebody's timed region
        while (env->ev.size() < 2 * 1024) {
            hipEvent_t x;
            HIPCHK(hipEventCreate(&x));
            env->ev.push_back(x);
            if (env->ev.size() % 2 == 0) env->ev_kind.push_back(0);
        }
    return BGAMD_OK;
}

const char *bgamd_build_flags(void)
{
    return EXPERIMENTAL_BUILD ? "experimental" : "default";
}

int bgamd_env_kernel_choice(bgamd_env *env, int32_t h_out[4])
{
    if (!env || !h_out) return BGAMD_E_INVALID;
    for (int i = 0; i < 3; ++i) h_out[i] = env->choice[i];
    h_out[3] = EXPERIMENTAL_BUILD ? 1 : 0;
    return BGAMD_OK;
}

int bgamd_env_kernel_times(bgamd_env *env, double h_ms[8], uint64_t h_launches[8])
{
    ENV_GUARD(env);
    const int rc = flush_events(env);
    if (rc) return rc;
    for (int i = 0; i < 8; ++i) {
        if (h_ms) h_ms[i] = env->t_ms[i];
        if (h_launches) h_launches[i] = env->t_n[i];
        env->t_ms[i] = 0; env->t_n[i] = 0;
    }
    return BGAMD_OK;
}

int bgamd_pack_rows(const int32_t *d_states28, const int32_t *d_turn, int64_t n, void *d_rows, void *stream)
{
    if (!d_states28 || !d_rows || n < 0) return BGAMD_E_INVALID;
    if (n == 0) return BGAMD_OK;
    hipLaunchKernelGGL(pack_rows_kernel, grid1(n, 128), dim3(128), 0, (hipStream_t)stream, d_states28, d_turn, (long long)n,
                       (uint4 *)d_rows, (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// host code only: the lanes of the internal envs as they stand (scratch_env keeps one that is large enough), nothing is launched
int bgamd_env_scratch_info(bgamd_env *env, int64_t h_out[3])
{
    if (!env || !h_out) return BGAMD_E_INVALID;
    h_out[0] = env->scratch ? (int64_t)env->scratch->v.n : 0;
    h_out[1] = env->rscratch ? (int64_t)env->rscratch->v.n : 0;
    h_out[2] = env->mid ? (int64_t)env->mid->v.n : 0;
    return BGAMD_OK;
}

}  // extern "C"

// ------------------------------------------- TD(lambda) learner -------------------------------------------
#include "bg_learner_host.h"

