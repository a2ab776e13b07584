// bg_learner_host.h -- host code of the TD(lambda) learner: the bgamd_td handle, the bgamd_td_* entry points of include/bgamd.h and the
// one collective of a multi-rank training step (RCCL, resolved at run time).  Included by bgamd.hip at its end, at file scope: the same
// translation unit, behind the env's host code, whose HIPCHK / g_hip_err / DevMem / grid1 it uses.  The kernels are in bg_learner.h and
// bg_fit.h, what is launched when in bg_td_plan.h.
#pragma once

struct bgamd_td {
    int device = 0;
    DevMem mem;                            // owns every device buffer of td_buffers that has been allocated
    long long max_games = 0;
    TdView v{};
    bool has_weights = false, begun = false;
    int n_cu = 256;
    TdTuning tune;                         // the thresholds and switches of the step's dispatch (bg_td_plan.h), read at create
    double scale = 1.0;                    // c: stored trace = e / c, the same for every game of the replay
    bool stream_mode = false;              // bgamd_td_begin_stream: slots take game after game, steps are not bounded by the log length
    hipStream_t last_stream = nullptr;     // the stream the replay at hand is issued on: what the readers below wait for (a learner replaying on
                                           //   its own stream beside an env at play must not wait for the env: no device-wide synchronisation)
    // the ONE collective of a multi-rank training step issued by the library: an RCCL communicator of the learner's own (bgamd_td_comm_init)
    void *rccl = nullptr;                  // dlopen handle of librccl.so.1 (the one already in the process when there is one)
    void *comm = nullptr;                  // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    float *d_upd = nullptr;                // [TD_P] the step's update, all-reduced in place
    // delayed update (bgamd_td_set_delay): the update of step t applied one step late, a training step = ONE launch (bg_learner.h)
    int delay = 0;
    float *theta2[2] = {nullptr, nullptr};      // [TD_LD] the weights a step reads / the next step's
    uint16_t *wl3_2[2] = {nullptr, nullptr};    // their bf16 x 3 planes
    float *partial2 = nullptr;                 // the second set of partial sums (+ zeroed tail): step t writes set t & 1 (set 0 = v.partial)
    bool timing = false;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    double trace_ms = 0;
    uint64_t trace_launches = 0, trace_game_steps = 0;
    // the supervised step (bgamd_td_fit_step, bg_fit.h)
    float *fit_run = nullptr;               // [TD_LD] the update summed over the chunks so far, internal order
    double *fit_part_sq = nullptr;          // [TD_MAX_GROUPS] per workgroup: Σ δ²
    long long *fit_part_cnt = nullptr;      // [TD_MAX_GROUPS][2] rows that counted | rows skipped
    double *fit_stat = nullptr;             // [4] x 8 B: Σ δ² (double) | rows | skipped (int64) since create / the last bgamd_td_fit_stats
    hipStream_t fit_stream = nullptr;       // the stream of the last fit step: what bgamd_td_fit_stats waits for
};

namespace {
// device -> host on the replay's own stream (never the null stream: a learner beside an env at play waits for its own work only)
hipError_t td_read(bgamd_td *td, void *dst, const void *src, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, td->last_stream);
    return e != hipSuccess ? e : hipStreamSynchronize(td->last_stream);
}
// The learner's device buffers, the ONE table of what to allocate and when: bgamd_td_create allocates those of TD_AT_CREATE, the delayed
// replay and bgamd_td_comm_init theirs at first use -- through td->mem, which bgamd_td_destroy releases.  A new buffer is its member and
// its line here: one left out is never allocated and stays null, which its first kernel trips over at once.
enum TdWhen { TD_AT_CREATE, TD_AT_DELAY, TD_AT_COMM };
struct TdBuf { DevBuf buf; TdWhen when; };
std::vector<TdBuf> td_buffers(bgamd_td *td)
{
    TdView &v = td->v;
    const size_t n = (size_t)td->max_games;
    const size_t partial_bytes = ((size_t)TD_MAX_GROUPS * TD_LD + 64) * 4;     // + a zeroed line: the dummy source of the pipelined trace pass
#define TDBUF(ptr, bytes, when) TdBuf{BG_BUF(ptr, bytes), when}
    return {
        TDBUF(v.theta, TD_LD * 4, TD_AT_CREATE),                  TDBUF(v.w1t, N_IN * N_HID * 4, TD_AT_CREATE),
        TDBUF(v.e, n * TD_LD * 4, TD_AT_CREATE),                  TDBUF(v.fac, n * TD_FLD * 4, TD_AT_CREATE),
        TDBUF(v.coef, n * 4, TD_AT_CREATE),                       TDBUF(v.sq, n * 8, TD_AT_CREATE),
        TDBUF(v.gmeta, n * 16, TD_AT_CREATE),                     TDBUF(v.partial, partial_bytes, TD_AT_CREATE),
        TDBUF(v.amask, n * TD_MASK_WORDS * 4, TD_AT_CREATE),      TDBUF(v.anew, n * TD_MASK_WORDS * 4, TD_AT_CREATE),
        TDBUF(v.act_cols, n * 4, TD_AT_CREATE),                   TDBUF(v.wr_cols, n * 4, TD_AT_CREATE),
        TDBUF(v.nupd, n * 4, TD_AT_CREATE),                       TDBUF(v.qcur, n * 4, TD_AT_CREATE),
        TDBUF(v.wl3, 3 * EVAL16_W_BYTES, TD_AT_CREATE),           TDBUF(v.lut, EVAL16_LUT_BYTES, TD_AT_CREATE),
        TDBUF(v.hid, n * 2 * N_HID * 4, TD_AT_CREATE),            TDBUF(td->fit_run, TD_LD * 4, TD_AT_CREATE),
        TDBUF(td->fit_part_sq, TD_MAX_GROUPS * 8, TD_AT_CREATE),  TDBUF(td->fit_part_cnt, TD_MAX_GROUPS * 2 * 8, TD_AT_CREATE),
        TDBUF(td->fit_stat, 4 * 8, TD_AT_CREATE),
        TDBUF(td->theta2[0], TD_LD * 4, TD_AT_DELAY),             TDBUF(td->wl3_2[0], 3 * EVAL16_W_BYTES, TD_AT_DELAY),
        TDBUF(td->theta2[1], TD_LD * 4, TD_AT_DELAY),             TDBUF(td->wl3_2[1], 3 * EVAL16_W_BYTES, TD_AT_DELAY),
        TDBUF(td->partial2, partial_bytes, TD_AT_DELAY),
        TDBUF(td->d_upd, TD_P * 4, TD_AT_COMM),
    };
#undef TDBUF
}
// allocate the buffers of `when` that are not there yet; the error text names the one that failed
int td_alloc(bgamd_td *td, TdWhen when)
{
    for (const TdBuf &b : td_buffers(td))
        if (b.when == when && !*b.buf.ptr) if (const int rc = td->mem.alloc(b.buf)) return rc;
    return BGAMD_OK;
}
// Σ over the slots of one of their 32-bit counters (nupd, act_cols, wr_cols)
int td_sum_slots(bgamd_td *td, const unsigned int *d_counter, uint64_t *h_sum)
{
    std::vector<unsigned int> c((size_t)td->v.n_games);
    if (!c.empty()) HIPCHK(td_read(td, c.data(), d_counter, c.size() * 4));
    uint64_t tot = 0;
    for (unsigned int x : c) tot += x;
    *h_sum = tot;
    return BGAMD_OK;
}
int td_flush(bgamd_td *td)
{
    for (size_t i = 0; i < td->ev_used; ++i) {
        HIPCHK(hipEventSynchronize(td->ev[2 * i + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, td->ev[2 * i], td->ev[2 * i + 1]));
        td->trace_ms += ms;
    }
    td->ev_used = 0;
    return BGAMD_OK;
}
}  // namespace

extern "C" {

int bgamd_td_create(bgamd_td **out, int64_t max_games, int device)
{
    if (!out || max_games <= 0 || max_games > (1ll << 22)) return BGAMD_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BGAMD_E_NODEVICE;
    HIPCHK(hipSetDevice(device));
    bgamd_td *td = new bgamd_td();
    td->device = device;
    td->max_games = max_games;
    TdView &v = td->v;
    if (td_alloc(td, TD_AT_CREATE)) { bgamd_td_destroy(td); return BGAMD_E_HIP; }
    HIPCHK(hipMemset(v.partial + (size_t)TD_MAX_GROUPS * TD_LD, 0, 64 * 4));
    HIPCHK(hipMemset(td->fit_stat, 0, 4 * 8));
#ifdef BGAMD_EXPERIMENTAL
    td->tune = td_tuning_from_env(getenv, true);
#else
    td->tune = td_tuning_from_env(getenv, false);
#endif
    v.dense = (int)td->tune.dense;
    {
        uint32_t lut[32];
        make_count_lut(lut);
        HIPCHK(hipMemcpy(v.lut, lut, EVAL16_LUT_BYTES, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(v.wl3, 0, 3 * EVAL16_W_BYTES));          // the padding lanes of the tail K-step stay zero
        HIPCHK(hipFuncSetAttribute((const void *)traj_hidden_bf16x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ROOT3_LDS_TOTAL));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        td->n_cu = prop.multiProcessorCount;
    }
    HIPCHK(hipMemset(v.act_cols, 0, (size_t)max_games * 4));
    HIPCHK(hipMemset(v.wr_cols, 0, (size_t)max_games * 4));
    HIPCHK(hipMemset(v.theta, 0, TD_LD * 4));
    HIPCHK(hipMemset(v.sq, 0, (size_t)max_games * 8));
    *out = td;
    return BGAMD_OK;
}

int bgamd_td_destroy(bgamd_td *td)
{
    if (!td) return BGAMD_OK;
    hipSetDevice(td->device);
    hipDeviceSynchronize();
    for (hipEvent_t e : td->ev) hipEventDestroy(e);
    bgamd_td_comm_destroy(td);
    td->mem.release_all();
    delete td;
    return BGAMD_OK;
}

int bgamd_td_set_weights(bgamd_td *td, const float *d_theta, void *stream)
{
    if (!td || !d_theta) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    hipLaunchKernelGGL(td_apply_kernel, grid1(TD_P, 256), dim3(256), 0, (hipStream_t)stream, td->v, d_theta, 1);
    HIPCHK(hipGetLastError());
    td->has_weights = true;
    return BGAMD_OK;
}

int bgamd_td_get_weights(bgamd_td *td, float *d_theta, void *stream)
{
    if (!td || !d_theta) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    if (!td->has_weights) return BGAMD_E_NOWEIGHTS;
    HIPCHK(hipMemcpyAsync(d_theta, td->v.theta, (size_t)TD_P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BGAMD_OK;
}

int bgamd_td_begin(bgamd_td *td, const void *d_rows, int64_t T, int64_t n_lanes, const int32_t *d_order, int64_t n_games,
                   const int32_t *d_length, const uint8_t *d_p1_won, void *stream)
{
    if (!td || !d_rows || !d_order || !d_length || !d_p1_won || T <= 0 || n_lanes <= 0 || n_games < 0 ||
        n_games > td->max_games || n_games > n_lanes)
        return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    TdView &v = td->v;
    v.rows = (const uint4 *)d_rows;
    v.order = d_order;
    v.length = d_length;
    v.p1_won = d_p1_won;
    v.T = T; v.n_lanes = n_lanes; v.n_games = n_games;
    v.queue = nullptr; v.qoff = nullptr;
    v.game_lane = nullptr; v.game_start = nullptr; v.n_table = n_lanes;
    td->last_stream = (hipStream_t)stream;
    if (n_games > 0) {
        hipLaunchKernelGGL(td_gather_kernel, grid1(n_games, 256), dim3(256), 0, (hipStream_t)stream, v);
        HIPCHK(hipGetLastError());
    }
    td->begun = true;
    td->stream_mode = false;
    return BGAMD_OK;
}

// Host-only, plain C++ (csrc/bg_schedule.h: also compiled with -fsanitize=address,undefined by tests/test_sanitizers_cpu.py)
int bgamd_td_stream_schedule(const int32_t *h_length, int64_t n_lanes, int64_t n_slots, int32_t *h_queue, int32_t *h_queue_offsets,
                             int64_t *h_n_games, int64_t *h_n_steps)
{
    return bg::td_stream_schedule(h_length, n_lanes, n_slots, h_queue, h_queue_offsets, h_n_games, h_n_steps) ? BGAMD_E_INVALID : BGAMD_OK;
}

static int td_begin_stream_impl(bgamd_td *td, const void *d_rows, int64_t T, int64_t n_lanes, const int32_t *d_queue,
                                const int32_t *d_queue_offsets, int64_t n_slots, int64_t n_table, const int32_t *d_game_lane,
                                const int32_t *d_game_start, const int32_t *d_length, const uint8_t *d_p1_won, void *stream)
{
    if (!td || !d_rows || !d_queue || !d_queue_offsets || !d_length || !d_p1_won || T <= 0 || n_lanes <= 0 || n_table <= 0 || n_slots < 0 ||
        n_slots > td->max_games || T > 0x3FFFFFFFll)
        return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    TdView &v = td->v;
    v.rows = (const uint4 *)d_rows;
    v.order = nullptr;
    v.length = d_length;
    v.p1_won = d_p1_won;
    v.T = T; v.n_lanes = n_lanes; v.n_games = n_slots;
    v.queue = d_queue; v.qoff = d_queue_offsets;
    v.game_lane = d_game_lane; v.game_start = d_game_start; v.n_table = n_table;
    if (n_slots > 0) {
        hipLaunchKernelGGL(td_gather_stream_kernel, grid1(n_slots, 256), dim3(256), 0, (hipStream_t)stream, v);
        HIPCHK(hipGetLastError());
    }
    td->begun = true;
    td->stream_mode = true;
    td->last_stream = (hipStream_t)stream;
    return BGAMD_OK;
}

int bgamd_td_begin_stream(bgamd_td *td, const void *d_rows, int64_t T, int64_t n_lanes, const int32_t *d_queue,
                          const int32_t *d_queue_offsets, int64_t n_slots, const int32_t *d_length, const uint8_t *d_p1_won, void *stream)
{
    return td_begin_stream_impl(td, d_rows, T, n_lanes, d_queue, d_queue_offsets, n_slots, n_lanes, nullptr, nullptr, d_length, d_p1_won, stream);
}

int bgamd_td_begin_stream_games(bgamd_td *td, const void *d_rows, int64_t ring_steps, int64_t n_lanes, const int32_t *d_queue,
                                const int32_t *d_queue_offsets, int64_t n_slots, int64_t n_games, const int32_t *d_game_lane,
                                const int32_t *d_game_start, const int32_t *d_length, const uint8_t *d_p1_won, void *stream)
{
    if (!d_game_lane || !d_game_start) return BGAMD_E_INVALID;
    return td_begin_stream_impl(td, d_rows, ring_steps, n_lanes, d_queue, d_queue_offsets, n_slots, n_games, d_game_lane, d_game_start, d_length,
                                d_p1_won, stream);
}

int bgamd_td_step(bgamd_td *td, int64_t t, int64_t n_active, double alpha, float lambda, float *d_update, void *stream)
{
    if (!td || !td->begun || t < 0 || (t >= td->v.T && !td->stream_mode) || t > 0x7FFFFFF0ll || n_active < 0 || n_active > td->v.n_games)
        return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    if (!td->has_weights) return BGAMD_E_NOWEIGHTS;
    hipStream_t s = (hipStream_t)stream;
    td->last_stream = s;
    if (n_active == 0) {                 // nothing to add, but the caller's collective still needs a defined buffer
        if (d_update) HIPCHK(hipMemsetAsync(d_update, 0, (size_t)TD_P * 4, s));
        return BGAMD_OK;
    }
    const TdScale sc = td_scale_step(t, lambda, td->tune.lazy, td->scale);
    td->v.full_step = sc.full;
    const TdView &v = td->v;
    const TdPlan p = td_plan(td->tune, td->n_cu, t, n_active, sc.full);
    const dim3 fgrid((unsigned)p.forward_grid);
    switch (p.forward) {
        case TdForward::NONE: break;
        case TdForward::MATRIX_PIPE:
            hipLaunchKernelGGL(traj_hidden_bf16x3_kernel, fgrid, dim3(ROOT3_THREADS), ROOT3_LDS_TOTAL, s, v.rows, (const int4 *)v.gmeta, (long long)t,
                               v.n_lanes, v.T, 2 * n_active, (const uint4 *)v.wl3, (const uint2 *)v.lut, (const float *)(v.theta + TD_OFF_B1), v.hid);
            hipLaunchKernelGGL(td_epilogue_wave_kernel, grid1(n_active, 4), dim3(256), 0, s, v, (long long)t, (long long)n_active, alpha);
            break;
        case TdForward::MFMA_FUSED:
            hipLaunchKernelGGL(td_forward_mfma_kernel, fgrid, dim3(ROOT3D_THREADS), 0, s, v, (long long)t, (long long)n_active, alpha);
            break;
        case TdForward::DIRECT:
#ifdef BGAMD_EXPERIMENTAL
            hipLaunchKernelGGL(traj_hidden_direct_kernel, fgrid, dim3(ROOT3D_THREADS), 0, s, v.rows, (const int4 *)v.gmeta, (long long)t, v.n_lanes,
                               v.T, 2 * n_active, (const uint4 *)v.wl3, (const uint2 *)v.lut, (const float *)(v.theta + TD_OFF_B1), v.hid);
            hipLaunchKernelGGL(td_epilogue_wave_kernel, grid1(n_active, 4), dim3(256), 0, s, v, (long long)t, (long long)n_active, alpha);
            break;
#else
            return BGAMD_E_INVALID;      // (not reached: only BGAMD_TD_FUSED=0 leads here, which this build does not read)
#endif
        case TdForward::VALU2:
            hipLaunchKernelGGL((td_forward_kernel<2, false>), fgrid, dim3(128), 0, s, v, (long long)t, (long long)n_active, alpha);
            break;
        case TdForward::VALU4:
            hipLaunchKernelGGL((td_forward_kernel<4, false>), fgrid, dim3(128), 0, s, v, (long long)t, (long long)n_active, alpha);
            break;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (td->timing) {
        if (td->ev_used * 2 + 2 > td->ev.size()) {
            if (td->ev.size() >= 2 * 4096) { const int rc = td_flush(td); if (rc) return rc; }
            else for (int i = 0; i < 2; ++i) { hipEvent_t x; HIPCHK(hipEventCreate(&x)); td->ev.push_back(x); }
        }
        e0 = td->ev[2 * td->ev_used]; e1 = td->ev[2 * td->ev_used + 1];
        td->ev_used++;
        HIPCHK(hipEventRecord(e0, s));
    }
    // every trace kernel has a <true> (FIRST) instance for step 0 and takes the same tail of arguments
    const dim3 tgrid(p.n_groups), wide(TD_WIDE_THREADS);
#define BG_TRACE_LAUNCH(K_FIRST, K_LATER, grid, block, ...)                                                                \
    do {                                                                                                                   \
        if (p.first) hipLaunchKernelGGL(K_FIRST, grid, block, 0, s, v, __VA_ARGS__, sc.emul, sc.ginv, sc.cmul, p.full);    \
        else hipLaunchKernelGGL(K_LATER, grid, block, 0, s, v, __VA_ARGS__, sc.emul, sc.ginv, sc.cmul, p.full);            \
    } while (0)
#define BG_FUSED_LAUNCH(G)                                                                                                 \
    BG_TRACE_LAUNCH((td_step_fused_kernel<true, G>), (td_step_fused_kernel<false, G>), tgrid, wide, (long long)t, (long long)n_active, alpha)
    switch (p.trace) {
        case TdTrace::FUSED:
            switch (p.fuse_g) {
                case 1: BG_FUSED_LAUNCH(1); break;
                case 2: BG_FUSED_LAUNCH(2); break;
                case 4: BG_FUSED_LAUNCH(4); break;
                case 8: BG_FUSED_LAUNCH(8); break;
                default: BG_FUSED_LAUNCH(16); break;
            }
            break;
        case TdTrace::PIPE:
            BG_TRACE_LAUNCH((td_trace_pipe_kernel<true>), (td_trace_pipe_kernel<false>), tgrid, wide, (long long)n_active);
            break;
        case TdTrace::WIDE_NT:
            BG_TRACE_LAUNCH((td_trace_wide_kernel<true, true>), (td_trace_wide_kernel<false, true>), tgrid, wide, (long long)n_active);
            break;
        case TdTrace::WIDE:
            hipLaunchKernelGGL((td_trace_wide_kernel<false, false>), tgrid, wide, 0, s, v, (long long)n_active, sc.emul, sc.ginv, sc.cmul, p.full);
            break;
        case TdTrace::SLICE:
            BG_TRACE_LAUNCH(td_trace_kernel<true>, td_trace_kernel<false>, dim3(TD_SLICES, p.n_groups), dim3(TD_TRACE_THREADS), (long long)n_active,
                            (int)p.ng);
            break;
    }
#undef BG_FUSED_LAUNCH
#undef BG_TRACE_LAUNCH
    if (td->timing) {
        HIPCHK(hipEventRecord(e1, s));
        td->trace_launches++;
        td->trace_game_steps += (uint64_t)n_active;
    }
    hipLaunchKernelGGL(td_reduce_kernel, grid1(TD_P, 64), dim3(256), 0, s, v, p.n_groups, d_update, d_update ? 0 : 1);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_td_apply(bgamd_td *td, const float *d_update, void *stream)
{
    if (!td || !d_update) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    if (!td->has_weights) return BGAMD_E_NOWEIGHTS;
    hipLaunchKernelGGL(td_apply_kernel, grid1(TD_P, 256), dim3(256), 0, (hipStream_t)stream, td->v, d_update, 0);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

// The supervised step (bg_fit.h): rows and targets -> update = Σ_i fp32(alpha · (y_i - V(x_i))) ∇V(x_i), in chunks of td->tune.fit_chunk rows;
// every chunk is fit_step_kernel + fit_reduce_kernel, the last reduce hands the update out or applies it.  Stream-ordered, no host wait;
// touches nothing of a replay's state but the partial sums, which are free between replays.
int bgamd_td_fit_step(bgamd_td *td, const void *d_rows, const float *d_target, int64_t n, double alpha, float *d_update, void *stream)
{
    if (!td || n < 0 || (n > 0 && (!d_rows || !d_target))) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    if (!td->has_weights) return BGAMD_E_NOWEIGHTS;
    hipStream_t s = (hipStream_t)stream;
    td->fit_stream = s;
    if (n == 0) {                        // a rank without rows still hands a defined buffer to the collective
        if (d_update) HIPCHK(hipMemsetAsync(d_update, 0, (size_t)TD_P * 4, s));
        return BGAMD_OK;
    }
    const long long chunk = td->tune.fit_chunk;
    const long long n_chunks = (n + chunk - 1) / chunk;
    for (long long c = 0; c < n_chunks; ++c) {
        const long long r0 = c * chunk;
        const long long m = n - r0 < chunk ? n - r0 : chunk;
        FitView f{};
        f.rows = (const uint4 *)d_rows + 2 * r0;
        f.target = d_target + r0;
        f.m = m;
        f.tiles = (int)((m + FIT_TILE - 1) / FIT_TILE);
        f.theta = td->v.theta; f.w1t = td->v.w1t;
        f.partial = td->v.partial;
        f.part_sq = td->fit_part_sq; f.part_cnt = td->fit_part_cnt;
        const int groups = f.tiles < td->tune.fit_groups ? f.tiles : (int)td->tune.fit_groups;
        hipLaunchKernelGGL(fit_step_kernel, dim3(groups), dim3(FIT_THREADS), 0, s, f, alpha);
        const int last = c + 1 == n_chunks ? 1 : 0;
        hipLaunchKernelGGL(fit_reduce_kernel, grid1(TD_P, 64), dim3(256), 0, s, td->v, groups, td->fit_run, c == 0 ? 1 : 0, last, d_update,
                           d_update ? 0 : 1, (const double *)td->fit_part_sq, (const long long *)td->fit_part_cnt, td->fit_stat,
                           (long long *)(td->fit_stat + 1));
    }
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}

int bgamd_td_fit_stats(bgamd_td *td, double *h_sq_sum, int64_t *h_rows, int64_t *h_skipped)
{
    if (!td) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    double h[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, td->fit_stat, sizeof(h), hipMemcpyDeviceToHost, td->fit_stream));
    HIPCHK(hipMemsetAsync(td->fit_stat, 0, sizeof(h), td->fit_stream));
    HIPCHK(hipStreamSynchronize(td->fit_stream));
    long long cnt[2];
    memcpy(cnt, &h[1], sizeof(cnt));
    if (h_sq_sum) *h_sq_sum = h[0];
    if (h_rows) *h_rows = cnt[0];
    if (h_skipped) *h_skipped = cnt[1];
    return BGAMD_OK;
}

}  // extern "C"

namespace {
// The delayed replay: every step ONE launch of td_step_fused_kernel<., ., DELAY = true> (bg_learner.h).  Step t reads weight buffer t & 1 and the
// partial sums of step t - 1, writes weight buffer (t + 1) & 1 and its own partial sums (set t & 1); one flush launch at the end applies the last
// update and leaves the result in the learner's canonical buffers.
int td_replay_delayed(bgamd_td *td, int64_t n_steps, long long k, int fuse_g, double alpha, float lambda, hipStream_t s)
{
    if (!td->partial2) {                 // (the last of its buffers in the list: there once all of them are)
        if (const int rc = td_alloc(td, TD_AT_DELAY)) return rc;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipMemset(td->theta2[b], 0, (size_t)TD_LD * 4));
            HIPCHK(hipMemset(td->wl3_2[b], 0, 3 * EVAL16_W_BYTES));
        }
        HIPCHK(hipMemset(td->partial2, 0, ((size_t)TD_MAX_GROUPS * TD_LD + 64) * 4));
    }
    td->last_stream = s;
    HIPCHK(hipMemcpyAsync(td->theta2[0], td->v.theta, (size_t)TD_LD * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(td->wl3_2[0], td->v.wl3, 3 * EVAL16_W_BYTES, hipMemcpyDeviceToDevice, s));
    float *part[2] = {td->v.partial, td->partial2};
    const int n_groups = (int)((k + fuse_g - 1) / fuse_g);
    for (int64_t t = 0; t < n_steps; ++t) {
        const TdScale sc = td_scale_step(t, lambda, td->tune.lazy, td->scale);
        TdView v = td->v;
        v.full_step = sc.full;
        v.theta = td->theta2[t & 1];
        v.wl3 = td->wl3_2[t & 1];
        v.partial = part[t & 1];
        const float *pprev = part[(t + 1) & 1];
        const int n_prev = t == 0 ? 0 : n_groups;
        float *thn = td->theta2[(t + 1) & 1];
        uint16_t *wln = td->wl3_2[(t + 1) & 1];
#define BG_DELAY_LAUNCH(G)                                                                                                                   \
    do {                                                                                                                                     \
        if (t == 0)                                                                                                                          \
            hipLaunchKernelGGL((td_step_fused_kernel<true, G, true>), dim3(n_groups), dim3(TD_WIDE_THREADS), 0, s, v, (long long)t,           \
                               (long long)k, alpha, sc.emul, sc.ginv, sc.cmul, 1, pprev, n_prev, thn, wln);                                  \
        else                                                                                                                                 \
            hipLaunchKernelGGL((td_step_fused_kernel<false, G, true>), dim3(n_groups), dim3(TD_WIDE_THREADS), 0, s, v, (long long)t,          \
                               (long long)k, alpha, sc.emul, sc.ginv, sc.cmul, sc.full, pprev, n_prev, thn, wln);                            \
    } while (0)
        switch (fuse_g) {
            case 1: BG_DELAY_LAUNCH(1); break;
            case 2: BG_DELAY_LAUNCH(2); break;
            case 4: BG_DELAY_LAUNCH(4); break;
            case 8: BG_DELAY_LAUNCH(8); break;
            default: BG_DELAY_LAUNCH(16); break;
        }
#undef BG_DELAY_LAUNCH
    }
    // the update of the last step is still outstanding: theta = buffer n_steps & 1 + the sum of the last step's partial sums
    hipLaunchKernelGGL(td_delay_flush_kernel, dim3(TD_DELAY_SLICES), dim3(256), 0, s, (const float *)part[(n_steps + 1) & 1], n_steps ? n_groups : 0,
                       (const float *)td->theta2[n_steps & 1], td->v.theta, td->v.wl3, td->v.w1t);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}
}  // namespace

extern "C" {

int bgamd_td_set_delay(bgamd_td *td, int delay)
{
    if (!td || delay < 0 || delay > 1) return BGAMD_E_INVALID;
    td->delay = delay;
    return BGAMD_OK;
}

int bgamd_td_replay(bgamd_td *td, int64_t n_steps, const int64_t *h_n_active, double alpha, float lambda, void *stream)
{
    if (!td || !h_n_active || n_steps < 0 || (td->begun && !td->stream_mode && n_steps > td->v.T)) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    if (td->delay && td->begun && td->stream_mode && td->has_weights && n_steps > 0) {
        // a streamed replay through a constant number of slots may take the one-launch step (td_delay_g).  Anything else replays exactly, update
        // by update.
        bool same = true;
        for (int64_t t = 1; t < n_steps; ++t) same = same && h_n_active[t] == h_n_active[0];
        const long long k = h_n_active[0];
        const int g = same && k <= td->v.n_games ? td_delay_g(td->tune, td->n_cu, k) : 0;
        if (g > 0) return td_replay_delayed(td, n_steps, k, g, alpha, lambda, (hipStream_t)stream);
    }
    for (int64_t t = 0; t < n_steps; ++t) {
        if (h_n_active[t] == 0) continue;
        const int rc = bgamd_td_step(td, t, h_n_active[t], alpha, lambda, nullptr, stream);
        if (rc != BGAMD_OK) return rc;
    }
    return BGAMD_OK;
}

int bgamd_td_stats(bgamd_td *td, double *h_sq_sum, int64_t *h_updates)
{
    ENV_GUARD(td);
    HIPCHK(hipStreamSynchronize(td->last_stream));
    if (h_sq_sum) {
        std::vector<double> sq((size_t)td->v.n_games);
        if (!sq.empty()) HIPCHK(td_read(td, sq.data(), td->v.sq, sq.size() * 8));
        double acc = 0;
        for (double x : sq) acc += x;
        *h_sq_sum = acc;
    }
    if (h_updates) {
        uint64_t updates = 0;
        if (const int rc = td_sum_slots(td, td->v.nupd, &updates)) return rc;
        *h_updates = (int64_t)updates;
    }
    return BGAMD_OK;
}

int bgamd_td_active_columns(bgamd_td *td, uint64_t *h_columns)
{
    if (!td || !h_columns) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    HIPCHK(hipStreamSynchronize(td->last_stream));
    return td_sum_slots(td, td->v.act_cols, h_columns);
}

int bgamd_td_slots(bgamd_td *td, int32_t *h_out)
{
    if (!td || !h_out) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    HIPCHK(hipStreamSynchronize(td->last_stream));
    const size_t n = (size_t)td->v.n_games;
    std::vector<int32_t> gm(4 * n), qc(n);
    std::vector<unsigned int> nu(n);
    if (n) {
        HIPCHK(td_read(td, gm.data(), td->v.gmeta, n * 16));
        HIPCHK(td_read(td, qc.data(), td->v.qcur, n * 4));
        HIPCHK(td_read(td, nu.data(), td->v.nupd, n * 4));
    }
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 4; ++k) h_out[6 * i + k] = gm[4 * i + k];
        h_out[6 * i + 2] &= 1;                                 // (the word also carries the game's first log row)
        h_out[6 * i + 4] = td->stream_mode ? qc[i] : -1;
        h_out[6 * i + 5] = (int32_t)nu[i];
    }
    return BGAMD_OK;
}

int bgamd_td_written_columns(bgamd_td *td, uint64_t *h_columns)
{
    if (!td || !h_columns) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    HIPCHK(hipStreamSynchronize(td->last_stream));
    return td_sum_slots(td, td->v.wr_cols, h_columns);
}

int bgamd_td_time(bgamd_td *td, int enable)
{
    ENV_GUARD(td);
    if (!enable && td->timing) { const int rc = td_flush(td); if (rc) return rc; }
    td->timing = enable != 0;
    return BGAMD_OK;
}

int bgamd_td_times(bgamd_td *td, double *h_trace_ms, uint64_t *h_launches, uint64_t *h_game_steps)
{
    ENV_GUARD(td);
    const int rc = td_flush(td);
    if (rc) return rc;
    if (h_trace_ms) *h_trace_ms = td->trace_ms;
    if (h_launches) *h_launches = td->trace_launches;
    if (h_game_steps) *h_game_steps = td->trace_game_steps;
    td->trace_ms = 0; td->trace_launches = 0; td->trace_game_steps = 0;
    return BGAMD_OK;
}

// ---- the ONE collective of a multi-rank training step, issued by the library -----------------------------------------------
// one all-reduce (sum) of the 25 601-float update per training step, in place, on the compute stream.  Rounds 1-3 drove
// it from Python (bgamd_td_step -> torch.distributed.all_reduce -> bgamd_td_apply): 9.5 us of host time per step for the dispatch
// alone.  Here the learner owns an RCCL communicator and a step is three enqueues from C on ONE stream: the step's kernels with the
// update handed out, ncclAllReduce in place, the apply kernel.  RCCL is resolved at run time -- the librccl.so.1 that is already in the
// process (PyTorch brings its own) or the one of the ROCm install -- so libbgamd.so has no link-time dependency on it.
}  // extern "C"

namespace {
struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi *rccl_api()
{
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.h ? &api : nullptr;
    tried = true;
    const char *names[] = {getenv("BGAMD_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names)                              // the copy that is already loaded wins: two RCCLs in one process is one too many
        if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char *n : names)
        if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) { g_hip_err = std::string("librccl.so.1 not found: ") + (dlerror() ? dlerror() : ""); return nullptr; }
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))dlsym(h, "ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.GetErrorString) {
        g_hip_err = "librccl: a symbol is missing";
        return nullptr;
    }
    api.h = h;
    return &api;
}

#define RCCLCHK(api, call)                                                                  \
    do {                                                                                    \
        ncclResult_t _r = (call);                                                           \
        if (_r != ncclSuccess) {                                                            \
            g_hip_err = std::string(#call) + ": " + (api)->GetErrorString(_r);              \
            return BGAMD_E_HIP;                                                             \
        }                                                                                   \
    } while (0)

// the tail of a multi-rank step: the rank's update in d_upd -> all-reduced in place -> applied, on the step's stream
int td_allreduce_apply(bgamd_td *td, hipStream_t s)
{
    RcclApi *api = rccl_api();
    RCCLCHK(api, api->AllReduce(td->d_upd, td->d_upd, (size_t)TD_P, ncclFloat32, ncclSum, (ncclComm_t)td->comm, s));
    hipLaunchKernelGGL(td_apply_kernel, grid1(TD_P, 256), dim3(256), 0, s, td->v, (const float *)td->d_upd, 0);
    HIPCHK(hipGetLastError());
    return BGAMD_OK;
}
}  // namespace

extern "C" {

int bgamd_td_comm_unique_id(uint8_t h_id[128])
{
    if (!h_id) return BGAMD_E_INVALID;
    RcclApi *api = rccl_api();
    if (!api) return BGAMD_E_HIP;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    RCCLCHK(api, api->GetUniqueId(&id));
    memcpy(h_id, &id, 128);
    return BGAMD_OK;
}

int bgamd_td_comm_init(bgamd_td *td, const uint8_t h_id[128], int rank, int world)
{
    if (!td || !h_id || world < 1 || rank < 0 || rank >= world) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    RcclApi *api = rccl_api();
    if (!api) return BGAMD_E_HIP;
    bgamd_td_comm_destroy(td);
    if (const int rc = td_alloc(td, TD_AT_COMM)) return rc;
    ncclUniqueId id;
    memcpy(&id, h_id, 128);
    ncclComm_t comm = nullptr;
    RCCLCHK(api, api->CommInitRank(&comm, world, id, rank));
    td->comm = comm; td->comm_rank = rank; td->comm_world = world;
    return BGAMD_OK;
}

int bgamd_td_comm_destroy(bgamd_td *td)
{
    if (!td) return BGAMD_E_INVALID;
    if (td->comm) {
        RcclApi *api = rccl_api();
        hipSetDevice(td->device);
        hipDeviceSynchronize();
        if (api) api->CommDestroy((ncclComm_t)td->comm);
        td->comm = nullptr; td->comm_world = 0;
    }
    return BGAMD_OK;
}

int bgamd_td_step_allreduce(bgamd_td *td, int64_t t, int64_t n_active, double alpha, float lambda, void *stream)
{
    if (!td || !td->comm || !td->d_upd) return BGAMD_E_INVALID;
    HIPCHK(hipSetDevice(td->device));
    hipStream_t s = (hipStream_t)stream;
    if (n_active > 0) {
        const int rc = bgamd_td_step(td, t, n_active, alpha, lambda, td->d_upd, stream);
        if (rc) return rc;
    } else {                                                 // this rank has nothing at step t: it still joins the collective
        if (!td->has_weights) return BGAMD_E_NOWEIGHTS;
        HIPCHK(hipMemsetAsync(td->d_upd, 0, (size_t)TD_P * 4, s));
        td->last_stream = s;
    }
    return td_allreduce_apply(td, s);
}

// the supervised step of a multi-rank fit: fit step with the update handed out -> ncclAllReduce -> apply, as bgamd_td_step_allreduce
int bgamd_td_fit_step_allreduce(bgamd_td *td, const void *d_rows, const float *d_target, int64_t n, double alpha, void *stream)
{
    if (!td || !td->comm || !td->d_upd) return BGAMD_E_INVALID;
    const int rc = bgamd_td_fit_step(td, d_rows, d_target, n, alpha, td->d_upd, stream);
    if (rc) return rc;
    return td_allreduce_apply(td, (hipStream_t)stream);
}

int bgamd_td_replay_allreduce(bgamd_td *td, int64_t n_steps, const int64_t *h_n_active, int64_t n_own_steps, double alpha, float lambda,
                              void *stream)
{
    if (!td || n_steps < 0 || n_own_steps < 0 || n_own_steps > n_steps || (n_own_steps > 0 && !h_n_active)) return BGAMD_E_INVALID;
    for (int64_t t = 0; t < n_steps; ++t) {
        const int rc = bgamd_td_step_allreduce(td, t, t < n_own_steps ? h_n_active[t] : 0, alpha, lambda, stream);
        if (rc != BGAMD_OK) return rc;
    }
    return BGAMD_OK;
}

}  // extern "C"
