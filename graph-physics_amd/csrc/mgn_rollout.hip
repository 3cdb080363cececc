// Validation rollout from resident trajectories (mgn.h, "Resident rollout"): the data work before and after
// the Simulator's evaluation forward of one autoregressive step (reference lightning_module.py:168-249), with
// the step counter on the device, so a whole trajectory is S replays of one captured graph.
//
// rollout_begin is feed_batch's mapping (mgn_feed.hip): one thread per element (r, c) of the [N, F] frame,
// consecutive lanes on consecutive floats, the graph of a row from the shared binary search. The step counter
// is one int32 every thread reads at the same address (a scalar load). From the second step on, the columns
// of the model's output (and of the previous-data channel) take the previous prediction instead of the frame.
//
// rollout_end is masked_mse's partial / final pair (mgn_graph.hip) with the masking, the feedback state and
// the stored prediction folded into the partial pass: the same grid, the same rows per block, the same strided
// rows, the same LDS tree and the same single final wave, over the row term of mgn_common.h, so loss[cursor] is
// mgn_masked_mse(y, pred)'s value bit for bit. One thread owns one row (d floats, 8 to 12 bytes for the
// velocity and position targets): the row's node type, its d targets, outputs and current values are read once
// and every result of the row is written from registers. Only the final kernel writes the step counter, so by
// stream order every earlier kernel of the step has read the old value. No atomics.
//
// rollout_begin_world is the begin stage for Lagrangian data: the batch row [world(3), obstacle displacement(3),
// the other frame columns] of mgn_feed_batch_world, noise-free, at frame + step, then the same feedback.
//
// rollout_begin_aneurysm is the begin stage for aneurysm data: the batch row [frame row, acceleration, pos, inflow
// statistics, node type] of mgn_feed_batch_aneurysm, noise-free, at frame + step, then the same feedback. One launch.
#include "mgn_common.h"

namespace {

__global__ __launch_bounds__(256) void rollout_begin(const float* __restrict__ traj, int64_t T, int64_t N, int F,
                                                     const int32_t* __restrict__ graph_ptr, int B,
                                                     const int32_t* __restrict__ frame,
                                                     const int32_t* __restrict__ cursor, int y_start, int y_end,
                                                     int o_start, int o_end, int p_start, int p_end,
                                                     const float* __restrict__ last, int64_t ld_last,
                                                     const float* __restrict__ last_prev, int64_t ld_prev,
                                                     float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                     int64_t ldy) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * F;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)  // uniform: the 32-bit division where it suffices
        r = (uint32_t)e / (uint32_t)F;
    else
        r = e / F;
    const int c = (int)(e - r * F);
    const int s = *cursor;
    const int64_t t = (int64_t)frame[graph_of_row(graph_ptr, B, r)] + s;
    if (t < 0 || t > T - 2) return;  // the host keeps frame + cursor inside the trajectory; never read past it
    const float* src = traj + (t * N + r) * F;
    float v = src[c];
    if (s > 0) {  // feed the previous prediction back (reference _make_prediction)
        if (c >= o_start && c < o_end)
            v = last[r * ld_last + (c - o_start)];
        else if (c >= p_start && c < p_end)
            v = last_prev[r * ld_prev + (c - p_start)];
    }
    x[r * ldx + c] = v;
    if (c >= y_start && c < y_end) y[r * ldy + (c - y_start)] = src[(int64_t)N * F + c];
}

// ---- the begin stage on Lagrangian data (mgn.h, "Resident rollout with world positions") ----
//
// rollout_world_mean is mgn_feed_batch_world's reduction (world_obstacle_mean_of_graph, mgn_common.h) at frame
// frame[g] + *cursor: one workgroup per graph, the same order, so the same bits as the feed's at that frame. The
// step counter and the graph's frame are the same for the whole workgroup, so a step outside the trajectory
// leaves it as one, ahead of the reduction's barrier.
__global__ __launch_bounds__(WORLD_MEAN_THREADS) void rollout_world_mean(
    const float* __restrict__ traj, int64_t T, int64_t N, int F, const int32_t* __restrict__ graph_ptr,
    const int32_t* __restrict__ frame, const int32_t* __restrict__ cursor, int type_index,
    float* __restrict__ mean) {
    const int g = blockIdx.x;
    const int64_t t = (int64_t)frame[g] + *cursor;
    if (t < 0 || t > T - 2) return;  // uniform: nothing of this graph is read or written
    const float* cur = traj + t * N * F;
    world_obstacle_mean_of_graph(cur, cur + N * F, F, graph_ptr[g], graph_ptr[g + 1], type_index,
                                 mean + 3 * (int64_t)g);
}

// feed_batch_world's fill (mgn_feed.hip) without the noise, at frame frame[g] + *cursor, then rollout_begin's
// feedback in batch-layout columns: one thread per element (r, c) of [N, F + 3], consecutive lanes on
// consecutive floats of x. The displacement and the mean always come from the clean frames; the thread of a
// world column c < 3 also stores the clean position into world_clean [N, 3] (12 bytes per row, contiguous over
// the rows), what the "frame" edge mode gathers from.
__global__ __launch_bounds__(256) void rollout_begin_world(
    const float* __restrict__ traj, int64_t T, int64_t N, int F, const int32_t* __restrict__ graph_ptr, int B,
    const int32_t* __restrict__ frame, const int32_t* __restrict__ cursor, int y_end, int type_index, int o_start,
    int o_end, int p_start, int p_end, const float* __restrict__ last, int64_t ld_last,
    const float* __restrict__ last_prev, int64_t ld_prev, float* __restrict__ x, int64_t ldx,
    float* __restrict__ y, int64_t ldy, const float* __restrict__ mean, float* __restrict__ world_clean) {
#pragma clang fp contract(off)
    const int Fx = F + 3;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * Fx;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)  // uniform: the 32-bit division where it suffices
        r = (uint32_t)e / (uint32_t)Fx;
    else
        r = e / Fx;
    const int c = (int)(e - r * Fx);
    const int g = graph_of_row(graph_ptr, B, r);
    const int s = *cursor;
    const int64_t t = (int64_t)frame[g] + s;
    if (t < 0 || t > T - 2) return;  // as rollout_begin: never read past the trajectory
    const float* a = traj + (t * N + r) * F;
    const float* n = a + (int64_t)N * F;
    float v;
    if (c < 3)
        v = a[c];
    else if (c < 6)
        v = a[type_index] == 1.f ? n[c - 3] - a[c - 3] : mean[3 * (int64_t)g + (c - 3)];
    else
        v = a[c - 3];
    if (c < 3 && world_clean != nullptr) world_clean[r * 3 + c] = v;
    if (s > 0) {  // feed the previous prediction back, after the fill (reference _make_prediction)
        if (c >= o_start && c < o_end)
            v = last[r * ld_last + (c - o_start)];
        else if (c >= p_start && c < p_end)
            v = last_prev[r * ld_prev + (c - p_start)];
    }
    x[r * ldx + c] = v;
    if (c < y_end) y[r * ldy + c] = n[c];  // y_start == 0 (checked on the host)
}

// ---- the begin stage on aneurysm data (mgn.h, "Resident rollout with the aneurysm features") ----
//
// feed_batch_aneurysm's fill (mgn_feed.hip) without the noise, at frame frame[g] + *cursor, then rollout_begin's
// feedback in batch-layout columns: one thread per element (r, c) of [N, F + 10], consecutive lanes on
// consecutive floats of x. The row comes from aneurysm_row_value (mgn_common.h), as the feed's does. Frame t − 1
// is read too, so a step is inside the trajectory when 1 <= t <= T − 2; outside it the thread returns before it
// forms an address. The statistics are row (t, g) of the clean-frame table: the inflow rows are masked back to the
// target on every step, so a recomputation from the prediction would give the same values.
__global__ __launch_bounds__(256) void rollout_begin_aneurysm(
    const float* __restrict__ traj, int64_t T, int64_t N, int F, const int32_t* __restrict__ graph_ptr, int B,
    const int32_t* __restrict__ frame, const int32_t* __restrict__ cursor, int y_start, int y_end,
    const float* __restrict__ pos, const float* __restrict__ node_type, const float* __restrict__ stats, int o_start,
    int o_end, int p_start, int p_end, const float* __restrict__ last, int64_t ld_last,
    const float* __restrict__ last_prev, int64_t ld_prev, float* __restrict__ x, int64_t ldx,
    float* __restrict__ y, int64_t ldy) {
#pragma clang fp contract(off)
    const int Fx = F + 10;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * Fx;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)  // uniform: the 32-bit division where it suffices
        r = (uint32_t)e / (uint32_t)Fx;
    else
        r = e / Fx;
    const int c = (int)(e - r * Fx);
    const int g = graph_of_row(graph_ptr, B, r);
    const int s = *cursor;
    const int64_t t = (int64_t)frame[g] + s;
    if (t < 1 || t > T - 2) return;  // frames t − 1, t and t + 1 are read: never leave the trajectory
    const float* a = traj + (t * N + r) * F;
    float v = aneurysm_row_value(a, a - (int64_t)N * F, F, c, pos + r * 3, stats + (t * B + g) * 3, node_type[r]);
    if (s > 0) {  // feed the previous prediction back, after the fill (reference _make_prediction)
        if (c >= o_start && c < o_end)
            v = last[r * ld_last + (c - o_start)];
        else if (c >= p_start && c < p_end)
            v = last_prev[r * ld_prev + (c - p_start)];
    }
    x[r * ldx + c] = v;
    if (c >= y_start && c < y_end) y[r * ldy + (c - y_start)] = (a + (int64_t)N * F)[c];  // y_end <= F
}

// part[3 * block] = {Σ m·err, Σ m, Σ err} of the block's rows
__global__ __launch_bounds__(256) void rollout_end_partial(const float* __restrict__ out, const float* __restrict__ y,
                                                           const float* __restrict__ x, int64_t N, int64_t ldx,
                                                           int type_index, unsigned tmask, int o_start, int d,
                                                           float* __restrict__ last, float* __restrict__ last_prev,
                                                           float* __restrict__ preds, int capacity,
                                                           const int32_t* __restrict__ cursor, int64_t rows_per_block,
                                                           float* __restrict__ part) {
    __shared__ float red[3][256];
    const int s = *cursor;
    if (s < 0 || s >= capacity) return;  // uniform; the host never enqueues more steps than the buffers hold
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    float* __restrict__ keep_to = preds ? preds + (int64_t)s * N * d : nullptr;
    float acc = 0.f, cnt = 0.f, all = 0.f;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const float* xr = x + r * ldx;
        const float type = xr[type_index];
        // build_mask: every node that is neither NORMAL (0) nor OUTFLOW (5) keeps its ground truth
        const bool keep = !(type == 0.f || type == 5.f);
        const float m = type_mask_of(xr + type_index, ldx, 0, tmask);
        float e = 0.f;
        for (int c = 0; c < d; ++c) {
            const float tgt = y[r * d + c];
            const float p = keep ? tgt : out[r * d + c];
            last[r * d + c] = p;
            if (last_prev) last_prev[r * d + c] = p - xr[o_start + c];
            if (keep_to) keep_to[r * d + c] = p;
            e = mse_col_add(e, p, tgt);
        }
        acc = mse_row_add(acc, m, e);
        cnt += m;
        all += e;
    }
    red[0][threadIdx.x] = acc;
    red[1][threadIdx.x] = cnt;
    red[2][threadIdx.x] = all;
    mse_block_tree<3>(red);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = red[0][0];
        part[3 * blockIdx.x + 1] = red[1][0];
        part[3 * blockIdx.x + 2] = red[2][0];
    }
}

__global__ __launch_bounds__(64) void rollout_end_final(const float* __restrict__ part, int nblocks, int d,
                                                        int capacity, int32_t* cursor, float* __restrict__ loss,
                                                        float* __restrict__ sq) {
    const int lane = threadIdx.x;
    const int s = *cursor;
    if (s < 0 || s >= capacity) return;
    float a = 0.f, c = 0.f, q = 0.f;
    for (int b = lane; b < nblocks; b += 64) {
        a += part[3 * b];
        c += part[3 * b + 1];
        q += part[3 * b + 2];
    }
    a = mse_wave_sum(a);
    c = mse_wave_sum(c);
    q = mse_wave_sum(q);
    if (lane == 0) {
        loss[s] = a / (c * (float)d);
        sq[s] = q;
        *cursor = s + 1;
    }
}

}  // namespace

extern "C" {

int mgn_rollout_begin(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                      const int32_t* frame, const int32_t* cursor, int32_t y_start, int32_t y_end,
                      int32_t out_start, int32_t out_end, int32_t prev_start, int32_t prev_end, const float* last,
                      int64_t ld_last, const float* last_prev, int64_t ld_prev, float* x, int64_t ldx, float* y,
                      int64_t ldy, mgn_stream_t stream) {
    MGN_REQUIRE(T >= 2, "rollout_begin: a trajectory needs at least 2 frames (x from frame t, y from t + 1)");
    MGN_REQUIRE(F >= 1, "rollout_begin: F must be >= 1");
    MGN_REQUIRE(N >= 0 && B >= 0, "rollout_begin: N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, "rollout_begin: graph_ptr is int32, N must fit it");
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, "rollout_begin: the y column range is outside [0, F]");
    MGN_REQUIRE(out_start >= 0 && out_start < out_end && out_end <= F,
                "rollout_begin: the output column range must be a non-empty range inside [0, F]");
    MGN_REQUIRE(prev_start >= 0 && prev_start <= prev_end && prev_end <= F,
                "rollout_begin: the previous-data column range is outside [0, F]");
    MGN_REQUIRE(prev_start == prev_end || prev_start >= out_end || out_start >= prev_end,
                "rollout_begin: the output and previous-data column ranges overlap");
    MGN_REQUIRE(ldx >= F, "rollout_begin: ldx is smaller than F");
    MGN_REQUIRE(ldy >= y_end - y_start, "rollout_begin: ldy is smaller than the y column count");
    MGN_REQUIRE(ld_last >= out_end - out_start, "rollout_begin: ld_last is smaller than the output column count");
    MGN_REQUIRE(prev_start == prev_end || ld_prev >= prev_end - prev_start,
                "rollout_begin: ld_prev is smaller than the previous-data column count");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && cursor && last && x && (y || y_start == y_end),
                "rollout_begin: a null pointer argument");
    MGN_REQUIRE(prev_start == prev_end || last_prev != nullptr,
                "rollout_begin: a previous-data column range without last_prev");
    const int64_t blocks = cdiv64(N * F, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, "rollout_begin: N * F is too large for one launch");
    hipLaunchKernelGGL(rollout_begin, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, T, N, (int)F,
                       graph_ptr, (int)B, frame, cursor, (int)y_start, (int)y_end, (int)out_start, (int)out_end,
                       (int)prev_start, (int)prev_end, last, ld_last, last_prev, ld_prev, x, ldx, y, ldy);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_rollout_begin_world(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                            const int32_t* frame, const int32_t* cursor, int32_t y_start, int32_t y_end,
                            int32_t type_index, int32_t out_start, int32_t out_end, int32_t prev_start,
                            int32_t prev_end, const float* last, int64_t ld_last, const float* last_prev,
                            int64_t ld_prev, float* x, int64_t ldx, float* y, int64_t ldy, float* obstacle_mean,
                            float* world_clean, mgn_stream_t stream) {
    const std::string who = "rollout_begin_world";
    MGN_REQUIRE(T >= 2, who + ": a trajectory needs at least 2 frames (x from frame t, y from t + 1)");
    MGN_REQUIRE(F >= 4 && F <= INT32_MAX - 3, who + ": F must be >= 4 (world position and a node type)");
    MGN_REQUIRE(N >= 0 && B >= 0, who + ": N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, who + ": graph_ptr is int32, N must fit it");
    const int32_t Fx = F + 3;  // the width of a batch row
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, who + ": the y column range is outside [0, F]");
    MGN_REQUIRE(y_start == 0 && y_end >= 3, who + ": the y columns must begin with the world position "
                                                  "(y_start == 0, y_end >= 3)");
    MGN_REQUIRE(type_index >= 3 && type_index < F,
                who + ": type_index must be a frame column outside the world position, in [3, F)");
    MGN_REQUIRE(out_start >= 0 && out_start < out_end && out_end <= Fx,
                who + ": the output column range must be a non-empty range inside [0, F + 3]");
    MGN_REQUIRE(prev_start >= 0 && prev_start <= prev_end && prev_end <= Fx,
                who + ": the previous-data column range is outside [0, F + 3]");
    MGN_REQUIRE(prev_start == prev_end || prev_start >= out_end || out_start >= prev_end,
                who + ": the output and previous-data column ranges overlap");
    MGN_REQUIRE(type_index + 3 < out_start || type_index + 3 >= out_end,
                who + ": the output column range contains the node type (batch column type_index + 3)");
    MGN_REQUIRE(prev_start == prev_end || type_index + 3 < prev_start || type_index + 3 >= prev_end,
                who + ": the previous-data column range contains the node type (batch column type_index + 3)");
    MGN_REQUIRE(ldx >= Fx, who + ": ldx is smaller than F + 3");
    MGN_REQUIRE(ldy >= y_end - y_start, who + ": ldy is smaller than the y column count");
    MGN_REQUIRE(ld_last >= out_end - out_start, who + ": ld_last is smaller than the output column count");
    MGN_REQUIRE(prev_start == prev_end || ld_prev >= prev_end - prev_start,
                who + ": ld_prev is smaller than the previous-data column count");
    MGN_REQUIRE(obstacle_mean != nullptr, who + ": obstacle_mean is null");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && cursor && x && y, who + ": a null pointer argument");
    MGN_REQUIRE(last != nullptr, who + ": an output column range without last");
    MGN_REQUIRE(prev_start == prev_end || last_prev != nullptr,
                who + ": a previous-data column range without last_prev");
    const int64_t blocks = cdiv64(N * Fx, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, who + ": N * (F + 3) is too large for one launch");
    hipLaunchKernelGGL(rollout_world_mean, dim3((unsigned)B), dim3(WORLD_MEAN_THREADS), 0, (hipStream_t)stream, traj,
                       T, N, (int)F, graph_ptr, frame, cursor, (int)type_index, obstacle_mean);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rollout_begin_world, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, T, N,
                       (int)F, graph_ptr, (int)B, frame, cursor, (int)y_end, (int)type_index, (int)out_start,
                       (int)out_end, (int)prev_start, (int)prev_end, last, ld_last, last_prev, ld_prev, x, ldx, y, ldy,
                       (const float*)obstacle_mean, world_clean);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_rollout_begin_aneurysm(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr,
                               int32_t B, const int32_t* frame, const int32_t* cursor, int32_t y_start,
                               int32_t y_end, const float* pos, const float* node_type, const float* stats,
                               int32_t out_start, int32_t out_end, int32_t prev_start, int32_t prev_end,
                               const float* last, int64_t ld_last, const float* last_prev, int64_t ld_prev, float* x,
                               int64_t ldx, float* y, int64_t ldy, mgn_stream_t stream) {
    const std::string who = "rollout_begin_aneurysm";
    MGN_REQUIRE(T >= 3, who + ": a trajectory needs at least 3 frames (x from frames t - 1 and t, y from t + 1)");
    MGN_REQUIRE(F >= 4 && F <= INT32_MAX - 10, who + ": F must be >= 4 (velocity and the wall flag)");
    MGN_REQUIRE(N >= 0 && B >= 0, who + ": N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, who + ": graph_ptr is int32, N must fit it");
    const int32_t Fx = F + 10;  // the width of a batch row; the node type is its last column
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, who + ": the y column range is outside [0, F]");
    MGN_REQUIRE(out_start >= 0 && out_start < out_end && out_end <= Fx,
                who + ": the output column range must be a non-empty range inside [0, F + 10]");
    MGN_REQUIRE(prev_start >= 0 && prev_start <= prev_end && prev_end <= Fx,
                who + ": the previous-data column range is outside [0, F + 10]");
    MGN_REQUIRE(prev_start == prev_end || prev_start >= out_end || out_start >= prev_end,
                who + ": the output and previous-data column ranges overlap");
    MGN_REQUIRE(out_end <= Fx - 1, who + ": the output column range contains the node type (batch column F + 9)");
    MGN_REQUIRE(prev_start == prev_end || prev_end <= Fx - 1,
                who + ": the previous-data column range contains the node type (batch column F + 9)");
    MGN_REQUIRE(ldx >= Fx, who + ": ldx is smaller than F + 10");
    MGN_REQUIRE(ldy >= y_end - y_start, who + ": ldy is smaller than the y column count");
    MGN_REQUIRE(ld_last >= out_end - out_start, who + ": ld_last is smaller than the output column count");
    MGN_REQUIRE(prev_start == prev_end || ld_prev >= prev_end - prev_start,
                who + ": ld_prev is smaller than the previous-data column count");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && cursor && pos && node_type && stats && x && (y || y_start == y_end),
                who + ": a null pointer argument");
    MGN_REQUIRE(last != nullptr, who + ": an output column range without last");
    MGN_REQUIRE(prev_start == prev_end || last_prev != nullptr,
                who + ": a previous-data column range without last_prev");
    const int64_t blocks = cdiv64(N * Fx, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, who + ": N * (F + 10) is too large for one launch");
    hipLaunchKernelGGL(rollout_begin_aneurysm, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, T, N,
                       (int)F, graph_ptr, (int)B, frame, cursor, (int)y_start, (int)y_end, pos, node_type, stats,
                       (int)out_start, (int)out_end, (int)prev_start, (int)prev_end, last, ld_last, last_prev, ld_prev,
                       x, ldx, y, ldy);
    MGN_LAUNCH_CHECK();
    return 0;
}

size_t mgn_rollout_end_workspace_bytes(int64_t N) {
    (void)N;
    return 3 * MSE_BLOCKS * sizeof(float);
}

int mgn_rollout_end(const float* out, const float* y, const float* x, int64_t N, int64_t ldx, int32_t type_index,
                    uint32_t loss_type_mask, int32_t out_start, int32_t d, float* last, float* last_prev,
                    float* preds, int32_t capacity, int32_t* cursor, float* loss, float* sq, void* ws,
                    size_t ws_bytes, mgn_stream_t stream) {
    MGN_REQUIRE(N >= 0, "rollout_end: N must be >= 0");
    MGN_REQUIRE(d >= 1, "rollout_end: d must be >= 1");
    MGN_REQUIRE(out_start >= 0 && (int64_t)out_start + d <= ldx, "rollout_end: the output columns are outside x");
    MGN_REQUIRE(type_index >= 0 && type_index < ldx, "rollout_end: type_index is outside x");
    MGN_REQUIRE(type_index < out_start || type_index >= out_start + d,
                "rollout_end: type_index lies inside the output columns");
    MGN_REQUIRE(capacity >= 1, "rollout_end: capacity must be >= 1");
    MGN_REQUIRE(ws_bytes >= mgn_rollout_end_workspace_bytes(N), "rollout_end: workspace too small");
    if (N == 0) return 0;
    MGN_REQUIRE(out && y && x && last && cursor && loss && sq && ws, "rollout_end: a null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    float* part = reinterpret_cast<float*>(ws);
    const int64_t rpb = mse_rows_per_block(N);
    const int nb = mse_blocks(N);
    hipLaunchKernelGGL(rollout_end_partial, dim3(nb), dim3(256), 0, st, out, y, x, N, ldx, (int)type_index,
                       loss_type_mask, (int)out_start, (int)d, last, last_prev, preds, (int)capacity,
                       (const int32_t*)cursor, rpb, part);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rollout_end_final, dim3(1), dim3(64), 0, st, (const float*)part, nb, (int)d, (int)capacity,
                       cursor, loss, sq);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
