// Training batches from resident trajectories (mgn.h, "Resident trajectories"): one launch writes the
// batch's x (frame[g] of every graph, the reference's add_noise on NORMAL rows; reference
// dataset/preprocessing.py:177-238) and y (the dynamic columns of the next clean frame;
// dataset/h5_dataset.py:81-92). traj is only ever read.
//
// One thread owns one element (r, c) of the [N, F] frame. Within a graph both the source (frame t of
// traj, rows graph_ptr[g] .. graph_ptr[g+1]) and x (when ldx == F) are one contiguous span, so consecutive
// lanes read and write consecutive floats: 256 B per wave and instruction, whatever F is. Rows are 3 to
// 24 floats and a graph's span starts at a multiple of 4·F bytes only, so wider per-lane accesses would
// need a peeled head and tail per graph for a kernel that moves well under a megabyte per launch. The
// thread of a y column also copies that column of frame t+1, so every byte of x, y, z and of the two frames
// is touched once; the node type of a row is re-read by the threads of its noisy columns from the line
// their own load of the row brought in. The graph of a row is a binary search of graph_ptr (B + 1 ints,
// the same few cache lines for every thread). The noisy ranges ride in the kernel arguments; the loop over
// them is unrolled with constant indices, so they stay in scalar registers.
#include "mgn_common.h"

namespace {

__global__ __launch_bounds__(256) void feed_batch(const float* __restrict__ traj, int64_t N, int F,
                                                  const int32_t* __restrict__ graph_ptr, int B,
                                                  const int32_t* __restrict__ frame, int y_start, int y_end,
                                                  int type_index, mgn_feed_ranges rg,
                                                  const float* __restrict__ scales, const float* __restrict__ z,
                                                  int64_t ldz, float* __restrict__ x, int64_t ldx,
                                                  float* __restrict__ y, int64_t ldy) {
#pragma clang fp contract(off)  // x + z·s: a rounded product, then a rounded sum (hipcc contracts by default)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * F;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)  // uniform: the 32-bit division where it suffices
        r = (uint32_t)e / (uint32_t)F;
    else
        r = e / F;
    const int c = (int)(e - r * F);
    const int64_t t = frame[graph_of_row(graph_ptr, B, r)];
    const float* src = traj + (t * N + r) * F;
    float v = src[c];
    if (z != nullptr) {
        int zc = -1, which = 0, w = 0;
#pragma unroll
        for (int i = 0; i < MGN_FEED_MAX_RANGES; ++i)
            if (i < rg.n) {
                if (c >= rg.start[i] && c < rg.end[i]) {
                    zc = w + c - rg.start[i];
                    which = i;
                }
                w += rg.end[i] - rg.start[i];
            }
        // torch's composition: the rounded product, then the rounded sum. Plain operators under the pragma
        // above: __fmul_rn / __fadd_rn are inline functions of the HIP headers, compiled with the headers'
        // own contraction setting, and their inlined product and sum were fused into one v_fmac_f32
        if (zc >= 0 && src[type_index] == 0.f) {
            const float noise = z[r * ldz + zc] * scales[which];
            v = v + noise;
        }
    }
    x[r * ldx + c] = v;
    if (c >= y_start && c < y_end) y[r * ldy + (c - y_start)] = src[(int64_t)N * F + c];
}

}  // namespace

extern "C" {

int mgn_feed_batch(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                   const int32_t* frame, int32_t y_start, int32_t y_end, int32_t type_index, mgn_feed_ranges ranges,
                   const float* scales, const float* z, int64_t ldz, float* x, int64_t ldx, float* y, int64_t ldy,
                   mgn_stream_t stream) {
    MGN_REQUIRE(T >= 2, "feed_batch: a trajectory needs at least 2 frames (x from frame t, y from t + 1)");
    MGN_REQUIRE(F >= 1, "feed_batch: F must be >= 1");
    MGN_REQUIRE(N >= 0 && B >= 0, "feed_batch: N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, "feed_batch: graph_ptr is int32, N must fit it");
    MGN_REQUIRE(ranges.n >= 0 && ranges.n <= MGN_FEED_MAX_RANGES, "feed_batch: at most 4 noisy column ranges");
    int64_t W = 0;
    for (int i = 0; i < ranges.n; ++i) {
        MGN_REQUIRE(ranges.start[i] >= 0 && ranges.start[i] <= ranges.end[i] && ranges.end[i] <= F,
                    "feed_batch: a noisy column range is outside [0, F]");
        for (int j = 0; j < i; ++j)
            MGN_REQUIRE(ranges.start[i] >= ranges.end[j] || ranges.start[j] >= ranges.end[i] ||
                            ranges.start[i] == ranges.end[i] || ranges.start[j] == ranges.end[j],
                        "feed_batch: noisy column ranges overlap");
        W += ranges.end[i] - ranges.start[i];
    }
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, "feed_batch: the y column range is outside [0, F]");
    MGN_REQUIRE(type_index >= 0 && type_index < F, "feed_batch: type_index is outside [0, F)");
    MGN_REQUIRE(ldx >= F, "feed_batch: ldx is smaller than F");
    MGN_REQUIRE(ldy >= y_end - y_start, "feed_batch: ldy is smaller than the y column count");
    MGN_REQUIRE(z == nullptr || ldz >= W, "feed_batch: ldz is smaller than the noisy column count");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && x && (y || y_start == y_end), "feed_batch: a null pointer argument");
    MGN_REQUIRE(z == nullptr || W == 0 || scales != nullptr, "feed_batch: noise (z) without scales");
    const int64_t blocks = cdiv64(N * F, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, "feed_batch: N * F is too large for one launch");
    hipLaunchKernelGGL(feed_batch, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, N, (int)F,
                       graph_ptr, (int)B, frame, (int)y_start, (int)y_end, (int)type_index, ranges, scales,
                       W > 0 ? z : nullptr, ldz, x, ldx, y, ldy);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
