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
//
// Rotation augmentation (the reference's Random3DRotate, dataset/preprocessing.py:277-366, one rotation per
// graph): feed_batch_rot is feed_batch with column triples and R [B, 9] (row-major 3x3 per graph, written
// by rotation_matrices from three angles). The thread of a column c of triple (s, s + 3) reads the three
// source values of its row — the cache line its own value sits on — and writes row vector times matrix,
// (a0·R[0][c-s] + a1·R[1][c-s]) + a2·R[2][c-s], every product and sum rounded on its own and in that order,
// so that the same expression written with torch's elementwise ops gives the same bits. Noise comes second.
// The thread of a y column does the same with the y columns of the next frame. rotate_rows is the rule on
// the rows of a [rows, cols] matrix (edge_attr) whose graph comes from row_graph. All of it stays one
// element per thread on consecutive floats, for the reasons above: a handful of loads and five flops.
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

// (a0·R[0][j] + a1·R[1][j]) + a2·R[2][j], R the row-major 3x3 at Rg: plain operators, the caller's function
// body is under fp contract(off) and so is this one (see feed_batch on __fmul_rn / __fadd_rn)
__device__ __forceinline__ float rot3(const float* __restrict__ a, const float* __restrict__ Rg, int j) {
#pragma clang fp contract(off)
    const float p0 = a[0] * Rg[j];
    const float p1 = a[1] * Rg[3 + j];
    const float p2 = a[2] * Rg[6 + j];
    const float s01 = p0 + p1;
    return s01 + p2;
}

// start of the triple that holds column c, or -1
__device__ __forceinline__ int triple_of(const mgn_feed_ranges& tr, int c) {
    int s = -1;
#pragma unroll
    for (int i = 0; i < MGN_FEED_MAX_RANGES; ++i)
        if (i < tr.n && c >= tr.start[i] && c < tr.start[i] + 3) s = tr.start[i];
    return s;
}

__global__ __launch_bounds__(64) void rotation_matrices(const float* __restrict__ angles, int B,
                                                        float* __restrict__ R) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B) return;
    float sa, ca, sb, cb, sg, cg;
    sincosf(angles[3 * g + 0], &sa, &ca);  // alpha: about z
    sincosf(angles[3 * g + 1], &sb, &cb);  // beta: about y
    sincosf(angles[3 * g + 2], &sg, &cg);  // gamma: about x
    float* o = R + 9 * (int64_t)g;
    o[0] = ca * cb;
    o[1] = ca * sb * sg + sa * cg;
    o[2] = -ca * sb * cg + sa * sg;
    o[3] = -sa * cb;
    o[4] = -sa * sb * sg + ca * cg;
    o[5] = sa * sb * cg + ca * sg;
    o[6] = sb;
    o[7] = -cb * sg;
    o[8] = cb * cg;
}

// feed_batch with the rotation in front of the noise; tr.n >= 1 (the host sends tr.n == 0 to feed_batch)
__global__ __launch_bounds__(256) void feed_batch_rot(const float* __restrict__ traj, int64_t N, int F,
                                                      const int32_t* __restrict__ graph_ptr, int B,
                                                      const int32_t* __restrict__ frame, int y_start, int y_end,
                                                      int type_index, mgn_feed_ranges rg,
                                                      const float* __restrict__ scales,
                                                      const float* __restrict__ z, int64_t ldz,
                                                      float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                      int64_t ldy, mgn_feed_ranges tr,
                                                      const float* __restrict__ R) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * F;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)
        r = (uint32_t)e / (uint32_t)F;
    else
        r = e / F;
    const int c = (int)(e - r * F);
    const int g = graph_of_row(graph_ptr, B, r);
    const int64_t t = frame[g];
    const float* src = traj + (t * N + r) * F;
    const float* Rg = R + 9 * (int64_t)g;
    float v = src[c];
    const int ts = triple_of(tr, c);
    if (ts >= 0) v = rot3(src + ts, Rg, c - ts);
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
        if (zc >= 0 && src[type_index] == 0.f) {  // type_index lies in no triple: the clean node type
            const float noise = z[r * ldz + zc] * scales[which];
            v = v + noise;
        }
    }
    x[r * ldx + c] = v;
    // the y range is 3 wide here (checked on the host): the rotated y columns of the next clean frame
    if (c >= y_start && c < y_end) y[r * ldy + (c - y_start)] = rot3(src + (int64_t)N * F + y_start, Rg, c - y_start);
}

__global__ __launch_bounds__(256) void rotate_rows(const float* __restrict__ src, int64_t rows, int cols,
                                                   int64_t ld_src, const int32_t* __restrict__ row_graph, int B,
                                                   mgn_feed_ranges tr, const float* __restrict__ R,
                                                   float* __restrict__ dst, int64_t ld_dst) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = rows * cols;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)
        r = (uint32_t)e / (uint32_t)cols;
    else
        r = e / cols;
    const int c = (int)(e - r * cols);
    const float* a = src + r * ld_src;
    float v = a[c];
    const int ts = triple_of(tr, c);
    if (ts >= 0) {
        const int g = row_graph[r];
        if (g >= 0 && g < B) v = rot3(a + ts, R + 9 * (int64_t)g, c - ts);  // else: copied, R is not read
    }
    dst[r * ld_dst + c] = v;
}

// ---- world positions (mgn.h, "World positions inside the feed"; reference add_obstacles_next_pos and
// add_world_pos_features, dataset/preprocessing.py:49-89, 143-174) ----
//
// obstacle_mean: one workgroup per graph, so the sum needs no second pass, no workspace and no atomics: the
// per-graph reduction of mgn_common.h (world_obstacle_mean_of_graph, shared with the rollout's begin stage), a
// fixed order, so the same bits on every replay. A row costs two partly used cache lines here (a thread per row);
// the kernel reads 2·rows·F floats in all, once per fill, and a DeformingPlate graph is about 1.4 k rows.
__global__ __launch_bounds__(WORLD_MEAN_THREADS) void world_obstacle_mean(
    const float* __restrict__ traj, int64_t N, int F, const int32_t* __restrict__ graph_ptr,
    const int32_t* __restrict__ frame, int type_index, float* __restrict__ mean) {
    const int g = blockIdx.x;
    const float* cur = traj + (int64_t)frame[g] * N * F;
    world_obstacle_mean_of_graph(cur, cur + N * F, F, graph_ptr[g], graph_ptr[g + 1], type_index,
                                 mean + 3 * (int64_t)g);
}

// feed_batch on the batch layout [world(3), displacement(3), the other F - 3 frame columns]: one thread per
// element (r, c) of [N, F + 3], so x (when ldx == F + 3) is written as one contiguous span and the frame row is
// read by consecutive lanes, as in feed_batch. y_start == 0 (checked on the host): the thread of column c < y_end
// also copies column c of the next frame.
__global__ __launch_bounds__(256) void feed_batch_world(const float* __restrict__ traj, int64_t N, int F,
                                                        const int32_t* __restrict__ graph_ptr, int B,
                                                        const int32_t* __restrict__ frame, int y_end,
                                                        int type_index, mgn_feed_ranges rg,
                                                        const float* __restrict__ scales,
                                                        const float* __restrict__ z, int64_t ldz,
                                                        float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                        int64_t ldy, const float* __restrict__ mean) {
#pragma clang fp contract(off)  // x + z·s: a rounded product, then a rounded sum (see feed_batch)
    const int Fx = F + 3;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * Fx;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)
        r = (uint32_t)e / (uint32_t)Fx;
    else
        r = e / Fx;
    const int c = (int)(e - r * Fx);
    const int g = graph_of_row(graph_ptr, B, r);
    const int64_t t = frame[g];
    const float* a = traj + (t * N + r) * F;
    const float* n = a + (int64_t)N * F;
    const float type = a[type_index];
    float v;
    if (c < 3)
        v = a[c];
    else if (c < 6)
        v = type == 1.f ? n[c - 3] - a[c - 3] : mean[3 * (int64_t)g + (c - 3)];
    else
        v = a[c - 3];
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
        if (zc >= 0 && type == 0.f) {
            const float noise = z[r * ldz + zc] * scales[which];
            v = v + noise;
        }
    }
    x[r * ldx + c] = v;
    if (c < y_end) y[r * ldy + c] = n[c];
}

// One thread per edge: the two gathered world positions of the (noisy) batch rows, their difference and its
// norm, (v0·v0 + v1·v1) + v2·v2 with every product and sum rounded on its own and a correctly rounded square
// root (hipcc's default for fp32 sqrtf). VEC: the four values leave as one 16-byte store (an instantiation of its
// own: as a run-time branch the compiler merged both paths into a 12-byte and a 4-byte store).
template <bool VEC>
__global__ __launch_bounds__(256) void world_edge_features(const int32_t* __restrict__ senders,
                                                           const int32_t* __restrict__ receivers, int64_t E,
                                                           const float* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ edge_attr, int64_t ld_ea, int s) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const float* p = x + (int64_t)senders[e] * ldx;
    const float* q = x + (int64_t)receivers[e] * ldx;
    const float v0 = p[0] - q[0], v1 = p[1] - q[1], v2 = p[2] - q[2];
    const float q0 = v0 * v0;
    const float q1 = v1 * v1;
    const float q2 = v2 * v2;
    const float s01 = q0 + q1;
    const float d = sqrtf(s01 + q2);
    float* o = edge_attr + e * ld_ea + s;
    if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(v0, v1, v2, d);
    } else {
        o[0] = v0;
        o[1] = v1;
        o[2] = v2;
        o[3] = d;
    }
}

// The host-side checks of column triples against a row of `width` columns; 0 or the status of MGN_REQUIRE.
int check_triples(const std::string& who, const mgn_feed_ranges& tr, int64_t width, const char* width_name) {
    MGN_REQUIRE(tr.n >= 0 && tr.n <= MGN_FEED_MAX_RANGES, who + ": at most 4 column triples");
    for (int i = 0; i < tr.n; ++i) {
        MGN_REQUIRE(tr.end[i] - (int64_t)tr.start[i] == 3, who + ": a column triple must be exactly 3 columns wide");
        MGN_REQUIRE(tr.start[i] >= 0 && tr.end[i] <= width,
                    who + ": a column triple is outside [0, " + width_name + ")");
        for (int j = 0; j < i; ++j)
            MGN_REQUIRE(tr.start[i] >= tr.end[j] || tr.start[j] >= tr.end[i], who + ": column triples overlap");
    }
    return 0;
}

// Every argument check mgn_feed_batch makes ahead of its N == 0 return; *W: the noisy column count. Fx: the
// width of a batch row, which the noisy ranges and ldx are checked against (F, or F + 3 for feed_batch_world).
int check_feed(const std::string& who, int64_t T, int64_t N, int32_t F, int32_t B, int32_t y_start, int32_t y_end,
               int32_t type_index, const mgn_feed_ranges& ranges, const float* z, int64_t ldz, int64_t ldx,
               int64_t ldy, int64_t* W_out, int32_t Fx) {
    const std::string width = Fx == F ? "F" : "F + 3";
    MGN_REQUIRE(T >= 2, who + ": a trajectory needs at least 2 frames (x from frame t, y from t + 1)");
    MGN_REQUIRE(F >= 1, who + ": F must be >= 1");
    MGN_REQUIRE(N >= 0 && B >= 0, who + ": N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, who + ": graph_ptr is int32, N must fit it");
    MGN_REQUIRE(ranges.n >= 0 && ranges.n <= MGN_FEED_MAX_RANGES, who + ": at most 4 noisy column ranges");
    int64_t W = 0;
    for (int i = 0; i < ranges.n; ++i) {
        MGN_REQUIRE(ranges.start[i] >= 0 && ranges.start[i] <= ranges.end[i] && ranges.end[i] <= Fx,
                    who + ": a noisy column range is outside [0, " + width + "]");
        for (int j = 0; j < i; ++j)
            MGN_REQUIRE(ranges.start[i] >= ranges.end[j] || ranges.start[j] >= ranges.end[i] ||
                            ranges.start[i] == ranges.end[i] || ranges.start[j] == ranges.end[j],
                        who + ": noisy column ranges overlap");
        W += ranges.end[i] - ranges.start[i];
    }
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, who + ": the y column range is outside [0, F]");
    MGN_REQUIRE(type_index >= 0 && type_index < F, who + ": type_index is outside [0, F)");
    MGN_REQUIRE(ldx >= Fx, who + ": ldx is smaller than " + width);
    MGN_REQUIRE(ldy >= y_end - y_start, who + ": ldy is smaller than the y column count");
    MGN_REQUIRE(z == nullptr || ldz >= W, who + ": ldz is smaller than the noisy column count");
    *W_out = W;
    return 0;
}

// ---- aneurysm features (mgn.h, "Aneurysm features inside the feed"; reference external/aneurysm.py
// build_features, then add_noise) ----
//
// inflow_stats: one workgroup per (graph, frame) pair, so the value set of a pair lives in one LDS array and needs
// no workspace and no atomics. The 3·M components of next − current on the graph's inflow rows (and one 0.0 when
// the graph has a row that is not inflow) are gathered, padded with +inf to a power of two and sorted by a bitonic
// network: 256 threads walk the P / 2 compare-exchanges of a stage 256 apart, a barrier between stages. Thread 0
// then walks the sorted values once: a value equal to its predecessor is skipped (the reference's .unique()), the
// others are added in fp64 in ascending order. The order is a function of the values alone, so the bits depend on
// neither B, nor the graph's place in the batch, nor the launch geometry. d + 0.0f turns -0.0 into +0.0: the two
// are one value, and min / max must not depend on which of them the network left in front.
constexpr int INFLOW_THREADS = 256;

__global__ __launch_bounds__(INFLOW_THREADS) void inflow_stats(const float* __restrict__ traj, int64_t N, int F,
                                                               const int32_t* __restrict__ graph_ptr, int B,
                                                               const int32_t* __restrict__ inflow_ptr,
                                                               const int32_t* __restrict__ inflow_rows,
                                                               float* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ float vals[MGN_FEED_INFLOW_CAPACITY];
    const int g = blockIdx.x;
    const int64_t t = blockIdx.y;
    const int i0 = inflow_ptr[g];
    const int M = inflow_ptr[g + 1] - i0;
    const int rows = graph_ptr[g + 1] - graph_ptr[g];
    const int zero = M < rows ? 1 : 0;  // the reference's next_acceleration[~inflow] = 0
    const int64_t cnt = 3 * (int64_t)M + zero;
    float* out = stats + (t * B + g) * 3;
    if (M <= 0 || cnt > MGN_FEED_INFLOW_CAPACITY) {  // uniform; the host refuses cnt > capacity before the launch
        if (threadIdx.x < 3) out[threadIdx.x] = M <= 0 ? 0.f : __builtin_nanf("");
        return;
    }
    int P = 1;
    while (P < cnt) P <<= 1;
    const float* cur = traj + t * N * F;
    const float* nxt = cur + N * F;
    for (int i = threadIdx.x; i < P; i += INFLOW_THREADS) {
        float v = __builtin_inff();
        if (i < 3 * M) {
            const int m = i / 3, j = i - 3 * m;
            const int64_t r = inflow_rows[i0 + m];
            v = 0.f;
            if (r >= 0 && r < N) v = (nxt[r * F + j] - cur[r * F + j]) + 0.f;
        } else if (i < cnt) {
            v = 0.f;
        }
        vals[i] = v;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += INFLOW_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const float a = vals[i], b = vals[o];
                    if ((i & k) == 0 ? a > b : a < b) {
                        vals[i] = b;
                        vals[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        double sum = 0.0;
        int n = 0;
        float prev = 0.f;
        for (int i = 0; i < (int)cnt; ++i) {
            const float v = vals[i];
            if (i == 0 || v != prev) {
                sum = sum + (double)v;
                ++n;
            }
            prev = v;
        }
        out[0] = (float)(sum / (double)n);
        out[1] = vals[0];
        out[2] = vals[cnt - 1];
    }
}

// feed_batch on the batch layout [frame row (F) ‖ a − p (3) ‖ pos (3) ‖ mean, min, max ‖ node type]: one thread
// per element (r, c) of [N, F + 10], so x (when ldx == F + 10) is written as one contiguous span. p is the frame
// before a (frame[g] >= 1, the host's check). The thread of a y column c < F also copies that column of the next
// frame. The node type comes from its own array (built once from frame 0), the statistics from row
// (frame[g], g) of the table inflow_stats wrote.
__global__ __launch_bounds__(256) void feed_batch_aneurysm(
    const float* __restrict__ traj, int64_t N, int F, const int32_t* __restrict__ graph_ptr, int B,
    const int32_t* __restrict__ frame, int y_start, int y_end, const float* __restrict__ pos,
    const float* __restrict__ node_type, const float* __restrict__ stats, mgn_feed_ranges8 rg,
    const float* __restrict__ scales, const float* __restrict__ z, int64_t ldz, float* __restrict__ x, int64_t ldx,
    float* __restrict__ y, int64_t ldy) {
#pragma clang fp contract(off)  // x + z·s: a rounded product, then a rounded sum (see feed_batch)
    const int Fx = F + 10;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = N * Fx;
    if (e >= total) return;
    int64_t r;
    if (total <= (int64_t)UINT32_MAX)
        r = (uint32_t)e / (uint32_t)Fx;
    else
        r = e / Fx;
    const int c = (int)(e - r * Fx);
    const int g = graph_of_row(graph_ptr, B, r);
    const int64_t t = frame[g];
    const float* a = traj + (t * N + r) * F;
    const float type = node_type[r];
    // the clean row: mgn_common.h, shared with the rollout's begin stage
    float v = aneurysm_row_value(a, a - (int64_t)N * F, F, c, pos + r * 3, stats + (t * B + g) * 3, type);
    if (z != nullptr) {
        int zc = -1, which = 0, w = 0;
#pragma unroll
        for (int i = 0; i < MGN_FEED_ANEURYSM_MAX_RANGES; ++i)
            if (i < rg.n) {
                if (c >= rg.start[i] && c < rg.end[i]) {
                    zc = w + c - rg.start[i];
                    which = i;
                }
                w += rg.end[i] - rg.start[i];
            }
        if (zc >= 0 && type == 0.f) {
            const float noise = z[r * ldz + zc] * scales[which];
            v = v + noise;
        }
    }
    x[r * ldx + c] = v;
    if (c >= y_start && c < y_end) y[r * ldy + (c - y_start)] = (a + (int64_t)N * F)[c];
}

}  // namespace

extern "C" {

int mgn_feed_batch(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                   const int32_t* frame, int32_t y_start, int32_t y_end, int32_t type_index, mgn_feed_ranges ranges,
                   const float* scales, const float* z, int64_t ldz, float* x, int64_t ldx, float* y, int64_t ldy,
                   mgn_stream_t stream) {
    int64_t W = 0;
    if (int rc = check_feed("feed_batch", T, N, F, B, y_start, y_end, type_index, ranges, z, ldz, ldx, ldy, &W, F))
        return rc;
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

int mgn_feed_rotation_matrices(const float* angles, int32_t B, float* R, mgn_stream_t stream) {
    MGN_REQUIRE(B >= 0, "feed_rotation_matrices: B must be >= 0");
    if (B == 0) return 0;
    MGN_REQUIRE(angles && R, "feed_rotation_matrices: a null pointer argument");
    hipLaunchKernelGGL(rotation_matrices, dim3((unsigned)cdiv64(B, 64)), dim3(64), 0, (hipStream_t)stream, angles,
                       (int)B, R);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_feed_batch_rot(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                       const int32_t* frame, int32_t y_start, int32_t y_end, int32_t type_index,
                       mgn_feed_ranges ranges, const float* scales, const float* z, int64_t ldz, float* x, int64_t ldx,
                       float* y, int64_t ldy, mgn_feed_ranges triples, const float* R, mgn_stream_t stream) {
    int64_t W = 0;
    if (int rc = check_feed("feed_batch_rot", T, N, F, B, y_start, y_end, type_index, ranges, z, ldz, ldx, ldy, &W, F))
        return rc;
    if (int rc = check_triples("feed_batch_rot", triples, F, "F")) return rc;
    for (int i = 0; i < triples.n; ++i)
        MGN_REQUIRE(type_index < triples.start[i] || type_index >= triples.end[i],
                    "feed_batch_rot: type_index lies inside a column triple");
    if (triples.n > 0) {
        MGN_REQUIRE(y_end - y_start == 0 || y_end - y_start == 3,
                    "feed_batch_rot: with column triples the y column range must be 3 wide (or empty)");
        MGN_REQUIRE(R != nullptr, "feed_batch_rot: column triples without R");
    }
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && x && (y || y_start == y_end), "feed_batch_rot: a null pointer argument");
    MGN_REQUIRE(z == nullptr || W == 0 || scales != nullptr, "feed_batch_rot: noise (z) without scales");
    const int64_t blocks = cdiv64(N * F, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, "feed_batch_rot: N * F is too large for one launch");
    if (triples.n == 0)  // no rotation: mgn_feed_batch's own kernel, so exactly its result
        hipLaunchKernelGGL(feed_batch, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, N, (int)F,
                           graph_ptr, (int)B, frame, (int)y_start, (int)y_end, (int)type_index, ranges, scales,
                           W > 0 ? z : nullptr, ldz, x, ldx, y, ldy);
    else
        hipLaunchKernelGGL(feed_batch_rot, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, N, (int)F,
                           graph_ptr, (int)B, frame, (int)y_start, (int)y_end, (int)type_index, ranges, scales,
                           W > 0 ? z : nullptr, ldz, x, ldx, y, ldy, triples, R);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_feed_rotate_rows(const float* src, int64_t rows, int32_t cols, int64_t ld_src, const int32_t* row_graph,
                         int32_t B, mgn_feed_ranges triples, const float* R, float* dst, int64_t ld_dst,
                         mgn_stream_t stream) {
    MGN_REQUIRE(rows >= 0 && B >= 0, "feed_rotate_rows: rows and B must be >= 0");
    MGN_REQUIRE(cols >= 1, "feed_rotate_rows: cols must be >= 1");
    if (int rc = check_triples("feed_rotate_rows", triples, cols, "cols")) return rc;
    MGN_REQUIRE(triples.n == 0 || R != nullptr, "feed_rotate_rows: column triples without R");
    MGN_REQUIRE(ld_src >= cols, "feed_rotate_rows: ld_src is smaller than cols");
    MGN_REQUIRE(ld_dst >= cols, "feed_rotate_rows: ld_dst is smaller than cols");
    if (rows == 0) return 0;
    MGN_REQUIRE(src && dst && (row_graph || triples.n == 0), "feed_rotate_rows: a null pointer argument");
    // a thread reads the three source values of its triple and writes one of them: in place would race
    MGN_REQUIRE(src + ((rows - 1) * ld_src + cols) <= dst || dst + ((rows - 1) * ld_dst + cols) <= src,
                "feed_rotate_rows: src and dst overlap");
    const int64_t blocks = cdiv64(rows * cols, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, "feed_rotate_rows: rows * cols is too large for one launch");
    hipLaunchKernelGGL(rotate_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, rows, (int)cols,
                       ld_src, row_graph, (int)B, triples, R, dst, ld_dst);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_feed_batch_world(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                         const int32_t* frame, int32_t y_start, int32_t y_end, int32_t type_index,
                         mgn_feed_ranges ranges, const float* scales, const float* z, int64_t ldz, float* x,
                         int64_t ldx, float* y, int64_t ldy, float* obstacle_mean, mgn_stream_t stream) {
    const std::string who = "feed_batch_world";
    MGN_REQUIRE(F >= 4 && F <= INT32_MAX - 3, who + ": F must be >= 4 (world position and a node type)");
    int64_t W = 0;
    if (int rc = check_feed(who, T, N, F, B, y_start, y_end, type_index, ranges, z, ldz, ldx, ldy, &W, F + 3)) return rc;
    MGN_REQUIRE(type_index >= 3, who + ": type_index lies inside the world position columns [0, 3)");
    MGN_REQUIRE(y_start == 0 && y_end >= 3, who + ": the y columns must begin with the world position "
                                                  "(y_start == 0, y_end >= 3)");
    for (int i = 0; i < ranges.n; ++i)
        MGN_REQUIRE(ranges.start[i] == ranges.end[i] || type_index + 3 < ranges.start[i] ||
                        type_index + 3 >= ranges.end[i],
                    who + ": a noisy column range contains the node type (batch column type_index + 3)");
    MGN_REQUIRE(obstacle_mean != nullptr, who + ": obstacle_mean is null");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && x && y, who + ": a null pointer argument");
    MGN_REQUIRE(z == nullptr || W == 0 || scales != nullptr, who + ": noise (z) without scales");
    const int64_t blocks = cdiv64(N * (F + 3), 256);
    MGN_REQUIRE(blocks <= INT32_MAX, who + ": N * (F + 3) is too large for one launch");
    hipLaunchKernelGGL(world_obstacle_mean, dim3((unsigned)B), dim3(WORLD_MEAN_THREADS), 0, (hipStream_t)stream, traj,
                       N, (int)F, graph_ptr, frame, (int)type_index, obstacle_mean);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(feed_batch_world, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, N, (int)F,
                       graph_ptr, (int)B, frame, (int)y_end, (int)type_index, ranges, scales, W > 0 ? z : nullptr,
                       ldz, x, ldx, y, ldy, obstacle_mean);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_feed_world_edge_features(const int32_t* senders, const int32_t* receivers, int64_t E, const float* x,
                                 int64_t ldx, float* edge_attr, int64_t ld_ea, int32_t start, mgn_stream_t stream) {
    const std::string who = "feed_world_edge_features";
    MGN_REQUIRE(E >= 0, who + ": E must be >= 0");
    MGN_REQUIRE(start >= 0, who + ": the start column must be >= 0");
    MGN_REQUIRE(ld_ea >= (int64_t)start + 4, who + ": ld_ea is smaller than start + 4");
    MGN_REQUIRE(ldx >= 3, who + ": ldx is smaller than 3");
    if (E == 0) return 0;
    MGN_REQUIRE(senders && receivers && x && edge_attr, who + ": a null pointer argument");
    const int64_t blocks = cdiv64(E, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, who + ": E is too large for one launch");
    const bool vec = start % 4 == 0 && ld_ea % 4 == 0 && reinterpret_cast<uintptr_t>(edge_attr) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(world_edge_features<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           senders, receivers, E, x, ldx, edge_attr, ld_ea, (int)start);
    else
        hipLaunchKernelGGL(world_edge_features<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           senders, receivers, E, x, ldx, edge_attr, ld_ea, (int)start);
    MGN_LAUNCH_CHECK();
    return 0;
}

int32_t mgn_feed_inflow_capacity(void) { return MGN_FEED_INFLOW_CAPACITY; }

int mgn_feed_inflow_stats(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                          const int32_t* inflow_ptr, const int32_t* inflow_rows, int64_t max_values, float* stats,
                          mgn_stream_t stream) {
    const std::string who = "feed_inflow_stats";
    MGN_REQUIRE(T >= 2, who + ": a trajectory needs at least 2 frames (the statistics of frame t read t + 1)");
    MGN_REQUIRE(F >= 4, who + ": F must be >= 4 (velocity and the wall flag)");
    MGN_REQUIRE(N >= 0 && B >= 0, who + ": N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, who + ": graph_ptr is int32, N must fit it");
    MGN_REQUIRE(max_values >= 0, who + ": max_values must be >= 0");
    MGN_REQUIRE(max_values <= MGN_FEED_INFLOW_CAPACITY,
                who + ": a graph's value set exceeds the capacity of " + std::to_string(MGN_FEED_INFLOW_CAPACITY) +
                    " values");
    MGN_REQUIRE(T - 1 <= 65535, who + ": more than 65535 frames with a successor in one launch");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && inflow_ptr && stats && (inflow_rows || max_values <= 1),
                who + ": a null pointer argument");
    hipLaunchKernelGGL(inflow_stats, dim3((unsigned)B, (unsigned)(T - 1)), dim3(INFLOW_THREADS), 0,
                       (hipStream_t)stream, traj, N, (int)F, graph_ptr, (int)B, inflow_ptr, inflow_rows, stats);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_feed_batch_aneurysm(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                            const int32_t* frame, int32_t y_start, int32_t y_end, const float* pos,
                            const float* node_type, const float* stats, mgn_feed_ranges8 ranges, const float* scales,
                            const float* z, int64_t ldz, float* x, int64_t ldx, float* y, int64_t ldy,
                            mgn_stream_t stream) {
    const std::string who = "feed_batch_aneurysm";
    MGN_REQUIRE(T >= 3, who + ": a trajectory needs at least 3 frames (x from frames t - 1 and t, y from t + 1)");
    MGN_REQUIRE(F >= 4 && F <= INT32_MAX - 10, who + ": F must be >= 4 (velocity and the wall flag)");
    MGN_REQUIRE(N >= 0 && B >= 0, who + ": N and B must be >= 0");
    MGN_REQUIRE(N <= INT32_MAX, who + ": graph_ptr is int32, N must fit it");
    const int32_t Fx = F + 10;
    MGN_REQUIRE(ranges.n >= 0 && ranges.n <= MGN_FEED_ANEURYSM_MAX_RANGES, who + ": at most 8 noisy column ranges");
    int64_t W = 0;
    for (int i = 0; i < ranges.n; ++i) {
        MGN_REQUIRE(ranges.start[i] >= 0 && ranges.start[i] <= ranges.end[i] && ranges.end[i] <= Fx,
                    who + ": a noisy column range is outside [0, F + 10]");
        for (int j = 0; j < i; ++j)
            MGN_REQUIRE(ranges.start[i] >= ranges.end[j] || ranges.start[j] >= ranges.end[i] ||
                            ranges.start[i] == ranges.end[i] || ranges.start[j] == ranges.end[j],
                        who + ": noisy column ranges overlap");
        MGN_REQUIRE(ranges.start[i] == ranges.end[i] || ranges.end[i] <= Fx - 1,
                    who + ": a noisy column range contains the node type (batch column F + 9)");
        W += ranges.end[i] - ranges.start[i];
    }
    MGN_REQUIRE(y_start >= 0 && y_start <= y_end && y_end <= F, who + ": the y column range is outside [0, F]");
    MGN_REQUIRE(ldx >= Fx, who + ": ldx is smaller than F + 10");
    MGN_REQUIRE(ldy >= y_end - y_start, who + ": ldy is smaller than the y column count");
    MGN_REQUIRE(z == nullptr || ldz >= W, who + ": ldz is smaller than the noisy column count");
    if (N == 0 || B == 0) return 0;
    MGN_REQUIRE(traj && graph_ptr && frame && pos && node_type && stats && x && (y || y_start == y_end),
                who + ": a null pointer argument");
    MGN_REQUIRE(z == nullptr || W == 0 || scales != nullptr, who + ": noise (z) without scales");
    const int64_t blocks = cdiv64(N * Fx, 256);
    MGN_REQUIRE(blocks <= INT32_MAX, who + ": N * (F + 10) is too large for one launch");
    hipLaunchKernelGGL(feed_batch_aneurysm, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, traj, N, (int)F,
                       graph_ptr, (int)B, frame, (int)y_start, (int)y_end, pos, node_type, stats, ranges, scales,
                       W > 0 ? z : nullptr, ldz, x, ldx, y, ldy);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
