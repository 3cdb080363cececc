// Shared device helpers for libmgn (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <cmath>

#include <string>

#include "mgn.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define MGN_WAVE 64
#define MGN_THREADS 256
#define RMS_EPS 1e-8f

// --------------------------------------------------------------------------- MFMA traits
// D[i][j] += sum_k A[i][k] * B[k][j], 16x16 tile per wave.
//   f32  (v_mfma_f32_16x16x4_f32):   lane l holds A[l&15][l>>4],          B[l>>4][l&15]
//   bf16 (v_mfma_f32_16x16x32_bf16): lane l holds A[l&15][8(l>>4)+v],     B[8(l>>4)+v][l&15]
//   C/D (both): lane l, reg r ->  D[(l>>4)*4 + r][l&15]
template <class T>
struct Mf;
template <>
struct Mf<float> {
    static constexpr int VEC = 1, KSTEP = 4;
    typedef float frag;
    static __device__ __forceinline__ f4 mma(frag a, frag b, f4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mf<__bf16> {
    static constexpr int VEC = 8, KSTEP = 32;
    typedef bf16x8 frag;
    static __device__ __forceinline__ f4 mma(frag a, frag b, f4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

template <class T>
__device__ __forceinline__ typename Mf<T>::frag ld_frag(const T* p) {
    return *reinterpret_cast<const typename Mf<T>::frag*>(p);
}

// --------------------------------------------------------------------------- conversions
__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(__bf16 x) { return (float)x; }
template <class T>
__device__ __forceinline__ T from_f(float x);
template <>
__device__ __forceinline__ float from_f<float>(float x) { return x; }
template <>
__device__ __forceinline__ __bf16 from_f<__bf16>(float x) { return (__bf16)x; }

__device__ __forceinline__ float load_any(const void* p, int dtype, int64_t i) {
    return dtype == MGN_F32 ? reinterpret_cast<const float*>(p)[i]
                            : (float)reinterpret_cast<const __bf16*>(p)[i];
}

// 4 consecutive values <-> f4
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ f4 ld4(const __bf16* p) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
// 4 consecutive fp32 with only 4-byte alignment guaranteed (parameters in an unpadded flat buffer)
__device__ __forceinline__ f4 ld4u(const float* p) { return f4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
__device__ __forceinline__ void st4(__bf16* p, f4 v) {
    bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<bf16x4*>(p) = o;
}

// 16-byte chunks: 4 floats or 8 bf16, returned as floats (up to 8)
template <class T>
struct Chunk;
template <>
struct Chunk<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float* p, float* o) {
        f4 v = *reinterpret_cast<const f4*>(p);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
    static __device__ __forceinline__ void store(float* p, const float* o) {
        *reinterpret_cast<f4*>(p) = f4{o[0], o[1], o[2], o[3]};
    }
};
template <>
struct Chunk<__bf16> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const __bf16* p, float* o) {
        bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
    }
    static __device__ __forceinline__ void store(__bf16* p, const float* o) {
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (__bf16)o[i];
        *reinterpret_cast<bf16x8*>(p) = v;
    }
};

__host__ __device__ __forceinline__ int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ int rup(int a, int b) { return cdiv(a, b) * b; }

// --------------------------------------------------------------------------- loss row mask
// 1 when node_type[r * ld] (a float column, e.g. a strided view of x) is an integer t < 32 with bit t of
// tmask set, else 0: the row mask of the masked losses (mgn_masked_mse, mgn_gmm_nll_diag).
__device__ __forceinline__ float type_mask_of(const float* nt, int64_t ld, int64_t r, unsigned tmask) {
    const float v = nt[r * ld];
    const int t = (int)v;
    return (v == (float)t && t >= 0 && t < 32 && ((tmask >> t) & 1u)) ? 1.f : 0.f;
}

// --------------------------------------------------------------------------- masked L2 sums
// The arithmetic of mgn_masked_mse, shared with mgn_rollout_end so both compile the same expressions and
// reduce in the same order (the rollout's per-step loss is masked_mse's value bit for bit): at most
// MSE_BLOCKS blocks of 256 threads, block b owns rows [b·rpb, (b+1)·rpb), thread i of it rows r0 + i,
// r0 + i + 256, ...; an LDS tree over the 256 threads; a single wave sums the blocks.
constexpr int MSE_BLOCKS = 64;
inline int64_t mse_rows_per_block(int64_t rows) {
    const int64_t rpb = cdiv64(rows > 0 ? rows : 1, MSE_BLOCKS);
    return rpb < 256 ? 256 : rpb;
}
inline int mse_blocks(int64_t rows) { return (int)cdiv64(rows > 0 ? rows : 1, mse_rows_per_block(rows)); }
// e + (p - t)²: one column's term of a row's squared error
__device__ __forceinline__ float mse_col_add(float e, float p, float t) {
    const float d = p - t;
    e += d * d;
    return e;
}
// acc + m·e: a row's masked term
__device__ __forceinline__ float mse_row_add(float acc, float m, float e) {
    acc += m * e;
    return acc;
}
// sum of K values per thread over the 256 threads of a block, pairwise in a fixed order; the sums end in
// s[k][0]. s[k][threadIdx.x] must hold thread threadIdx.x's values (the call begins with a barrier).
template <int K>
__device__ __forceinline__ void mse_block_tree(float (*s)[256]) {
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + w];
        }
        __syncthreads();
    }
}
// one wave's sum of a value per lane (xor butterfly, every lane ends with the sum)
__device__ __forceinline__ float mse_wave_sum(float v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
    return v;
}

// --------------------------------------------------------------------------- resident trajectories
// The graph g of node r, graph_ptr[g] <= r < graph_ptr[g + 1], from the B + 1 node offsets (empty graphs
// are stepped over; the same few cache lines for every thread).
__device__ __forceinline__ int graph_of_row(const int32_t* __restrict__ graph_ptr, int B, int64_t r) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)graph_ptr[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// The mean obstacle displacement of one graph, by one workgroup of WORLD_MEAN_THREADS threads (every thread of it
// calls this; it holds a barrier): rows [r0, r1) of the frame at cur and of the next frame at nxt, both [N, F]
// with the world position in columns [0, 3). A thread walks the rows WORLD_MEAN_THREADS apart and adds the
// displacement n[j] - a[j] of its OBSTACLE rows; the 64 lanes of a wave are summed by a shuffle tree, the wave
// sums by thread 0 in wave order: a fixed order, so the same bits on every replay, and the same bits from
// mgn_feed_batch_world and mgn_rollout_begin_world, which both reduce here. Thread 0 writes mean[0..3).
constexpr int WORLD_MEAN_THREADS = 1024;

__device__ __forceinline__ void world_obstacle_mean_of_graph(const float* __restrict__ cur,
                                                             const float* __restrict__ nxt, int F, int64_t r0,
                                                             int64_t r1, int type_index, float* __restrict__ mean) {
#pragma clang fp contract(off)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    int m = 0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += WORLD_MEAN_THREADS) {
        const float* a = cur + r * F;
        const float* n = nxt + r * F;
        if (a[type_index] == 1.f) {  // NodeType.OBSTACLE
            const float d0 = n[0] - a[0], d1 = n[1] - a[1], d2 = n[2] - a[2];
            s0 = s0 + d0;
            s1 = s1 + d1;
            s2 = s2 + d2;
            ++m;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // lane 0 ends with the wave's sum
        s0 = s0 + __shfl_down(s0, off, 64);
        s1 = s1 + __shfl_down(s1, off, 64);
        s2 = s2 + __shfl_down(s2, off, 64);
        m += __shfl_down(m, off, 64);
    }
    constexpr int WAVES = WORLD_MEAN_THREADS / 64;
    __shared__ float ws[WAVES][3];
    __shared__ int wm[WAVES];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        ws[w][0] = s0;
        ws[w][1] = s1;
        ws[w][2] = s2;
        wm[w] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t0 = ws[0][0], t1 = ws[0][1], t2 = ws[0][2];
        int M = wm[0];
        for (int w = 1; w < WAVES; ++w) {
            t0 = t0 + ws[w][0];
            t1 = t1 + ws[w][1];
            t2 = t2 + ws[w][2];
            M += wm[w];
        }
        // torch.mean's division by the count (correctly rounded: hipcc's default for fp32 division); a graph
        // without an OBSTACLE row writes 0 where the reference's mean of nothing is NaN
        const float cnt = (float)M;
        mean[0] = M > 0 ? t0 / cnt : 0.f;
        mean[1] = M > 0 ? t1 / cnt : 0.f;
        mean[2] = M > 0 ? t2 / cnt : 0.f;
    }
}

// Element c of the clean aneurysm batch row [frame row (F) ‖ a − p (3) ‖ pos (3) ‖ mean, min, max ‖ node type] of
// one node (mgn.h, "Aneurysm features inside the feed"): a = the node's row of frame t, p = its row of frame t − 1,
// pos3 = its position, stats3 = row (t, g) of the inflow statistics table, type = its node type. Only the element's
// own operands are loaded; the acceleration is one rounded fp32 difference. mgn_feed_batch_aneurysm and
// mgn_rollout_begin_aneurysm both take the row from here, so both write the same bits.
__device__ __forceinline__ float aneurysm_row_value(const float* __restrict__ a, const float* __restrict__ p, int F,
                                                    int c, const float* __restrict__ pos3,
                                                    const float* __restrict__ stats3, float type) {
#pragma clang fp contract(off)
    if (c < F) return a[c];
    if (c < F + 3) return a[c - F] - p[c - F];
    if (c < F + 6) return pos3[c - F - 3];
    if (c < F + 9) return stats3[c - F - 6];
    return type;
}

// --------------------------------------------------------------------------- packed weights
// Forward fragments of W[n][k] (nn.Linear weight [out, in]):
//   pack[((nt*KS + ks)*64 + lane)*VEC + v] = W[nt*16 + (lane&15)][ks*KSTEP + VEC*(lane>>4) + v]
// Transposed fragments (A operand of dX = dY·W):
//   packT[((kt*NS + ns)*64 + lane)*VEC + v] = W[ns*KSTEP + VEC*(lane>>4) + v][kt*16 + (lane&15)]
// kt runs over round_up(ceil(K/16), 8) tiles so a backward chunk of hidden/16 tiles never reads
// past the layer. Both use the same per-layer element count. An fp32 Linear with n == 128 and k a
// multiple of 128 also carries a 128x128 "chain image" of its first 128 input columns after the
// fragments of either region (the register-chained fp32 edge kernels' LDS-DMA source, mgn_mlp.hip):
//   image[((nt*8 + t)*64 + lane)*4 + r]  = W[nt*16 + (lane&15)][t*16 + 4*(lane>>4) + r]   (forward)
//   imageT[((kt*8 + t)*64 + lane)*4 + r] = W[t*16 + 4*(lane>>4) + r][kt*16 + (lane&15)]   (transposed)
// — one such image per 128-column block of the input (round 5: the chained fp32 node MLP's layer 0
// reads both blocks of its [x ‖ aggr] weight, the next block's projections the x_i / x_j blocks of the
// edge W0), block b's image of columns 128b .. 128b + 127 at chain_image_off(n, k, b) (mgn_mlp.hip).
__host__ __device__ inline int chain_images(int n, int k, int dtype) {
    return dtype == MGN_F32 && n == 128 && k > 0 && k % 128 == 0 ? k / 128 : 0;
}
__host__ __device__ inline bool has_chain_image(int n, int k, int dtype) { return chain_images(n, k, dtype) > 0; }
__host__ __device__ inline int64_t linear_pack_elems(int n, int k, int dtype) {
    const int vec = dtype == MGN_BF16 ? 8 : 1, kstep = 4 * vec;
    int64_t fwd = (int64_t)cdiv(n, 16) * cdiv(k, kstep);
    int64_t bwd = (int64_t)rup(cdiv(k, 16), 8) * cdiv(n, kstep);
    return (fwd > bwd ? fwd : bwd) * 64 * vec + (int64_t)chain_images(n, k, dtype) * 128 * 128;
}

// Layer shapes of build_mlp(in, hidden, out, L)
__host__ __device__ inline void mlp_layer_shape(const mgn_mlp& m, int l, int* n, int* k) {
    *k = l == 0 ? m.in_dim : m.hidden;
    *n = l == m.n_layers - 1 ? m.out_dim : m.hidden;
}

// --------------------------------------------------------------------------- errors
void mgn_set_error(const std::string& s);
#define MGN_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            mgn_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));          \
            return (int)_e;                                                            \
        }                                                                              \
    } while (0)
#define MGN_REQUIRE(cond, msg)                                                         \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            mgn_set_error(msg);                                                        \
            return 1000;                                                               \
        }                                                                              \
    } while (0)
#define MGN_LAUNCH_CHECK() MGN_TRY(hipGetLastError())

// --------------------------------------------------------------------------- opt-in profiler
// Kernel classes timed by mgn_profile_* (HIP events on the launch stream; off by default).
enum MgnProfKind {
    PROF_FWD_EDGE = 0, PROF_FWD_NODE, PROF_FWD_DENSE, PROF_BWD_EDGE, PROF_BWD_NODE, PROF_BWD_DENSE,
    PROF_WGRAD, PROF_WGRAD_REDUCE, PROF_COMBINE, PROF_PACK, PROF_ADAMW, PROF_PROJ, PROF_WGRAD_DENSE, PROF_KINDS
};
int mgn_prof_begin(int kind, hipStream_t st);  // returns slot or -1 when disabled
void mgn_prof_end(int slot, hipStream_t st);
struct ProfScope {
    int slot;
    hipStream_t st;
    ProfScope(int kind, hipStream_t s) : slot(mgn_prof_begin(kind, s)), st(s) {}
    ~ProfScope() { mgn_prof_end(slot, st); }
};

// --------------------------------------------------------------------------- saved-activation layout
// Row-octet ("R8") layout of a [rows x cols] matrix: element (m, c) at ((m/8)*cols + c)*8 + m%8.
// Eight consecutive rows of one column are contiguous (16 B in bf16): exactly one MFMA operand
// fragment when the reduction runs over rows (weight gradients), so the weight-gradient GEMMs load
// operands straight from HBM/L2 with 16-byte loads and no LDS transposition.
__host__ __device__ __forceinline__ int64_t r8_index(int64_t m, int64_t c, int64_t cols) {
    return ((m >> 3) * cols + c) * 8 + (m & 7);
}
// Saved buffers cover rows padded to 64 (every tile, including pure-padding rows, is written).
// compute units of the current device (read once; 256 on MI355X)
// CUs the persistent kernels size their grids for. MGN_MAX_CUS (read once) caps it, so two streams
// can each run a persistent kernel on part of the chip at the same time (intra-GPU data parallelism
// experiments: tools/exp_dual.py).
// Per-call options (mgn_call_opts, ABI v17; replaces v13's process-global mgn_set_grid_cus): the CU
// caps of the persistent grids of every launch except the weight-gradient launches (data_cus) and of
// the weight-gradient launches (wgrad_cus; 0 = none), so a block's weight gradients can run on a stream
// of their own beside the next block's data gradients, each on its own share of the CUs; and the device
// error word the hand-off waits of the recomputed weight gradients report a timeout to. CallScope
// installs a call's options for the duration of that call only, on the calling thread (restored on
// return), so two models, streams or threads never see each other's caps. Read when a launch is issued
// (a captured graph keeps its grids).
struct MgnCallCtx {
    int data_cus, wgrad_cus;
    uint32_t* err_word;
};
extern thread_local MgnCallCtx g_call;
struct CallScope {
    MgnCallCtx saved;
    explicit CallScope(const mgn_call_opts* o) : saved(g_call) {
        g_call = MgnCallCtx{o ? o->data_cus : 0, o ? o->wgrad_cus : 0, o ? o->err_word : nullptr};
    }
    ~CallScope() { g_call = saved; }
};
inline int hw_cus();
inline int device_cus() {
    const int c = hw_cus();
    return g_call.data_cus > 0 && g_call.data_cus < c ? g_call.data_cus : c;
}
inline int wgrad_cus() {
    const int c = hw_cus();
    return g_call.wgrad_cus > 0 && g_call.wgrad_cus < c ? g_call.wgrad_cus : c;
}
inline int hw_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cus = n;
        else
            cus = 256;
        if (const char* e = getenv("MGN_MAX_CUS")) {
            const int c = atoi(e);
            if (c > 0 && c < cus) cus = c;
        }
    }
    return cus;
}
__host__ __device__ __forceinline__ int64_t rows_pad(int64_t M) { return (M + 63) / 64 * 64; }
// RMSNorm's d^(-1/2) (layers.py:59-74) of an MLP: the true feature count (norm_dim) of a padded MLP
inline float norm_dinv(const mgn_mlp* m) {
    const int d = m->norm_dim > 0 ? m->norm_dim : m->out_dim;
    return (float)(1.0 / sqrt((double)d));
}
__host__ __device__ __forceinline__ int kstep_of(int dtype) { return dtype == MGN_BF16 ? 32 : 4; }
// R8 column count of the saved INPUT of layer l (layer 0: padded MLP input; else padded hidden)
__host__ __device__ inline int act_cols(const mgn_mlp& m, int l) {
    const int ks = kstep_of(m.dtype);
    return l == 0 ? rup(m.in_dim, ks) : rup(m.hidden, ks);
}
// gathered != 0: MLP of a GraphNetBlock, whose layer-0 input ([e‖x_i‖x_j] or [x‖aggr]) is not
// saved (the weight-gradient kernel re-gathers it); layer 0's block then has zero size.
__host__ __device__ inline int64_t act_off(const mgn_mlp& m, int64_t M, int l, int gathered = 0) {
    int64_t o = 0;
    for (int j = 0; j < l; ++j) o += (gathered && j == 0) ? 0 : rows_pad(M) * act_cols(m, j);
    return o;
}
// ReLU masks of the hidden-layer outputs: per layer, per (16-row tile, 16-col tile), 4 ballot words
__host__ __device__ inline int64_t mask_words_per_layer(const mgn_mlp& m, int64_t M) {
    return rows_pad(M) / 16 * (m.hidden / 16) * 4;
}
