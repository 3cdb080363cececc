// Gated MLP (the dense half of the reference's Transformer block, layers.py:198-262, 548-627), forward and
// backward:
//
//   n1 = s_a ⊙ x  / (‖x‖₂  · h^-½ + 1e-8)        n = s_b ⊙ n1 / (‖n1‖₂ · h^-½ + 1e-8)
//   u  = n W1ᵀ + b1    v = n W2ᵀ + b2    g = GELU(u) ⊙ v (erf GELU)    y = x + g W3ᵀ + b3
//
// Mapping. A workgroup of 4 waves owns a tile of 64 rows, a wave 16 of them; workgroup b takes the tiles
// b, b + grid, ... (grid = min(tiles, GATED_MAX_BLOCKS)). The hidden size is zero-padded to a kernel width
// HP ∈ {64, 128, 256}; the norms divide by the true size. A wave keeps n (and, in the backward, dy) of its
// rows as MFMA A fragments in registers: lane (q = l >> 4, c = l & 15) holds row c, columns
// [q·HP/4, (q+1)·HP/4) — the reduction index of an MFMA may be permuted as long as both operands agree, so
// every lane's share of a row is contiguous. The expanded dimension (3h) is streamed in chunks of CH
// columns (16 fp32, 32 bf16): the workgroup stages W1[c,:], W2[c,:], W3[:,c] of the chunk in LDS, read from
// the fp32 master weights (converted to bf16 on the way in MGN_BF16), so a launch always sees the
// parameters as they are when it runs; u_c, v_c come out of the MFMAs in registers, g_c goes through a
// per-wave LDS scratch into A layout and is accumulated into the tile's output accumulators. Nothing of
// size [rows, 3h] is written by the forward.
//
// Backward, three launches. (1) per row tile: recompute n, u, v from x, dg = dy·W3, du, dv, g; accumulate
// dn = du·W1 + dv·W2 in registers, finish the two norm backwards, write dx, the per-workgroup column sums of
// the two scale gradients, and du, dv, g, n, dy as GEMM operands into the workspace in a row-group layout
// (V = 4 fp32 / 8 bf16 consecutive rows of one column contiguous: one 16-byte load is a lane's reduction
// share when the reduction runs over rows). (2) the weight gradients as GEMMs over rows, split into S row
// slabs whose partial sums go to the workspace; n and g carry a column of ones, so the bias gradients are
// one more column of the same GEMMs. (3) the slabs and the column sums are added in slab order into the
// flat gradient. No atomics, every workgroup independent, every sum in a fixed order.
#include "mgn_common.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace {

constexpr int GATED_TILE = 64;          // rows per workgroup tile (4 waves x 16)
constexpr int GATED_MAX_BLOCKS = 512;   // grid of the row-tile kernels: min(tiles, this)
constexpr int GATED_EXT = 16;           // extra operand columns of n and g: [1, 0 x 15]

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
int64_t pad_rows(int64_t rows) { return (rows + GATED_TILE - 1) / GATED_TILE * GATED_TILE; }
int width_of(int h) { return h <= 64 ? 64 : h <= 128 ? 128 : 256; }
int chunk_of(int dtype) { return dtype == MGN_BF16 ? 32 : 16; }
int expand_pad(int h, int dtype) { return rup(3 * h, chunk_of(dtype)); }
int slabs_of(int64_t rows, int HP) {
    const int64_t s = pad_rows(rows) / 512;
    const int cap = HP > 128 ? 16 : 32;
    return (int)(s < 1 ? 1 : s > cap ? cap : s);
}
// max_blocks > 0 (mgn_gated_mlp::max_blocks) lowers the cap: fewer workgroups, each over more tiles
int blocks_of(int64_t rows, int max_blocks) {
    const int64_t t = pad_rows(rows) / GATED_TILE;
    const int cap = max_blocks > 0 && max_blocks < GATED_MAX_BLOCKS ? max_blocks : GATED_MAX_BLOCKS;
    return (int)(t < cap ? t : cap);
}

template <class T>
struct Cfg {
    static constexpr int V = 16 / (int)sizeof(T);  // elements of a 16-byte group
    static constexpr int CH = 4 * V;               // chunk of the expanded dimension: 16 fp32, 32 bf16
    static constexpr int KS = Mf<T>::KSTEP, VEC = Mf<T>::VEC;
    // row strides of the LDS arrays: [.][HP] arrays keep 16-byte rows; [.][CH] arrays are written transposed
    // (consecutive threads, consecutive rows), so fp32 rows get an odd stride (bf16 fragments need 16 bytes)
    static constexpr int PADW = V, PADC = sizeof(T) == 4 ? 1 : 8;
};

// element (m, c) of a [rows x cols] operand in the row-group layout
template <class T>
__device__ __forceinline__ int64_t rg_index(int64_t m, int64_t c, int64_t cols) {
    constexpr int V = Cfg<T>::V;
    return ((m / V) * cols + c) * V + (m % V);
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

template <class T>
__device__ __forceinline__ typename Mf<T>::frag make_frag(const float* v);
template <>
__device__ __forceinline__ float make_frag<float>(const float* v) { return v[0]; }
template <>
__device__ __forceinline__ bf16x8 make_frag<__bf16>(const float* v) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];
    return o;
}

struct GArgs {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *sa, *sb;
    const float* x;
    int64_t ldx, rows;
    float* y;
    int64_t ldy;
    float* saved;       // [rows, 2] {‖x‖, ‖n1‖}; forward: nullable
    const float* dy;
    int64_t lddy;
    float* dx;          // [rows, h]
    void *du, *dv, *gx, *nx, *dyt;  // backward operands (row-group layout)
    float* part_s;      // [grid, 2, HP] column sums of the scale gradients
    int h, E;           // hidden, 3·hidden
    float dinv;
    int vec;            // x rows readable with 16-byte loads
};

// a lane's share of a row in A layout: columns [q·HP/4, (q+1)·HP/4), zero past h or for a NULL row
template <int HP>
__device__ __forceinline__ void load_row_a(const float* __restrict__ row, int h, int q, bool vec, float* o) {
    constexpr int Q = HP / 4;
    if (row == nullptr) {
#pragma unroll
        for (int i = 0; i < Q; ++i) o[i] = 0.f;
    } else if (vec) {  // h % 4 == 0: a group of 4 columns is inside or outside the row as a whole
#pragma unroll
        for (int i = 0; i < Q; i += 4) {
            const int col = q * Q + i;
            f4 v = col < h ? ld4(row + col) : f4{0.f, 0.f, 0.f, 0.f};
            o[i] = v[0]; o[i + 1] = v[1]; o[i + 2] = v[2]; o[i + 3] = v[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            const int col = q * Q + i;
            o[i] = col < h ? row[col] : 0.f;
        }
    }
}

__device__ __forceinline__ float quad_sum(float v) {  // over the 4 lanes that share a row (q = 0..3)
    v += __shfl_xor(v, 16, MGN_WAVE);
    v += __shfl_xor(v, 32, MGN_WAVE);
    return v;
}
__device__ __forceinline__ float col16_sum(float v) {  // over the 16 lanes that share q
    v += __shfl_xor(v, 1, MGN_WAVE);
    v += __shfl_xor(v, 2, MGN_WAVE);
    v += __shfl_xor(v, 4, MGN_WAVE);
    v += __shfl_xor(v, 8, MGN_WAVE);
    return v;
}

// the double RMSNorm of a lane's share xa of a row -> nv; returns the two norms
template <int HP>
__device__ __forceinline__ void double_norm(const float* xa, const float* __restrict__ sa,
                                            const float* __restrict__ sb, int h, int q, float dinv, float* nv,
                                            float* nrm1, float* nrm2) {
    constexpr int Q = HP / 4;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < Q; ++i) ss += xa[i] * xa[i];
    const float n1n = sqrtf(quad_sum(ss));
    const float r1 = 1.f / (n1n * dinv + RMS_EPS);
    float ss2 = 0.f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int col = q * Q + i;
        nv[i] = col < h ? sa[col] * xa[i] * r1 : 0.f;
        ss2 += nv[i] * nv[i];
    }
    const float n2n = sqrtf(quad_sum(ss2));
    const float r2 = 1.f / (n2n * dinv + RMS_EPS);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int col = q * Q + i;
        nv[i] = col < h ? sb[col] * nv[i] * r2 : 0.f;
    }
    *nrm1 = n1n;
    *nrm2 = n2n;
}

// stage rows [j0, j0 + CH) of W [E, h] (row-major fp32) as dst[jj][k] (ld LDW) and, when dstT, dstT[k][jj]
template <class T, int HP>
__device__ __forceinline__ void stage_rows(const float* __restrict__ w, int j0, int E, int h, T* dst, T* dstT) {
    constexpr int CH = Cfg<T>::CH, V = Cfg<T>::V, LDW = HP + Cfg<T>::PADW, LD3 = CH + Cfg<T>::PADC;
    for (int idx = threadIdx.x; idx < CH * HP; idx += MGN_THREADS) {
        const int jj = idx / HP, k = idx - jj * HP;
        const float v = (j0 + jj < E && k < h) ? w[(int64_t)(j0 + jj) * h + k] : 0.f;
        dst[jj * LDW + k] = from_f<T>(v);
        if (dstT) dstT[k * LD3 + jj] = from_f<T>(v);
    }
}
// stage columns [j0, j0 + CH) of W3 [h, E] as dst[i][jj] (ld LD3, nullable) and dstT[jj][i] (ld LDW, nullable)
template <class T, int HP>
__device__ __forceinline__ void stage_cols(const float* __restrict__ w, int j0, int E, int h, T* dst, T* dstT) {
    constexpr int CH = Cfg<T>::CH, V = Cfg<T>::V, LDW = HP + Cfg<T>::PADW, LD3 = CH + Cfg<T>::PADC;
    for (int idx = threadIdx.x; idx < CH * HP; idx += MGN_THREADS) {
        const int i = idx / CH, jj = idx - i * CH;
        const float v = (j0 + jj < E && i < h) ? w[(int64_t)i * E + j0 + jj] : 0.f;
        if (dst) dst[i * LD3 + jj] = from_f<T>(v);
        if (dstT) dstT[jj * LDW + i] = from_f<T>(v);
    }
}

// ---------------------------------------------------------------------------------------- forward
template <class T, int HP>
__global__ __launch_bounds__(MGN_THREADS) void gated_fwd_kernel(GArgs a) {
    constexpr int CH = Cfg<T>::CH, V = Cfg<T>::V, KS = Cfg<T>::KS, VEC = Cfg<T>::VEC;
    constexpr int Q = HP / 4, KT = HP / 16, NS = HP / KS, LDW = HP + Cfg<T>::PADW, LD3 = CH + Cfg<T>::PADC, CS = CH / KS, CT = CH / 16;
    typedef typename Mf<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* sW1 = reinterpret_cast<T*>(smem);
    T* sW2 = sW1 + CH * LDW;
    T* sW3 = sW2 + CH * LDW;
    T* sG = sW3 + HP * LD3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
    T* gs = sG + wave * 16 * LD3;
    const int h = a.h, E = a.E;
    const int64_t ntiles = (a.rows + GATED_TILE - 1) / GATED_TILE;
    const int nch = (E + CH - 1) / CH;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t rb = tile * GATED_TILE + wave * 16;
        const int64_t row = rb + c;
        frag nf[NS];
        {
            float xa[Q], nv[Q], n1n, n2n;
            load_row_a<HP>(row < a.rows ? a.x + row * a.ldx : nullptr, h, q, a.vec != 0, xa);
            double_norm<HP>(xa, a.sa, a.sb, h, q, a.dinv, nv, &n1n, &n2n);
#pragma unroll
            for (int s = 0; s < NS; ++s) nf[s] = make_frag<T>(nv + s * VEC);
            if (a.saved != nullptr && q == 0 && row < a.rows) {
                a.saved[row * 2] = n1n;
                a.saved[row * 2 + 1] = n2n;
            }
        }
        f4 acc[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ch = 0; ch < nch; ++ch) {
            const int j0 = ch * CH;
            __syncthreads();  // the previous chunk's readers are done
            stage_rows<T, HP>(a.w1, j0, E, h, sW1, nullptr);
            stage_rows<T, HP>(a.w2, j0, E, h, sW2, nullptr);
            stage_cols<T, HP>(a.w3, j0, E, h, sW3, nullptr);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                f4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
                const T* p1 = sW1 + (t * 16 + c) * LDW + q * Q;
                const T* p2 = sW2 + (t * 16 + c) * LDW + q * Q;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    u = Mf<T>::mma(nf[s], ld_frag<T>(p1 + s * VEC), u);
                    v = Mf<T>::mma(nf[s], ld_frag<T>(p2 + s * VEC), v);
                }
                const int j = j0 + t * 16 + c;
                const float bu = j < E ? a.b1[j] : 0.f, bv = j < E ? a.b2[j] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    gs[(4 * q + r) * LD3 + t * 16 + c] = from_f<T>(gelu_f(u[r] + bu) * (v[r] + bv));
            }
            __syncthreads();
            frag ga[CS];
#pragma unroll
            for (int s = 0; s < CS; ++s) ga[s] = ld_frag<T>(gs + c * LD3 + q * (CH / 4) + s * VEC);
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const T* p3 = sW3 + (t * 16 + c) * LD3 + q * (CH / 4);
#pragma unroll
                for (int s = 0; s < CS; ++s) acc[t] = Mf<T>::mma(ga[s], ld_frag<T>(p3 + s * VEC), acc[t]);
            }
        }
        // y = x + g W3ᵀ + b3 in C layout: lane (q, c), register r -> row rb + 4q + r, column 16t + c
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int col = t * 16 + c;
            if (col < h) {
                const float b = a.b3[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t rr = rb + 4 * q + r;
                    if (rr < a.rows) a.y[rr * a.ldy + col] = a.x[rr * a.ldx + col] + acc[t][r] + b;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- backward, data
template <class T, int HP>
__global__ __launch_bounds__(MGN_THREADS, HP <= 64 ? 2 : 1) void gated_bwd_kernel(GArgs a) {
    constexpr int CH = Cfg<T>::CH, V = Cfg<T>::V, KS = Cfg<T>::KS, VEC = Cfg<T>::VEC;
    constexpr int Q = HP / 4, KT = HP / 16, NS = HP / KS, LDW = HP + Cfg<T>::PADW, LD3 = CH + Cfg<T>::PADC, CS = CH / KS, CT = CH / 16;
    typedef typename Mf<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* sW1 = reinterpret_cast<T*>(smem);  // [CH][LDW]
    T* sW2 = sW1 + CH * LDW;              // [CH][LDW]
    T* sW3T = sW2 + CH * LDW;             // [CH][LDW]: W3[i][j0 + jj] at [jj][i]
    T* sW1T = sW3T + CH * LDW;            // [HP][LD3]: W1[j0 + jj][k] at [k][jj]
    T* sW2T = sW1T + HP * LD3;            // [HP][LD3]
    T* sD = sW2T + HP * LD3;              // per wave: du [16][LD3], dv [16][LD3]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
    T* dus = sD + wave * 2 * 16 * LD3;
    T* dvs = dus + 16 * LD3;
    const int h = a.h, E = a.E;
    const int EP = (E + CH - 1) / CH * CH;
    const int64_t ntiles = (a.rows + GATED_TILE - 1) / GATED_TILE;
    const int nch = EP / CH;
    T* du = reinterpret_cast<T*>(a.du);
    T* dv = reinterpret_cast<T*>(a.dv);
    T* gx = reinterpret_cast<T*>(a.gx);
    T* nx = reinterpret_cast<T*>(a.nx);
    T* dyt = reinterpret_cast<T*>(a.dyt);
    float psa[KT], psb[KT];  // this lane's share of the scale gradients' column sums, over the workgroup's tiles
#pragma unroll
    for (int t = 0; t < KT; ++t) psa[t] = psb[t] = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t rb = tile * GATED_TILE + wave * 16;
        const int64_t row = rb + c;
        const bool live = row < a.rows;
        // the scales are re-read per tile (cache hits): hoisted out of the tile loop they would occupy
        // HP/2 + HP/8 registers for the whole kernel, so the pointers are made opaque here
        const float *sa_p = a.sa, *sb_p = a.sb;
        asm volatile("" : "+s"(sa_p), "+s"(sb_p));
        frag nf[NS], df[NS];
        {
            float xa[Q], nv[Q], n1n, n2n;
            load_row_a<HP>(live ? a.x + row * a.ldx : nullptr, h, q, a.vec != 0, xa);
            double_norm<HP>(xa, sa_p, sb_p, h, q, a.dinv, nv, &n1n, &n2n);
#pragma unroll
            for (int s = 0; s < NS; ++s) nf[s] = make_frag<T>(nv + s * VEC);
            // column c of a row sits c·V elements past column 0: constant offsets from one base per lane
            T* nxr = nx + rg_index<T>(row, q * Q, HP + GATED_EXT);
#pragma unroll
            for (int i = 0; i < Q; ++i) nxr[i * V] = from_f<T>(nv[i]);
            load_row_a<HP>(live ? a.dy + row * a.lddy : nullptr, h, q, false, xa);
#pragma unroll
            for (int s = 0; s < NS; ++s) df[s] = make_frag<T>(xa + s * VEC);
            T* dyr = dyt + rg_index<T>(row, q * Q, HP);
#pragma unroll
            for (int i = 0; i < Q; ++i) dyr[i * V] = from_f<T>(xa[i]);
            // the column of ones (bias gradients) and its zero padding: 16 x 16 per wave, 4 per lane
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = q * 4 + i;
                const T one = from_f<T>(e == 0 && live ? 1.f : 0.f);
                nxr[((4 - q) * Q + e) * V] = one;  // column HP + e
                gx[rg_index<T>(row, EP + e, EP + GATED_EXT)] = one;
            }
        }
        f4 dn[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) dn[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ch = 0; ch < nch; ++ch) {
            const int j0 = ch * CH;
            __syncthreads();
            stage_rows<T, HP>(a.w1, j0, E, h, sW1, sW1T);
            stage_rows<T, HP>(a.w2, j0, E, h, sW2, sW2T);
            stage_cols<T, HP>(a.w3, j0, E, h, nullptr, sW3T);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                f4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f}, dg = {0.f, 0.f, 0.f, 0.f};
                const T* p1 = sW1 + (t * 16 + c) * LDW + q * Q;
                const T* p2 = sW2 + (t * 16 + c) * LDW + q * Q;
                const T* p3 = sW3T + (t * 16 + c) * LDW + q * Q;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    u = Mf<T>::mma(nf[s], ld_frag<T>(p1 + s * VEC), u);
                    v = Mf<T>::mma(nf[s], ld_frag<T>(p2 + s * VEC), v);
                    dg = Mf<T>::mma(df[s], ld_frag<T>(p3 + s * VEC), dg);
                }
                const int jc = t * 16 + c, j = j0 + jc;
                const float bu = j < E ? a.b1[j] : 0.f, bv = j < E ? a.b2[j] : 0.f;
                f4 duv, dvv, gv;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool lr = rb + 4 * q + r < a.rows;
                    const float uu = u[r] + bu, vv = v[r] + bv, ge = gelu_f(uu);
                    duv[r] = dg[r] * vv * gelu_grad_f(uu);
                    dvv[r] = dg[r] * ge;
                    gv[r] = lr ? ge * vv : 0.f;
                    dus[(4 * q + r) * LD3 + jc] = from_f<T>(duv[r]);
                    dvs[(4 * q + r) * LD3 + jc] = from_f<T>(dvv[r]);
                }
                // operands of the weight-gradient GEMMs: rows rb + 4q .. + 3 of column j are contiguous
                const int64_t o = rg_index<T>(rb + 4 * q, j, EP), og = rg_index<T>(rb + 4 * q, j, EP + GATED_EXT);
                st4(du + o, duv);
                st4(dv + o, dvv);
                st4(gx + og, gv);
            }
            __syncthreads();
            frag da[CS], va[CS];
#pragma unroll
            for (int s = 0; s < CS; ++s) {
                da[s] = ld_frag<T>(dus + c * LD3 + q * (CH / 4) + s * VEC);
                va[s] = ld_frag<T>(dvs + c * LD3 + q * (CH / 4) + s * VEC);
            }
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const T* p1 = sW1T + (t * 16 + c) * LD3 + q * (CH / 4);
                const T* p2 = sW2T + (t * 16 + c) * LD3 + q * (CH / 4);
#pragma unroll
                for (int s = 0; s < CS; ++s) {
                    dn[t] = Mf<T>::mma(da[s], ld_frag<T>(p1 + s * VEC), dn[t]);
                    dn[t] = Mf<T>::mma(va[s], ld_frag<T>(p2 + s * VEC), dn[t]);
                }
            }
        }
        // the two norm backwards in C layout: lane (q, c), register r -> row rb + 4q + r, column 16t + c
        float r1[4], r2[4], k1[4], k2[4], dot[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t rr = rb + 4 * q + r;
            const float n1n = rr < a.rows ? a.saved[rr * 2] : 0.f, n2n = rr < a.rows ? a.saved[rr * 2 + 1] : 0.f;
            r1[r] = 1.f / (n1n * a.dinv + RMS_EPS);
            r2[r] = 1.f / (n2n * a.dinv + RMS_EPS);
            k1[r] = n1n > 0.f ? r1[r] * r1[r] * a.dinv / n1n : 0.f;
            k2[r] = n2n > 0.f ? r2[r] * r2[r] * a.dinv / n2n : 0.f;
            dot[r] = 0.f;
        }
        f4 xs[KT];  // x at this lane's C-layout positions (0 outside the matrix)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t rr = rb + 4 * q + r;
            const float* xr = a.x + rr * a.ldx + c;  // dereferenced only inside the matrix
#pragma unroll
            for (int t = 0; t < KT; ++t) xs[t][r] = (t * 16 + c < h && rr < a.rows) ? xr[t * 16] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int col = t * 16 + c;
            const float sa = col < h ? sa_p[col] : 0.f, sb = col < h ? sb_p[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float n1 = sa * xs[t][r] * r1[r];
                psb[t] += dn[t][r] * n1 * r2[r];
                dot[r] += dn[t][r] * sb * n1;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dot[r] = col16_sum(dot[r]);
        float dot1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int col = t * 16 + c;
            const float sa = col < h ? sa_p[col] : 0.f, sb = col < h ? sb_p[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xv = xs[t][r];
                const float n1 = sa * xv * r1[r];
                const float d1 = dn[t][r] * sb * r2[r] - n1 * dot[r] * k2[r];  // d loss / d n1
                psa[t] += d1 * xv * r1[r];
                dn[t][r] = d1 * sa;
                dot1[r] += d1 * sa * xv;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dot1[r] = col16_sum(dot1[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t rr = rb + 4 * q + r;
            if (rr < a.rows) {
                const float* dyr = a.dy + rr * a.lddy + c;
                float* dxr = a.dx + rr * h + c;
#pragma unroll
                for (int t = 0; t < KT; ++t)
                    if (t * 16 + c < h) dxr[t * 16] = dyr[t * 16] + dn[t][r] * r1[r] - xs[t][r] * dot1[r] * k1[r];
            }
        }
    }
    // column sums of the scale gradients over the workgroup's rows: lanes of a wave, then the 4 waves in order
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][2][HP]
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const float s1 = quad_sum(psa[t]), s2 = quad_sum(psb[t]);
        if (q == 0) {
            red[(wave * 2 + 0) * HP + t * 16 + c] = s1;
            red[(wave * 2 + 1) * HP + t * 16 + c] = s2;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * HP; i += MGN_THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[w * 2 * HP + i];
        a.part_s[(int64_t)blockIdx.x * 2 * HP + i] = s;
    }
}

// ---------------------------------------------------------------------------------------- backward, weights
// part[s][m][n] = Σ_{r in slab s} A[r][m] B[r][n] for operands in the row-group layout, the three weight
// gradients (jobs) in one launch. Grid (max ⌈MT/4⌉, max ⌈NT/4⌉, 3 S): wave w of block (bx, by) owns the
// 16 x 64 tile at m = 16(4bx + w), n = 64 by of job z / S, slab z % S; blocks past a job's tiles leave.
struct WJobs {
    const void *A[3], *B[3];
    float* part[3];
    int colsA[3], colsB[3];
};
template <class T>
__global__ __launch_bounds__(MGN_THREADS) void gated_wgrad_kernel(WJobs jobs, int64_t rounds, int S) {
    constexpr int V = Cfg<T>::V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
    const int job = blockIdx.z / S, s = blockIdx.z - job * S;
    const T* __restrict__ A = reinterpret_cast<const T*>(jobs.A[job]);
    const T* __restrict__ B = reinterpret_cast<const T*>(jobs.B[job]);
    float* __restrict__ part = jobs.part[job];
    const int colsA = jobs.colsA[job], colsB = jobs.colsB[job], MT = colsA / 16, NT = colsB / 16;
    const int mt = blockIdx.x * 4 + wave;
    const int nt0 = blockIdx.y * 4;
    if (mt >= MT || nt0 >= NT) return;
    const int64_t per = (rounds + S - 1) / S;
    const int64_t lo = s * per, hi = lo + per < rounds ? lo + per : rounds;
    f4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
    for (int64_t rd = lo; rd < hi; ++rd) {
        const int64_t grp = rd * 4 + q;  // row group: V consecutive rows
        const u32x4 av = *reinterpret_cast<const u32x4*>(A + (grp * colsA + mt * 16 + c) * V);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (nt0 + j < NT) {
                const u32x4 bv = *reinterpret_cast<const u32x4*>(B + (grp * colsB + (nt0 + j) * 16 + c) * V);
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(av[i]), __uint_as_float(bv[i]),
                                                                      acc[j], 0, 0, 0);
                } else {
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av),
                                                                     __builtin_bit_cast(bf16x8, bv), acc[j], 0, 0, 0);
                }
            }
        }
    }
    const int64_t ncols = (int64_t)NT * 16;
    float* out = part + (int64_t)s * MT * 16 * ncols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (nt0 + j < NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(int64_t)(mt * 16 + 4 * q + r) * ncols + (nt0 + j) * 16 + c] = acc[j][r];
        }
    }
}

// grads (flat: scale_a [h], scale_b [h], W1 [3h, h], b1 [3h], W2, b2, W3 [h, 3h], b3 [h]) = the slabs and the
// per-workgroup column sums added in slab order
__global__ __launch_bounds__(MGN_THREADS) void gated_reduce_kernel(const float* __restrict__ part_s, int nblk,
                                                                   const float* __restrict__ p1,
                                                                   const float* __restrict__ p2,
                                                                   const float* __restrict__ p3, int S, int h, int E,
                                                                   int HP, int EP, float* __restrict__ grads) {
    const int64_t total = 2 * (int64_t)h + 2 * ((int64_t)E * h + E) + (int64_t)h * E + h;
    const int64_t i = (int64_t)blockIdx.x * MGN_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t n1c = HP + GATED_EXT, n3c = EP + GATED_EXT;
    const float* src;
    int64_t stride, cnt = S;
    int64_t k = i;
    if (k < 2 * h) {
        src = part_s + (k < h ? k : HP + (k - h));
        stride = 2 * HP;
        cnt = nblk;
    } else {
        k -= 2 * h;
        const int64_t wsz = (int64_t)E * h + E;
        if (k < 2 * wsz) {
            const float* p = k < wsz ? p1 : p2;
            if (k >= wsz) k -= wsz;
            src = k < (int64_t)E * h ? p + (k / h) * n1c + k % h : p + (k - (int64_t)E * h) * n1c + HP;
            stride = (int64_t)EP * n1c;
        } else {
            k -= 2 * wsz;
            src = k < (int64_t)h * E ? p3 + (k / E) * n3c + k % E : p3 + (k - (int64_t)h * E) * n3c + EP;
            stride = (int64_t)HP * n3c;
        }
    }
    float s = 0.f;
    int64_t j = 0;
    for (; j + 8 <= cnt; j += 8) {  // eight loads in flight, added in slab order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(j + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; j < cnt; ++j) s += src[j * stride];
    grads[i] = s;
}

// ---------------------------------------------------------------------------------------- host side
int check_desc(const mgn_gated_mlp* m) {
    MGN_REQUIRE(m != nullptr, "gated MLP: descriptor is NULL");
    MGN_REQUIRE(m->hidden >= 1 && m->hidden <= 256,
                "gated MLP: hidden must be in [1, 256] (got " + std::to_string(m->hidden) + ")");
    MGN_REQUIRE(m->expand == 3 * m->hidden, "gated MLP: expand (" + std::to_string(m->expand) +
                                                ") must be 3 * hidden (" + std::to_string(3 * m->hidden) + ")");
    MGN_REQUIRE(m->dtype == MGN_F32 || m->dtype == MGN_BF16, "gated MLP: dtype must be MGN_F32 or MGN_BF16");
    MGN_REQUIRE(m->max_blocks >= 0, "gated MLP: max_blocks must be >= 0 (0: the default grid)");
    MGN_REQUIRE(m->norm_dim >= 0 && m->norm_dim <= m->hidden,
                "gated MLP: norm_dim must be 0 (= hidden) or in [1, hidden]");
    MGN_REQUIRE(m->w1 && m->w2 && m->w3 && m->b1 && m->b2 && m->b3 && m->scale_a && m->scale_b,
                "gated MLP: NULL parameter pointer");
    return 0;
}

struct WsLayout {
    size_t du, dv, gx, nx, dyt, part_s, p1, p2, p3, total;
};
WsLayout ws_layout(const mgn_gated_mlp* m, int64_t rows) {
    const int HP = width_of(m->hidden), EP = expand_pad(m->hidden, m->dtype);
    const size_t R = (size_t)pad_rows(rows), sz = m->dtype == MGN_BF16 ? 2 : 4;
    const size_t S = (size_t)slabs_of(rows, HP);
    WsLayout l;
    size_t o = 0;
    l.du = o; o += al256(R * EP * sz);
    l.dv = o; o += al256(R * EP * sz);
    l.gx = o; o += al256(R * (EP + GATED_EXT) * sz);
    l.nx = o; o += al256(R * (HP + GATED_EXT) * sz);
    l.dyt = o; o += al256(R * HP * sz);
    l.part_s = o; o += al256((size_t)blocks_of(rows, m->max_blocks) * 2 * HP * sizeof(float));
    l.p1 = o; o += al256(S * EP * (HP + GATED_EXT) * sizeof(float));
    l.p2 = o; o += al256(S * EP * (HP + GATED_EXT) * sizeof(float));
    l.p3 = o; o += al256(S * HP * (EP + GATED_EXT) * sizeof(float));
    l.total = o;
    return l;
}

size_t fwd_lds(int HP, int dtype) {
    const size_t sz = dtype == MGN_BF16 ? 2 : 4, V = 16 / sz, CH = 4 * V, PC = dtype == MGN_BF16 ? 8 : 1;
    return (2 * CH * (HP + V) + HP * (CH + PC) + 4 * 16 * (CH + PC)) * sz;
}
size_t bwd_lds(int HP, int dtype) {
    const size_t sz = dtype == MGN_BF16 ? 2 : 4, V = 16 / sz, CH = 4 * V, PC = dtype == MGN_BF16 ? 8 : 1;
    const size_t b = (3 * CH * (HP + V) + 2 * HP * (CH + PC) + 4 * 2 * 16 * (CH + PC)) * sz;
    const size_t red = (size_t)4 * 2 * HP * sizeof(float);
    return b > red ? b : red;
}

// kernels that need more than 64 KB of dynamic LDS get the function attribute once per (device, kernel)
int allow_lds(const void* fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    MGN_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = done.find({dev, fn});
    if (it != done.end() && it->second >= bytes) return 0;
    MGN_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[{dev, fn}] = bytes;
    return 0;
}

template <class T, int HP>
int launch_fwd(const GArgs& a, unsigned blocks, size_t lds, hipStream_t st) {
    if (int rc = allow_lds((const void*)gated_fwd_kernel<T, HP>, lds)) return rc;
    hipLaunchKernelGGL((gated_fwd_kernel<T, HP>), dim3(blocks), dim3(MGN_THREADS), lds, st, a);
    return 0;
}
template <class T, int HP>
int launch_bwd(const GArgs& a, unsigned blocks, size_t lds, hipStream_t st) {
    if (int rc = allow_lds((const void*)gated_bwd_kernel<T, HP>, lds)) return rc;
    hipLaunchKernelGGL((gated_bwd_kernel<T, HP>), dim3(blocks), dim3(MGN_THREADS), lds, st, a);
    return 0;
}
#define GATED_DISPATCH(FN, dtype, HP, ...)                                             \
    ((dtype) == MGN_F32 ? ((HP) == 64    ? FN<float, 64>(__VA_ARGS__)                  \
                           : (HP) == 128 ? FN<float, 128>(__VA_ARGS__)                 \
                                         : FN<float, 256>(__VA_ARGS__))                \
                        : ((HP) == 64    ? FN<__bf16, 64>(__VA_ARGS__)                 \
                           : (HP) == 128 ? FN<__bf16, 128>(__VA_ARGS__)                \
                                         : FN<__bf16, 256>(__VA_ARGS__)))

template <class T>
void launch_wgrad(const WJobs& jobs, int64_t R, int S, hipStream_t st) {
    int mg = 0, ng = 0;
    for (int j = 0; j < 3; ++j) {
        mg = std::max(mg, cdiv(jobs.colsA[j] / 16, 4));
        ng = std::max(ng, cdiv(jobs.colsB[j] / 16, 4));
    }
    const int64_t rounds = R / (4 * Cfg<T>::V);
    hipLaunchKernelGGL((gated_wgrad_kernel<T>), dim3(mg, ng, 3 * S), dim3(MGN_THREADS), 0, st, jobs, rounds, S);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

GArgs base_args(const mgn_gated_mlp* m, const float* x, int64_t ldx, int64_t rows) {
    GArgs a{};
    a.w1 = m->w1; a.b1 = m->b1; a.w2 = m->w2; a.b2 = m->b2; a.w3 = m->w3; a.b3 = m->b3;
    a.sa = m->scale_a; a.sb = m->scale_b;
    a.x = x; a.ldx = ldx; a.rows = rows;
    a.h = m->hidden; a.E = m->expand;
    a.dinv = (float)(1.0 / sqrt((double)(m->norm_dim > 0 ? m->norm_dim : m->hidden)));
    a.vec = m->hidden % 4 == 0 && ldx % 4 == 0 && aligned16(x);
    return a;
}

}  // namespace

extern "C" {

int32_t mgn_gated_mlp_row_tile(void) { return GATED_TILE; }

int32_t mgn_gated_mlp_blocks(int64_t rows, int32_t max_blocks) { return rows > 0 ? blocks_of(rows, max_blocks) : 0; }

size_t mgn_gated_mlp_saved_bytes(const mgn_gated_mlp* m, int64_t rows) {
    if (m == nullptr || rows <= 0) return 0;
    return (size_t)rows * 2 * sizeof(float);
}

int mgn_gated_mlp_forward(const mgn_gated_mlp* m, const float* x, int64_t ldx, int64_t rows, float* y, int64_t ldy,
                          void* saved, mgn_stream_t stream) {
    if (int rc = check_desc(m)) return rc;
    MGN_REQUIRE(rows >= 0, "gated MLP forward: rows must be >= 0");
    MGN_REQUIRE(ldx >= m->hidden && ldy >= m->hidden, "gated MLP forward: ldx and ldy must be >= hidden");
    if (rows == 0) return 0;
    MGN_REQUIRE(x && y, "gated MLP forward: NULL tensor");
    GArgs a = base_args(m, x, ldx, rows);
    a.y = y;
    a.ldy = ldy;
    a.saved = (float*)saved;
    const int HP = width_of(m->hidden);
    if (int rc = GATED_DISPATCH(launch_fwd, m->dtype, HP, a, (unsigned)blocks_of(rows, m->max_blocks), fwd_lds(HP, m->dtype),
                                (hipStream_t)stream))
        return rc;
    MGN_LAUNCH_CHECK();
    return 0;
}

size_t mgn_gated_mlp_backward_workspace_bytes(const mgn_gated_mlp* m, int64_t rows) {
    if (m == nullptr || rows <= 0 || m->hidden < 1 || m->hidden > 256) return 0;
    return ws_layout(m, rows).total;
}

int mgn_gated_mlp_backward(const mgn_gated_mlp* m, const float* x, int64_t ldx, int64_t rows, const void* saved,
                           const float* dy, int64_t lddy, float* dx, float* grads, void* ws, size_t ws_bytes,
                           mgn_stream_t stream) {
    if (int rc = check_desc(m)) return rc;
    MGN_REQUIRE(rows >= 0, "gated MLP backward: rows must be >= 0");
    MGN_REQUIRE(ldx >= m->hidden && lddy >= m->hidden, "gated MLP backward: ldx and lddy must be >= hidden");
    MGN_REQUIRE(ws_bytes >= mgn_gated_mlp_backward_workspace_bytes(m, rows),
                "gated MLP backward: workspace too small (mgn_gated_mlp_backward_workspace_bytes)");
    if (rows == 0) return 0;
    MGN_REQUIRE(x && saved && dy && dx && grads, "gated MLP backward: NULL tensor");
    MGN_REQUIRE(ws != nullptr, "gated MLP backward: NULL workspace");
    const int h = m->hidden, E = m->expand, HP = width_of(h), EP = expand_pad(h, m->dtype);
    const WsLayout l = ws_layout(m, rows);
    char* w = (char*)ws;
    GArgs a = base_args(m, x, ldx, rows);
    a.saved = (float*)saved;
    a.dy = dy;
    a.lddy = lddy;
    a.dx = dx;
    a.du = w + l.du; a.dv = w + l.dv; a.gx = w + l.gx; a.nx = w + l.nx; a.dyt = w + l.dyt;
    a.part_s = (float*)(w + l.part_s);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = blocks_of(rows, m->max_blocks), S = slabs_of(rows, HP);
    const int64_t R = pad_rows(rows);
    if (int rc = GATED_DISPATCH(launch_bwd, m->dtype, HP, a, (unsigned)nblk, bwd_lds(HP, m->dtype), st)) return rc;
    MGN_LAUNCH_CHECK();
    float *p1 = (float*)(w + l.p1), *p2 = (float*)(w + l.p2), *p3 = (float*)(w + l.p3);
    const WJobs jobs{{a.du, a.dv, a.dyt}, {a.nx, a.nx, a.gx}, {p1, p2, p3}, {EP, EP, HP},
                     {HP + GATED_EXT, HP + GATED_EXT, EP + GATED_EXT}};
    if (m->dtype == MGN_F32)
        launch_wgrad<float>(jobs, R, S, st);
    else
        launch_wgrad<__bf16>(jobs, R, S, st);
    MGN_LAUNCH_CHECK();
    const int64_t total = 2 * (int64_t)h + 2 * ((int64_t)E * h + E) + (int64_t)h * E + h;
    hipLaunchKernelGGL(gated_reduce_kernel, dim3((unsigned)cdiv64(total, MGN_THREADS)), dim3(MGN_THREADS), 0, st,
                       (const float*)a.part_s, nblk, (const float*)p1, (const float*)p2, (const float*)p3, S, h, E, HP,
                       EP, grads);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
