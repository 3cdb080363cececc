// Sparse graph attention (the attention core of the reference's Transformer block, DGL branch:
// layers.py:395-457 bsddmm / softmax / bspmm over the mesh adjacency), forward and backward.
//
//   s[e,b] = (1/sqrt(H)) Σ_d q[row_e, dH+b] k[col_e, dH+b]      (heads interleaved: feature c -> head c % H)
//   p[e,b] = softmax of s over the out-edges of row_e, per head
//   y[i, dH+b] = Σ_{e: row_e = i} p[e,b] v[col_e, dH+b]
//
// Mapping (all three kernels): a GROUP of G lanes (G = power of two >= hidden / CH, CH = the features
// of one 16-byte chunk: 4 fp32 / 8 bf16) owns one node; lane g of the group owns features
// [g*CH, g*CH + CH) of every row it touches, so a gathered row is read with one 16-byte load per lane
// and a wave holds 64/G nodes x 4 edge rows in flight. A lane's chunk covers HL = min(H, CH) heads
// ("slots": element j of the chunk -> slot j % HL -> head (g % (H/HL))*HL + j % HL); per-head dot
// products are butterfly sums over the lanes of the group that hold the same heads. Every workgroup is
// independent, every sum has a fixed order, there are no atomics.
#include "mgn_common.h"

namespace {

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

template <class T, bool VEC>
__device__ __forceinline__ void load_chunk(const T* __restrict__ row, int c0, int hidden, float* o) {
    constexpr int CH = Chunk<T>::N;
    if (VEC) {
        if (c0 < hidden) {
            Chunk<T>::load(row + c0, o);
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j) o[j] = 0.f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CH; ++j) o[j] = c0 + j < hidden ? to_f(row[c0 + j]) : 0.f;
    }
}

template <class T, bool VEC>
__device__ __forceinline__ void store_chunk(T* __restrict__ row, int c0, int hidden, const float* o) {
    constexpr int CH = Chunk<T>::N;
    if (VEC) {
        if (c0 < hidden) Chunk<T>::store(row + c0, o);
    } else {
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (c0 + j < hidden) row[c0 + j] = from_f<T>(o[j]);
    }
}

template <class T, int H>
struct Slots {
    static constexpr int CH = Chunk<T>::N;
    static constexpr int HL = H < CH ? H : CH;  // heads one lane's chunk covers
    static constexpr int STRIDE = H / HL;        // lanes g, g + STRIDE, ... hold the same heads
};

// sums v[0..n) over the lanes of the group that hold the same heads (every such lane gets the sum)
template <int STRIDE, int n>
__device__ __forceinline__ void group_sum(float* v, int G) {
    for (int off = STRIDE; off < G; off <<= 1) {
#pragma unroll
        for (int s = 0; s < n; ++s) v[s] += __shfl_xor(v[s], off, MGN_WAVE);
    }
}

constexpr int EDGES_IN_FLIGHT = 4;

// ---------------------------------------------------------------------------------------- forward
template <class T, int H, bool VEC>
__global__ __launch_bounds__(MGN_THREADS) void attn_fwd_kernel(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ row_perm, const int32_t* __restrict__ csc_dst,
    int64_t N, const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t ld, int hidden,
    int G, float scale, T* __restrict__ y, float* __restrict__ lse) {
    constexpr int CH = Slots<T, H>::CH, HL = Slots<T, H>::HL, STRIDE = Slots<T, H>::STRIDE, U = EDGES_IN_FLIGHT;
    const int64_t gid = (int64_t)blockIdx.x * MGN_THREADS + threadIdx.x;
    const int64_t i = gid / G;
    if (i >= N) return;  // whole groups leave together (G divides the block size)
    const int g = (int)(gid - i * G);
    const int c0 = g * CH;
    float qv[CH], acc[CH], m[HL], l[HL];
    load_chunk<T, VEC>(q + i * ld, c0, hidden, qv);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        qv[j] *= scale;
        acc[j] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < HL; ++s) {
        m[s] = -INFINITY;
        l[s] = 0.f;
    }
    const int pb = row_ptr[i], pe = row_ptr[i + 1];
    for (int p = pb; p < pe; p += U) {
        float kv[U][CH], vv[U][CH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + u < pe) {
                const int64_t j = csc_dst[row_perm[p + u]];
                load_chunk<T, VEC>(k + j * ld, c0, hidden, kv[u]);
                load_chunk<T, VEC>(v + j * ld, c0, hidden, vv[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + u < pe) {  // uniform over the group
                float s[HL];
#pragma unroll
                for (int t = 0; t < HL; ++t) s[t] = 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j) s[j % HL] += qv[j] * kv[u][j];
                group_sum<STRIDE, HL>(s, G);
                float w[HL], corr[HL];
#pragma unroll
                for (int t = 0; t < HL; ++t) {
                    const float mn = fmaxf(m[t], s[t]);
                    corr[t] = expf(m[t] - mn);  // first edge: exp(-inf) = 0
                    w[t] = expf(s[t] - mn);
                    l[t] = l[t] * corr[t] + w[t];
                    m[t] = mn;
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) acc[j] = acc[j] * corr[j % HL] + w[j % HL] * vv[u][j];
            }
        }
    }
    const bool any = pe > pb;
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = any ? acc[j] / l[j % HL] : 0.f;
    store_chunk<T, VEC>(y + i * hidden, c0, hidden, acc);
    if (g < STRIDE) {
#pragma unroll
        for (int s = 0; s < HL; ++s) lse[i * H + g * HL + s] = any ? m[s] + logf(l[s]) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------- backward, pass 1
// Grouped by source node. With dP[e,b] = Σ_d dy[row_e] v[col_e] and δ[i,b] = Σ_{e: row_e = i} p dP (the
// softmax backward's row term, summed from the edges themselves rather than as Σ_d dy·y from the stored —
// in bf16 rounded — y, so that Σ_e dS = 0 per node holds to fp32 rounding): dS = p (dP − δ) and
//   dq[i] = scale (Σ_e p dP k[col_e] − δ Σ_e p k[col_e]).
// Writes p and dP of every edge at the edge's target-sorted position, ws[t*2H + b] = p[e,b],
// ws[t*2H + H + b] = dP[e,b], and delta[i*H + b] = δ[i,b] for pass 2.
template <class T, int H, bool VEC>
__global__ __launch_bounds__(MGN_THREADS) void attn_bwd_src_kernel(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ row_perm, const int32_t* __restrict__ csc_dst,
    int64_t N, const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t ld,
    const float* __restrict__ lse, const T* __restrict__ dy, int hidden, int G, float scale,
    T* __restrict__ dq, float* __restrict__ ws, float* __restrict__ delta) {
    constexpr int CH = Slots<T, H>::CH, HL = Slots<T, H>::HL, STRIDE = Slots<T, H>::STRIDE, U = EDGES_IN_FLIGHT;
    const int64_t gid = (int64_t)blockIdx.x * MGN_THREADS + threadIdx.x;
    const int64_t i = gid / G;
    if (i >= N) return;
    const int g = (int)(gid - i * G);
    const int c0 = g * CH;
    const int hb = (g % STRIDE) * HL;  // first head of this lane's slots
    float qv[CH], dyv[CH], acc[CH], pk[CH], dl[HL], ls[HL];
    load_chunk<T, VEC>(q + i * ld, c0, hidden, qv);
    load_chunk<T, VEC>(dy + i * hidden, c0, hidden, dyv);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        qv[j] *= scale;
        acc[j] = pk[j] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < HL; ++s) {
        ls[s] = lse[i * H + hb + s];
        dl[s] = 0.f;
    }
    const int pb = row_ptr[i], pe = row_ptr[i + 1];
    for (int p = pb; p < pe; p += U) {
        float kv[U][CH], vv[U][CH];
        int tpos[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + u < pe) {
                tpos[u] = row_perm[p + u];
                const int64_t j = csc_dst[tpos[u]];
                load_chunk<T, VEC>(k + j * ld, c0, hidden, kv[u]);
                load_chunk<T, VEC>(v + j * ld, c0, hidden, vv[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + u < pe) {
                float r[2 * HL];  // [s ‖ dP]
#pragma unroll
                for (int t = 0; t < 2 * HL; ++t) r[t] = 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    r[j % HL] += qv[j] * kv[u][j];
                    r[HL + j % HL] += dyv[j] * vv[u][j];
                }
                group_sum<STRIDE, 2 * HL>(r, G);
                float pr[HL], pd[HL];
#pragma unroll
                for (int t = 0; t < HL; ++t) {
                    pr[t] = expf(r[t] - ls[t]);
                    pd[t] = pr[t] * r[HL + t];
                    dl[t] += pd[t];
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    acc[j] += pd[j % HL] * kv[u][j];
                    pk[j] += pr[j % HL] * kv[u][j];
                }
                if (g < STRIDE) {
                    float* w = ws + (int64_t)tpos[u] * (2 * H) + hb;
#pragma unroll
                    for (int t = 0; t < HL; ++t) {
                        w[t] = pr[t];
                        w[H + t] = r[HL + t];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = scale * (acc[j] - dl[j % HL] * pk[j]);
    store_chunk<T, VEC>(dq + i * hidden, c0, hidden, acc);
    if (g < STRIDE) {
#pragma unroll
        for (int s = 0; s < HL; ++s) delta[i * H + hb + s] = dl[s];
    }
}

// ---------------------------------------------------------------------------------------- backward, pass 2
// Grouped by target node, in target-sorted order: with dS[e] = p[e] (dP[e] − δ[row_e]),
// dk[j] = scale Σ dS[e] q[row_e], dv[j] = Σ p[e] dy[row_e].
template <class T, int H, bool VEC>
__global__ __launch_bounds__(MGN_THREADS) void attn_bwd_dst_kernel(
    const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ csc_src, int64_t N, const T* __restrict__ q,
    int64_t ld, const T* __restrict__ dy, const float* __restrict__ ws, const float* __restrict__ delta, int hidden,
    int G, float scale, T* __restrict__ dk, T* __restrict__ dv) {
    constexpr int CH = Slots<T, H>::CH, HL = Slots<T, H>::HL, STRIDE = Slots<T, H>::STRIDE, U = EDGES_IN_FLIGHT;
    const int64_t gid = (int64_t)blockIdx.x * MGN_THREADS + threadIdx.x;
    const int64_t jn = gid / G;
    if (jn >= N) return;
    const int g = (int)(gid - jn * G);
    const int c0 = g * CH;
    const int hb = (g % STRIDE) * HL;
    float ak[CH], av[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) ak[j] = av[j] = 0.f;
    const int tb = col_ptr[jn], te = col_ptr[jn + 1];
    for (int t = tb; t < te; t += U) {
        float qv[U][CH], dyv[U][CH], pr[U][HL], ds[U][HL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t + u < te) {
                const int64_t i = csc_src[t + u];
                load_chunk<T, VEC>(q + i * ld, c0, hidden, qv[u]);
                load_chunk<T, VEC>(dy + i * hidden, c0, hidden, dyv[u]);
                const float* w = ws + (int64_t)(t + u) * (2 * H) + hb;
                const float* dl = delta + i * H + hb;
#pragma unroll
                for (int s = 0; s < HL; ++s) {
                    pr[u][s] = w[s];
                    ds[u][s] = w[s] * (w[H + s] - dl[s]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t + u < te) {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    ak[j] += ds[u][j % HL] * qv[u][j];
                    av[j] += pr[u][j % HL] * dyv[u][j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) ak[j] *= scale;
    store_chunk<T, VEC>(dk + jn * hidden, c0, hidden, ak);
    store_chunk<T, VEC>(dv + jn * hidden, c0, hidden, av);
}

// ---------------------------------------------------------------------------------------- host side
int check_shape(int32_t hidden, int32_t heads, int32_t dtype) {
    MGN_REQUIRE(dtype == MGN_F32 || dtype == MGN_BF16, "graph attention: dtype must be MGN_F32 or MGN_BF16");
    MGN_REQUIRE(heads == 1 || heads == 2 || heads == 4 || heads == 8,
                "graph attention: heads must be 1, 2, 4 or 8 (got " + std::to_string(heads) + ")");
    MGN_REQUIRE(hidden >= 1 && hidden <= 256,
                "graph attention: hidden must be in [1, 256] (got " + std::to_string(hidden) + ")");
    MGN_REQUIRE(hidden % heads == 0, "graph attention: hidden (" + std::to_string(hidden) +
                                         ") must be a multiple of heads (" + std::to_string(heads) + ")");
    return 0;
}

int group_lanes(int hidden, int dtype) {
    const int nch = cdiv(hidden, dtype == MGN_F32 ? 4 : 8);
    int G = 1;
    while (G < nch) G <<= 1;
    return G;
}

size_t edge_ws_bytes(const mgn_topology* t, int heads) {
    return al256((size_t)t->num_edges * 2 * (size_t)heads * sizeof(float));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct FwdArgs {
    const mgn_topology* t;
    const void *q, *k, *v;
    int64_t ld;
    int hidden, G;
    float scale;
    void* y;
    float* lse;
    hipStream_t st;
    unsigned blocks;
};
template <class T, int H, bool VEC>
void launch_fwd(const FwdArgs& a) {
    hipLaunchKernelGGL((attn_fwd_kernel<T, H, VEC>), dim3(a.blocks), dim3(MGN_THREADS), 0, a.st, a.t->row_ptr,
                       a.t->row_perm, a.t->csc_dst, a.t->num_nodes, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.ld,
                       a.hidden, a.G, a.scale, (T*)a.y, a.lse);
}

struct BwdArgs {
    const mgn_topology* t;
    const void *q, *k, *v, *dy;
    const float* lse;
    int64_t ld;
    int hidden, G;
    float scale;
    void *dq, *dk, *dv;
    float *ws, *delta;
    hipStream_t st;
    unsigned blocks;
};
template <class T, int H, bool VEC>
void launch_bwd(const BwdArgs& a) {
    hipLaunchKernelGGL((attn_bwd_src_kernel<T, H, VEC>), dim3(a.blocks), dim3(MGN_THREADS), 0, a.st, a.t->row_ptr,
                       a.t->row_perm, a.t->csc_dst, a.t->num_nodes, (const T*)a.q, (const T*)a.k, (const T*)a.v, a.ld,
                       a.lse, (const T*)a.dy, a.hidden, a.G, a.scale, (T*)a.dq, a.ws, a.delta);
    hipLaunchKernelGGL((attn_bwd_dst_kernel<T, H, VEC>), dim3(a.blocks), dim3(MGN_THREADS), 0, a.st, a.t->col_ptr,
                       a.t->csc_src, a.t->num_nodes, (const T*)a.q, a.ld, (const T*)a.dy, (const float*)a.ws,
                       (const float*)a.delta, a.hidden, a.G, a.scale, (T*)a.dk, (T*)a.dv);
}

// dispatch on (dtype, heads, 16-byte rows) to the launcher template F<T, H, VEC>
#define ATTN_DISPATCH(FN, args, dtype, heads, vec)                    \
    do {                                                              \
        if ((dtype) == MGN_F32) {                                     \
            ATTN_DISPATCH_H(FN, float, args, heads, vec);             \
        } else {                                                      \
            ATTN_DISPATCH_H(FN, __bf16, args, heads, vec);            \
        }                                                             \
    } while (0)
#define ATTN_DISPATCH_H(FN, T, args, heads, vec)                      \
    switch (heads) {                                                  \
        case 1: ATTN_DISPATCH_V(FN, T, 1, args, vec); break;          \
        case 2: ATTN_DISPATCH_V(FN, T, 2, args, vec); break;          \
        case 4: ATTN_DISPATCH_V(FN, T, 4, args, vec); break;          \
        default: ATTN_DISPATCH_V(FN, T, 8, args, vec); break;         \
    }
#define ATTN_DISPATCH_V(FN, T, H, args, vec)                          \
    do {                                                              \
        if (vec)                                                      \
            FN<T, H, true>(args);                                     \
        else                                                          \
            FN<T, H, false>(args);                                    \
    } while (0)

}  // namespace

extern "C" {

size_t mgn_graph_attention_workspace_bytes(const mgn_topology* t, int32_t hidden, int32_t heads, int32_t dtype) {
    if (t == nullptr || heads < 1 || t->num_edges < 0 || t->num_nodes < 0) return 0;
    // (p, dP) per edge and head, then δ per node and head
    return edge_ws_bytes(t, heads) + al256((size_t)t->num_nodes * (size_t)heads * sizeof(float));
}

int mgn_graph_attention_forward(const mgn_topology* t, const void* q, const void* k, const void* v, int64_t ld,
                                int32_t hidden, int32_t heads, int32_t dtype, void* y, float* lse,
                                mgn_stream_t stream) {
    if (int rc = check_shape(hidden, heads, dtype)) return rc;
    MGN_REQUIRE(t != nullptr, "graph attention: topology is NULL");
    MGN_REQUIRE(ld >= hidden, "graph attention: ld (row stride of q, k, v) must be >= hidden");
    const int64_t N = t->num_nodes;
    if (N == 0) return 0;
    MGN_REQUIRE(q && k && v && y && lse, "graph attention forward: NULL tensor");
    const int ch = dtype == MGN_F32 ? 4 : 8;
    const bool vec = hidden % ch == 0 && ld % ch == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(y);
    FwdArgs a{t, q, k, v, ld, hidden, group_lanes(hidden, dtype), (float)(1.0 / sqrt((double)heads)), y, lse,
              (hipStream_t)stream, 0};
    a.blocks = (unsigned)cdiv64(N * a.G, MGN_THREADS);
    ATTN_DISPATCH(launch_fwd, a, dtype, heads, vec);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_graph_attention_backward(const mgn_topology* t, const void* q, const void* k, const void* v, const void* y,
                                 const float* lse, const void* dy, int64_t ld, int32_t hidden, int32_t heads,
                                 int32_t dtype, void* dq, void* dk, void* dv, void* ws, size_t ws_bytes,
                                 mgn_stream_t stream) {
    if (int rc = check_shape(hidden, heads, dtype)) return rc;
    MGN_REQUIRE(t != nullptr, "graph attention: topology is NULL");
    MGN_REQUIRE(ld >= hidden, "graph attention: ld (row stride of q, k, v) must be >= hidden");
    MGN_REQUIRE(ws_bytes >= mgn_graph_attention_workspace_bytes(t, hidden, heads, dtype),
                "graph attention backward: workspace too small (mgn_graph_attention_workspace_bytes)");
    const int64_t N = t->num_nodes;
    if (N == 0) return 0;
    MGN_REQUIRE(q && k && v && y && lse && dy && dq && dk && dv, "graph attention backward: NULL tensor");
    MGN_REQUIRE(ws != nullptr, "graph attention backward: NULL workspace");
    const int ch = dtype == MGN_F32 ? 4 : 8;
    const bool vec = hidden % ch == 0 && ld % ch == 0 && aligned16(q) && aligned16(k) && aligned16(v) &&
                     aligned16(dy) && aligned16(dq) && aligned16(dk) && aligned16(dv);
    BwdArgs a{t, q, k, v, dy, lse, ld, hidden, group_lanes(hidden, dtype), (float)(1.0 / sqrt((double)heads)),
              dq, dk, dv, (float*)ws, (float*)((char*)ws + edge_ws_bytes(t, heads)), (hipStream_t)stream, 0};
    a.blocks = (unsigned)cdiv64(N * a.G, MGN_THREADS);
    ATTN_DISPATCH(launch_bwd, a, dtype, heads, vec);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
