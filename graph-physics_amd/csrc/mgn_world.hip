// Per-frame world edges as a topology, built without the host (mgn.h, "World edges inside the step"), gfx950.
//
// The reference's add_world_edges (dataset/preprocessing.py:92-140) runs per sample: cKDTree.query_pairs(radius)
// over the world positions, the pairs filtered to OBSTACLE–NORMAL, appended to the mesh edges, to_undirected. The
// result is a new edge_index per sample, so a model whose attention is masked by the adjacency (the transformer
// configs) sees a new mask per sample. mgn_radius_pairs + mgn_coalesce + mgn_topology_build do that with three host
// read-backs and two radix sorts; nothing of it can sit in a captured step.
//
// Here the mesh adjacency is static CSR (sorted, symmetric, unique) and only the world pairs change, so the
// (row, col) order of the union is a per-node MERGE of two ascending lists, and the target-sorted order of a
// symmetric adjacency is the same lists again: no sort of the edge list, no data-dependent launch shape.
//   world_search   one thread per node i, 256 per workgroup. The candidates — the rows of the graphs the workgroup's
//                  256 nodes belong to — are staged through LDS in tiles of WORLD_TILE (position and type: 16 bytes a
//                  candidate, every lane reads the same address, a broadcast). A NORMAL node keeps the OBSTACLE
//                  nodes of its own graph within the radius, an OBSTACLE node the NORMAL ones; a candidate found in
//                  the node's mesh list (binary search) is dropped. The survivors go, ascending, into wl[i·W ..],
//                  their count into wc[i]. Both directions evaluate the same fp64 expression on the same two rows
//                  (the difference only changes sign), so the lists are symmetric.
//   world_scan     one workgroup: the exclusive scan of mesh_deg + wc, into col_ptr and row_ptr, and num_edges.
//   world_merge    eight lanes per node i: mesh[i] and wl[i] are merged into its segment of csc_src / csc_dst (the
//                  lists share no value, so an entry's merged place is its index plus its rank in the other list),
//                  and for every merged edge (j → i) the rank of i among j's neighbours (two binary searches) is
//                  the edge's place in (row, col) order, which gives csc_eid, row_perm and both edge_index rows.
// Brute force per graph is deliberate: contact sets are small, it needs no bounding box, no grid and no sort, and
// the order of every list is fixed. Every grid is a function of N alone.
//
// Random long-range edges (mgn.h, "Random edges inside the step"; the reference's _add_random_edges,
// dataset/dataset.py:104-137) reuse the scan and the merge: only the producer of the per-node lists differs.
//   random_map     one thread per candidate c: the graph whose candidate range holds c (binary search) and the mapped
//                  endpoints (a, b) = (lo_g + u % n_g, lo_g + v % n_g), so that the search loads plain pairs.
//   random_search  pass 1, mapped like world_search: one thread per node i, 256 per workgroup. The candidates of the
//                  graphs that own the workgroup's nodes are staged through LDS in tiles of RANDOM_TILE (loaded into
//                  registers one tile ahead), each entry the mapped endpoints (a, b), 8 bytes, read by every lane at
//                  the same address (a broadcast); one unsigned minimum over a ^ i and b ^ i per chunk of eight. The
//                  candidates that touch i are queued per lane (in LDS) and walked, in order, at the end: one
//                  that is no self-pair and no mesh edge (binary search) and whose other endpoint j is not yet in
//                  the node's list (a linear look-up, the list holds at most 64) is appended to wl[i*W ..] with its
//                  candidate id beside it in wid[i*W ..]; when the list is full the candidate is flagged instead
//                  (flag[c] = 1, a plain store: both endpoints may write the same 1).
//   random_filter  pass 2, one thread per node: the entries whose candidate is unflagged, insertion-sorted ascending
//                  in place, and their count into wc[i]. A pair survives exactly when its first candidate is
//                  unflagged, which both endpoints see alike, so the lists are symmetric, as world_merge needs.
// No atomics, no read-back; the grids are functions of N and of the candidate count, both fixed at construction.
//
// Both together (mgn.h, "World and random edges inside the step"; the reference's order: add_world_edges, then
// _add_random_edges on top of the edge_index that left): world_search fills the world lists, random_search takes them
// as a second exclusion list (a candidate that is a world edge of this build is skipped like a mesh edge: one more
// binary search in the queued drain, over a list that is symmetric, so both endpoints see the same verdict),
// random_filter sorts the random lists, and ONE scan and ONE merge run over three ascending, pairwise-disjoint lists
// per node: mesh, world, random. A null third list leaves the scan and the merge of the two builds above as they were.
#include "mgn_common.h"

namespace {

constexpr int WORLD_THREADS = 256;
constexpr int WORLD_TILE = 1024;
constexpr int WORLD_CHUNK = 8;
constexpr int WORLD_MERGE_LANES = 8;  // lanes that share one node's edges in world_merge
constexpr int WORLD_SCAN_THREADS = 1024;

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// first position in the ascending a[0, n) whose value is >= v
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(WORLD_THREADS) void world_search(
    const float* __restrict__ pos, int64_t ldp, const float* __restrict__ nt, int64_t ldt,
    const int32_t* __restrict__ graph_ptr, int B, int N, const int32_t* __restrict__ mesh_ptr,
    const int32_t* __restrict__ mesh_nbr, int E_m, double r2, int W, int32_t* __restrict__ wl,
    int32_t* __restrict__ wc, uint32_t* __restrict__ err) {
#pragma clang fp contract(off)  // (v0·v0 + v1·v1) + v2·v2 in fp64, every product and sum rounded on its own
    __shared__ f4 cand[WORLD_TILE];  // x, y, z, node type
    const int b0 = blockIdx.x * WORLD_THREADS;
    const int b1 = min(N, b0 + WORLD_THREADS);  // b0 < N: the grid is cdiv(N, 256)
    const int i = b0 + threadIdx.x;
    const bool active = i < N;
    // the rows of every graph that owns one of this workgroup's nodes: uniform over the workgroup
    const int c0 = clampi(graph_ptr[graph_of_row(graph_ptr, B, b0)], 0, N);
    const int c1 = clampi(graph_ptr[graph_of_row(graph_ptr, B, b1 - 1) + 1], 0, N);
    int r0 = 0, r1 = 0, m0 = 0, md = 0;
    float want = -1.f;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (active) {
        const int g = graph_of_row(graph_ptr, B, i);
        r0 = graph_ptr[g];
        r1 = graph_ptr[g + 1];
        const float a = nt[(int64_t)i * ldt];
        if (a == 0.f) want = 1.f;       // NORMAL looks for OBSTACLE
        else if (a == 1.f) want = 0.f;  // OBSTACLE looks for NORMAL; every other type (and NaN) has no world edges
        m0 = clampi(mesh_ptr[i], 0, E_m);
        md = clampi(mesh_ptr[i + 1], m0, E_m) - m0;
        const float* p = pos + (int64_t)i * ldp;
        px = (double)p[0];
        py = (double)p[1];
        pz = (double)p[2];
    }
    const bool searching = want >= 0.f;
    int cnt = 0;
    for (int t0 = c0; t0 < c1; t0 += WORLD_TILE) {
        const int nc = min(WORLD_TILE, c1 - t0);
        for (int c = threadIdx.x; c < nc; c += WORLD_THREADS) {
            const float* p = pos + (int64_t)(t0 + c) * ldp;
            cand[c] = f4{p[0], p[1], p[2], nt[(int64_t)(t0 + c) * ldt]};
        }
        __syncthreads();
        if (searching) {
            const int lo = max(r0, t0) - t0, hi = min(r1, t0 + nc) - t0;  // the node's own graph within the tile
            // WORLD_CHUNK candidates at a time: their LDS reads are issued together, ahead of the tests, so the
            // wave does not wait for every read on its own
            for (int c = lo; c < hi; c += WORLD_CHUNK) {
                f4 q[WORLD_CHUNK];
#pragma unroll
                for (int u = 0; u < WORLD_CHUNK; ++u) q[u] = cand[min(c + u, hi - 1)];
#pragma unroll
                for (int u = 0; u < WORLD_CHUNK; ++u) {
                    if (c + u >= hi || q[u][3] != want) continue;
                    const double v0 = px - (double)q[u][0], v1 = py - (double)q[u][1], v2 = pz - (double)q[u][2];
                    double d2 = v0 * v0;
                    d2 = d2 + v1 * v1;
                    d2 = d2 + v2 * v2;
                    if (!(d2 <= r2)) continue;
                    const int j = t0 + c + u;
                    const int at = lower_bound_i32(mesh_nbr + m0, md, j);
                    if (at < md && mesh_nbr[m0 + at] == j) continue;  // already a mesh edge: to_undirected keeps one
                    if (cnt < W) wl[(int64_t)i * W + cnt] = j;
                    ++cnt;
                }
            }
        }
        __syncthreads();
    }
    if (active) {
        wc[i] = cnt < W ? cnt : W;
        if (cnt > W) atomicOr(err, MGN_ERR_WORLD_CAPACITY);
    }
}

// ptr[i] = Σ_{r < i} (mesh_deg[r] + wc[r] + wc2[r]) for i in [0, N], into col_ptr and row_ptr; *num_edges = ptr[N].
// wc2: the counts of a third list per node (the combined build), or null. One workgroup: a thread sums a contiguous
// chunk, the chunk sums are scanned in LDS (Hillis–Steele), the thread walks its chunk again. Integers: any order gives
// the same result.
__global__ __launch_bounds__(WORLD_SCAN_THREADS) void world_scan(const int32_t* __restrict__ mesh_ptr, int E_m,
                                                                 const int32_t* __restrict__ wc,
                                                                 const int32_t* __restrict__ wc2, int N, int E_cap,
                                                                 int32_t* __restrict__ col_ptr,
                                                                 int32_t* __restrict__ row_ptr,
                                                                 int32_t* __restrict__ num_edges) {
    __shared__ int part[WORLD_SCAN_THREADS];
    const int chunk = (N + WORLD_SCAN_THREADS - 1) / WORLD_SCAN_THREADS;
    const int a = min(N, (int)threadIdx.x * chunk), b = min(N, a + chunk);
    int s = 0;
    for (int r = a; r < b; ++r) {
        const int m0 = clampi(mesh_ptr[r], 0, E_m);
        s += clampi(mesh_ptr[r + 1], m0, E_m) - m0 + wc[r] + (wc2 ? wc2[r] : 0);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < WORLD_SCAN_THREADS; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;  // exclusive
    for (int r = a; r < b; ++r) {
        const int v = clampi(run, 0, E_cap);  // a valid mesh never exceeds E_cap; a broken one stays in bounds
        col_ptr[r] = v;
        row_ptr[r] = v;
        const int m0 = clampi(mesh_ptr[r], 0, E_m);
        run += clampi(mesh_ptr[r + 1], m0, E_m) - m0 + wc[r] + (wc2 ? wc2[r] : 0);
    }
    if (threadIdx.x == WORLD_SCAN_THREADS - 1) {
        const int total = clampi(part[threadIdx.x], 0, E_cap);
        col_ptr[N] = total;
        row_ptr[N] = total;
        *num_edges = total;
    }
}

__global__ __launch_bounds__(256) void world_merge(const int32_t* __restrict__ mesh_ptr,
                                                   const int32_t* __restrict__ mesh_nbr, int E_m,
                                                   const int32_t* __restrict__ wl, const int32_t* __restrict__ wc,
                                                   int W, const int32_t* __restrict__ wl2,
                                                   const int32_t* __restrict__ wc2, int W2, int N, int E_cap,
                                                   const int32_t* __restrict__ col_ptr,
                                                   int32_t* __restrict__ csc_src, int32_t* __restrict__ csc_dst,
                                                   int32_t* __restrict__ csc_eid, int32_t* __restrict__ row_perm,
                                                   int64_t* __restrict__ edge_index, uint32_t* __restrict__ err) {
    // WORLD_MERGE_LANES lanes per node, lane s taking the node's edges s, s + 8, ...: the lists share no value, so an
    // entry's place in the merged list is its own index plus its rank in every OTHER list; no lane waits for another.
    // wl2 / wc2: a third ascending list per node, disjoint from the other two (the combined build), or null (no entry)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / WORLD_MERGE_LANES), sub = (int)(t % WORLD_MERGE_LANES);
    if (i >= N) return;
    const int m0 = clampi(mesh_ptr[i], 0, E_m);
    const int md = clampi(mesh_ptr[i + 1], m0, E_m) - m0;
    const int32_t* ma = mesh_nbr + m0;
    const int32_t* wa = wl + (int64_t)i * W;
    const int wd = wc[i];
    const int32_t* ra = wl2 ? wl2 + (int64_t)i * W2 : nullptr;
    const int rd = wl2 ? wc2[i] : 0;
    const int base = col_ptr[i];
    bool bad = false;
    for (int p = sub; p < md + wd + rd; p += WORLD_MERGE_LANES) {
        int j, at;
        if (p < md) {
            j = ma[p];
            at = p + lower_bound_i32(wa, wd, j);
            if (rd > 0) at += lower_bound_i32(ra, rd, j);
        } else if (p < md + wd) {
            j = wa[p - md];
            at = p - md + lower_bound_i32(ma, md, j);
            if (rd > 0) at += lower_bound_i32(ra, rd, j);
        } else {
            j = ra[p - md - wd];
            at = p - md - wd + lower_bound_i32(ma, md, j) + lower_bound_i32(wa, wd, j);
        }
        if (j < 0 || j >= N) {  // a mesh neighbour outside [0, N): flagged, clamped, every access stays in bounds
            bad = true;
            j = clampi(j, 0, N - 1);
        }
        // the rank of i among j's neighbours: edge (j → i) is the e-th in (row, col) order
        const int jm0 = clampi(mesh_ptr[j], 0, E_m);
        const int jmd = clampi(mesh_ptr[j + 1], jm0, E_m) - jm0;
        int e = col_ptr[j] + lower_bound_i32(mesh_nbr + jm0, jmd, i) + lower_bound_i32(wl + (int64_t)j * W, wc[j], i);
        if (wl2) e += lower_bound_i32(wl2 + (int64_t)j * W2, wc2[j], i);
        e = clampi(e, 0, E_cap - 1);  // equal to its exact value unless a list overflowed (see MGN_ERR_WORLD_CAPACITY)
        const int k = base + at;  // at <= md + wd + rd - 1 for sorted, disjoint lists; guarded for anything else
        if (k >= 0 && k < E_cap) {
            csc_src[k] = j;
            csc_dst[k] = i;
            csc_eid[k] = e;
            row_perm[e] = k;
            edge_index[e] = j;
            edge_index[(int64_t)E_cap + e] = i;
        }
    }
    if (bad) atomicOr(err, MGN_ERR_EDGE_INDEX);
}

constexpr int RANDOM_TILE = 1024;  // candidates per LDS tile: 8 KiB
constexpr int RANDOM_CHUNK = 8;
constexpr int RANDOM_QUEUE = 32;  // hits a lane queues before it walks them: at least 2 * RANDOM_CHUNK
constexpr int RANDOM_MAX_NEW = 64;

constexpr int RANDOM_STAGE = (RANDOM_TILE + RANDOM_CHUNK + WORLD_THREADS - 1) / WORLD_THREADS;  // entries a thread stages

// mapped[c] = the endpoints (a, b) of candidate c: one thread per candidate. The graph whose candidate range holds c
// is found by binary search; (-1, -1), which matches no node, for a graph without nodes. The draws are non-negative;
// the mask keeps any other bits in range as well.
__global__ __launch_bounds__(WORLD_THREADS) void random_map(const int32_t* __restrict__ pairs,
                                                            const int32_t* __restrict__ cand_ptr, int C,
                                                            const int32_t* __restrict__ graph_ptr, int B, int N,
                                                            const int32_t* __restrict__ enabled,
                                                            int2* __restrict__ mapped) {
    const int c = blockIdx.x * WORLD_THREADS + threadIdx.x;
    if (c >= C || *enabled == 0) return;  // switched off, the search reads no candidate
    const int g = graph_of_row(cand_ptr, B, c);
    const int lo = clampi(graph_ptr[g], 0, N);
    const int n = clampi(graph_ptr[g + 1], lo, N) - lo;
    int2 e = make_int2(-1, -1);
    if (n > 0) {
        const int u = pairs[2 * (int64_t)c] & 0x7fffffff, v = pairs[2 * (int64_t)c + 1] & 0x7fffffff;
        e = make_int2(lo + u % n, lo + v % n);
    }
    mapped[c] = e;
}

__global__ __launch_bounds__(WORLD_THREADS) void random_search(
    const int2* __restrict__ mapped, const int32_t* __restrict__ cand_ptr, int C,
    const int32_t* __restrict__ graph_ptr, int B, int N, const int32_t* __restrict__ mesh_ptr,
    const int32_t* __restrict__ mesh_nbr, int E_m, const int32_t* __restrict__ xl, const int32_t* __restrict__ xc,
    int XW, int W, const int32_t* __restrict__ enabled, int32_t* wl, int32_t* wid, int32_t* __restrict__ wc,
    int32_t* __restrict__ flag) {
    // xl / xc / XW: a second exclusion list per node, ascending, xc[i] entries at xl[i * XW ..] (the world neighbours of
    // the combined build), or null / 0
    // the mapped endpoints (a, b) of a tile; (-1, -1) behind its end, so that a chunk may be read whole
    __shared__ int2 cand[RANDOM_TILE + RANDOM_CHUNK];
    __shared__ int32_t queue[RANDOM_QUEUE][WORLD_THREADS];  // per lane: the candidates that touch its node
    const int b0 = blockIdx.x * WORLD_THREADS;
    const int b1 = min(N, b0 + WORLD_THREADS);  // b0 < N: the grid is cdiv(N, 256)
    const int i = b0 + threadIdx.x;
    const bool active = i < N;
    // the candidates of every graph that owns one of this workgroup's nodes: uniform over the workgroup. Switched
    // off (the device word is 0), the range is empty and every list stays empty
    int c0 = 0, c1 = 0;
    if (*enabled != 0) {
        c0 = clampi(cand_ptr[graph_of_row(graph_ptr, B, b0)], 0, C);
        c1 = clampi(cand_ptr[graph_of_row(graph_ptr, B, b1 - 1) + 1], c0, C);
    }
    int q0 = 0, q1 = 0, m0 = 0, md = 0, xd = 0;
    if (active) {
        const int g = graph_of_row(graph_ptr, B, i);
        q0 = clampi(cand_ptr[g], c0, c1);
        q1 = clampi(cand_ptr[g + 1], q0, c1);
        m0 = clampi(mesh_ptr[i], 0, E_m);
        md = clampi(mesh_ptr[i + 1], m0, E_m) - m0;
        if (xl) xd = clampi(xc[i], 0, XW);
    }
    const int32_t* excl = xl ? xl + (int64_t)i * XW : nullptr;  // read only below xd, which is 0 for an inactive lane
    int32_t* mine = wl + (int64_t)i * W;
    int32_t* mine_id = wid + (int64_t)i * W;
    int cnt = 0, qn = 0;
    // Pass 1 on this lane's queued hits, in candidate order. A hit costs a chain of dependent global loads (the
    // mesh's binary search, the look-up in the node's own list), and a wave that handled every hit where it found
    // it would pay that chain once per hit of any of its lanes, one after the other; queued, the lanes walk their
    // own hits side by side: once at the end, and before that only for a lane whose queue is nearly full
    auto drain = [&]() {
        for (int s = 0; s < qn; ++s) {
            const int c = queue[s][threadIdx.x];
            const int2 q = mapped[c];
            if (q.x == q.y) continue;  // a self-pair
            const int j = q.x == i ? q.y : q.x;
            const int at = lower_bound_i32(mesh_nbr + m0, md, j);
            if (at < md && mesh_nbr[m0 + at] == j) continue;  // a mesh edge already
            if (xd > 0) {
                const int xa = lower_bound_i32(excl, xd, j);
                if (xa < xd && excl[xa] == j) continue;  // an edge of the second list already (a world edge)
            }
            bool seen = false;
            for (int k = 0; k < cnt; ++k) seen = seen || mine[k] == j;
            if (seen) continue;  // a repeat
            if (cnt == W) {
                flag[c] = 1;  // dropped: pass 2 removes it at the other endpoint as well
            } else {
                mine[cnt] = j;
                mine_id[cnt] = c;
                ++cnt;
            }
        }
        qn = 0;
    };
    // a tile's entries are loaded into registers one tile ahead, before the scan of the tile in LDS, so that the scan
    // hides their latency
    int2 next[RANDOM_STAGE];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int k = 0; k < RANDOM_STAGE; ++k) {
            const int c = threadIdx.x + k * WORLD_THREADS;
            next[k] = c < RANDOM_TILE && t0 + c < c1 ? mapped[t0 + c] : make_int2(-1, -1);
        }
    };
    fetch(c0);
    for (int t0 = c0; t0 < c1; t0 += RANDOM_TILE) {
        const int nc = min(RANDOM_TILE, c1 - t0);
#pragma unroll
        for (int k = 0; k < RANDOM_STAGE; ++k) {
            const int c = threadIdx.x + k * WORLD_THREADS;
            if (c < RANDOM_TILE + RANDOM_CHUNK) cand[c] = next[k];
        }
        fetch(t0 + RANDOM_TILE);
        __syncthreads();
        if (active) {
            // the node's own graph within the tile, from a chunk boundary on: the candidates ahead of lo and behind
            // hi are other graphs' (their endpoints are other graphs' nodes) or the padding, and match no i
            const int lo = max(q0, t0) - t0, hi = min(q1, t0 + nc) - t0;
            // RANDOM_CHUNK candidates at a time: their LDS reads are issued together, and one unsigned minimum over
            // a ^ i and b ^ i says whether any of them touches i (three VALU operations a candidate, no branch)
            for (int c = lo & ~(RANDOM_CHUNK - 1); c < hi; c += RANDOM_CHUNK) {
                int2 q[RANDOM_CHUNK];
#pragma unroll
                for (int u = 0; u < RANDOM_CHUNK; ++u) q[u] = cand[c + u];
                unsigned none = ~0u;
#pragma unroll
                for (int u = 0; u < RANDOM_CHUNK; ++u)
                    none = min(none, min((unsigned)(q[u].x ^ i), (unsigned)(q[u].y ^ i)));
                if (none != 0u) continue;
#pragma unroll
                for (int u = 0; u < RANDOM_CHUNK; ++u)
                    if (c + u >= lo && c + u < hi && (q[u].x == i || q[u].y == i)) queue[qn++][threadIdx.x] = t0 + c + u;
                if (qn > RANDOM_QUEUE - RANDOM_CHUNK) drain();  // room for the next chunk's hits
            }
        }
        __syncthreads();
    }
    if (active) {
        drain();
        wc[i] = cnt;
    }
}

__global__ __launch_bounds__(WORLD_THREADS) void random_filter(int N, int W, int C, int32_t* wl,
                                                               const int32_t* __restrict__ wid,
                                                               int32_t* __restrict__ wc,
                                                               const int32_t* __restrict__ flag) {
    const int i = blockIdx.x * WORLD_THREADS + threadIdx.x;
    if (i >= N) return;
    int32_t* mine = wl + (int64_t)i * W;
    const int32_t* mine_id = wid + (int64_t)i * W;
    const int n = clampi(wc[i], 0, W);
    int k = 0;
    for (int p = 0; p < n; ++p) {
        const int c = mine_id[p], j = mine[p];
        if (c < 0 || c >= C || flag[c] != 0) continue;
        int q = k;  // k <= p: entry p was read above, the entries behind it are untouched
        for (; q > 0 && mine[q - 1] > j; --q) mine[q] = mine[q - 1];
        mine[q] = j;
        ++k;
    }
    wc[i] = k;
}

}  // namespace

extern "C" {

size_t mgn_world_topology_workspace_bytes(int64_t num_nodes, int32_t max_neighbors) {
    const int64_t n = num_nodes < 1 ? 1 : num_nodes, w = max_neighbors < 1 ? 1 : max_neighbors;
    return al((size_t)n * 4) + al((size_t)n * (size_t)w * 4);
}

int mgn_world_topology_build(const float* pos, int64_t ld_pos, const float* node_type, int64_t ld_type,
                             const int32_t* graph_ptr, int32_t B, int64_t N, const int32_t* mesh_ptr,
                             const int32_t* mesh_nbr, int64_t E_m, double radius, int32_t W, int32_t* csc_src,
                             int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr, int32_t* row_ptr, int32_t* row_perm,
                             int64_t* edge_index, int32_t* num_edges, uint32_t* err_word, void* ws, size_t ws_bytes,
                             mgn_stream_t stream) {
    const std::string who = "world_topology_build";
    MGN_REQUIRE(N >= 0 && B >= 0 && E_m >= 0, who + ": N, B and E_m must be >= 0");
    MGN_REQUIRE(W >= 1, who + ": max_neighbors must be >= 1");
    MGN_REQUIRE(radius > 0.0 && std::isfinite(radius), who + ": radius must be positive and finite");
    MGN_REQUIRE(ld_pos >= 3, who + ": ld_pos is smaller than 3");
    MGN_REQUIRE(ld_type >= 1, who + ": ld_type must be >= 1");
    MGN_REQUIRE(N <= (1ll << 30) && E_m <= INT32_MAX && E_m + N * (int64_t)W <= INT32_MAX,
                who + ": N must be <= 2^30 and E_m + N * max_neighbors must fit int32");
    MGN_REQUIRE(err_word != nullptr, who + ": NULL error word");
    MGN_REQUIRE(num_edges != nullptr && col_ptr != nullptr && row_ptr != nullptr, who + ": a null pointer argument");
    MGN_REQUIRE(ws_bytes >= mgn_world_topology_workspace_bytes(N, W), who + ": workspace too small");
    if (N == 0) return 0;
    MGN_REQUIRE(B >= 1, who + ": nodes without a graph (B == 0)");
    MGN_REQUIRE(pos && node_type && graph_ptr && mesh_ptr && (mesh_nbr || E_m == 0) && csc_src && csc_dst &&
                    csc_eid && row_perm && edge_index && ws,
                who + ": a null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    char* w = reinterpret_cast<char*>(ws);
    int32_t* wc = reinterpret_cast<int32_t*>(w); w += al((size_t)N * 4);
    int32_t* wl = reinterpret_cast<int32_t*>(w);
    const int n = (int)N, e_m = (int)E_m, e_cap = (int)(E_m + N * (int64_t)W);
    hipLaunchKernelGGL(world_search, dim3((unsigned)cdiv64(N, WORLD_THREADS)), dim3(WORLD_THREADS), 0, st, pos, ld_pos,
                       node_type, ld_type, graph_ptr, (int)B, n, mesh_ptr, mesh_nbr, e_m, radius * radius, (int)W, wl,
                       wc, err_word);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_scan, dim3(1), dim3(WORLD_SCAN_THREADS), 0, st, mesh_ptr, e_m, wc,
                       (const int32_t*)nullptr, n, e_cap, col_ptr, row_ptr, num_edges);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_merge, dim3((unsigned)cdiv64(N * WORLD_MERGE_LANES, 256)), dim3(256), 0, st, mesh_ptr,
                       mesh_nbr, e_m, wl, wc, (int)W, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, n, e_cap,
                       col_ptr, csc_src, csc_dst, csc_eid, row_perm, edge_index, err_word);
    MGN_LAUNCH_CHECK();
    return 0;
}

size_t mgn_random_topology_workspace_bytes(int64_t num_nodes, int32_t max_new, int64_t num_candidates) {
    const int64_t n = num_nodes < 1 ? 1 : num_nodes, w = max_new < 1 ? 1 : max_new;
    const int64_t c = num_candidates < 1 ? 1 : num_candidates;
    // wc, wl, the candidate id beside every entry of wl, the flags, the mapped endpoints, and the word world_merge
    // flags a bad mesh in
    return al((size_t)n * 4) + 2 * al((size_t)n * (size_t)w * 4) + al((size_t)c * 4) + al((size_t)c * 8) + al(4);
}

int mgn_random_topology_build(const int32_t* pairs, const int32_t* cand_ptr, int64_t C, const int32_t* graph_ptr,
                              int32_t B, int64_t N, const int32_t* mesh_ptr, const int32_t* mesh_nbr, int64_t E_m,
                              int32_t W, const int32_t* enabled, int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid,
                              int32_t* col_ptr, int32_t* row_ptr, int32_t* row_perm, int64_t* edge_index,
                              int32_t* num_edges, void* ws, size_t ws_bytes, mgn_stream_t stream) {
    const std::string who = "random_topology_build";
    MGN_REQUIRE(N >= 0 && B >= 0 && E_m >= 0 && C >= 0, who + ": N, B, E_m and num_candidates must be >= 0");
    MGN_REQUIRE(W >= 1 && W <= RANDOM_MAX_NEW, who + ": max_new must lie in [1, 64]");
    MGN_REQUIRE(N <= (1ll << 30) && E_m <= INT32_MAX && E_m + N * (int64_t)W <= INT32_MAX,
                who + ": N must be <= 2^30 and E_m + N * max_new must fit int32");
    MGN_REQUIRE(C <= (1ll << 30), who + ": num_candidates must be <= 2^30");
    MGN_REQUIRE(enabled != nullptr, who + ": NULL enabled word");
    MGN_REQUIRE(num_edges != nullptr && col_ptr != nullptr && row_ptr != nullptr, who + ": a null pointer argument");
    MGN_REQUIRE(ws_bytes >= mgn_random_topology_workspace_bytes(N, W, C), who + ": workspace too small");
    if (N == 0) return 0;
    MGN_REQUIRE(B >= 1, who + ": nodes without a graph (B == 0)");
    MGN_REQUIRE((pairs || C == 0) && cand_ptr && graph_ptr && mesh_ptr && (mesh_nbr || E_m == 0) && csc_src &&
                    csc_dst && csc_eid && row_perm && edge_index && ws,
                who + ": a null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    char* w = reinterpret_cast<char*>(ws);
    int32_t* wc = reinterpret_cast<int32_t*>(w); w += al((size_t)N * 4);
    int32_t* wl = reinterpret_cast<int32_t*>(w); w += al((size_t)N * (size_t)W * 4);
    int32_t* wid = reinterpret_cast<int32_t*>(w); w += al((size_t)N * (size_t)W * 4);
    int32_t* flag = reinterpret_cast<int32_t*>(w); w += al((size_t)(C < 1 ? 1 : C) * 4);
    int2* mapped = reinterpret_cast<int2*>(w); w += al((size_t)(C < 1 ? 1 : C) * 8);
    uint32_t* sink = reinterpret_cast<uint32_t*>(w);  // world_merge's error word: the caller validated the mesh
    const int n = (int)N, e_m = (int)E_m, e_cap = (int)(E_m + N * (int64_t)W);
    const unsigned blocks = (unsigned)cdiv64(N, WORLD_THREADS);
    if (C > 0) {
        MGN_TRY(hipMemsetAsync(flag, 0, (size_t)C * 4, st));
        hipLaunchKernelGGL(random_map, dim3((unsigned)cdiv64(C, WORLD_THREADS)), dim3(WORLD_THREADS), 0, st, pairs,
                           cand_ptr, (int)C, graph_ptr, (int)B, n, enabled, mapped);
        MGN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(random_search, dim3(blocks), dim3(WORLD_THREADS), 0, st, mapped, cand_ptr, (int)C, graph_ptr,
                       (int)B, n, mesh_ptr, mesh_nbr, e_m, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, (int)W,
                       enabled, wl, wid, wc, flag);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(random_filter, dim3(blocks), dim3(WORLD_THREADS), 0, st, n, (int)W, (int)C, wl, wid, wc, flag);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_scan, dim3(1), dim3(WORLD_SCAN_THREADS), 0, st, mesh_ptr, e_m, wc,
                       (const int32_t*)nullptr, n, e_cap, col_ptr, row_ptr, num_edges);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_merge, dim3((unsigned)cdiv64(N * WORLD_MERGE_LANES, 256)), dim3(256), 0, st, mesh_ptr,
                       mesh_nbr, e_m, wl, wc, (int)W, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, n, e_cap,
                       col_ptr, csc_src, csc_dst, csc_eid, row_perm, edge_index, sink);
    MGN_LAUNCH_CHECK();
    return 0;
}

size_t mgn_world_random_topology_workspace_bytes(int64_t num_nodes, int32_t max_neighbors, int32_t max_new,
                                                 int64_t num_candidates) {
    const int64_t n = num_nodes < 1 ? 1 : num_nodes, w = max_neighbors < 1 ? 1 : max_neighbors;
    const int64_t r = max_new < 1 ? 1 : max_new, c = num_candidates < 1 ? 1 : num_candidates;
    // the world counts and lists; the random counts, lists and the candidate id beside every entry; the flags; the
    // mapped endpoints
    return al((size_t)n * 4) + al((size_t)n * (size_t)w * 4) + al((size_t)n * 4) + 2 * al((size_t)n * (size_t)r * 4) +
           al((size_t)c * 4) + al((size_t)c * 8);
}

int mgn_world_random_topology_build(const float* pos, int64_t ld_pos, const float* node_type, int64_t ld_type,
                                    const int32_t* pairs, const int32_t* cand_ptr, int64_t C,
                                    const int32_t* graph_ptr, int32_t B, int64_t N, const int32_t* mesh_ptr,
                                    const int32_t* mesh_nbr, int64_t E_m, double radius, int32_t W, int32_t R,
                                    const int32_t* enabled, int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid,
                                    int32_t* col_ptr, int32_t* row_ptr, int32_t* row_perm, int64_t* edge_index,
                                    int32_t* num_edges, uint32_t* err_word, void* ws, size_t ws_bytes,
                                    mgn_stream_t stream) {
    const std::string who = "world_random_topology_build";
    MGN_REQUIRE(N >= 0 && B >= 0 && E_m >= 0 && C >= 0, who + ": N, B, E_m and num_candidates must be >= 0");
    MGN_REQUIRE(W >= 1, who + ": max_neighbors must be >= 1");
    MGN_REQUIRE(R >= 1 && R <= RANDOM_MAX_NEW, who + ": max_new must lie in [1, 64]");
    MGN_REQUIRE(radius > 0.0 && std::isfinite(radius), who + ": radius must be positive and finite");
    MGN_REQUIRE(ld_pos >= 3, who + ": ld_pos is smaller than 3");
    MGN_REQUIRE(ld_type >= 1, who + ": ld_type must be >= 1");
    MGN_REQUIRE(N <= (1ll << 30) && E_m <= INT32_MAX && E_m + N * ((int64_t)W + (int64_t)R) <= INT32_MAX,
                who + ": N must be <= 2^30 and E_m + N * (max_neighbors + max_new) must fit int32");
    MGN_REQUIRE(C <= (1ll << 30), who + ": num_candidates must be <= 2^30");
    MGN_REQUIRE(err_word != nullptr, who + ": NULL error word");
    MGN_REQUIRE(enabled != nullptr, who + ": NULL enabled word");
    MGN_REQUIRE(num_edges != nullptr && col_ptr != nullptr && row_ptr != nullptr, who + ": a null pointer argument");
    MGN_REQUIRE(ws_bytes >= mgn_world_random_topology_workspace_bytes(N, W, R, C), who + ": workspace too small");
    if (N == 0) return 0;
    MGN_REQUIRE(B >= 1, who + ": nodes without a graph (B == 0)");
    MGN_REQUIRE(pos && node_type && (pairs || C == 0) && cand_ptr && graph_ptr && mesh_ptr && (mesh_nbr || E_m == 0) &&
                    csc_src && csc_dst && csc_eid && row_perm && edge_index && ws,
                who + ": a null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    char* w = reinterpret_cast<char*>(ws);
    int32_t* wcW = reinterpret_cast<int32_t*>(w); w += al((size_t)N * 4);
    int32_t* wlW = reinterpret_cast<int32_t*>(w); w += al((size_t)N * (size_t)W * 4);
    int32_t* wcR = reinterpret_cast<int32_t*>(w); w += al((size_t)N * 4);
    int32_t* wlR = reinterpret_cast<int32_t*>(w); w += al((size_t)N * (size_t)R * 4);
    int32_t* wid = reinterpret_cast<int32_t*>(w); w += al((size_t)N * (size_t)R * 4);
    int32_t* flag = reinterpret_cast<int32_t*>(w); w += al((size_t)(C < 1 ? 1 : C) * 4);
    int2* mapped = reinterpret_cast<int2*>(w);
    const int n = (int)N, e_m = (int)E_m, e_cap = (int)(E_m + N * ((int64_t)W + (int64_t)R));
    const unsigned blocks = (unsigned)cdiv64(N, WORLD_THREADS);
    hipLaunchKernelGGL(world_search, dim3(blocks), dim3(WORLD_THREADS), 0, st, pos, ld_pos, node_type, ld_type,
                       graph_ptr, (int)B, n, mesh_ptr, mesh_nbr, e_m, radius * radius, (int)W, wlW, wcW, err_word);
    MGN_LAUNCH_CHECK();
    if (C > 0) {
        MGN_TRY(hipMemsetAsync(flag, 0, (size_t)C * 4, st));
        hipLaunchKernelGGL(random_map, dim3((unsigned)cdiv64(C, WORLD_THREADS)), dim3(WORLD_THREADS), 0, st, pairs,
                           cand_ptr, (int)C, graph_ptr, (int)B, n, enabled, mapped);
        MGN_LAUNCH_CHECK();
    }
    // the world lists of this build are the search's second exclusion list: a candidate that is a world edge is
    // skipped like a mesh edge, at both endpoints alike (the world lists are symmetric)
    hipLaunchKernelGGL(random_search, dim3(blocks), dim3(WORLD_THREADS), 0, st, mapped, cand_ptr, (int)C, graph_ptr,
                       (int)B, n, mesh_ptr, mesh_nbr, e_m, (const int32_t*)wlW, (const int32_t*)wcW, (int)W, (int)R,
                       enabled, wlR, wid, wcR, flag);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(random_filter, dim3(blocks), dim3(WORLD_THREADS), 0, st, n, (int)R, (int)C, wlR, wid, wcR, flag);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_scan, dim3(1), dim3(WORLD_SCAN_THREADS), 0, st, mesh_ptr, e_m, wcW, (const int32_t*)wcR, n,
                       e_cap, col_ptr, row_ptr, num_edges);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(world_merge, dim3((unsigned)cdiv64(N * WORLD_MERGE_LANES, 256)), dim3(256), 0, st, mesh_ptr,
                       mesh_nbr, e_m, wlW, wcW, (int)W, (const int32_t*)wlR, (const int32_t*)wcR, (int)R, n, e_cap,
                       col_ptr, csc_src, csc_dst, csc_eid, row_perm, edge_index, err_word);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
