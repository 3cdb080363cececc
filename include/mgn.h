/*
 * libmgn — MI355X-native (gfx950) MeshGraphNet message-passing library. C ABI.
 *
 * This is the drop-in boundary for the hot path of cviviers/graph-physics: everything the
 * reference executes from EncodeProcessDecode.forward downwards (reference
 * graphphysics/models/processors.py:111-137) and its autograd backward:
 *
 *   mgn_topology_build   replaces the index bookkeeping torch-geometric 2.6.1 does inside
 *                        MessagePassing.propagate for edge_index[2,E] (reference
 *                        graphphysics/models/layers.py:688-696: row,col = edge_index; x[col],
 *                        x[row]; scatter-add over edge_index[1] with dim_size = x.size(0)).
 *   mgn_mlp_pack         nn.Linear weights of build_mlp (layers.py:77-113) → MFMA fragment order.
 *   mgn_mlp_forward      build_mlp forward (Linear/ReLU chain + RMSNorm layers.py:49-74);
 *                        used for nodes_encoder / edges_encoder / decode_module
 *                        (processors.py:72-90,127-128,136).
 *   mgn_mlp_backward     its backward (data + weight gradients).
 *   mgn_block_forward    GraphNetBlock.forward (layers.py:667-746): edge MLP on
 *                        [e ‖ x[col] ‖ x[row]], sum-aggregation into targets, node MLP on
 *                        [x ‖ aggr], both residuals.
 *   mgn_block_backward   its backward (index_put_/gather/addmm backward of the reference).
 *   mgn_adamw            torch.optim.AdamW step (lightning_module.py:275-282) over a flat
 *                        parameter buffer.
 *
 * Conventions
 *  - All device memory is owned by the caller (PyTorch caching allocator); raw pointers + sizes.
 *    The library holds no device allocations and no global mutable state besides the
 *    thread-local error string (per-call options such as CU caps are arguments: mgn_call_opts;
 *    ABI v17). Every call is asynchronous on the given stream except mgn_topology_build (which reads back one validation word; mgn_topology_build_async does not).
 *  - Input validation that needs the data (edge_index range, node-type range) never reads back to
 *    the host on the asynchronous entry points: kernels OR an MGN_ERR_* bit into a caller-owned
 *    device word (uint32, zeroed by the caller), keep every access in bounds (clamped index /
 *    all-zero one-hot row), and the caller checks the word lazily and raises the reference's
 *    exception (IndexError / RuntimeError).
 *  - Return value: 0 on success, otherwise a nonzero status; mgn_last_error() describes it.
 *  - Edge order inside the library is target-sorted ("CSC" order: stable sort of the caller's
 *    edges by edge_index[1]); csc_eid maps it back to the caller's order.
 *  - dtype: MGN_F32 = fp32 storage + exact fp32 MFMA (parity path);
 *           MGN_BF16 = bf16 storage of activations/packed weights, fp32 accumulation and fp32
 *           epilogues (RMSNorm, residual), fp32 master weights and gradients.
 *  - Deterministic: no floating-point atomics; every reduction has a fixed order.
 */
#ifndef MGN_H
#define MGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mgn_stream_t; /* == hipStream_t */

#define MGN_ABI_VERSION 17
#define MGN_F32 0
#define MGN_BF16 1
#define MGN_MAX_LAYERS 8

/* ---------------------------------------------------------------- status */
int mgn_abi_version(void);
const char* mgn_last_error(void);

/* bits of the device error word */
#define MGN_ERR_EDGE_INDEX 1u /* edge_index outside [0, N): reference IndexError (ATen index)         */
#define MGN_ERR_TYPE_NEG 2u   /* node type < 0 or NaN: F.one_hot "Class values must be non-negative." */
#define MGN_ERR_TYPE_BIG 4u   /* node type >= n_types: "Class values must be smaller than num_classes." */
#define MGN_ERR_HANDOFF 8u    /* ABI v17: a bounded hand-off wait inside a pipelined kernel (the recomputed
                                 weight gradients, mgn_block_backward_deferred3) timed out; the kernel
                                 wrote NaN into its partial sums instead of a partial result           */
#define MGN_ERR_WORLD_CAPACITY 16u /* a node has more world neighbours than max_neighbors
                                      (mgn_world_topology_build kept the smallest; the topology is unspecified)  */
#define MGN_ERR_ANY 0xFFFFu   /* any validation error (bits 0-15)                                      */
/* State updates are predicated on the word, so an error raised lazily (one call late) leaves the
 * training state as the reference's immediate exception would (ABI v11): mgn_adamw_dev skips its
 * update while any MGN_ERR_ANY bit is set, counts the skip in bits 16-23 (MGN_ERR_SKIP_ONE each,
 * saturating at 255) and sets MGN_ERR_STALE; mgn_simulator_preamble skips the node / edge
 * normalizers' accumulation while any bit is set (the reference's F.one_hot raises after the output
 * normalizer has accumulated, simulator.py:_build_input_graph) and the output normalizer's once
 * MGN_ERR_STALE is set (the error belongs to an earlier step the reference would have stopped at). */
#define MGN_ERR_SKIP_ONE (1u << 16)
#define MGN_ERR_SKIP_MASK (0xFFu << 16)
#define MGN_ERR_STALE (1u << 31)

/* ---------------------------------------------------------------- topology */
typedef struct mgn_topology {
    int64_t num_nodes;
    int64_t num_edges;
    const int32_t* csc_src;  /* [E] source node (edge_index[0]) of the k-th target-sorted edge  */
    const int32_t* csc_dst;  /* [E] target node (edge_index[1]), non-decreasing                  */
    const int32_t* csc_eid;  /* [E] caller edge id of the k-th target-sorted edge                */
    const int32_t* col_ptr;  /* [N+1] in-edge segment of node i = [col_ptr[i], col_ptr[i+1])     */
    const int32_t* row_ptr;  /* [N+1] out-edge segment of node j within row_perm                 */
    const int32_t* row_perm; /* [E] target-sorted positions, stably sorted by source node         */
} mgn_topology;

size_t mgn_topology_workspace_bytes(int64_t num_edges, int64_t num_nodes);
/* edge_index: device int64 [2,E] row-major (reference layout). Fails with a nonzero status and
 * "edge_index out of range" if any index is outside [0, N) (the reference raises IndexError). */
int mgn_topology_build(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes,
                       int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr,
                       int32_t* row_ptr, int32_t* row_perm, void* ws, size_t ws_bytes,
                       mgn_stream_t stream);
/* The same without any host read-back (a new batch's topology never synchronises): an index
 * outside [0, N) sets MGN_ERR_EDGE_INDEX in *err_word and is clamped into range. Host-side
 * failures (sizes, N = 0 with E > 0) still return a nonzero status. */
int mgn_topology_build_async(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes,
                             int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr,
                             int32_t* row_ptr, int32_t* row_perm, void* ws, size_t ws_bytes,
                             uint32_t* err_word, mgn_stream_t stream);

/* ---------------------------------------------------------------- MLP (build_mlp) */
typedef struct mgn_mlp {
    int32_t n_layers; /* number of nn.Linear (reference nb_of_layers, >= 2)                    */
    int32_t in_dim;   /* input features of Linear 0                                          */
    int32_t hidden;   /* hidden width the kernels run (16, 32, 64, 128 or 256)                */
    int32_t out_dim;  /* output features of the last Linear (== hidden, or 1..16)            */
    int32_t has_norm; /* RMSNorm(out_dim) after the last Linear                              */
    int32_t dtype;    /* MGN_F32 | MGN_BF16                                                  */
    int32_t norm_dim; /* ABI v11: the RMSNorm's d in rms = |x|·d^(-1/2) (0: out_dim). A model of hidden
                         size h the kernels do not instantiate runs on the next supported width with
                         exactly-zero padded channels; its RMSNorm still divides by the true h      */
    int32_t reserved;
    const void* wpack;  /* forward fragments, mgn_mlp_pack_elems() elements of dtype         */
    const void* wtpack; /* transposed fragments (backward), same element count                */
    const float* bias[MGN_MAX_LAYERS]; /* fp32 master biases                                  */
    const float* scale;                /* fp32 RMSNorm scale [out_dim] or NULL                */
} mgn_mlp;

/* Forward state kept for the backward. `act` holds the INPUT of every Linear (layer 0: the
 * MLP input — not for GraphNetBlock MLPs; layer l>0: the ReLU output of layer l-1) in the row-octet
 * layout (element (m,c) at ((m/8)*cols + c)*8 + m%8, rows padded to 64) that makes every weight-
 * gradient MFMA fragment one 16-byte load; `mask` holds the hidden layers' ReLU masks (64-bit
 * wave-ballot words, or the chained kernels' per-lane words — opaque to callers: only the backward of
 * the same MLP reads it). Sizes: mgn_mlp_saved_elems(). */
typedef struct mgn_mlp_saved {
    void* act;    /* act_elems elements of dtype                                             */
    void* mask;   /* mask_words x 8 bytes                                                    */
    void* z;      /* [M, hidden] last Linear output before RMSNorm (dtype); NULL w/o norm    */
    float* rden;  /* [M] RMSNorm denominator rms+eps; NULL w/o norm                          */
} mgn_mlp_saved;
/* block_mlp != 0 for the edge/node MLPs of a GraphNetBlock: their layer-0 input is not saved (the
 * weight-gradient kernel re-gathers [e ‖ x_i ‖ x_j] / [x ‖ aggr]). */
int mgn_mlp_saved_elems(const mgn_mlp* m, int64_t rows, int32_t block_mlp, int64_t* act_elems,
                        int64_t* mask_words);

/* Pack job: one nn.Linear weight [n, k] fp32 row-major → fragment buffers (dtype). */
typedef struct mgn_pack_job {
    const float* w;
    void* dst;   /* forward fragments  */
    void* dstT;  /* transposed fragments */
    int32_t n, k, dtype;
    /* ABI v11, zero-padded packs (0: none): the source w is [n_src][k_src] row-major, packed as the
     * [n][k] matrix whose rows >= n_src are 0 and whose k axis is blocks of kb_pad columns holding
     * kb_src source columns each (rest 0): e.g. [e ‖ x_i ‖ x_j] of hidden h on width H: kb_src = h,
     * kb_pad = H */
    int32_t n_src, k_src, kb_src, kb_pad, reserved;
} mgn_pack_job;

/* ABI v15: an fp32 Linear with n == 128 and k a multiple of 128 carries one 128x128 "chain image" per
 * 128-column input block (v14: of the first block only) — the register-chained fp32 edge and node MLP
 * kernels' LDS-DMA source; the count changes, the layout stays opaque to callers. */
int64_t mgn_linear_pack_elems(int32_t n, int32_t k, int32_t dtype);
int64_t mgn_mlp_pack_elems(const mgn_mlp* m); /* Σ over layers of mgn_linear_pack_elems */
/* jobs: DEVICE array of njobs mgn_pack_job; max_elems = max over jobs of n*k. One launch. */
int mgn_pack_weights(const mgn_pack_job* jobs, int32_t njobs, int64_t max_elems,
                     mgn_stream_t stream);

/* Input description of a dense MLP: rows r of `in` (ld elements apart), optionally gathered
 * through in_rows[r]; in_dtype MGN_F32 or the MLP dtype. */
int mgn_mlp_forward(const mgn_mlp* m, const void* in, int32_t in_dtype, int64_t in_ld,
                    const int32_t* in_rows, int64_t rows, void* out, int32_t out_dtype,
                    mgn_mlp_saved* saved, mgn_stream_t stream);
size_t mgn_mlp_backward_workspace_bytes(const mgn_mlp* m, int64_t rows);
/* grads: flat fp32 [W0, b0, W1, b1, ..., W_{L-1}, b_{L-1}, scale] (nn.Module parameter order),
 * overwritten. din (optional, NULL to skip): gradient w.r.t. the (gathered) input rows. */
int mgn_mlp_backward(const mgn_mlp* m, const void* in, int32_t in_dtype, int64_t in_ld,
                     const int32_t* in_rows, int64_t rows, const mgn_mlp_saved* saved,
                     const void* dout, int32_t dout_dtype, void* din, int32_t din_dtype,
                     float* grads, void* ws, size_t ws_bytes, mgn_stream_t stream);

/* ---------------------------------------------------------------- GraphNetBlock */
typedef struct mgn_block_saved {
    mgn_mlp_saved edge; /* rows = E (target-sorted order) */
    mgn_mlp_saved node; /* rows = N */
    void* aggr;         /* [N, hidden] aggregated messages (dtype) */
    /* ABI v16: NULL, or (training forward of a chained bf16 h=128 block) the block's forward workspace
     * `ws`, which the caller then keeps intact until the block's backward: the forward writes no R8
     * inputs of the edge MLP's hidden layers (edge.act is not written) and the backward recomputes them
     * from e and the node projections in ws for those layers' weight gradients (one pass, no re-read
     * of saved activations). */
    void* proj;
} mgn_block_saved;

/* x:[N,h], e:[E,h] (target-sorted edge order), dtype of the MLPs. x_out/e_out may not alias.
 * The edge MLP's first Linear on [e ‖ x_i ‖ x_j] is evaluated as e·W0aᵀ + P_i[dst] + P_j[src]
 * with the node projections P = [x·W0bᵀ ‖ x·W0cᵀ] (fp32, N rows) computed once per block into
 * ws (scratch, free again when the call's work has run).
 * Inference (no autograd, e.g. the reference's validation/rollout _make_prediction under
 * torch.no_grad, lightning_module.py:168-202): saved->edge.act = saved->node.act = NULL selects
 * kernels that write only the edge MLP's z/rden (scratch the node MLP's aggregation reads) and no
 * backward saves; aggr and the node saves may be NULL. Available where
 * mgn_block_forward_inference_supported() is 1 (bf16, h = 128, 4 layers + RMSNorm). */
int mgn_block_forward_inference_supported(const mgn_mlp* edge, const mgn_mlp* node);
size_t mgn_block_forward_workspace_bytes(const mgn_topology* t, const mgn_mlp* edge,
                                         const mgn_mlp* node);
int mgn_block_forward(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                      const void* x, const void* e, void* x_out, void* e_out,
                      mgn_block_saved* saved, void* ws, size_t ws_bytes, mgn_stream_t stream);
/* A processor stack of blocks (processors.py:129-131, `for block in self.processor_list`) chained:
 * the same forward, plus two hand-offs between consecutive blocks. proj_ready = 1: ws already holds
 * this block's node projections (written by the previous call's next_ws). next_edge / next_ws
 * (optional): the NEXT block's edge MLP and its workspace — the node-MLP kernel then also computes
 * that block's projections from this block's x_out (no projection launch of its own) and sets
 * *next_proj_ready = 1; it stays 0 where the chained bf16 h=128 kernels do not apply (the caller
 * then passes proj_ready = 0 to the next call). Results are those of mgn_block_forward. */
int mgn_block_forward_chain(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                            const void* x, const void* e, void* x_out, void* e_out,
                            mgn_block_saved* saved, void* ws, size_t ws_bytes, int proj_ready,
                            const mgn_mlp* next_edge, void* next_ws, size_t next_ws_bytes,
                            int* next_proj_ready, mgn_stream_t stream);
/* ABI v17: mgn_block_forward_chain with a scratch buffer for the edge-side aggregation. For graphs of
 * high in-degree (default E >= 16 N; env MGN_EDGE_AGG = 0 / 1 forces it off / on for chained blocks, "fwd"
 * / "bwd" one direction only) the training forward's edge-MLP kernel also sums each 16-edge tile's
 * messages per run of equal target and the node-MLP kernel adds those partial rows — a few per node —
 * instead of re-reading every in-edge's output row (reference layers.py:694-696, the sum aggregation; the
 * fp32 sums re-associated, in a fixed order). The backward does the same for the target-direction sums of
 * the edge MLP's layer-0 gradient (the index backward of x[col]) inside mgn_block_backward*'s workspace
 * (mgn_block_backward_workspace_bytes includes it). mgn_block_forward_scratch_bytes: the scratch it needs, 0 where it does not apply (then the call
 * is mgn_block_forward_chain). The scratch is free again when the call's work has run (one buffer can
 * serve every block of a stack). */
size_t mgn_block_forward_scratch_bytes(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node);
int mgn_block_forward_chain2(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                             const void* x, const void* e, void* x_out, void* e_out,
                             mgn_block_saved* saved, void* ws, size_t ws_bytes, int proj_ready,
                             const mgn_mlp* next_edge, void* next_ws, size_t next_ws_bytes,
                             int* next_proj_ready, void* scratch, size_t scratch_bytes,
                             mgn_stream_t stream);
size_t mgn_block_backward_workspace_bytes(const mgn_topology* t, const mgn_mlp* edge,
                                          const mgn_mlp* node);
/* dx/de: gradients w.r.t. the block inputs (overwritten). edge_grads/node_grads: flat fp32 as
 * in mgn_mlp_backward (overwritten). de_out may be NULL (a zero edge-output gradient: the last
 * processor block, whose e' EncodeProcessDecode discards) where
 * mgn_block_forward_inference_supported() is 1. */
int mgn_block_backward(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                       const void* x, const void* e, const mgn_block_saved* saved,
                       const void* dx_out, const void* de_out, void* dx, void* de,
                       float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                       mgn_stream_t stream);
/* Deferred weight-gradient reduction (a processor stack's backward, processors.py:129-131 in
 * reverse): mgn_block_backward_deferred is mgn_block_backward except that, for the chained bf16
 * h=128 MLPs, the fixed-order reduction of the weight-gradient slabs is NOT launched: the slabs and
 * RMSNorm-scale partials go to `keep` (mgn_block_backward_keep_bytes, one buffer per block, alive
 * until the reduction) and reduce2[0..1] describe the reduction; mgn_wgrad_reduce_many then runs
 * every block's in ONE launch — the same sums in the same order, one launch instead of one per
 * block. Deferred for the chained bf16 h=128 MLPs, the fp32 h=128 ones (fp32 ring) and (ABI v12) the
 * generic hidden 16/32/64 MLPs (one multi-job weight-gradient launch per block); other shapes (e.g.
 * hidden 256: generic kernels, 128 x 128 weight-gradient tiles) are reduced at once (reduce2 zeroed). */
typedef struct mgn_wgrad_reduce {
    const float* part;
    const float* dsp;
    float* grads;
    int64_t G;
    int32_t nchunks, ntiles, NS, blocks;
    int32_t w0_n, w0_k, xcol0, nchunks_x; /* W0 columns >= xcol0 sum only nchunks_x slabs */
    int64_t hoff;                         /* ABI v16: outputs g >= hoff > 0 sum only nchunks_h slabs */
    int32_t nchunks_h, pad;
} mgn_wgrad_reduce;
size_t mgn_block_backward_keep_bytes(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node);
int mgn_block_backward_deferred(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                                const void* x, const void* e, const mgn_block_saved* saved,
                                const void* dx_out, const void* de_out, void* dx, void* de,
                                float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                                void* keep, size_t keep_bytes, mgn_wgrad_reduce* reduce2,
                                mgn_stream_t stream);
/* mgn_block_backward_deferred with row layouts of the gradients handed between consecutive chained
 * processor blocks (flags; 0 = mgn_block_backward_deferred): the pair layout stores feature
 * 16t + 4g + r of a row at 32(t>>1) + 8g + 4(t&1) + r (libmgn's gather layout: one 16-byte load per
 * lane and tile pair). MGN_BWD_DE_OUT_PAIR / MGN_BWD_DX_OUT_PAIR: de_out / dx_out are in it (the
 * previous call's de / dx written with MGN_BWD_DE_PAIR / MGN_BWD_DX_PAIR). The caller keeps
 * row-major for gradients handed in from outside and for the de / dx it consumes itself (the first
 * block's, for the encoders). Chained bf16 h=128 edge + node MLPs only (else an error status,
 * mgn_last_error). keep = NULL: nothing deferred — the block's weight gradients are reduced at once
 * (mgn_block_backward with the layout flags; reduce2 zeroed). */
#define MGN_BWD_DE_OUT_PAIR 1
#define MGN_BWD_DE_PAIR 2
#define MGN_BWD_DX_OUT_PAIR 4
#define MGN_BWD_DX_PAIR 8
/* ABI v13: the same call split in two halves over the same arguments (keep != NULL): DATA_ONLY runs
 * the data gradients (dx, de, and what the weight gradients read: dZ saves in `ws`, partials in
 * `keep`); WGRAD_ONLY then runs the block's single weight-gradient launch and fills reduce2. The
 * WGRAD_ONLY call may be issued on another stream (ordered after DATA_ONLY by the caller) and run
 * beside the next block's DATA_ONLY call on ANOTHER workspace; mgn_block_backward_deferred3's
 * mgn_call_opts gives each its CUs. */
#define MGN_BWD_DATA_ONLY 16
#define MGN_BWD_WGRAD_ONLY 32
int mgn_block_backward_deferred2(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                                 const void* x, const void* e, const mgn_block_saved* saved,
                                 const void* dx_out, const void* de_out, void* dx, void* de,
                                 float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                                 void* keep, size_t keep_bytes, mgn_wgrad_reduce* reduce2,
                                 int32_t flags, mgn_stream_t stream);
int mgn_wgrad_reduce_many(const mgn_wgrad_reduce* reds, int32_t n, mgn_stream_t stream);
/* ABI v14: mgn_mlp_backward_deferred in two halves over the same arguments (flags 0 = the whole call):
 * MGN_BWD_DATA_ONLY runs the data gradients (din, and the dZ saves / partials the weight gradients read
 * in `ws` / `keep`) and leaves in reduce1 only the partial-row count; MGN_BWD_WGRAD_ONLY, given that
 * reduce1, runs the weight gradients (on another stream if the caller orders it after DATA_ONLY) and
 * fills reduce1 for mgn_wgrad_reduce_many. EncodeProcessDecode's decoder (reference processors.py:131)
 * uses it to run its weight gradients beside the first processor block's data gradients. */
int mgn_mlp_backward_deferred2(const mgn_mlp* m, const void* in, int32_t in_dtype, int64_t in_ld,
                               const int32_t* in_rows, int64_t rows, const mgn_mlp_saved* saved,
                               const void* dout, int32_t dout_dtype, void* din, int32_t din_dtype,
                               float* grads, void* ws, size_t ws_bytes, void* keep, size_t keep_bytes,
                               mgn_wgrad_reduce* reduce1, int32_t flags, mgn_stream_t stream);
/* ABI v17: per-call options of the backward entry points (NULL = none; replaces v13's process-global
 * mgn_set_grid_cus, which two models or streams in one process shared):
 *   data_cus / wgrad_cus  caps on the CUs the persistent grids of this call's launches are sized for
 *                         (0 = the whole device): data_cus for every launch except the weight-gradient
 *                         launches, wgrad_cus for those. The results do not depend on the caps except
 *                         for the weight-gradient slab partition (summation order of the fp32 reductions).
 *                         A captured hipGraph keeps the grids it recorded.
 *   err_word              device word (as mgn_topology_build_async's) the call's pipelined kernels OR
 *                         MGN_ERR_HANDOFF into when a bounded hand-off wait times out (NULL: the NaN
 *                         partials alone report it). mgn_adamw_dev skips its update while it is set. */
typedef struct mgn_call_opts {
    int32_t data_cus;
    int32_t wgrad_cus;
    uint32_t* err_word;
} mgn_call_opts;
/* mgn_block_backward_deferred2 / mgn_mlp_backward_deferred2 with per-call options (same flags; for the
 * MLP, flags 0 = the whole deferred call, mgn_mlp_backward_deferred). */
int mgn_block_backward_deferred3(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                                 const void* x, const void* e, const mgn_block_saved* saved,
                                 const void* dx_out, const void* de_out, void* dx, void* de,
                                 float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                                 void* keep, size_t keep_bytes, mgn_wgrad_reduce* reduce2,
                                 int32_t flags, const mgn_call_opts* opts, mgn_stream_t stream);
int mgn_mlp_backward_deferred3(const mgn_mlp* m, const void* in, int32_t in_dtype, int64_t in_ld,
                               const int32_t* in_rows, int64_t rows, const mgn_mlp_saved* saved,
                               const void* dout, int32_t dout_dtype, void* din, int32_t din_dtype,
                               float* grads, void* ws, size_t ws_bytes, void* keep, size_t keep_bytes,
                               mgn_wgrad_reduce* reduce1, int32_t flags, const mgn_call_opts* opts,
                               mgn_stream_t stream);
/* The node side of a block's data gradients on its own (the last launch of mgn_block_backward_data):
 *   dP_i[v] = Σ dz0[k]            over k in [col_ptr[v], col_ptr[v+1])      fp32 sums in edge order,
 *   dP_j[v] = Σ dz0[row_perm[k]]  over k in [row_ptr[v], row_ptr[v+1])      rounded to the MLP's dtype
 *   dx      = dx_part + dP_i·W0b + dP_j·W0c                                 W0 = [W0a | W0b | W0c]: edge layer 0
 * dz0 [E, h] (target-sorted edges), dx_part and dx [N, h], dP8 [2][rows padded to 64][h] in the row-octet
 * layout (dP_i, then dP_j; padded rows zero), all of edge->dtype; only edge->wtpack (layer 0) is read.
 * dx_pair != 0 (bf16 h = 128): dx in the pair layout (MGN_BWD_DX_PAIR). impl: 0 = the kernel
 * mgn_block_backward_data would launch, 1 = the generic kernel, 2 = the chained kernel (bf16, h = 128; a
 * nonzero status elsewhere); both write the same bits. opts: as mgn_block_backward_deferred3 (data_cus).
 * The added symbol does not change MGN_ABI_VERSION; MGN_HAS_NODE_GRAD marks headers that declare it. */
#define MGN_HAS_NODE_GRAD 1
int mgn_node_grad(const mgn_topology* t, const mgn_mlp* edge, const void* dz0, const void* dx_part,
                  void* dP8, void* dx, int32_t dx_pair, int32_t impl, const mgn_call_opts* opts,
                  mgn_stream_t stream);
/* Diagnostics builds (MGN_STAMPS) only, else an error status: per-wave [start, end] s_memrealtime ticks
 * (100 MHz) of the last launch of a chained kernel kind (0 edge fwd, 1 edge bwd, 2 node fwd, 3 node
 * bwd), n <= 4096 waves in workgroup-major order. */
int mgn_debug_wave_times(int32_t kind, uint64_t* out, int32_t n);
/* ABI v12: mgn_mlp_backward (the encoders / decoder of processors.py:71-109, 129-137) with the
 * reduction deferred like mgn_block_backward_deferred: the RMSNorm-scale partials and weight-gradient
 * slabs go to `keep` (mgn_mlp_backward_keep_bytes, alive until the reduction) and *reduce1 describes
 * the reduction for mgn_wgrad_reduce_many — so a whole EncodeProcessDecode backward ends in ONE
 * reduction launch. */
size_t mgn_mlp_backward_keep_bytes(const mgn_mlp* m, int64_t rows);
int mgn_mlp_backward_deferred(const mgn_mlp* m, const void* in, int32_t in_dtype, int64_t in_ld,
                              const int32_t* in_rows, int64_t rows, const mgn_mlp_saved* saved,
                              const void* dout, int32_t dout_dtype, void* din, int32_t din_dtype,
                              float* grads, void* ws, size_t ws_bytes, void* keep, size_t keep_bytes,
                              mgn_wgrad_reduce* reduce1, mgn_stream_t stream);
/* The same backward as two calls over one workspace (same arguments): _data writes dx, de (and, for
 * MLPs outside the chained bf16 h=128 kernels, the node-MLP weight gradients); _wgrad then writes the
 * weight gradients from what _data left in `ws` plus the forward saves, and may run on another
 * stream (ordered after _data by the caller) concurrently with the next block's _data on ANOTHER
 * workspace — the weight-gradient launch overlaps the latency-bound kernels of the next block. */
int mgn_block_backward_data(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                            const void* x, const void* e, const mgn_block_saved* saved,
                            const void* dx_out, const void* de_out, void* dx, void* de,
                            float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                            mgn_stream_t stream);
int mgn_block_backward_wgrad(const mgn_topology* t, const mgn_mlp* edge, const mgn_mlp* node,
                             const void* x, const void* e, const mgn_block_saved* saved,
                             const void* dx_out, const void* de_out, void* dx, void* de,
                             float* edge_grads, float* node_grads, void* ws, size_t ws_bytes,
                             mgn_stream_t stream);

/* ---------------------------------------------------------------- sparse graph attention */
/* The attention core of the reference's Transformer block, DGL branch (layers.py:395-457: bsddmm,
 * SparseMatrix.softmax, bspmm over the mesh adjacency; Attention.forward 503-545 reshapes to
 * (N, head_dim, num_heads)), N nodes, hidden features, H heads, row = edge_index[0], col = edge_index[1]:
 *   s[e,b] = (1/sqrt(H)) Σ_d q[row_e, dH+b] k[col_e, dH+b]    feature c is component c / H of head c % H;
 *                                                            the scale is 1/sqrt(H), as the reference's
 *   p[e,b] = exp(s[e,b]) / Σ_{e': row_e' = row_e} exp(s[e',b])  softmax per source node and head; duplicate
 *                                                            edges are separate entries
 *   y[i, dH+b] = Σ_{e: row_e = i} p[e,b] v[col_e, dH+b]        0 for a node without out-edges
 * q, k, v: [N, hidden] with row stride ld elements (they may be column slices of one [N, 3 hidden]
 * projection output); y, dy, dq, dk, dv: dense [N, hidden]; all of storage type dtype (MGN_F32 |
 * MGN_BF16). Scores, softmax and every sum are fp32. lse [N, H] fp32 = log Σ exp(s) per (node, head), 0
 * without out-edges; y and lse are all the backward needs from the forward. Supported: heads 1, 2, 4, 8,
 * hidden % heads == 0, hidden <= 256; anything else is a nonzero status before any launch. The added
 * symbols do not change MGN_ABI_VERSION (no existing signature changed); MGN_HAS_GRAPH_ATTENTION marks
 * headers that declare them.
 * Backward: two passes without atomics — grouped by source node (dq; p and dP = Σ_d dy v of every edge
 * and δ = Σ_e p dP of every node into ws), then by target node in target-sorted order (dk, dv, with
 * dS = p (dP − δ)). δ is summed from the edges, not as Σ_d dy y from the stored (in bf16 rounded) y, so
 * the y argument is not read. ws: mgn_graph_attention_workspace_bytes (2 H floats per edge + H floats
 * per node), scratch. */
#define MGN_HAS_GRAPH_ATTENTION 1
size_t mgn_graph_attention_workspace_bytes(const mgn_topology* t, int32_t hidden, int32_t heads, int32_t dtype);
int mgn_graph_attention_forward(const mgn_topology* t, const void* q, const void* k, const void* v,
                                int64_t ld, int32_t hidden, int32_t heads, int32_t dtype,
                                void* y, float* lse /* [N, heads] */, mgn_stream_t stream);
int mgn_graph_attention_backward(const mgn_topology* t, const void* q, const void* k, const void* v,
                                 const void* y, const float* lse, const void* dy, int64_t ld,
                                 int32_t hidden, int32_t heads, int32_t dtype,
                                 void* dq, void* dk, void* dv, void* ws, size_t ws_bytes, mgn_stream_t stream);

/* ---------------------------------------------------------------- primitives */
/* out[k,:] = in[idx[k],:] (gather), or out[idx[k],:] = in[k,:] when scatter != 0. */
int mgn_permute_rows(const void* in, void* out, const int32_t* idx, int64_t rows, int32_t cols,
                     int32_t in_dtype, int32_t out_dtype, int32_t scatter, mgn_stream_t stream);
/* Segment sum over target-sorted edges: out[i,:] = Σ_{k in [col_ptr[i], col_ptr[i+1])} src[k,:].
 * The stand-alone form of the aggregation fused into mgn_block_forward. */
int mgn_segment_sum(const void* src, const int32_t* seg_ptr, int64_t segments, int32_t cols,
                    int32_t dtype, void* out, mgn_stream_t stream);

/* Column sums and sums of squares of a row-major fp32 [rows, cols] matrix (row stride ld), the
 * batch statistics of Normalizer._accumulate (reference layers.py:333-352): sums[0:cols] = Σ_r x,
 * sums[cols:2cols] = Σ_r x². cols <= 32. Fixed reduction order (deterministic). */
size_t mgn_column_stats_workspace_bytes(int64_t rows, int32_t cols);
int mgn_column_stats(const float* x, int64_t rows, int32_t cols, int64_t ld, float* sums, void* ws,
                     size_t ws_bytes, mgn_stream_t stream);

/* Normalizer.forward (reference layers.py:265-392, _accumulate 333-352, _mean/_std_with_epsilon
 * 354-369) on a row-major fp32 [rows, cols] matrix x (row stride ld), cols <= 32: when
 * accumulate != 0 and *num_acc < max_acc, the batch statistics — column sums of x and x² and the
 * row count, or the caller's pending = float[2*cols + 1] {Σx, Σx², count} (e.g. already summed
 * over ranks) — are added to the module's fp32 buffers acc_sum[cols], acc_sum_sq[cols],
 * *acc_count and *num_acc (+1); then out[rows, cols] (contiguous) = (x - mean) / max(sqrt(max(var,
 * 0)), eps), mean = acc_sum / max(acc_count, 1), var = acc_sum_sq / max(acc_count, 1) - mean².
 * Same fp32 expressions as the reference's torch ops (bit-identical results). */
size_t mgn_normalizer_workspace_bytes(int64_t rows, int32_t cols);
int mgn_normalizer_forward(const float* x, int64_t rows, int32_t cols, int64_t ld, int32_t accumulate,
                           const float* pending, float* acc_sum, float* acc_sum_sq, float* acc_count, float* num_acc,
                           float max_acc, float eps, float* out, void* ws, size_t ws_bytes, mgn_stream_t stream);

/* The Simulator's train/eval preamble (reference simulator.py:206-290, Simulator._build_input_graph):
 * the three Normalizer.forward calls of mgn_normalizer_forward on
 *   target delta   y[:, 0:oe-os] - x[:, os:oe]                          -> target_out [N, oe-os]
 *   node features  [x[:, fs:fe] ‖ one_hot(long(x[:, type_index]), n_types)] -> node_out [N, fe-fs+n_types]
 *   edge_attr      [E, edge_cols] (row stride lde; edge_norm NULL: none)  -> edge_out [E, edge_cols]
 * read straight from x [N, ldx], y [N, ldy] and edge_attr (no intermediate tensors), in 3 launches.
 * Statistics, buffers and outputs are bit-identical to the torch expressions + three
 * mgn_normalizer_forward calls (same partition and order). A node type outside [0, n_types) gives an
 * all-zero one-hot row and sets MGN_ERR_TYPE_NEG / MGN_ERR_TYPE_BIG in *err_word (if non-NULL); the
 * caller raises F.one_hot's RuntimeError from it. Output columns <= 32 per normalizer. */
typedef struct mgn_normalizer_state {
    float* acc_sum;      /* [cols] */
    float* acc_sum_sq;   /* [cols] */
    float* acc_count;    /* scalar */
    float* num_acc;      /* scalar */
    const float* pending; /* NULL or float[2*cols + 1] {Σx, Σx², count} (see mgn_normalizer_forward) */
    float max_acc, eps;
} mgn_normalizer_state;
size_t mgn_simulator_preamble_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int mgn_simulator_preamble(const float* x, int64_t N, int64_t ldx, int32_t feat_start, int32_t feat_end,
                           int32_t type_index, int32_t n_types, int32_t out_start, int32_t out_end,
                           const float* y, int64_t ldy, const float* edge_attr, int64_t E,
                           int32_t edge_cols, int64_t lde, int32_t accumulate,
                           const mgn_normalizer_state* out_norm, const mgn_normalizer_state* node_norm,
                           const mgn_normalizer_state* edge_norm, float* target_out, float* node_out,
                           float* edge_out, uint32_t* err_word, void* ws, size_t ws_bytes,
                           mgn_stream_t stream);

/* The batch statistics of the same three normalizers without updating them (the data-parallel
 * prologue: summed over ranks, then handed to mgn_simulator_preamble as `pending`): packed =
 * [Σ target delta, Σ target delta², N, Σ node features, Σ node features², N, (Σ edge_attr,
 * Σ edge_attr², E if edge_attr != NULL)] — each block the float[2*cols + 1] layout of `pending`, with
 * the same sums as mgn_column_stats. Workspace: mgn_simulator_preamble_workspace_bytes. Node types
 * are validated as in mgn_simulator_preamble (err_word may be NULL). */
int mgn_simulator_statistics(const float* x, int64_t N, int64_t ldx, int32_t feat_start, int32_t feat_end,
                             int32_t type_index, int32_t n_types, int32_t out_start, int32_t out_end,
                             const float* y, int64_t ldy, const float* edge_attr, int64_t E,
                             int32_t edge_cols, int64_t lde, float* packed, uint32_t* err_word, void* ws,
                             size_t ws_bytes, mgn_stream_t stream);

/* Masked L2 loss (reference utils/loss.py:10-65): *loss = Σ_r m_r Σ_c (pred - target)² / (count ·
 * cols) over row-major fp32 [rows, cols] pred/target, m_r = 1 when node_type[r·nt_ld] (a float
 * column, e.g. a strided view of x) is an integer t < 32 with bit t of type_mask set; count =
 * *count when given (data-parallel global count), else Σ m (written to *count_out if non-null).
 * Backward: grad = (*grad_loss or 1) · 2 (pred - target) · m / (count · cols). Deterministic. */
size_t mgn_masked_mse_workspace_bytes(int64_t rows);
int mgn_masked_mse(const float* pred, const float* target, int64_t rows, int32_t cols, const float* node_type,
                   int64_t nt_ld, uint32_t type_mask, const float* count, float* loss, float* count_out, void* ws,
                   size_t ws_bytes, mgn_stream_t stream);
int mgn_masked_mse_backward(const float* pred, const float* target, int64_t rows, int32_t cols,
                            const float* node_type, int64_t nt_ld, uint32_t type_mask, const float* count,
                            const float* grad_loss, float* grad, mgn_stream_t stream);

/* Diagonal Gaussian-mixture head (reference layers.py:157-195, utils/loss.py:111-199,
 * models/simulator.py:13-57) in a masked form without data-dependent shapes. params [rows, K(2d+1)]
 * row-major fp32: component k of a row is [logit, mean_0..mean_{d-1}, log_std_0..log_std_{d-1}].
 * With a = softmax(logit), s = temperature · exp(log_std),
 *   lc_k = Σ_j −½ (2 log(s + 1e-12) + (target_j − mean_kj)² / (s² + 1e-12) + log 2π)
 *   L    = logsumexp_k (log(a_k + 1e-12) + lc_k)                     (maximum subtracted)
 * *loss = −Σ_r m_r L_r / c, m as in mgn_masked_mse, c = *count when given, else Σ m (written to
 * *count_out if non-null); c == 0: the loss and every gradient are 0. Per-block partial sums in a fixed
 * order and a single-wave final pass, no atomics: bit-reproducible. Backward (one launch, recomputes the
 * row, written not accumulated): grad [rows, K(2d+1)] = (*grad_loss or 1) · d loss / d params, zero
 * rows where m = 0. Sampler: the component is the smallest k whose running sum of a exceeds u[r] (the
 * last one catches the rest), out[r, j] = mean_kj + temperature · exp(log_std_kj) · z[r, j].
 * Supported: 1 <= K <= 16, 1 <= d <= 8; anything else is a nonzero status before any launch. The added
 * symbols do not change MGN_ABI_VERSION; MGN_HAS_GMM marks headers that declare them. */
#define MGN_HAS_GMM 1
size_t mgn_gmm_nll_workspace_bytes(int64_t rows);
int mgn_gmm_nll_diag(const float* params, const float* target /* [rows, d] */, int64_t rows, int32_t d, int32_t K,
                     float temperature, const float* node_type, int64_t nt_ld, uint32_t type_mask,
                     const float* count, float* loss, float* count_out, void* ws, size_t ws_bytes,
                     mgn_stream_t stream);
int mgn_gmm_nll_diag_backward(const float* params, const float* target, int64_t rows, int32_t d, int32_t K,
                              float temperature, const float* node_type, int64_t nt_ld, uint32_t type_mask,
                              const float* count, const float* grad_loss, float* grad, mgn_stream_t stream);
int mgn_gmm_sample_diag(const float* params, int64_t rows, int32_t d, int32_t K, float temperature,
                        const float* u /* [rows] */, const float* z /* [rows, d] */, float* out /* [rows, d] */,
                        mgn_stream_t stream);

/* Resident trajectories: a training batch's x and y from trajectories kept clean on the device, in one
 * launch (the reference's Dataset.__getitem__ frame pick, dataset/h5_dataset.py:81-92, and its add_noise,
 * dataset/preprocessing.py:177-238). traj [T, N, F] contiguous fp32: T frames of the N nodes of the batch's
 * B graphs concatenated; graph g owns rows graph_ptr[g] .. graph_ptr[g+1] - 1 (graph_ptr[0] == 0,
 * graph_ptr[B] == N, non-decreasing; empty graphs allowed). For a node r of graph g, with t = frame[g]:
 *   x[r, c] = traj[t, r, c]                                   for every c < F
 *   x[r, c] = traj[t, r, c] + z[r, zc] * scales[i]            c inside noisy range i and
 *                                                             traj[t, r, type_index] == 0 (NodeType.NORMAL)
 *   y[r, j] = traj[t + 1, r, y_start + j]                     always the clean next frame
 * zc is the running column index over the ranges in the order given (range 0 owns z columns
 * 0 .. end[0]-start[0]-1, and so on). The sum is torch's fp32 composition bit for bit: the rounded product,
 * then the rounded add, never an FMA. z == NULL: no noise. traj is never written; columns of x at or
 * beyond F (ldx > F) are left alone. scales and frame are read on the device at run time: the host may
 * rewrite them between replays of a captured launch. frame[g] must lie in [0, T-2]: a precondition (the
 * caller owns frame), not checked on the device. One launch, no atomics, no workspace; N == 0 or B == 0
 * returns 0 without launching. Before any launch, a nonzero status for T < 2, F < 1, a range outside
 * [0, F], overlapping ranges, a y range outside [0, F], type_index outside [0, F), n > 4, or an ld too
 * small. The added symbol does not change MGN_ABI_VERSION; MGN_HAS_FEED marks headers that declare it. */
#define MGN_HAS_FEED 1
#define MGN_FEED_MAX_RANGES 4
typedef struct mgn_feed_ranges {           /* passed by value at launch */
    int32_t n;                             /* 0..MGN_FEED_MAX_RANGES noisy column ranges */
    int32_t start[MGN_FEED_MAX_RANGES], end[MGN_FEED_MAX_RANGES];   /* columns of a frame row */
} mgn_feed_ranges;
int mgn_feed_batch(const float* traj, int64_t T, int64_t N, int32_t F,   /* [T, N, F] contiguous fp32 */
                   const int32_t* graph_ptr, int32_t B,    /* device, [B+1] node offsets, graph_ptr[B] == N */
                   const int32_t* frame,                   /* device, [B], 0 <= frame[g] <= T-2 */
                   int32_t y_start, int32_t y_end,         /* y = traj[frame+1][:, y_start:y_end] */
                   int32_t type_index,                     /* node-type column of a frame row */
                   mgn_feed_ranges ranges,
                   const float* scales,                    /* device, [ranges.n] (host may rewrite between replays) */
                   const float* z, int64_t ldz,            /* device standard normals [N, Σ(end-start)]; NULL: no noise */
                   float* x, int64_t ldx, float* y, int64_t ldy, mgn_stream_t stream);

/* Rotation augmentation inside the feed (the reference's Random3DRotate, dataset/preprocessing.py:277-366): one
 * rotation per graph, applied to column triples of a row as row vector times matrix, before the noise.
 *   mgn_feed_rotation_matrices   R[g] (row-major 3x3) from angles[g] = {alpha (z), beta (y), gamma (x)} in
 *                                radians, the reference's _build_rotation_matrix in fp32. One thread per graph.
 *   mgn_feed_batch_rot           mgn_feed_batch, and for a column c of a triple (s, s + 3), with a = traj[t, r]:
 *                                  x[r, c] = (a[s]*R[g][0][c-s] + a[s+1]*R[g][1][c-s]) + a[s+2]*R[g][2][c-s]
 *                                then the noise rule of mgn_feed_batch on top of that value (the node type is read
 *                                from the clean row). With n = traj[t + 1, r]:
 *                                  y[r, j] = (n[y_start]*R[g][0][j] + n[y_start+1]*R[g][1][j]) + n[y_start+2]*R[g][2][j]
 *                                Every product and every sum is rounded on its own, in that order, never an FMA:
 *                                the same expression in torch's elementwise fp32 ops gives the same bits.
 *                                triples.n == 0: exactly mgn_feed_batch (R is not read, y is a copy). One launch.
 *   mgn_feed_rotate_rows         dst[r, c] = the same three-term rule on row r of src [rows, cols] with
 *                                R[row_graph[r]] for a column of a triple, src[r, c] bit for bit for any other
 *                                column and for every column of a row whose row_graph[r] is outside [0, B)
 *                                (R is not read for it). For edge_attr. src and dst must not overlap. One launch.
 * triples: `end` must equal `start + 3`. Before any launch, a nonzero status for a triple that is not 3 wide, a
 * triple outside [0, F) ([0, cols) for _rotate_rows), overlapping triples, type_index inside a triple, triples
 * with a y range that is neither empty nor 3 wide, triples with R == NULL, an ld smaller than its column count,
 * overlapping src and dst, and everything mgn_feed_batch refuses. N == 0, B == 0 and rows == 0 return 0 without a
 * launch. angles and R are read on the device at run time. No allocation, no synchronisation: capturable. The
 * added symbols do not change MGN_ABI_VERSION; MGN_HAS_FEED_ROTATE marks headers that declare them. */
#define MGN_HAS_FEED_ROTATE 1
int mgn_feed_rotation_matrices(const float* angles /* device, [B, 3] */, int32_t B, float* R /* device, [B, 9] */,
                               mgn_stream_t stream);
int mgn_feed_batch_rot(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                       const int32_t* frame, int32_t y_start, int32_t y_end, int32_t type_index,
                       mgn_feed_ranges ranges, const float* scales, const float* z, int64_t ldz,
                       float* x, int64_t ldx, float* y, int64_t ldy,
                       mgn_feed_ranges triples,                /* column triples of a frame row, end = start + 3 */
                       const float* R,                         /* device, [B, 9]; may be NULL when triples.n == 0 */
                       mgn_stream_t stream);
int mgn_feed_rotate_rows(const float* src, int64_t rows, int32_t cols, int64_t ld_src,
                         const int32_t* row_graph /* device, [rows] */, int32_t B, mgn_feed_ranges triples,
                         const float* R /* device, [B, 9] */, float* dst, int64_t ld_dst, mgn_stream_t stream);

/* World positions inside the feed (Lagrangian data: the reference's world_pos_parameters stages,
 * dataset/preprocessing.py:49-89 add_obstacles_next_pos and :143-174 add_world_pos_features, in the order of
 * build_preprocessing :401-442: obstacle displacement, then noise, then the relative world positions of the edges).
 * With a = traj[t, r, :F] (t = frame[g]) and n = traj[t + 1, r, :F], world position in columns [0, 3), the node
 * type in frame column type_index:
 *   mgn_feed_batch_world   writes batch rows of width F + 3:
 *       y[r, j]      = n[y_start + j]                          always clean (y_start must be 0, y_end >= 3)
 *       disp[r, j]   = n[j] - a[j], j < 3                      from clean values, one rounded fp32 difference
 *       mean[g][j]   = (sum of disp[r, j] over the rows of g with a[type_index] == 1, OBSTACLE) / (float) M_g
 *                      an fp32 sum in a fixed order (per thread over rows 1024 apart, a shuffle tree over the
 *                      wave, the waves in order), then a true, correctly rounded division by the count M_g, as
 *                      torch.mean: not a product with a reciprocal. M_g == 0 writes 0 (the reference: NaN).
 *       x[r, 0:3]    = a[0:3]
 *       x[r, 3:6]    = disp[r] for an OBSTACLE row, mean[g] for any other
 *       x[r, 6 + c]  = a[3 + c]                                the node type lands in batch column type_index + 3
 *     then mgn_feed_batch's noise rule on top of that value, with `ranges` in BATCH-layout columns (the
 *     reference's noise_index_start / _end of such a config), NORMAL rows only, the type read from the clean row,
 *     the rounded product then the rounded add, never an FMA. obstacle_mean [B, 3] is caller-owned and written.
 *     Columns of x at or beyond F + 3 are left alone; traj is never written. Two launches: one workgroup per
 *     graph for the mean, then the fill. No float atomics, no workspace: the same bits on every replay.
 *   mgn_feed_world_edge_features   for edge e, from the (noisy) x just written, senders = edge_index[0]:
 *       v = x[senders[e], 0:3] - x[receivers[e], 0:3]
 *       edge_attr[e, start : start + 3] = v
 *       edge_attr[e, start + 3]         = sqrt((v0*v0 + v1*v1) + v2*v2)   every product and sum rounded on its
 *                                         own, the square root correctly rounded
 *     Other columns of edge_attr are not touched. senders / receivers must lie in [0, rows of x): a precondition
 *     (the caller validates them once), not checked on the device. One launch, one thread per edge; the four
 *     values are one 16-byte store when start, ld_ea and the address of edge_attr are multiples of 4 floats.
 * frame, scales and z are read on the device at run time. No allocation, no synchronisation: capturable.
 * N == 0, B == 0 and E == 0 return 0 without a launch. Before any launch, a nonzero status for everything
 * mgn_feed_batch refuses (ranges and ldx checked against F + 3), F < 4, type_index < 3 or >= F, y_start != 0,
 * y_end < 3, a noisy range containing batch column type_index + 3, obstacle_mean == NULL; for the edge features
 * ld_ea < start + 4, start < 0, ldx < 3, null pointers with E > 0. Not covered: previous_data, rotation together
 * with world positions; world edges that change from frame to frame are mgn_world_topology_build below; the
 * Lagrangian rollout is mgn_rollout_begin_world below. The added symbols do not change MGN_ABI_VERSION; MGN_HAS_FEED_WORLD marks headers that declare them. */
#define MGN_HAS_FEED_WORLD 1
int mgn_feed_batch_world(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                         const int32_t* frame, int32_t y_start, int32_t y_end,
                         int32_t type_index,                   /* node-type column of a FRAME row, in [3, F) */
                         mgn_feed_ranges ranges,               /* noisy columns of a BATCH row, inside [0, F + 3] */
                         const float* scales, const float* z, int64_t ldz,
                         float* x, int64_t ldx /* >= F + 3 */, float* y, int64_t ldy,
                         float* obstacle_mean /* device, [B, 3], written */, mgn_stream_t stream);
int mgn_feed_world_edge_features(const int32_t* senders /* device, [E] */, const int32_t* receivers /* device, [E] */,
                                 int64_t E, const float* x, int64_t ldx, float* edge_attr, int64_t ld_ea,
                                 int32_t start, mgn_stream_t stream);

/* World edges inside the step (the reference's add_world_edges, dataset/preprocessing.py:92-140, which
 * build_preprocessing runs per item after the noise: every sample gets its own OBSTACLE–NORMAL contact edges, and a
 * transformer's attention is masked by them). One call builds, with no host read-back, the topology of
 *     mesh edges  ∪  both directions of every world pair
 * for a batch of graphs, each graph searched on its own.
 *   Pair rule. Nodes i and j of the SAME graph (graph_ptr [B + 1] node offsets) are a pair when one has node type 0
 *     (NORMAL), the other 1 (OBSTACLE) — node_type[r * ld_type], compared as floats — and
 *         ((double) pos[i][0] - (double) pos[j][0])² + (…[1])² + (…[2])²  <=  radius * radius
 *     in fp64, the squares added in dimension order, every product and sum rounded on its own: mgn_radius_pairs'
 *     arithmetic, whose pairs are scipy cKDTree.query_pairs'. Nodes of different graphs are never paired (the
 *     reference preprocesses before it batches). A pair that is already a mesh edge appears once (to_undirected).
 *   Mesh. mesh_ptr [N + 1] / mesh_nbr [E_m]: the static adjacency as CSR, the neighbours of a node ascending, symmetric,
 *     without duplicates, every edge inside one graph, mesh_ptr[0] = 0 and mesh_ptr[N] = E_m — what FaceToEdge +
 *     to_undirected emit, read row by row. These are preconditions the caller validates once; a neighbour outside
 *     [0, N) sets MGN_ERR_EDGE_INDEX and is clamped.
 *   Result, with E = E_m + (number of directed world edges) and capacity E_cap = E_m + N * max_neighbors:
 *     edge_index [2, E_cap] int64, rows E_cap apart: the first E columns are the reference's edge_index of the
 *       batch, sorted by (row, col); columns at and beyond E are unspecified.
 *     csc_src, csc_dst, csc_eid, row_perm [E_cap] and col_ptr, row_ptr [N + 1]: entry for entry what
 *       mgn_topology_build gives for that edge_index — within a target's segment the sources ascend, row_ptr ==
 *       col_ptr, row_perm[r] = the target-sorted position of the r-th edge in (row, col) order, csc_eid its inverse —
 *       so every kernel that reads a mgn_topology sums in the same order as on a host-built one. Entries at and
 *       beyond E are unspecified. A mgn_topology over these arrays carries num_edges = E_cap (workspace sizes).
 *     *num_edges (device int32) = E = col_ptr[N].
 *   Capacity. A node with more than max_neighbors world neighbours keeps its max_neighbors smallest and ORs
 *     MGN_ERR_WORLD_CAPACITY into *err_word (inside MGN_ERR_ANY: mgn_adamw_dev skips the update). The topology's
 *     contents are then unspecified, but every index this call writes lies inside its array and inside [0, N), and
 *     col_ptr / row_ptr stay non-decreasing within [0, E_cap]; entries the call did not write keep their previous
 *     values, so the caller initialises the six arrays and edge_index once (zeros) before the first build.
 * Three launches (search: one thread per node, the candidates of its graph staged through LDS; one exclusive scan of
 * the degrees; merge: eight lanes per node, two ascending lists merged, the rank in the source's lists by binary
 * search). Every grid is a function of N alone; no allocation, no synchronisation, no float reduction, no sort:
 * capturable, the same bits on every replay. ws: mgn_world_topology_workspace_bytes(N, max_neighbors), caller-owned.
 * N == 0 returns 0 without a launch. Before any launch, a nonzero status for NULL pointers, max_neighbors < 1,
 * radius <= 0 or not finite, ld_pos < 3, ld_type < 1, N > 0 with B == 0, N > 2^30, E_m + N * max_neighbors beyond int32, a
 * workspace too small. The added symbols do not change MGN_ABI_VERSION; MGN_HAS_WORLD_TOPOLOGY marks headers that
 * declare them. */
#define MGN_HAS_WORLD_TOPOLOGY 1
size_t mgn_world_topology_workspace_bytes(int64_t num_nodes, int32_t max_neighbors);
int mgn_world_topology_build(const float* pos, int64_t ld_pos /* >= 3 */,
                             const float* node_type, int64_t ld_type,   /* e.g. a column of the batch's x */
                             const int32_t* graph_ptr, int32_t B, int64_t num_nodes,
                             const int32_t* mesh_ptr, const int32_t* mesh_nbr, int64_t num_mesh_edges,
                             double radius, int32_t max_neighbors,
                             int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr, int32_t* row_ptr,
                             int32_t* row_perm, int64_t* edge_index, int32_t* num_edges /* device */,
                             uint32_t* err_word, void* ws, size_t ws_bytes, mgn_stream_t stream);

/* Random edges inside the step (the reference's BaseDataset._add_random_edges, dataset/dataset.py:104-137, the
 * dataset.new_edges_ratio of every transformer config: per item, PyG's add_random_edge(p, force_undirected=True) adds
 * "random jumps" to the adjacency that masks the attention). One call builds, with no host read-back, the topology of
 *     mesh edges  ∪  both directions of every surviving random pair
 * from a tensor of random bits, with the mesh, the result arrays and the capacity E_cap = E_m + N * max_new exactly as
 * mgn_world_topology_build has them (see there).
 *   Candidates. Graph g owns the candidates [cand_ptr[g], cand_ptr[g + 1]) of pairs [C, 2] (device int32, values
 *     >= 0; cand_ptr: device int32 [B + 1], non-decreasing from 0 to C = num_candidates, fixed by the caller — the
 *     Python side takes round(ratio * E_g) / 2 of them, as add_random_edge does, and none for a graph of fewer than
 *     two nodes). Candidate c of graph g, with n_g nodes from lo_g on, has the endpoints a = lo_g + pairs[c][0] % n_g
 *     and b = lo_g + pairs[c][1] % n_g.
 *   Pass 1, per node i over its graph's candidates in order: a candidate with i as one endpoint, a != b, whose other
 *     endpoint j is no mesh neighbour of i is live for i. A live candidate whose j is already in i's list is skipped;
 *     else, when the list holds max_new entries, the candidate is dropped (flagged); else j is appended, c beside it.
 *   Pass 2: i's new neighbours are the entries of its list whose candidate is not flagged, ascending.
 *     An unordered pair survives exactly when its first candidate is unflagged, at both endpoints alike, so the
 *     lists are symmetric. Dropping is the capacity policy: no error bit, the step goes on (the number of new
 *     neighbours of a node is about Poisson; a rare overflow must not stop a training run).
 *   *enabled (device int32): 0 makes every list empty, so the result is the mesh adjacency (validation).
 *   A mesh neighbour outside [0, N) is clamped and NOT flagged here: the caller validates the mesh once. cand_ptr is
 *     read on the device only; values outside [0, C] or out of order are clamped, every access stays in bounds.
 * One memset node (the flags) and five launches (the endpoints of every candidate, one thread each; pass 1: one thread
 * per node, the mapped candidates staged through LDS; pass 2: one thread per node, an insertion sort; then
 * mgn_world_topology_build's scan and merge). Every grid is a function of N and num_candidates alone; no atomics, no allocation, no synchronisation: capturable, the same bits on every replay for the same
 * pairs. ws: mgn_random_topology_workspace_bytes(N, max_new, num_candidates), caller-owned. N == 0 returns 0 without
 * a launch. Before any launch, a nonzero status for NULL pointers, max_new outside [1, 64], a negative count, N > 0
 * with B == 0, N or num_candidates > 2^30, E_m + N * max_new beyond int32, a workspace too small. The added symbols
 * do not change MGN_ABI_VERSION; MGN_HAS_RANDOM_EDGES marks headers that declare them. */
#define MGN_HAS_RANDOM_EDGES 1
size_t mgn_random_topology_workspace_bytes(int64_t num_nodes, int32_t max_new, int64_t num_candidates);
int mgn_random_topology_build(const int32_t* pairs /* device, [C, 2] */, const int32_t* cand_ptr /* device, [B + 1] */,
                              int64_t num_candidates, const int32_t* graph_ptr, int32_t B, int64_t num_nodes,
                              const int32_t* mesh_ptr, const int32_t* mesh_nbr, int64_t num_mesh_edges,
                              int32_t max_new, const int32_t* enabled /* device, [1] */,
                              int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr, int32_t* row_ptr,
                              int32_t* row_perm, int64_t* edge_index, int32_t* num_edges /* device */,
                              void* ws, size_t ws_bytes, mgn_stream_t stream);

/* World and random edges inside the step: both of the above in one topology, in the reference's order —
 * _apply_preprocessing runs add_world_edges on the sample's frame, _add_random_edges then adds its random jumps on top
 * of the edge_index that left (dataset/h5_dataset.py:102-105). One call builds, with no host read-back, the topology of
 *     mesh edges  ∪  both directions of every world pair  ∪  both directions of every surviving random pair
 * with the capacity E_cap = E_m + N * (max_neighbors + max_new); the mesh, the result arrays, the pair rule and
 * MGN_ERR_WORLD_CAPACITY are mgn_world_topology_build's, the candidates, both passes, *enabled and the dropping
 * policy mgn_random_topology_build's, with one addition: a candidate whose other endpoint is a WORLD neighbour of
 * this build is not live either (like a mesh edge, it is discarded without a redraw). max_new caps the new random
 * neighbours only. The world lists are symmetric, so both endpoints see the same verdict and the random lists stay
 * symmetric. cand_ptr is the caller's, fixed at construction (the Python side counts it from the mesh edges alone; the
 * reference counts round(p * E) over mesh plus world edges of the sample, a number that changes per sample and so
 * cannot size a recorded launch).
 *   *enabled == 0: the result equals mgn_world_topology_build's on the same inputs, entry for entry (the six arrays,
 *     the first *num_edges columns of edge_index, *num_edges); only E_cap, the distance of edge_index's rows, differs.
 *   A node over max_neighbors sets MGN_ERR_WORLD_CAPACITY as above: the topology is then unspecified (the truncated
 *     world lists need not be symmetric), every index written stays inside its array and inside [0, N). A mesh
 *     neighbour outside [0, N) sets MGN_ERR_EDGE_INDEX and is clamped.
 * One memset node and six launches: mgn_world_topology_build's search; the endpoints of every candidate; pass 1 with
 * the world lists as a second exclusion list (one more binary search per queued hit); pass 2; ONE scan over the three
 * degrees; ONE merge of three ascending, pairwise-disjoint lists per node (an entry's place is its own index plus its
 * rank in each of the other two; the id of edge (j -> i) is col_ptr[j] plus the rank of i in each of j's three lists).
 * Every grid is a function of N and num_candidates alone; no atomics beyond the OR into *err_word, no allocation, no
 * synchronisation: capturable. ws: mgn_world_random_topology_workspace_bytes(N, max_neighbors, max_new,
 * num_candidates), caller-owned. N == 0 returns 0 without a launch. Before any launch, a nonzero status for what
 * either build refuses, with E_m + N * (max_neighbors + max_new) beyond int32 in place of their capacity checks. The
 * added symbols do not change MGN_ABI_VERSION; MGN_HAS_WORLD_RANDOM_EDGES marks headers that declare them. */
#define MGN_HAS_WORLD_RANDOM_EDGES 1
size_t mgn_world_random_topology_workspace_bytes(int64_t num_nodes, int32_t max_neighbors, int32_t max_new,
                                                 int64_t num_candidates);
int mgn_world_random_topology_build(const float* pos, int64_t ld_pos /* >= 3 */,
                                    const float* node_type, int64_t ld_type,
                                    const int32_t* pairs /* device, [C, 2] */,
                                    const int32_t* cand_ptr /* device, [B + 1] */, int64_t num_candidates,
                                    const int32_t* graph_ptr, int32_t B, int64_t num_nodes,
                                    const int32_t* mesh_ptr, const int32_t* mesh_nbr, int64_t num_mesh_edges,
                                    double radius, int32_t max_neighbors, int32_t max_new,
                                    const int32_t* enabled /* device, [1] */,
                                    int32_t* csc_src, int32_t* csc_dst, int32_t* csc_eid, int32_t* col_ptr,
                                    int32_t* row_ptr, int32_t* row_perm, int64_t* edge_index,
                                    int32_t* num_edges /* device */, uint32_t* err_word, void* ws, size_t ws_bytes,
                                    mgn_stream_t stream);

/* Aneurysm features inside the feed (the reference's external/aneurysm.py build_features, which train.py hard-wires
 * as extra_node_features, then add_noise; coarse-aneurysm.json is written for this row). Frame rows are
 * [velocity (3), wall flag, ...], F >= 4; pos [N, 3] and node_type [N] are static, caller-owned and only read.
 *   mgn_feed_inflow_stats   for every frame t in [0, T - 2] and every graph g, one launch, a workgroup per pair:
 *       S = the 3 * M_g components of traj[t + 1, r, 0:3] - traj[t, r, 0:3] (one rounded fp32 difference) over the
 *           rows r = inflow_rows[inflow_ptr[g] .. inflow_ptr[g + 1]) of the graph, plus 0.0 when the graph has a row
 *           that is not listed (M_g < graph_ptr[g + 1] - graph_ptr[g]): what the reference's
 *           next_acceleration[~inflow] = 0; .unique() yields. Equal values (==; -0.0 and 0.0 are one value, kept
 *           as +0.0) count once.
 *       stats[t, g] = { mean, min, max } of S: min and max exact; mean = the fp64 sum of the distinct values in
 *           ascending order, divided in fp64 by their count, rounded once to fp32. M_g == 0 writes (0, 0, 0).
 *     The values are sorted in LDS (a bitonic network); no float atomics, no workspace, and the bits depend on
 *     neither B, nor the graph's place in the batch, nor the launch geometry. A graph's set may hold at most
 *     MGN_FEED_INFLOW_CAPACITY values (3 * M_g, plus the zero); max_values is the largest such count over the
 *     graphs, computed by the host that built inflow_ptr. inflow_rows must lie in [0, N) (a row outside counts as
 *     0.0). Non-finite values: unspecified results, no fault.
 *   mgn_feed_batch_aneurysm   writes batch rows of width F + 10; with t = frame[g], a = traj[t, r], p = traj[t - 1, r]
 *     and n = traj[t + 1, r]:
 *       x[r, 0:F]          = a
 *       x[r, F:F+3]        = a[0:3] - p[0:3]                one rounded fp32 difference
 *       x[r, F+3:F+6]      = pos[r]
 *       x[r, F+6:F+9]      = stats[t, g]                    mean, min, max
 *       x[r, F+9]          = node_type[r]
 *       y[r, j]            = n[y_start + j]                 always clean
 *     then mgn_feed_batch's noise rule on top of that value, with `ranges` (up to 8, a struct of its own) in
 *     BATCH-layout columns, on the rows with node_type[r] == 0, the rounded product then the rounded add, never an
 *     FMA. Columns of x at or beyond F + 10 are left alone; traj is never written. One launch. frame[g] must lie in
 *     [1, T - 2]: a precondition (the caller owns frame), not checked on the device.
 * Both are asynchronous, allocate nothing and are capturable. N == 0 or B == 0 returns 0 without a launch. Before
 * any launch, a nonzero status for null pointers, F < 4, T < 2 (stats) or T < 3 (fill), max_values outside
 * [0, MGN_FEED_INFLOW_CAPACITY], more than 8 ranges, a range outside [0, F + 10], overlapping ranges, a range
 * that contains column F + 9, a y range outside [0, F], an ld too small. Not covered: rotation together with these
 * features, a wall flag that changes over time (node_type is built once); their resident rollout is
 * mgn_rollout_begin_aneurysm below. The added symbols do not change MGN_ABI_VERSION; MGN_HAS_FEED_ANEURYSM marks
 * headers that declare them. */
#define MGN_HAS_FEED_ANEURYSM 1
#define MGN_FEED_ANEURYSM_MAX_RANGES 8
#define MGN_FEED_INFLOW_CAPACITY 4096      /* values per (frame, graph) set: 16 KiB of LDS */
typedef struct mgn_feed_ranges8 {          /* passed by value at launch */
    int32_t n;                             /* 0..MGN_FEED_ANEURYSM_MAX_RANGES noisy column ranges */
    int32_t start[MGN_FEED_ANEURYSM_MAX_RANGES], end[MGN_FEED_ANEURYSM_MAX_RANGES];   /* columns of a batch row */
} mgn_feed_ranges8;
int32_t mgn_feed_inflow_capacity(void);    /* MGN_FEED_INFLOW_CAPACITY of the library that was built */
int mgn_feed_inflow_stats(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                          const int32_t* inflow_ptr /* device, [B + 1] offsets into inflow_rows */,
                          const int32_t* inflow_rows /* device, rows of the batch, grouped by graph */,
                          int64_t max_values /* host: the largest value-set size over the graphs */,
                          float* stats /* device, [T - 1, B, 3], written */, mgn_stream_t stream);
int mgn_feed_batch_aneurysm(const float* traj, int64_t T, int64_t N, int32_t F, const int32_t* graph_ptr, int32_t B,
                            const int32_t* frame /* device, [B], 1 <= frame[g] <= T - 2 */,
                            int32_t y_start, int32_t y_end, const float* pos /* device, [N, 3] */,
                            const float* node_type /* device, [N] */, const float* stats /* device, [T - 1, B, 3] */,
                            mgn_feed_ranges8 ranges, const float* scales, const float* z, int64_t ldz,
                            float* x, int64_t ldx /* >= F + 10 */, float* y, int64_t ldy, mgn_stream_t stream);

/* Resident rollout: the data work of one autoregressive validation step (reference lightning_module.py:17-25,
 * 168-249) around the Simulator's evaluation forward, driven by a step counter on the device (*cursor, int32),
 * so a trajectory is S replays of one captured begin -> forward -> end. traj, graph_ptr and frame as in
 * mgn_feed_batch; no noise. With s = *cursor and t = frame[g] + s for a node r of graph g:
 *   mgn_rollout_begin   x[r, c] = traj[t, r, c] for every c < F, except, when s > 0,
 *                         x[r, out_start + j]  = last[r, j]         (the previous step's prediction)
 *                         x[r, prev_start + j] = last_prev[r, j]    (prev_start < prev_end: previous data)
 *                       y[r, j] = traj[t + 1, r, y_start + j]. traj is never written; columns of x at or beyond
 *                       F are left alone. One launch.
 *   mgn_rollout_end     keep = x[r, type_index] is neither 0 (NORMAL) nor 5 (OUTFLOW)   (build_mask)
 *                       pred[r, j] = keep ? y[r, j] : out[r, j]          out: the forward's outputs [N, d]
 *                       last = pred; last_prev = pred - x[r, out_start + j] (when non-null);
 *                       preds[s] = pred (when non-null, preds [capacity, N, d]);
 *                       loss[s] = mgn_masked_mse(pred, y, node type x[:, type_index], loss_type_mask), bit for
 *                       bit: the same blocks, rows per block, trees and final wave over the same row term;
 *                       sq[s] = Σ_r Σ_j (pred - y)²; then *cursor = s + 1. Two launches (per-block partial sums
 *                       {Σ m·err, Σ m, Σ err} into the workspace, a single-wave final pass in a fixed order),
 *                       no atomics: bit-reproducible. Only the final pass writes *cursor.
 * out, y (of _end), last, last_prev: row-major [N, d] without padding. frame[g] + *cursor in [0, T-2] and
 * *cursor in [0, capacity) are the caller's to keep (it writes frame and knows how many steps it enqueued);
 * outside them nothing is loaded or stored out of bounds: _begin skips the row, _end the whole step, and the
 * counter stops. No allocation, no synchronisation: capturable. N == 0 (or B == 0) returns 0 without a launch.
 * Before any launch, a nonzero status for T < 2, F < 1, a column range outside [0, F] (x's row for _end), an
 * empty output range, overlapping output and previous-data ranges, type_index inside the output columns, an ld
 * too small, capacity < 1 or a workspace too small. The added symbols do not change MGN_ABI_VERSION;
 * MGN_HAS_ROLLOUT marks headers that declare them. */
#define MGN_HAS_ROLLOUT 1
int mgn_rollout_begin(const float* traj, int64_t T, int64_t N, int32_t F,   /* [T, N, F] contiguous fp32 */
                      const int32_t* graph_ptr, int32_t B,    /* device, [B+1] node offsets, graph_ptr[B] == N */
                      const int32_t* frame,                   /* device, [B]: the trajectory's first frame per graph */
                      const int32_t* cursor,                  /* device, the step counter s */
                      int32_t y_start, int32_t y_end,         /* y = traj[frame+s+1][:, y_start:y_end] */
                      int32_t out_start, int32_t out_end,     /* columns of x the model predicts */
                      int32_t prev_start, int32_t prev_end,   /* previous-data columns; equal: none */
                      const float* last, int64_t ld_last, const float* last_prev, int64_t ld_prev,
                      float* x, int64_t ldx, float* y, int64_t ldy, mgn_stream_t stream);
size_t mgn_rollout_end_workspace_bytes(int64_t N);
int mgn_rollout_end(const float* out, const float* y, const float* x, int64_t N, int64_t ldx, int32_t type_index,
                    uint32_t loss_type_mask, int32_t out_start, int32_t d, float* last, float* last_prev,
                    float* preds, int32_t capacity, int32_t* cursor, float* loss, float* sq, void* ws,
                    size_t ws_bytes, mgn_stream_t stream);

/* Resident rollout with world positions (Lagrangian data such as DeformingPlate): the begin stage of a validation
 * step on the batch layout of mgn_feed_batch_world, following the reference's lightning_module.py:168-232 over a
 * dataset item built by dataset/preprocessing.py:49-89, 143-174, 401-427. With s = *cursor, t = frame[g] + s,
 * a = traj[t, r, :F] and n = traj[t + 1, r, :F]:
 *   mgn_rollout_begin_world
 *     the noise-free fill: y, disp, mean[g] and x[r, 0 : F + 3] exactly as mgn_feed_batch_world writes them with
 *       frame[g] = t and z == NULL, bit for bit, obstacle_mean included: both run one per-graph reduction (the
 *       same order: per thread over rows 1024 apart, a shuffle tree over the wave, the waves in order; a true
 *       division by the count; 0 for a graph without an OBSTACLE row);
 *     the feedback, after the fill and only when s > 0, in BATCH-layout columns:
 *       x[r, out_start + j]  = last[r, j]          x[r, prev_start + j] = last_prev[r, j]
 *       disp and mean always come from the clean frames: as in the reference, neither is recomputed from the
 *       fed-back positions;
 *     world_clean[r, 0:3] = a[0:3] when world_clean is non-null ([N, 3] contiguous): the clean world positions
 *       of frame t.
 *   The relative world positions of the edges need no kernel of their own: call mgn_feed_world_edge_features
 *   after this stage, with x = world_clean, ldx = 3 for edge features that follow the ground-truth frame (the
 *   reference's validation), or with the batch x for edge features that follow the positions the model sees (from
 *   step 1 on the fed-back ones). mgn_rollout_end is used as it is, with the batch-layout type_index (the frame's
 *   + 3), out_start and ldx.
 * Two launches: one workgroup per graph for the mean, then the fill, one thread per element of [N, F + 3]. No
 * float atomics, no workspace: the same bits on every replay. *cursor is only read; mgn_rollout_end's final pass
 * remains its only writer. If t is outside [0, T-2] nothing of that graph is written — its rows of x, y and
 * world_clean, obstacle_mean[g] — and nothing is read out of bounds. traj is never written; columns of x at or
 * beyond F + 3 are left alone. N == 0 or B == 0 returns 0 without a launch. No allocation, no synchronisation:
 * capturable. Before any launch, a nonzero status for everything mgn_rollout_begin refuses (ranges and ldx
 * checked against F + 3), F < 4, type_index < 3 or >= F, y_start != 0, y_end < 3 or > F, an output or
 * previous-data range containing batch column type_index + 3, obstacle_mean == NULL (also at N == 0), last == NULL
 * with a non-empty output range, last_prev == NULL with a non-empty previous-data range. Not covered: world edges
 * that change from frame to frame, rotation together with world positions. The added symbol does not change
 * MGN_ABI_VERSION; MGN_HAS_ROLLOUT_WORLD marks headers that declare it. */
#define MGN_HAS_ROLLOUT_WORLD 1
int mgn_rollout_begin_world(const float* traj, int64_t T, int64_t N, int32_t F,
                            const int32_t* graph_ptr, int32_t B, const int32_t* frame, const int32_t* cursor,
                            int32_t y_start, int32_t y_end,
                            int32_t type_index,                    /* node-type column of a FRAME row, in [3, F) */
                            int32_t out_start, int32_t out_end,    /* BATCH-layout columns, inside [0, F + 3] */
                            int32_t prev_start, int32_t prev_end,  /* BATCH layout; equal: none */
                            const float* last, int64_t ld_last, const float* last_prev, int64_t ld_prev,
                            float* x, int64_t ldx /* >= F + 3 */, float* y, int64_t ldy,
                            float* obstacle_mean /* device, [B, 3], written */,
                            float* world_clean /* device, [N, 3] contiguous, or NULL */, mgn_stream_t stream);

/* Resident rollout with the aneurysm features: the begin stage of a validation step on the batch layout of
 * mgn_feed_batch_aneurysm, following the reference's lightning_module.py:168-232 over a dataset item built by
 * external/aneurysm.py:27-64. With s = *cursor, t = frame[g] + s, a = traj[t, r], p = traj[t - 1, r] and
 * n = traj[t + 1, r]:
 *   mgn_rollout_begin_aneurysm
 *     the noise-free fill: x[r, 0 : F + 10] = [a ‖ a[0:3] - p[0:3] ‖ pos[r] ‖ stats[t, g] ‖ node_type[r]] and
 *       y[r, j] = n[y_start + j], exactly as mgn_feed_batch_aneurysm writes them with frame[g] = t and z == NULL,
 *       bit for bit: both kernels take the row from one inline function;
 *     the feedback, after the fill and only when s > 0, in BATCH-layout columns:
 *       x[r, out_start + j]  = last[r, j]          x[r, prev_start + j] = last_prev[r, j]
 *       so previous-data columns (F, F + 3) put the previous step's predicted - current into the acceleration
 *       columns (the reference's train.py default, use_previous_data = True, 4, 7 on F = 4), and without them the
 *       acceleration follows the clean frames. Nothing else is recomputed from the prediction: the statistics are
 *       those of the clean frames, which is also what a recomputation would give, because the INFLOW rows are
 *       masked back to the target on every step.
 *   mgn_rollout_end is used as it is, with type_index = F + 9, out_start and ldx of the batch row.
 * One launch, one thread per element of [N, F + 10]; no atomics, no workspace: the same bits on every replay.
 * *cursor is only read; mgn_rollout_end's final pass remains its only writer. traj, pos, node_type and stats are
 * only read. If t is outside [1, T-2] (frame t - 1 is read too) none of that graph's rows of x or y is written and
 * nothing is read out of bounds. Columns of x at or beyond F + 10 are left alone. N == 0 or B == 0 returns 0 without
 * a launch. No allocation, no synchronisation: capturable. Before any launch, a nonzero status for everything
 * mgn_rollout_begin refuses (ranges and ldx checked against F + 10), F < 4, T < 3, a y range outside [0, F], an
 * output or previous-data range containing column F + 9, null pos, node_type or stats, last == NULL with a
 * non-empty output range, last_prev == NULL with a non-empty previous-data range. Not covered: rotation together
 * with the aneurysm features, a wall flag that changes over time (node types are those of frame 0). The added
 * symbol does not change MGN_ABI_VERSION; MGN_HAS_ROLLOUT_ANEURYSM marks headers that declare it. */
#define MGN_HAS_ROLLOUT_ANEURYSM 1
int mgn_rollout_begin_aneurysm(const float* traj, int64_t T, int64_t N, int32_t F,
                               const int32_t* graph_ptr, int32_t B,
                               const int32_t* frame /* device, [B]: 1 <= frame[g] + *cursor <= T - 2 */,
                               const int32_t* cursor, int32_t y_start, int32_t y_end,
                               const float* pos /* device, [N, 3] */, const float* node_type /* device, [N] */,
                               const float* stats /* device, [T - 1, B, 3]: mgn_feed_inflow_stats */,
                               int32_t out_start, int32_t out_end,    /* BATCH-layout columns, inside [0, F + 9] */
                               int32_t prev_start, int32_t prev_end,  /* BATCH layout; equal: none */
                               const float* last, int64_t ld_last, const float* last_prev, int64_t ld_prev,
                               float* x, int64_t ldx /* >= F + 10 */, float* y, int64_t ldy, mgn_stream_t stream);

/* ---------------------------------------------------------------- gated MLP (transformer block, dense half) */
/* The second line of the reference's Transformer block (layers.py:198-262, 548-627), x + gated_mlp(norm2(x)):
 *   n1 = scale_a ⊙ x / (‖x‖₂ · d^-½ + 1e-8)      n = scale_b ⊙ n1 / (‖n1‖₂ · d^-½ + 1e-8)     (d = norm_dim)
 *   u = n W1ᵀ + b1,  v = n W2ᵀ + b2,  g = GELU(u) ⊙ v (erf GELU),  y = x + g W3ᵀ + b3
 * x, y, dy, dx fp32 (x, y, dy with row strides >= hidden, dx [rows, hidden] contiguous). The descriptor points
 * at the fp32 MASTER parameters, W1, W2 [expand, hidden] and W3 [hidden, expand] row-major without padding
 * (nn.Linear weights), any 4-byte alignment: the kernels read them when they run (MGN_BF16 rounds them to bf16
 * on the way into LDS), so a call issued — or a graph replayed — after an optimizer step sees the new values
 * without a repack. MGN_F32: exact fp32 MFMA throughout. MGN_BF16: the GEMM operands (n, g, the weights, and
 * dy, du, dv in the backward) are bf16, accumulation fp32; norms, u, v, GELU, the gate product, the residual,
 * y, dx and every parameter gradient are fp32. hidden in [1, 256] is zero-padded to a kernel width inside the
 * kernels; norm_dim (0: hidden) is the size the norms divide by.
 *   _forward   saved NULL: inference. Else saved (mgn_gated_mlp_saved_bytes) receives the two row norms; u, v
 *              and g are recomputed by the backward, nothing of size [rows, expand] is written by a forward.
 *   _backward  dx and grads, the flat gradient in module parameter order {scale_a [h], scale_b [h], W1, b1, W2,
 *              b2, W3, b3}, 2h + 9h² + 7h floats, overwritten. ws: mgn_gated_mlp_backward_workspace_bytes.
 * Rows are processed in tiles of mgn_gated_mlp_row_tile() rows by mgn_gated_mlp_blocks(rows, max_blocks) =
 * min(tiles, 512, max_blocks when > 0) workgroups, workgroup b the tiles b, b + blocks, ...; max_blocks leaves
 * part of the device to other streams and does not change a result bit of y or dx (the scale gradients' column
 * sums are added per workgroup, so their rounding follows the grid). The first call per device and kernel sets
 * a function attribute (dynamic LDS): make one eager call before capturing a graph. Caller-owned memory, asynchronous on the stream, no host
 * read-back (capturable), no atomics: every sum has a fixed order and two launches on the same inputs are
 * bitwise equal; every workgroup is independent. rows == 0 returns 0 without a launch. Before any launch, a
 * nonzero status (mgn_last_error) for hidden outside [1, 256], expand != 3·hidden, an unknown dtype, max_blocks < 0, a NULL
 * required pointer, a row stride < hidden or a workspace too small. The added symbols do not change
 * MGN_ABI_VERSION; MGN_HAS_GATED_MLP marks headers that declare them. */
#define MGN_HAS_GATED_MLP 1
typedef struct mgn_gated_mlp {
    int32_t hidden, expand; /* expand == 3 * hidden */
    int32_t dtype;          /* MGN_F32 | MGN_BF16 */
    int32_t norm_dim;       /* 0: hidden */
    int32_t max_blocks;     /* 0: the default grid; > 0: at most this many workgroups for the row-tile kernels */
    int32_t reserved;       /* 0 */
    const float *w1, *b1;   /* gated_mlp.1.linear1 [expand, hidden], [expand] */
    const float *w2, *b2;   /* gated_mlp.1.linear2 */
    const float *w3, *b3;   /* gated_mlp.2 [hidden, expand], [hidden] */
    const float *scale_a;   /* norm2.scale [hidden] */
    const float *scale_b;   /* gated_mlp.0.scale [hidden] */
} mgn_gated_mlp;
int32_t mgn_gated_mlp_row_tile(void);
int32_t mgn_gated_mlp_blocks(int64_t rows, int32_t max_blocks);
size_t mgn_gated_mlp_saved_bytes(const mgn_gated_mlp* m, int64_t rows);
int mgn_gated_mlp_forward(const mgn_gated_mlp* m, const float* x, int64_t ldx, int64_t rows, float* y, int64_t ldy,
                          void* saved, mgn_stream_t stream);
size_t mgn_gated_mlp_backward_workspace_bytes(const mgn_gated_mlp* m, int64_t rows);
int mgn_gated_mlp_backward(const mgn_gated_mlp* m, const float* x, int64_t ldx, int64_t rows, const void* saved,
                           const float* dy, int64_t lddy, float* dx, float* grads, void* ws, size_t ws_bytes,
                           mgn_stream_t stream);

/* torch.optim.AdamW semantics (decoupled weight decay p *= 1 - lr*wd, bias-corrected moments,
 * denominator sqrt(v)/sqrt(1-beta2^t) + eps), fp32, over n contiguous elements. */
int mgn_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
              double lr, double beta1, double beta2, double eps, double weight_decay,
              int64_t step, mgn_stream_t stream);

/* As mgn_adamw with lr and step read from device memory: hyper = double[2] {lr, step}. The launch
 * can be captured in a hipGraph and replayed with a new schedule (host updates hyper). err_word
 * (nullable, ABI v11): no update while a validation error is pending on it (see MGN_ERR_STALE). */
int mgn_adamw_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const double* hyper, double beta1, double beta2, double eps, double weight_decay,
                  uint32_t* err_word, mgn_stream_t stream);
/* ABI v12: as mgn_adamw_dev; a skipped update is counted in err_word's MGN_ERR_SKIP_* field only when
 * count_skip != 0 — an optimizer step that issues several launches (one per parameter group or
 * parameter) passes 1 on its first launch and 0 on the others, so the field counts STEPS.
 * mgn_adamw_dev == mgn_adamw_dev2(..., count_skip = 1, ...). Replaces the same optimizer step as
 * mgn_adamw (reference lightning_module.py:275-282). */
int mgn_adamw_dev2(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   const double* hyper, double beta1, double beta2, double eps, double weight_decay,
                   uint32_t* err_word, int32_t count_skip, mgn_stream_t stream);

/* ---------------------------------------------------------------- graph construction */
/* On-device replacements for the reference's per-sample host preprocessing (SURVEY.md §8(f)
 * rows 1 and 4). Edge lists are int64 [2, E] row-major (row block, then col block). Outputs are
 * coalesced: sorted by (row, col), duplicates removed. These calls synchronise the stream once to
 * return the data-dependent count to the host. Indices outside [0, num_nodes) fail with
 * "edge_index out of range" (the reference raises from ATen). */
#define MGN_COALESCE_SYMMETRIZE 1      /* add (col, row) for every (row, col): to_undirected */
#define MGN_COALESCE_DROP_SELF_LOOPS 2 /* drop (i, i)                                          */
size_t mgn_coalesce_workspace_bytes(int64_t num_keys);
/* torch_geometric.utils.to_undirected(edge_index, num_nodes) / torch sparse coalesce() of the
 * pattern (reference dataset/preprocessing.py:135, utils/torch_graph.py:32-36). out capacity:
 * 2·num_keys int64, num_keys = num_edges (·2 with MGN_COALESCE_SYMMETRIZE); out[0:2E] holds the
 * [2, E] result, *num_out = E (host). */
int mgn_coalesce(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, int32_t flags,
                 int64_t* out, int64_t* num_out, void* ws, size_t ws_bytes, mgn_stream_t stream);
/* T.FaceToEdge(remove_faces=False) (reference dataset/preprocessing.py:410,431): cells [k, C]
 * int64 row-major, k = 3 (triangles: pairs (f0,f1), (f1,f2), (f0,f2)) or k = 4 (tetrahedra split
 * into the 4 triangles of utils/torch_graph.py:173-181), then to_undirected. Workspace and out
 * capacity from num_keys = mgn_face_to_edge_keys(k, C). */
int64_t mgn_face_to_edge_keys(int32_t verts_per_cell, int64_t num_cells);
int mgn_face_to_edge(const int64_t* cells, int32_t verts_per_cell, int64_t num_cells, int64_t num_nodes,
                     int64_t* edge_index, int64_t* num_edges, void* ws, size_t ws_bytes, mgn_stream_t stream);
/* One hop of compute_k_hop_edge_index (reference utils/torch_graph.py:38-51): the pattern of
 * A_k + A_k·A with self loops removed, coalesced. edge_index_a = A must be coalesced (sorted by
 * row); A_k any edge list. Two calls: mgn_khop_count returns the candidate count num_keys
 * (= E_k + Σ_k deg_A(col_k)), then mgn_khop_hop (workspace mgn_khop_workspace_bytes, out capacity
 * 2·num_keys) produces the result and *num_out. */
size_t mgn_khop_count_workspace_bytes(int64_t num_edges_k, int64_t num_edges_a, int64_t num_nodes);
int mgn_khop_count(const int64_t* edge_index_k, int64_t num_edges_k, const int64_t* edge_index_a,
                   int64_t num_edges_a, int64_t num_nodes, int64_t* num_keys, void* ws, size_t ws_bytes,
                   mgn_stream_t stream);
size_t mgn_khop_workspace_bytes(int64_t num_keys, int64_t num_edges_k, int64_t num_nodes);
int mgn_khop_hop(const int64_t* edge_index_k, int64_t num_edges_k, const int64_t* edge_index_a,
                 int64_t num_edges_a, int64_t num_nodes, int64_t num_keys, int64_t* out, int64_t* num_out,
                 void* ws, size_t ws_bytes, mgn_stream_t stream);
/* T.Cartesian(norm=False) ‖ T.Distance(norm=False) (reference dataset/preprocessing.py:16-23) and
 * add_world_pos_features (143-174): out[k, 0:dim] = pos[row_k] − pos[col_k], out[k, dim] = its
 * L2 norm; fp32, pos row stride pos_ld, out row stride out_ld >= dim + 1, dim <= 3. ws >= 4 B. */
int mgn_edge_features(const float* pos, int64_t pos_ld, int32_t dim, const int64_t* edge_index,
                      int64_t num_edges, int64_t num_nodes, float* out, int64_t out_ld, void* ws,
                      size_t ws_bytes, mgn_stream_t stream);
/* cKDTree(pos).query_pairs(radius) of add_world_edges (reference dataset/preprocessing.py:114-121):
 * all (i, j), i < j, with the fp64 distance <= radius, as a [2, P] int64 list in out[0:2P]
 * (out[0:P] = i, out[P:2P] = j); pair order unspecified. node_type (float
 * column, stride node_type_ld) non-null keeps only OBSTACLE(1)–NORMAL(0) pairs in either order
 * (preprocessing.py:123-133). *num_pairs = P always; nothing is written when out is NULL or
 * capacity < P (call again with capacity >= P). */
size_t mgn_radius_pairs_workspace_bytes(int64_t num_nodes);
int mgn_radius_pairs(const float* pos, int64_t pos_ld, int32_t dim, int64_t num_nodes, double radius,
                     const float* node_type, int64_t node_type_ld, int64_t* out, int64_t capacity,
                     int64_t* num_pairs, void* ws, size_t ws_bytes, mgn_stream_t stream);

/* ---------------------------------------------------------------- opt-in profiler */
/* Kernel classes: 0 edge-MLP fwd, 1 node-MLP fwd, 2 dense-MLP fwd, 3 edge-MLP bwd-data,
 * 4 node-MLP bwd-data, 5 dense-MLP bwd-data, 6 weight-grad, 7 weight-grad reduce,
 * 8 node-gradient combine (segment sums of dZ0 + dP·W0[:, h:3h] GEMM), 9 weight pack,
 * 10 AdamW, 11 node projection x·W0[:, h:3h]ᵀ. */
int mgn_profile_enable(int on);
int mgn_profile_collect(int kind, double* total_ms, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* MGN_H */
