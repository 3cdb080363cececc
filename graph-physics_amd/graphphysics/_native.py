"""ctypes binding of libmgn (include/mgn.h) — the MI355X-native hot path.

The library is built in-tree by `python __graft_entry__.py` (hipcc --offload-arch=gfx950) into
graph-physics_amd/graphphysics/_lib/libmgn.so. There is NO fallback: every model entry point
raises if the library or a HIP device is missing.
"""
import ctypes
import os

import torch

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libmgn.so")
ABI_VERSION = 17  # include/mgn.h MGN_ABI_VERSION these bindings are written for

MGN_F32 = 0
MGN_BF16 = 1
MGN_BWD_DE_OUT_PAIR = 1  # mgn.h: de_out in the pair layout
MGN_BWD_DE_PAIR = 2      # mgn.h: write de in the pair layout
MGN_BWD_DX_OUT_PAIR = 4  # mgn.h: dx_out in the pair layout
MGN_BWD_DX_PAIR = 8      # mgn.h: write dx in the pair layout
MGN_BWD_DATA_ONLY = 16   # mgn.h (v13): the data-gradient half of mgn_block_backward_deferred2
MGN_BWD_WGRAD_ONLY = 32  # mgn.h (v13): its weight-gradient half
MGN_MAX_LAYERS = 8

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_sz = ctypes.c_size_t
_dbl = ctypes.c_double
_f32 = ctypes.c_float
_u32 = ctypes.c_uint32


class Topology(ctypes.Structure):
    _fields_ = [("num_nodes", _i64), ("num_edges", _i64), ("csc_src", _vp), ("csc_dst", _vp),
                ("csc_eid", _vp), ("col_ptr", _vp), ("row_ptr", _vp), ("row_perm", _vp)]


class Mlp(ctypes.Structure):
    _fields_ = [("n_layers", _i32), ("in_dim", _i32), ("hidden", _i32), ("out_dim", _i32),
                ("has_norm", _i32), ("dtype", _i32), ("norm_dim", _i32), ("reserved", _i32),
                ("wpack", _vp), ("wtpack", _vp), ("bias", _vp * MGN_MAX_LAYERS), ("scale", _vp)]


class MlpSaved(ctypes.Structure):
    _fields_ = [("act", _vp), ("mask", _vp), ("z", _vp), ("rden", _vp)]


class BlockSaved(ctypes.Structure):
    _fields_ = [("edge", MlpSaved), ("node", MlpSaved), ("aggr", _vp), ("proj", _vp)]


class WgradReduce(ctypes.Structure):
    _fields_ = [("part", _vp), ("dsp", _vp), ("grads", _vp), ("G", _i64), ("nchunks", _i32), ("ntiles", _i32),
                ("NS", _i32), ("blocks", _i32), ("w0_n", _i32), ("w0_k", _i32), ("xcol0", _i32), ("nchunks_x", _i32),
                ("hoff", _i64), ("nchunks_h", _i32), ("pad", _i32)]


class CallOpts(ctypes.Structure):
    """mgn_call_opts (ABI v17): per-call CU caps and the device error word (mgn.h)."""
    _fields_ = [("data_cus", _i32), ("wgrad_cus", _i32), ("err_word", _vp)]


class NormalizerState(ctypes.Structure):
    _fields_ = [("acc_sum", _vp), ("acc_sum_sq", _vp), ("acc_count", _vp), ("num_acc", _vp), ("pending", _vp),
                ("max_acc", _f32), ("eps", _f32)]


class PackJob(ctypes.Structure):
    _fields_ = [("w", _vp), ("dst", _vp), ("dstT", _vp), ("n", _i32), ("k", _i32), ("dtype", _i32),
                ("n_src", _i32), ("k_src", _i32), ("kb_src", _i32), ("kb_pad", _i32), ("reserved", _i32)]


MGN_FEED_MAX_RANGES = 4


class FeedRanges(ctypes.Structure):
    """mgn_feed_ranges: the noisy column ranges of mgn_feed_batch, passed by value (mgn.h)."""
    _fields_ = [("n", _i32), ("start", _i32 * MGN_FEED_MAX_RANGES), ("end", _i32 * MGN_FEED_MAX_RANGES)]


MGN_FEED_ANEURYSM_MAX_RANGES = 8
MGN_FEED_INFLOW_CAPACITY = 4096  # mgn.h: values per (frame, graph) set of mgn_feed_inflow_stats; checked by load()


class FeedRanges8(ctypes.Structure):
    """mgn_feed_ranges8: the noisy column ranges of mgn_feed_batch_aneurysm, passed by value (mgn.h)."""
    _fields_ = [("n", _i32), ("start", _i32 * MGN_FEED_ANEURYSM_MAX_RANGES),
                ("end", _i32 * MGN_FEED_ANEURYSM_MAX_RANGES)]


class GatedMlp(ctypes.Structure):
    """mgn_gated_mlp: the fp32 master parameters of a Transformer block's norm2 + gated_mlp (mgn.h)."""
    _fields_ = [("hidden", _i32), ("expand", _i32), ("dtype", _i32), ("norm_dim", _i32), ("max_blocks", _i32),
                ("reserved", _i32), ("w1", _vp), ("b1", _vp),
                ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp), ("scale_a", _vp), ("scale_b", _vp)]


EXPORTS = {
    "mgn_abi_version": (_i32, []),
    "mgn_last_error": (ctypes.c_char_p, []),
    "mgn_topology_workspace_bytes": (_sz, [_i64, _i64]),
    "mgn_topology_build": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_topology_build_async": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "mgn_linear_pack_elems": (_i64, [_i32, _i32, _i32]),
    "mgn_mlp_pack_elems": (_i64, [ctypes.POINTER(Mlp)]),
    "mgn_pack_weights": (_i32, [_vp, _i32, _i64, _vp]),
    "mgn_mlp_forward": (_i32, [ctypes.POINTER(Mlp), _vp, _i32, _i64, _vp, _i64, _vp, _i32,
                               ctypes.POINTER(MlpSaved), _vp]),
    "mgn_mlp_backward_workspace_bytes": (_sz, [ctypes.POINTER(Mlp), _i64]),
    "mgn_mlp_saved_elems": (_i32, [ctypes.POINTER(Mlp), _i64, _i32, _vp, _vp]),
    "mgn_mlp_backward": (_i32, [ctypes.POINTER(Mlp), _vp, _i32, _i64, _vp, _i64,
                                ctypes.POINTER(MlpSaved), _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "mgn_mlp_backward_keep_bytes": (_sz, [ctypes.POINTER(Mlp), _i64]),
    "mgn_mlp_backward_deferred": (_i32, [ctypes.POINTER(Mlp), _vp, _i32, _i64, _vp, _i64,
                                         ctypes.POINTER(MlpSaved), _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp, _sz,
                                         ctypes.POINTER(WgradReduce), _vp]),
    "mgn_mlp_backward_deferred2": (_i32, [ctypes.POINTER(Mlp), _vp, _i32, _i64, _vp, _i64,
                                          ctypes.POINTER(MlpSaved), _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp, _sz,
                                          ctypes.POINTER(WgradReduce), _i32, _vp]),
    "mgn_block_forward_inference_supported": (_i32, [ctypes.POINTER(Mlp), ctypes.POINTER(Mlp)]),
    "mgn_block_forward_workspace_bytes": (_sz, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp),
                                                ctypes.POINTER(Mlp)]),
    "mgn_block_forward": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                 _vp, _vp, _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _sz, _vp]),
    "mgn_block_forward_chain": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                       _vp, _vp, _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _sz, _i32,
                                       ctypes.POINTER(Mlp), _vp, _sz, ctypes.POINTER(ctypes.c_int32), _vp]),
    "mgn_block_forward_scratch_bytes": (_sz, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp)]),
    "mgn_block_forward_chain2": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                        _vp, _vp, _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _sz, _i32,
                                        ctypes.POINTER(Mlp), _vp, _sz, ctypes.POINTER(ctypes.c_int32), _vp, _sz, _vp]),
    "mgn_block_backward_workspace_bytes": (_sz, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp),
                                                 ctypes.POINTER(Mlp)]),
    "mgn_block_backward": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                  _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _sz, _vp]),
    "mgn_block_backward_data": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                       _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _sz, _vp]),
    "mgn_block_backward_wgrad": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                        _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _sz, _vp]),
    "mgn_block_backward_keep_bytes": (_sz, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp)]),
    "mgn_block_backward_deferred": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                           _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _sz, _vp, _sz, ctypes.POINTER(WgradReduce), _vp]),
    "mgn_block_backward_deferred2": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                            _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _sz, _vp, _sz, ctypes.POINTER(WgradReduce), _i32, _vp]),
    "mgn_wgrad_reduce_many": (_i32, [ctypes.POINTER(WgradReduce), _i32, _vp]),
    "mgn_block_backward_deferred3": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), ctypes.POINTER(Mlp),
                                            _vp, _vp, ctypes.POINTER(BlockSaved), _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _sz, _vp, _sz, ctypes.POINTER(WgradReduce), _i32,
                                            ctypes.POINTER(CallOpts), _vp]),
    "mgn_mlp_backward_deferred3": (_i32, [ctypes.POINTER(Mlp), _vp, _i32, _i64, _vp, _i64,
                                          ctypes.POINTER(MlpSaved), _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp, _sz,
                                          ctypes.POINTER(WgradReduce), _i32, ctypes.POINTER(CallOpts), _vp]),
    "mgn_node_grad": (_i32, [ctypes.POINTER(Topology), ctypes.POINTER(Mlp), _vp, _vp, _vp, _vp, _i32, _i32,
                             ctypes.POINTER(CallOpts), _vp]),
    "mgn_debug_wave_times": (_i32, [_i32, _vp, _i32]),
    "mgn_graph_attention_workspace_bytes": (_sz, [ctypes.POINTER(Topology), _i32, _i32, _i32]),
    "mgn_graph_attention_forward": (_i32, [ctypes.POINTER(Topology), _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp,
                                           _vp, _vp]),
    "mgn_graph_attention_backward": (_i32, [ctypes.POINTER(Topology), _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32,
                                            _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_gated_mlp_row_tile": (_i32, []),
    "mgn_gated_mlp_blocks": (_i32, [_i64, _i32]),
    "mgn_gated_mlp_saved_bytes": (_sz, [ctypes.POINTER(GatedMlp), _i64]),
    "mgn_gated_mlp_forward": (_i32, [ctypes.POINTER(GatedMlp), _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "mgn_gated_mlp_backward_workspace_bytes": (_sz, [ctypes.POINTER(GatedMlp), _i64]),
    "mgn_gated_mlp_backward": (_i32, [ctypes.POINTER(GatedMlp), _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _sz,
                                      _vp]),
    "mgn_permute_rows": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "mgn_segment_sum": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "mgn_column_stats_workspace_bytes": (_sz, [_i64, _i32]),
    "mgn_column_stats": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _sz, _vp]),
    "mgn_normalizer_workspace_bytes": (_sz, [_i64, _i32]),
    "mgn_normalizer_forward": (_i32, [_vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _vp,
                                      _vp, _sz, _vp]),
    "mgn_simulator_preamble_workspace_bytes": (_sz, [_i64, _i64]),
    "mgn_simulator_preamble": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i64,
                                      _i32, _i64, _i32, ctypes.POINTER(NormalizerState),
                                      ctypes.POINTER(NormalizerState), ctypes.POINTER(NormalizerState), _vp, _vp,
                                      _vp, _vp, _vp, _sz, _vp]),
    "mgn_simulator_statistics": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i64,
                                        _i32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mgn_masked_mse_workspace_bytes": (_sz, [_i64]),
    "mgn_masked_mse": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _u32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_masked_mse_backward": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _u32, _vp, _vp, _vp, _vp]),
    "mgn_gmm_nll_workspace_bytes": (_sz, [_i64]),
    "mgn_gmm_nll_diag": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _vp, _i64, _u32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_gmm_nll_diag_backward": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _vp, _i64, _u32, _vp, _vp, _vp, _vp]),
    "mgn_gmm_sample_diag": (_i32, [_vp, _i64, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "mgn_feed_batch": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _i32, _i32, FeedRanges, _vp, _vp, _i64,
                              _vp, _i64, _vp, _i64, _vp]),
    "mgn_feed_rotation_matrices": (_i32, [_vp, _i32, _vp, _vp]),
    "mgn_feed_batch_rot": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _i32, _i32, FeedRanges, _vp, _vp,
                                  _i64, _vp, _i64, _vp, _i64, FeedRanges, _vp, _vp]),
    "mgn_feed_rotate_rows": (_i32, [_vp, _i64, _i32, _i64, _vp, _i32, FeedRanges, _vp, _vp, _i64, _vp]),
    "mgn_feed_batch_world": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _i32, _i32, FeedRanges, _vp, _vp,
                                    _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "mgn_feed_world_edge_features": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp]),
    "mgn_world_topology_workspace_bytes": (_sz, [_i64, _i32]),
    "mgn_world_topology_build": (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _i64, _dbl, _i32, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_random_topology_workspace_bytes": (_sz, [_i64, _i32, _i64]),
    "mgn_random_topology_build": (_i32, [_vp, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mgn_world_random_topology_workspace_bytes": (_sz, [_i64, _i32, _i32, _i64]),
    "mgn_world_random_topology_build": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _i64,
                                               _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _sz, _vp]),
    "mgn_feed_inflow_capacity": (_i32, []),
    "mgn_feed_inflow_stats": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp]),
    "mgn_feed_batch_aneurysm": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, FeedRanges8,
                                       _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "mgn_rollout_begin": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp,
                                 _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "mgn_rollout_begin_world": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                       _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "mgn_rollout_begin_aneurysm": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32,
                                          _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "mgn_rollout_end_workspace_bytes": (_sz, [_i64]),
    "mgn_rollout_end": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _u32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                               _vp, _sz, _vp]),
    "mgn_adamw": (_i32, [_vp, _vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, _dbl, _dbl, _i64, _vp]),
    "mgn_adamw_dev": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _dbl, _dbl, _dbl, _dbl, _vp, _vp]),
    "mgn_adamw_dev2": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _dbl, _dbl, _dbl, _dbl, _vp, _i32, _vp]),
    "mgn_coalesce_workspace_bytes": (_sz, [_i64]),
    "mgn_coalesce": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mgn_face_to_edge_keys": (_i64, [_i32, _i64]),
    "mgn_face_to_edge": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mgn_khop_count_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mgn_khop_count": (_i32, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _sz, _vp]),
    "mgn_khop_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "mgn_khop_hop": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "mgn_edge_features": (_i32, [_vp, _i64, _i32, _vp, _i64, _i64, _vp, _i64, _vp, _sz, _vp]),
    "mgn_radius_pairs_workspace_bytes": (_sz, [_i64]),
    "mgn_radius_pairs": (_i32, [_vp, _i64, _i32, _i64, _dbl, _vp, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "mgn_profile_enable": (_i32, [_i32]),
    "mgn_profile_collect": (_i32, [_i32, _vp, _vp]),
}

PROF_KINDS = ["fwd_edge", "fwd_node", "fwd_dense", "bwd_edge", "bwd_node", "bwd_dense", "wgrad",
              "wgrad_reduce", "combine", "pack", "adamw", "proj", "wgrad_dense"]


def profile_enable(on=True):
    check(lib().mgn_profile_enable(int(on)))


def profile_collect():
    """{kernel class: (total_ms, launches)} since the last profile_enable()."""
    out = {}
    for i, name in enumerate(PROF_KINDS):
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        check(lib().mgn_profile_collect(i, ctypes.byref(ms), ctypes.byref(cnt)))
        out[name] = (ms.value, cnt.value)
    return out

_lib = None


def load(path=LIB_PATH):
    """Load libmgn and bind every exported symbol (no device needed)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"libmgn not built ({path} missing): run `python __graft_entry__.py` (hipcc gfx950). "
            "The MGN path has no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:  # symbols added without an ABI bump (e.g. mgn_graph_attention_*): a stale build
            raise RuntimeError(f"libmgn at {path} does not export {name}: it is older than these bindings, "
                               "rebuild (python __graft_entry__.py)") from None
        fn.restype = res
        fn.argtypes = args
    if lib.mgn_abi_version() != ABI_VERSION:  # a stale build would mis-read changed signatures
        raise RuntimeError(f"libmgn ABI {lib.mgn_abi_version()} at {path}, these bindings need {ABI_VERSION}: "
                           "rebuild (python __graft_entry__.py)")
    if lib.mgn_feed_inflow_capacity() != MGN_FEED_INFLOW_CAPACITY:
        raise RuntimeError(f"libmgn at {path} was built with MGN_FEED_INFLOW_CAPACITY = "
                           f"{lib.mgn_feed_inflow_capacity()}, these bindings say {MGN_FEED_INFLOW_CAPACITY}")
    _lib = lib
    return lib


def lib():
    return _lib if _lib is not None else load()


def check(rc):
    if rc != 0:
        msg = lib().mgn_last_error().decode(errors="replace")
        if "out of range" in msg:
            raise IndexError(msg)
        raise RuntimeError(f"libmgn error {rc}: {msg}")


# ---------------------------------------------------------------- device error word (ABI v7)
ERR_EDGE_INDEX, ERR_TYPE_NEG, ERR_TYPE_BIG = 1, 2, 4
ERR_HANDOFF = 8  # ABI v17: a pipelined kernel's bounded hand-off wait timed out (mgn.h MGN_ERR_HANDOFF)
ERR_WORLD_CAPACITY = 16  # mgn.h MGN_ERR_WORLD_CAPACITY: a node with more world neighbours than max_neighbors
ERR_ANY, ERR_SKIP_SHIFT, ERR_STALE = 0xFFFF, 16, 1 << 31  # ABI v11 (include/mgn.h)


def _raise_for(bits):
    """The exception the reference raises for the validation failure in `bits`. The exception's
    `mgn_skipped_updates` is the number of optimizer steps mgn_adamw_dev skipped because the error
    was pending (the caller rewinds its host-side step counters by as many)."""
    ex = None
    if bits & ERR_EDGE_INDEX:
        ex = IndexError("edge_index out of range: an index is outside [0, num_nodes) "
                        "(libmgn device check; the reference's ATen gather raises IndexError)")
    elif bits & ERR_TYPE_NEG:
        ex = RuntimeError("Class values must be non-negative.")  # F.one_hot (reference simulator one-hot)
    elif bits & ERR_TYPE_BIG:
        ex = RuntimeError("Class values must be smaller than num_classes.")
    elif bits & ERR_HANDOFF:
        # not a validation error of the batch: a libmgn kernel (the recomputed edge weight gradients)
        # gave up waiting inside its pipeline and wrote NaN partial sums; the optimizer step was skipped
        ex = RuntimeError("libmgn: a hand-off wait of the recomputed weight gradients timed out "
                          "(MGN_ERR_HANDOFF); the step's gradients are invalid and its optimizer update was skipped")
    elif bits & ERR_WORLD_CAPACITY:
        ex = world_capacity_error()
    if ex is not None:
        ex.mgn_skipped_updates = (bits >> ERR_SKIP_SHIFT) & 0xFF
        raise ex


def world_capacity_error():
    """The ValueError of MGN_ERR_WORLD_CAPACITY (the device check of mgn_world_topology_build, and the host check
    of dataset.resident.world_topology_torch)."""
    return ValueError("dynamic_edges: a node has more world neighbours within the radius than max_neighbors; the "
                      "step's topology is invalid and its optimizer update was skipped: raise max_neighbors")


class ErrorWord:
    """One uint32 device word per device that libmgn's validating kernels OR MGN_ERR_* bits into
    (mgn_topology_build_async, mgn_simulator_preamble / _statistics), so a new batch never forces a
    host read-back. arm() queues a non-blocking copy to pinned host memory behind the launches;
    poll() raises (and clears the word) once a queued copy has landed with a bit set — at most one
    call late, without synchronising; check() synchronises and raises now."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.event = None

    def ptr(self):
        return _vp(self.dev.data_ptr())

    def arm(self):
        """Queue the device word's copy-back (skipped while a hipGraph is being captured: a captured
        step's owner arms after each replay)."""
        if torch.cuda.is_current_stream_capturing():
            return
        self.host.copy_(self.dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.event = ev

    def poll(self):
        ev = self.event
        if ev is None or torch.cuda.is_current_stream_capturing() or not ev.query():
            return
        self.event = None
        bits = int(self.host[0])
        if bits:
            self._clear()
            _raise_for(bits)

    def check(self):
        if torch.cuda.is_current_stream_capturing():
            return
        torch.cuda.current_stream(self.device).synchronize()
        bits = int(self.dev[0].item())
        self.event = None
        if bits:
            self._clear()
            _raise_for(bits)

    def _clear(self):
        self.dev.zero_()
        self.host.zero_()


_ERR_WORDS = {}


def error_word(device):
    d = torch.device(device)
    if d.index is None:
        d = torch.device(d.type, torch.cuda.current_device())
    w = _ERR_WORDS.get(d)
    if w is None:
        if torch.cuda.is_current_stream_capturing():  # its storage must outlive any graph pool
            raise RuntimeError("libmgn: run one eager call on this device before capturing a graph")
        w = _ERR_WORDS[d] = ErrorWord(d)
    return w


def poll_errors(device=None):
    """Raise a validation error some earlier libmgn launch flagged, if its copy-back has landed."""
    for d, w in list(_ERR_WORDS.items()):
        if device is None or torch.device(device) == d or torch.device(device).index is None:
            w.poll()


def check_errors(device=None):
    """Synchronise and raise any validation error libmgn flagged on the device word(s)."""
    for d, w in list(_ERR_WORDS.items()):
        if device is None or torch.device(device) == d or torch.device(device).index is None:
            w.check()


def require_device(t):
    if not t.is_cuda:
        raise RuntimeError("the MI355X MGN path needs tensors on a HIP device (no CPU fallback)")


def stream_ptr(device=None):
    return _vp(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device address of a tensor (None -> NULL; raw ints / c_void_p pass through)."""
    if t is None:
        return _vp(0)
    if isinstance(t, _vp):
        return t
    if isinstance(t, int):
        return _vp(t)
    return _vp(t.data_ptr())


def mgn_dtype(torch_dtype):
    if torch_dtype == torch.float32:
        return MGN_F32
    if torch_dtype == torch.bfloat16:
        return MGN_BF16
    raise ValueError(f"unsupported compute dtype {torch_dtype}")


def torch_dtype(mdt):
    return torch.float32 if mdt == MGN_F32 else torch.bfloat16


NODE_GRAD_AUTO, NODE_GRAD_GENERIC, NODE_GRAD_CHAINED = 0, 1, 2  # mgn_node_grad's impl


def node_grad(topo, edge, dz0, dx_part, dP8, dx, dx_pair=False, impl=NODE_GRAD_AUTO, data_cus=0):
    """mgn_node_grad: dP8 (R8 [2][rows padded to 64][h]: the segment sums of dz0 over in- and out-edges) and
    dx = dx_part + dP_i·W0b + dP_j·W0c, written in place. topo: a Topology struct, edge: the edge MLP's Mlp
    struct (its wtpack), the tensors contiguous and of the MLP's dtype; data_cus: the call's CU cap (0: none)."""
    require_device(dx)
    opts = CallOpts(int(data_cus), 0, None)
    check(lib().mgn_node_grad(ctypes.byref(topo), ctypes.byref(edge), ptr(dz0), ptr(dx_part), ptr(dP8), ptr(dx),
                              int(bool(dx_pair)), int(impl), ctypes.byref(opts), stream_ptr(dx.device)))


def column_stats(x):
    """(Σ_rows x, Σ_rows x²) of a 2-D fp32 HIP tensor as two [1, cols] tensors (mgn_column_stats)."""
    import torch

    require_device(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        x = x.float().contiguous()
    rows, cols = x.shape
    out = torch.empty(2 * cols, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(lib().mgn_column_stats_workspace_bytes(rows, cols)), 4), dtype=torch.uint8,
                     device=x.device)
    check(lib().mgn_column_stats(ptr(x), rows, cols, x.stride(0), ptr(out), ptr(ws), ws.numel(),
                                 stream_ptr(x.device)))
    return out[:cols].view(1, cols), out[cols:].view(1, cols)


def normalizer_state(n, accumulate):
    """mgn_normalizer_state of a graphphysics Normalizer module (buffers updated in place)."""
    pend = n._pending_packed if accumulate else None
    return NormalizerState(n._acc_sum.data_ptr(), n._acc_sum_squared.data_ptr(), n._acc_count.data_ptr(),
                           n._num_accumulations.data_ptr(), pend.data_ptr() if pend is not None else None,
                           float(n._max_accumulations), n._eps())


def simulator_preamble(x, y, edge_attr, feat, out, type_index, n_types, accumulate, out_norm, node_norm,
                       edge_norm):
    """Simulator._build_input_graph's three Normalizer.forward calls on libmgn
    (mgn_simulator_preamble): returns (target_normalized [N, out], node_features_normalized
    [N, nf + n_types], edge_attr_normalized [E, de] or None)."""
    import torch

    require_device(x)
    N, E = x.shape[0], (edge_attr.shape[0] if edge_norm is not None else 0)
    dev = x.device
    to = torch.empty((N, out[1] - out[0]), dtype=torch.float32, device=dev)
    no = torch.empty((N, feat[1] - feat[0] + n_types), dtype=torch.float32, device=dev)
    eo = torch.empty((E, edge_attr.shape[1]), dtype=torch.float32, device=dev) if edge_norm is not None else None
    ws = torch.empty(int(lib().mgn_simulator_preamble_workspace_bytes(N, E)), dtype=torch.uint8, device=dev)
    acc = bool(accumulate)
    st = [normalizer_state(n, acc) if n is not None else None for n in (out_norm, node_norm, edge_norm)]
    check(lib().mgn_simulator_preamble(
        ptr(x), N, x.stride(0), feat[0], feat[1], type_index, n_types, out[0], out[1], ptr(y), y.stride(0),
        ptr(edge_attr) if eo is not None else None, E, edge_attr.shape[1] if eo is not None else 0,
        edge_attr.stride(0) if eo is not None else 0, int(acc), ctypes.byref(st[0]), ctypes.byref(st[1]),
        ctypes.byref(st[2]) if st[2] is not None else None, ptr(to), ptr(no), ptr(eo), error_word(dev).ptr(),
        ptr(ws), ws.numel(), stream_ptr(dev)))
    error_word(dev).arm()
    return to, no, eo


def simulator_statistics(x, y, edge_attr, feat, out, type_index, n_types, packed):
    """Batch statistics of the Simulator's three normalizers into `packed` (mgn_simulator_statistics);
    edge_attr None: two normalizers."""
    import torch

    require_device(x)
    N = x.shape[0]
    E = edge_attr.shape[0] if edge_attr is not None else 0
    ws = torch.empty(int(lib().mgn_simulator_preamble_workspace_bytes(N, E)), dtype=torch.uint8, device=x.device)
    check(lib().mgn_simulator_statistics(
        ptr(x), N, x.stride(0), feat[0], feat[1], type_index, n_types, out[0], out[1], ptr(y), y.stride(0),
        ptr(edge_attr), E, edge_attr.shape[1] if edge_attr is not None else 0,
        edge_attr.stride(0) if edge_attr is not None else 0, ptr(packed), error_word(x.device).ptr(), ptr(ws),
        ws.numel(), stream_ptr(x.device)))
    error_word(x.device).arm()
    return packed


def normalizer_forward(x, accumulate, pending, acc_sum, acc_sum_sq, acc_count, num_acc, max_acc, eps):
    """Normalizer.forward on libmgn (mgn_normalizer_forward): updates the fp32 buffers in place when
    accumulating and returns (x - mean) / std as a new contiguous fp32 tensor. pending: None or a
    float32 [2*cols + 1] device tensor {Σx, Σx², count}."""
    import torch

    require_device(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        x = x.float().contiguous()
    rows, cols = x.shape
    out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(lib().mgn_normalizer_workspace_bytes(rows, cols)), 4), dtype=torch.uint8,
                     device=x.device)
    check(lib().mgn_normalizer_forward(ptr(x), rows, cols, x.stride(0), int(bool(accumulate)),
                                       ptr(pending) if pending is not None else None, ptr(acc_sum),
                                       ptr(acc_sum_sq), ptr(acc_count), ptr(num_acc), float(max_acc),
                                       float(eps), ptr(out), ptr(ws), ws.numel(), stream_ptr(x.device)))
    return out


def feed_ranges(ranges):
    """mgn_feed_ranges of [(start, end), ...] (at most MGN_FEED_MAX_RANGES; the library checks the values)."""
    ranges = list(ranges)
    if len(ranges) > MGN_FEED_MAX_RANGES:
        raise ValueError(f"at most {MGN_FEED_MAX_RANGES} noisy column ranges, got {len(ranges)}")
    r = FeedRanges()
    r.n = len(ranges)
    for i, (s, e) in enumerate(ranges):
        r.start[i], r.end[i] = int(s), int(e)
    return r


def feed_batch(traj, graph_ptr, frame, y_columns, type_index, ranges, scales, z, x, y, triples=None, R=None):
    """One training batch from resident trajectories (mgn_feed_batch): x[:, :F] = frame[g] of traj [T, N, F]
    for the nodes of graph g, plus z * scales on the noisy column ranges of NORMAL rows; y = columns
    y_columns of the next clean frame. graph_ptr / frame: int32 device tensors [B+1] / [B]; z None: no
    noise. Writes x and y in place (x may be wider than F) on the current stream. triples (column triples
    [(s, s + 3), ...] or a FeedRanges) and R (fp32 [B, 9]): mgn_feed_batch_rot, the triples of x and y rotated
    by R[g] ahead of the noise."""
    import torch

    require_device(traj)
    if triples is not None and (triples.n if isinstance(triples, FeedRanges) else len(triples)) > 0:
        if R is None or R.dtype != torch.float32 or not R.is_contiguous() or R.device != traj.device or \
                tuple(R.shape) != (frame.numel(), 9):
            raise ValueError(f"feed_batch: R must be a contiguous fp32 [{frame.numel()}, 9] tensor on traj's device")
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError("feed_batch: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    for name, t, rows in (("x", x, N), ("y", y, N), ("z", z, N)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or
                              (t.shape[1] > 1 and t.stride(1) != 1) or t.device != traj.device):
            raise ValueError(f"feed_batch: {name} must be an fp32 [{rows}, cols] tensor on traj's device with "
                             "unit column stride")
    if graph_ptr.dtype != torch.int32 or frame.dtype != torch.int32 or graph_ptr.numel() != frame.numel() + 1:
        raise ValueError("feed_batch: graph_ptr [B+1] and frame [B] must be int32 tensors")
    if x.shape[1] < F or y.shape[1] != y_columns[1] - y_columns[0]:
        raise ValueError("feed_batch: x needs at least F columns and y exactly y_columns[1] - y_columns[0]")
    rg = ranges if isinstance(ranges, FeedRanges) else feed_ranges(ranges)
    args = (ptr(traj), T, N, F, ptr(graph_ptr), frame.numel(), ptr(frame), int(y_columns[0]), int(y_columns[1]),
            int(type_index), rg, ptr(scales), ptr(z), z.stride(0) if z is not None else 0, ptr(x), x.stride(0),
            ptr(y), y.stride(0))
    if triples is None:
        check(lib().mgn_feed_batch(*args, stream_ptr(traj.device)))
    else:
        tr = triples if isinstance(triples, FeedRanges) else feed_ranges(triples)
        check(lib().mgn_feed_batch_rot(*args, tr, ptr(R), stream_ptr(traj.device)))


def feed_rotation_matrices(angles, R):
    """R[g] = the reference's _build_rotation_matrix(*angles[g]) in fp32, row-major (mgn_feed_rotation_matrices).
    angles fp32 [B, 3] in radians {alpha (z), beta (y), gamma (x)}, R fp32 [B, 9], both contiguous on one HIP
    device; written in place on the current stream."""
    import torch

    require_device(angles)
    B = angles.shape[0]
    ok = angles.dtype == torch.float32 and R.dtype == torch.float32 and tuple(angles.shape) == (B, 3) and \
        tuple(R.shape) == (B, 9) and angles.is_contiguous() and R.is_contiguous() and R.device == angles.device
    if not ok:
        raise ValueError("feed_rotation_matrices: angles [B, 3] and R [B, 9] must be contiguous fp32 tensors on one "
                         "device")
    check(lib().mgn_feed_rotation_matrices(ptr(angles), B, ptr(R), stream_ptr(angles.device)))


def feed_rotate_rows(src, row_graph, triples, R, dst):
    """dst[:, :cols] = the rows of src [rows, cols] with the column triples rotated by R[row_graph[r]]
    (mgn_feed_rotate_rows); other columns, and rows whose graph id is outside [0, B), are copied. dst may be
    wider than src; src and dst must not overlap. On the current stream."""
    import torch

    require_device(src)
    rows, cols = src.shape
    for name, t in (("src", src), ("dst", dst)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or t.device != src.device or \
                (t.shape[1] > 1 and t.stride(1) != 1) or t.shape[1] < cols:
            raise ValueError(f"feed_rotate_rows: {name} must be an fp32 [{rows}, >= {cols}] tensor on src's device "
                             "with unit column stride")
    if row_graph.dtype != torch.int32 or row_graph.numel() != rows or not row_graph.is_contiguous() or \
            row_graph.device != src.device:
        raise ValueError(f"feed_rotate_rows: row_graph must be a contiguous int32 tensor of {rows} elements")
    if R.dtype != torch.float32 or R.dim() != 2 or R.shape[1] != 9 or not R.is_contiguous() or R.device != src.device:
        raise ValueError("feed_rotate_rows: R must be a contiguous fp32 [B, 9] tensor on src's device")
    tr = triples if isinstance(triples, FeedRanges) else feed_ranges(triples)
    check(lib().mgn_feed_rotate_rows(ptr(src), rows, cols, src.stride(0), ptr(row_graph), R.shape[0], tr, ptr(R),
                                     ptr(dst), dst.stride(0), stream_ptr(src.device)))


def feed_batch_world(traj, graph_ptr, frame, y_columns, type_index, ranges, scales, z, x, y, obstacle_mean):
    """One Lagrangian training batch from resident trajectories (mgn_feed_batch_world): x[:, :F + 3] =
    [world(3), obstacle displacement(3), the other columns] of frame[g] of traj [T, N, F], y = y_columns of the
    next clean frame, obstacle_mean [B, 3] = the per-graph mean displacement of the OBSTACLE rows. type_index is
    the node-type column of a frame row; ranges are noisy columns of the batch row. Writes x, y and obstacle_mean
    in place on the current stream."""
    import torch

    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError("feed_batch_world: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    for name, t, rows in (("x", x, N), ("y", y, N), ("z", z, N)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or
                              (t.shape[1] > 1 and t.stride(1) != 1) or t.device != traj.device):
            raise ValueError(f"feed_batch_world: {name} must be an fp32 [{rows}, cols] tensor on traj's device with "
                             "unit column stride")
    if graph_ptr.dtype != torch.int32 or frame.dtype != torch.int32 or graph_ptr.numel() != frame.numel() + 1:
        raise ValueError("feed_batch_world: graph_ptr [B+1] and frame [B] must be int32 tensors")
    if x.shape[1] < F + 3 or y.shape[1] != y_columns[1] - y_columns[0]:
        raise ValueError("feed_batch_world: x needs at least F + 3 columns and y exactly y_columns[1] - y_columns[0]")
    m = obstacle_mean
    if m.dtype != torch.float32 or tuple(m.shape) != (frame.numel(), 3) or not m.is_contiguous() or \
            m.device != traj.device:
        raise ValueError(f"feed_batch_world: obstacle_mean must be a contiguous fp32 [{frame.numel()}, 3] tensor on "
                         "traj's device")
    rg = ranges if isinstance(ranges, FeedRanges) else feed_ranges(ranges)
    check(lib().mgn_feed_batch_world(ptr(traj), T, N, F, ptr(graph_ptr), frame.numel(), ptr(frame), int(y_columns[0]),
                                     int(y_columns[1]), int(type_index), rg, ptr(scales), ptr(z),
                                     z.stride(0) if z is not None else 0, ptr(x), x.stride(0), ptr(y), y.stride(0),
                                     ptr(m), stream_ptr(traj.device)))


def feed_world_edge_features(senders, receivers, x, edge_attr, start):
    """edge_attr[:, start:start + 4] = [x[senders, 0:3] - x[receivers, 0:3] ‖ its norm]
    (mgn_feed_world_edge_features); other columns of edge_attr are not touched. senders / receivers: contiguous
    int32 [E] with node ids inside [0, rows of x) — the caller's precondition, not checked here. On the current
    stream."""
    import torch

    require_device(x)
    E = senders.numel()
    for name, t in (("senders", senders), ("receivers", receivers)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != E or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"feed_world_edge_features: {name} must be a contiguous int32 [{E}] tensor on x's device")
    for name, t, rows, cols in (("x", x, x.shape[0], 3), ("edge_attr", edge_attr, E, int(start) + 4)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or \
                t.stride(1) != 1 or t.device != x.device:
            raise ValueError(f"feed_world_edge_features: {name} must be an fp32 [{rows}, >= {cols}] tensor on x's "
                             "device with unit column stride")
    check(lib().mgn_feed_world_edge_features(ptr(senders), ptr(receivers), E, ptr(x), x.stride(0), ptr(edge_attr),
                                             edge_attr.stride(0), int(start), stream_ptr(x.device)))


def world_topology_workspace(N, max_neighbors, device):
    """The scratch of one mgn_world_topology_build over N nodes (uint8, caller-kept)."""
    import torch

    return torch.empty(max(int(lib().mgn_world_topology_workspace_bytes(int(N), int(max_neighbors))), 1),
                       dtype=torch.uint8, device=device)


def world_topology_build(pos, node_type, graph_ptr, mesh_ptr, mesh_nbr, radius, max_neighbors, csc_src, csc_dst,
                         csc_eid, col_ptr, row_ptr, row_perm, edge_index, num_edges, ws):
    """The topology of mesh edges ∪ OBSTACLE–NORMAL pairs within `radius`, per graph (mgn_world_topology_build):
    pos fp32 [N, >= 3] with unit column stride, node_type an fp32 [N] view of any stride (a column of x), graph_ptr
    int32 [B + 1], mesh_ptr int32 [N + 1] / mesh_nbr int32 [E_m] the static adjacency as CSR. Writes the six arrays
    ([E_cap] and [N + 1] int32, E_cap = E_m + N · max_neighbors), edge_index int64 [2, E_cap] and num_edges int32
    [1] in place on the current stream; a node over capacity flags the device error word (ValueError at the next
    poll). Nothing is read back."""
    import torch

    require_device(pos)
    dev, N, E_m, W = pos.device, pos.shape[0], mesh_nbr.numel(), int(max_neighbors)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] < 3 or pos.stride(1) != 1:
        raise ValueError("world_topology_build: pos must be an fp32 [N, >= 3] tensor with unit column stride")
    t = node_type
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != N or t.device != dev or (N > 1 and t.stride(0) < 1):
        raise ValueError(f"world_topology_build: node_type must be an fp32 [{N}] tensor (a view of any positive "
                         "stride) on pos's device")
    if W < 1:
        raise ValueError(f"world_topology_build: max_neighbors {W} must be >= 1")
    if not float(radius) > 0.0 or float(radius) == float("inf"):
        raise ValueError(f"world_topology_build: radius {radius} must be positive and finite")
    E_cap = E_m + N * W
    for name, a, n in (("graph_ptr", graph_ptr, None), ("mesh_ptr", mesh_ptr, N + 1), ("mesh_nbr", mesh_nbr, E_m),
                       ("csc_src", csc_src, max(E_cap, 1)), ("csc_dst", csc_dst, max(E_cap, 1)),
                       ("csc_eid", csc_eid, max(E_cap, 1)), ("row_perm", row_perm, max(E_cap, 1)),
                       ("col_ptr", col_ptr, N + 1), ("row_ptr", row_ptr, N + 1), ("num_edges", num_edges, 1)):
        if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous() or a.device != dev or \
                (n is not None and a.numel() != n):
            raise ValueError(f"world_topology_build: {name} must be a contiguous int32 "
                             f"[{'B + 1' if n is None else n}] tensor on pos's device")
    if graph_ptr.numel() < 1 or (N > 0 and graph_ptr.numel() < 2):
        raise ValueError("world_topology_build: graph_ptr must hold B + 1 node offsets")
    ei = edge_index
    if ei.dtype != torch.int64 or tuple(ei.shape) != (2, max(E_cap, 1)) or not ei.is_contiguous() or ei.device != dev:
        raise ValueError(f"world_topology_build: edge_index must be a contiguous int64 [2, {max(E_cap, 1)}] tensor on "
                         "pos's device")
    wsb = int(lib().mgn_world_topology_workspace_bytes(N, W))
    if ws.dtype != torch.uint8 or ws.numel() < wsb or ws.device != dev:
        raise ValueError(f"world_topology_build: ws must hold {wsb} bytes on pos's device")
    ew = error_word(dev)
    check(lib().mgn_world_topology_build(
        ptr(pos), pos.stride(0) if N > 1 else max(pos.stride(0), 3), ptr(t), t.stride(0) if N > 1 else 1,
        ptr(graph_ptr), graph_ptr.numel() - 1, N, ptr(mesh_ptr), ptr(mesh_nbr), E_m, float(radius), W, ptr(csc_src),
        ptr(csc_dst), ptr(csc_eid), ptr(col_ptr), ptr(row_ptr), ptr(row_perm), ptr(ei), ptr(num_edges), ew.ptr(),
        ptr(ws), ws.numel(), stream_ptr(dev)))
    ew.arm()


RANDOM_MAX_NEW = 64  # mgn.h: the largest max_new of mgn_random_topology_build


def random_topology_workspace(N, max_new, num_candidates, device):
    """The scratch of one mgn_random_topology_build over N nodes and num_candidates pairs (uint8, caller-kept)."""
    import torch

    n = lib().mgn_random_topology_workspace_bytes(int(N), int(max_new), int(num_candidates))
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=device)


def random_topology_build(pairs, cand_ptr, graph_ptr, mesh_ptr, mesh_nbr, max_new, enabled, csc_src, csc_dst, csc_eid,
                          col_ptr, row_ptr, row_perm, edge_index, num_edges, ws):
    """The topology of mesh edges ∪ the surviving random pairs of `pairs` (mgn_random_topology_build; the rule:
    dataset.resident.random_topology_torch): pairs int32 [C, 2] of non-negative draws, cand_ptr int32 [B + 1] the
    candidate offsets of every graph (from 0 to C, non-decreasing: the caller built it on the host), graph_ptr int32
    [B + 1], mesh_ptr int32 [N + 1] / mesh_nbr int32 [E_m] the static adjacency as CSR, enabled int32 [1] (0: the mesh
    alone). Writes the six arrays ([E_cap] and [N + 1] int32, E_cap = E_m + N · max_new), edge_index int64 [2, E_cap]
    and num_edges int32 [1] in place on the current stream. Nothing is read back and no error bit is set: a node over
    capacity drops candidates."""
    import torch

    require_device(pairs)
    dev, N, E_m, W = pairs.device, mesh_ptr.numel() - 1, mesh_nbr.numel(), int(max_new)
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise ValueError("random_topology_build: pairs must be a contiguous int32 [C, 2] tensor")
    C = pairs.shape[0]
    if not 1 <= W <= RANDOM_MAX_NEW:
        raise ValueError(f"random_topology_build: max_new {W} must lie in [1, {RANDOM_MAX_NEW}]")
    E_cap = E_m + N * W
    B1 = graph_ptr.numel()
    for name, a, n in (("graph_ptr", graph_ptr, None), ("cand_ptr", cand_ptr, B1), ("mesh_ptr", mesh_ptr, N + 1),
                       ("mesh_nbr", mesh_nbr, E_m), ("enabled", enabled, 1),
                       ("csc_src", csc_src, max(E_cap, 1)), ("csc_dst", csc_dst, max(E_cap, 1)),
                       ("csc_eid", csc_eid, max(E_cap, 1)), ("row_perm", row_perm, max(E_cap, 1)),
                       ("col_ptr", col_ptr, N + 1), ("row_ptr", row_ptr, N + 1), ("num_edges", num_edges, 1)):
        if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous() or a.device != dev or \
                (n is not None and a.numel() != n):
            raise ValueError(f"random_topology_build: {name} must be a contiguous int32 "
                             f"[{'B + 1' if n is None else n}] tensor on pairs' device")
    if B1 < 1 or (N > 0 and B1 < 2):
        raise ValueError("random_topology_build: graph_ptr must hold B + 1 node offsets")
    ei = edge_index
    if ei.dtype != torch.int64 or tuple(ei.shape) != (2, max(E_cap, 1)) or not ei.is_contiguous() or ei.device != dev:
        raise ValueError(f"random_topology_build: edge_index must be a contiguous int64 [2, {max(E_cap, 1)}] tensor on "
                         "pairs' device")
    wsb = int(lib().mgn_random_topology_workspace_bytes(N, W, C))
    if ws.dtype != torch.uint8 or ws.numel() < wsb or ws.device != dev:
        raise ValueError(f"random_topology_build: ws must hold {wsb} bytes on pairs' device")
    check(lib().mgn_random_topology_build(
        ptr(pairs), ptr(cand_ptr), C, ptr(graph_ptr), B1 - 1, N, ptr(mesh_ptr), ptr(mesh_nbr), E_m, W, ptr(enabled),
        ptr(csc_src), ptr(csc_dst), ptr(csc_eid), ptr(col_ptr), ptr(row_ptr), ptr(row_perm), ptr(ei), ptr(num_edges),
        ptr(ws), ws.numel(), stream_ptr(dev)))


def world_random_topology_workspace(N, max_neighbors, max_new, num_candidates, device):
    """The scratch of one mgn_world_random_topology_build over N nodes and num_candidates pairs (uint8, caller-kept)."""
    import torch

    n = lib().mgn_world_random_topology_workspace_bytes(int(N), int(max_neighbors), int(max_new), int(num_candidates))
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=device)


def world_random_topology_build(pos, node_type, pairs, cand_ptr, graph_ptr, mesh_ptr, mesh_nbr, radius, max_neighbors,
                                max_new, enabled, csc_src, csc_dst, csc_eid, col_ptr, row_ptr, row_perm, edge_index,
                                num_edges, ws):
    """The topology of mesh edges ∪ OBSTACLE–NORMAL pairs within `radius` ∪ the surviving random pairs of `pairs`
    (mgn_world_random_topology_build; the rule: dataset.resident.world_random_topology_torch): the arguments of
    world_topology_build and random_topology_build together, E_cap = E_m + N · (max_neighbors + max_new). Writes the
    six arrays, edge_index int64 [2, E_cap] and num_edges int32 [1] in place on the current stream; a node over
    max_neighbors flags the device error word (ValueError at the next poll), a node over max_new drops candidates.
    Nothing is read back."""
    import torch

    require_device(pos)
    dev, N, E_m, W, R = pos.device, pos.shape[0], mesh_nbr.numel(), int(max_neighbors), int(max_new)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] < 3 or pos.stride(1) != 1:
        raise ValueError("world_random_topology_build: pos must be an fp32 [N, >= 3] tensor with unit column stride")
    t = node_type
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != N or t.device != dev or (N > 1 and t.stride(0) < 1):
        raise ValueError(f"world_random_topology_build: node_type must be an fp32 [{N}] tensor (a view of any positive "
                         "stride) on pos's device")
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous() or \
            pairs.device != dev:
        raise ValueError("world_random_topology_build: pairs must be a contiguous int32 [C, 2] tensor on pos's device")
    C = pairs.shape[0]
    if W < 1:
        raise ValueError(f"world_random_topology_build: max_neighbors {W} must be >= 1")
    if not 1 <= R <= RANDOM_MAX_NEW:
        raise ValueError(f"world_random_topology_build: max_new {R} must lie in [1, {RANDOM_MAX_NEW}]")
    if not float(radius) > 0.0 or float(radius) == float("inf"):
        raise ValueError(f"world_random_topology_build: radius {radius} must be positive and finite")
    E_cap = E_m + N * (W + R)
    B1 = graph_ptr.numel()
    for name, a, n in (("graph_ptr", graph_ptr, None), ("cand_ptr", cand_ptr, B1), ("mesh_ptr", mesh_ptr, N + 1),
                       ("mesh_nbr", mesh_nbr, E_m), ("enabled", enabled, 1),
                       ("csc_src", csc_src, max(E_cap, 1)), ("csc_dst", csc_dst, max(E_cap, 1)),
                       ("csc_eid", csc_eid, max(E_cap, 1)), ("row_perm", row_perm, max(E_cap, 1)),
                       ("col_ptr", col_ptr, N + 1), ("row_ptr", row_ptr, N + 1), ("num_edges", num_edges, 1)):
        if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous() or a.device != dev or \
                (n is not None and a.numel() != n):
            raise ValueError(f"world_random_topology_build: {name} must be a contiguous int32 "
                             f"[{'B + 1' if n is None else n}] tensor on pos's device")
    if B1 < 1 or (N > 0 and B1 < 2):
        raise ValueError("world_random_topology_build: graph_ptr must hold B + 1 node offsets")
    ei = edge_index
    if ei.dtype != torch.int64 or tuple(ei.shape) != (2, max(E_cap, 1)) or not ei.is_contiguous() or ei.device != dev:
        raise ValueError(f"world_random_topology_build: edge_index must be a contiguous int64 [2, {max(E_cap, 1)}] "
                         "tensor on pos's device")
    wsb = int(lib().mgn_world_random_topology_workspace_bytes(N, W, R, C))
    if ws.dtype != torch.uint8 or ws.numel() < wsb or ws.device != dev:
        raise ValueError(f"world_random_topology_build: ws must hold {wsb} bytes on pos's device")
    ew = error_word(dev)
    check(lib().mgn_world_random_topology_build(
        ptr(pos), pos.stride(0) if N > 1 else max(pos.stride(0), 3), ptr(t), t.stride(0) if N > 1 else 1, ptr(pairs),
        ptr(cand_ptr), C, ptr(graph_ptr), B1 - 1, N, ptr(mesh_ptr), ptr(mesh_nbr), E_m, float(radius), W, R,
        ptr(enabled), ptr(csc_src), ptr(csc_dst), ptr(csc_eid), ptr(col_ptr), ptr(row_ptr), ptr(row_perm), ptr(ei),
        ptr(num_edges), ew.ptr(), ptr(ws), ws.numel(), stream_ptr(dev)))
    ew.arm()


def feed_ranges8(ranges):
    """mgn_feed_ranges8 of [(start, end), ...] (at most MGN_FEED_ANEURYSM_MAX_RANGES; the library checks the values)."""
    ranges = list(ranges)
    if len(ranges) > MGN_FEED_ANEURYSM_MAX_RANGES:
        raise ValueError(f"at most {MGN_FEED_ANEURYSM_MAX_RANGES} noisy column ranges, got {len(ranges)}")
    r = FeedRanges8()
    r.n = len(ranges)
    for i, (s, e) in enumerate(ranges):
        r.start[i], r.end[i] = int(s), int(e)
    return r


def feed_inflow_stats(traj, graph_ptr, inflow_ptr, inflow_rows, max_values, stats):
    """stats[t, g] = (mean, min, max) of the distinct next-frame accelerations on the inflow rows of graph g, for
    every frame t with a successor (mgn_feed_inflow_stats; the rule: dataset.resident.inflow_stats_torch).
    graph_ptr / inflow_ptr: int32 [B + 1] device tensors, inflow_rows: int32 rows of the batch grouped by graph,
    max_values: the largest value-set size over the graphs (host int), stats: contiguous fp32 [T - 1, B, 3], written
    in place on the current stream."""
    import torch

    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError("feed_inflow_stats: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    B = graph_ptr.numel() - 1
    for name, t, n in (("graph_ptr", graph_ptr, B + 1), ("inflow_ptr", inflow_ptr, B + 1),
                       ("inflow_rows", inflow_rows, None)):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != traj.device or \
                (n is not None and t.numel() != n):
            raise ValueError(f"feed_inflow_stats: {name} must be a contiguous int32 tensor on traj's device"
                             + (f" of {n} elements" if n is not None else ""))
    if stats.dtype != torch.float32 or tuple(stats.shape) != (T - 1, B, 3) or not stats.is_contiguous() or \
            stats.device != traj.device:
        raise ValueError(f"feed_inflow_stats: stats must be a contiguous fp32 [{T - 1}, {B}, 3] tensor on traj's "
                         "device")
    check(lib().mgn_feed_inflow_stats(ptr(traj), T, N, F, ptr(graph_ptr), B, ptr(inflow_ptr), ptr(inflow_rows),
                                      int(max_values), ptr(stats), stream_ptr(traj.device)))


def feed_batch_aneurysm(traj, graph_ptr, frame, y_columns, pos, node_type, stats, ranges, scales, z, x, y):
    """One aneurysm training batch from resident trajectories (mgn_feed_batch_aneurysm): x[:, :F + 10] = [frame row ‖
    a − p ‖ pos ‖ mean, min, max ‖ node type] of frame[g] of traj [T, N, F], plus z * scales on the noisy ranges
    (batch-layout columns) of the rows with node_type == 0; y = y_columns of the next clean frame. pos fp32 [N, 3],
    node_type fp32 [N], stats fp32 [T - 1, B, 3] (feed_inflow_stats), all contiguous. Writes x and y in place on the
    current stream."""
    import torch

    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError("feed_batch_aneurysm: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    B = frame.numel()
    for name, t, rows in (("x", x, N), ("y", y, N), ("z", z, N)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or
                              (t.shape[1] > 1 and t.stride(1) != 1) or t.device != traj.device):
            raise ValueError(f"feed_batch_aneurysm: {name} must be an fp32 [{rows}, cols] tensor on traj's device "
                             "with unit column stride")
    if graph_ptr.dtype != torch.int32 or frame.dtype != torch.int32 or graph_ptr.numel() != B + 1:
        raise ValueError("feed_batch_aneurysm: graph_ptr [B+1] and frame [B] must be int32 tensors")
    if x.shape[1] < F + 10 or y.shape[1] != y_columns[1] - y_columns[0]:
        raise ValueError("feed_batch_aneurysm: x needs at least F + 10 columns and y exactly y_columns[1] - "
                         "y_columns[0]")
    for name, t, shape in (("pos", pos, (N, 3)), ("node_type", node_type, (N,)), ("stats", stats, (T - 1, B, 3))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != traj.device:
            raise ValueError(f"feed_batch_aneurysm: {name} must be a contiguous fp32 {list(shape)} tensor on traj's "
                             "device")
    rg = ranges if isinstance(ranges, FeedRanges8) else feed_ranges8(ranges)
    check(lib().mgn_feed_batch_aneurysm(ptr(traj), T, N, F, ptr(graph_ptr), B, ptr(frame), int(y_columns[0]),
                                        int(y_columns[1]), ptr(pos), ptr(node_type), ptr(stats), rg, ptr(scales),
                                        ptr(z), z.stride(0) if z is not None else 0, ptr(x), x.stride(0), ptr(y),
                                        y.stride(0), stream_ptr(traj.device)))


def _rollout_2d(fn, name, t, rows, dev, cols=None):
    import torch

    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or t.device != dev or \
            (t.shape[1] > 1 and t.stride(1) != 1) or (cols is not None and t.shape[1] != cols):
        want = "cols" if cols is None else str(cols)
        raise ValueError(f"{fn}: {name} must be an fp32 [{rows}, {want}] tensor on {dev} with unit column stride")


def rollout_begin(traj, graph_ptr, frame, cursor, y_columns, out_columns, prev_columns, last, last_prev, x, y):
    """Step s = cursor of a resident rollout, before the forward (mgn_rollout_begin): x[:, :F] = frame[g] + s of
    traj [T, N, F] for the nodes of graph g, with `last` in out_columns and `last_prev` in prev_columns when
    s > 0; y = y_columns of the next frame. prev_columns None (or empty): no previous data. cursor: int32 device
    tensor of one element. Writes x and y in place (x may be wider than F) on the current stream."""
    import torch

    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError("rollout_begin: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    (ys, ye), (os_, oe) = (int(v) for v in y_columns), (int(v) for v in out_columns)
    ps, pe = (int(v) for v in prev_columns) if prev_columns is not None else (0, 0)
    _rollout_2d("rollout_begin", "x", x, N, traj.device)
    _rollout_2d("rollout_begin", "y", y, N, traj.device, ye - ys)
    _rollout_2d("rollout_begin", "last", last, N, traj.device, oe - os_)
    if pe > ps:
        if last_prev is None:
            raise ValueError("rollout_begin: previous-data columns without last_prev")
        _rollout_2d("rollout_begin", "last_prev", last_prev, N, traj.device, pe - ps)
    for name, t, n in (("graph_ptr", graph_ptr, frame.numel() + 1), ("frame", frame, frame.numel()),
                       ("cursor", cursor, 1)):
        if t.dtype != torch.int32 or t.numel() != n or t.device != traj.device or not t.is_contiguous():
            raise ValueError(f"rollout_begin: {name} must be a contiguous int32 tensor of {n} elements on {traj.device}")
    if x.shape[1] < F:
        raise ValueError("rollout_begin: x needs at least F columns")
    check(lib().mgn_rollout_begin(ptr(traj), T, N, F, ptr(graph_ptr), frame.numel(), ptr(frame), ptr(cursor), ys, ye,
                                  os_, oe, ps, pe, ptr(last), last.stride(0), ptr(last_prev if pe > ps else None),
                                  last_prev.stride(0) if pe > ps else 0, ptr(x), x.stride(0), ptr(y), y.stride(0),
                                  stream_ptr(traj.device)))


def rollout_begin_world(traj, graph_ptr, frame, cursor, y_columns, type_index, out_columns, prev_columns, last,
                        last_prev, x, y, obstacle_mean, world_clean=None):
    """Step s = cursor of a resident rollout on Lagrangian data, before the forward (mgn_rollout_begin_world):
    x[:, :F + 3] = [world(3), obstacle displacement(3), the other columns] of frame[g] + s of traj [T, N, F],
    noise-free and bit for bit what feed_batch_world writes at that frame, then `last` in out_columns and
    `last_prev` in prev_columns (batch-layout columns) when s > 0; y = y_columns of the next frame;
    obstacle_mean [B, 3] = the per-graph mean displacement of the OBSTACLE rows; world_clean [N, 3] (None: not
    kept) = the clean world positions of the frame. type_index is the node-type column of a frame row.
    prev_columns None (or empty): no previous data. Writes in place on the current stream."""
    import torch

    fn = "rollout_begin_world"
    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError(f"{fn}: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    (ys, ye), (os_, oe) = (int(v) for v in y_columns), (int(v) for v in out_columns)
    ps, pe = (int(v) for v in prev_columns) if prev_columns is not None else (0, 0)
    _rollout_2d(fn, "x", x, N, traj.device)
    _rollout_2d(fn, "y", y, N, traj.device, ye - ys)
    _rollout_2d(fn, "last", last, N, traj.device, oe - os_)
    if pe > ps:
        if last_prev is None:
            raise ValueError(f"{fn}: previous-data columns without last_prev")
        _rollout_2d(fn, "last_prev", last_prev, N, traj.device, pe - ps)
    B = frame.numel()
    for name, t, n in (("graph_ptr", graph_ptr, B + 1), ("frame", frame, B), ("cursor", cursor, 1)):
        if t.dtype != torch.int32 or t.numel() != n or t.device != traj.device or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be a contiguous int32 tensor of {n} elements on {traj.device}")
    if x.shape[1] < F + 3:
        raise ValueError(f"{fn}: x needs at least F + 3 columns")
    for name, t, rows in (("obstacle_mean", obstacle_mean, B), ("world_clean", world_clean, N)):
        if t is None and name == "world_clean":  # optional
            continue
        if t is None or t.dtype != torch.float32 or tuple(t.shape) != (rows, 3) or not t.is_contiguous() or \
                t.device != traj.device:
            raise ValueError(f"{fn}: {name} must be a contiguous fp32 [{rows}, 3] tensor on {traj.device}")
    check(lib().mgn_rollout_begin_world(ptr(traj), T, N, F, ptr(graph_ptr), B, ptr(frame), ptr(cursor), ys, ye,
                                        int(type_index), os_, oe, ps, pe, ptr(last), last.stride(0),
                                        ptr(last_prev if pe > ps else None), last_prev.stride(0) if pe > ps else 0,
                                        ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(obstacle_mean),
                                        ptr(world_clean), stream_ptr(traj.device)))


def rollout_begin_aneurysm(traj, graph_ptr, frame, cursor, y_columns, pos, node_type, stats, out_columns,
                           prev_columns, last, last_prev, x, y):
    """Step s = cursor of a resident rollout on aneurysm data, before the forward (mgn_rollout_begin_aneurysm):
    x[:, :F + 10] = [frame row ‖ a − p ‖ pos ‖ mean, min, max ‖ node type] of frame[g] + s of traj [T, N, F],
    noise-free and bit for bit what feed_batch_aneurysm writes at that frame, then `last` in out_columns and
    `last_prev` in prev_columns (batch-layout columns) when s > 0; y = y_columns of the next frame. pos fp32 [N, 3],
    node_type fp32 [N], stats fp32 [T - 1, B, 3] (feed_inflow_stats), all contiguous and only read. prev_columns None
    (or empty): no previous data. Writes x and y in place on the current stream."""
    import torch

    fn = "rollout_begin_aneurysm"
    require_device(traj)
    if traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
        raise ValueError(f"{fn}: traj must be a contiguous fp32 [T, N, F] tensor")
    T, N, F = traj.shape
    (ys, ye), (os_, oe) = (int(v) for v in y_columns), (int(v) for v in out_columns)
    ps, pe = (int(v) for v in prev_columns) if prev_columns is not None else (0, 0)
    _rollout_2d(fn, "x", x, N, traj.device)
    _rollout_2d(fn, "y", y, N, traj.device, ye - ys)
    _rollout_2d(fn, "last", last, N, traj.device, oe - os_)
    if pe > ps:
        if last_prev is None:
            raise ValueError(f"{fn}: previous-data columns without last_prev")
        _rollout_2d(fn, "last_prev", last_prev, N, traj.device, pe - ps)
    B = frame.numel()
    for name, t, n in (("graph_ptr", graph_ptr, B + 1), ("frame", frame, B), ("cursor", cursor, 1)):
        if t.dtype != torch.int32 or t.numel() != n or t.device != traj.device or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be a contiguous int32 tensor of {n} elements on {traj.device}")
    if x.shape[1] < F + 10:
        raise ValueError(f"{fn}: x needs at least F + 10 columns")
    for name, t, shape in (("pos", pos, (N, 3)), ("node_type", node_type, (N,)), ("stats", stats, (T - 1, B, 3))):
        if t is None or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or \
                t.device != traj.device:
            raise ValueError(f"{fn}: {name} must be a contiguous fp32 {list(shape)} tensor on {traj.device}")
    check(lib().mgn_rollout_begin_aneurysm(ptr(traj), T, N, F, ptr(graph_ptr), B, ptr(frame), ptr(cursor), ys, ye,
                                           ptr(pos), ptr(node_type), ptr(stats), os_, oe, ps, pe, ptr(last),
                                           last.stride(0), ptr(last_prev if pe > ps else None),
                                           last_prev.stride(0) if pe > ps else 0, ptr(x), x.stride(0), ptr(y),
                                           y.stride(0), stream_ptr(traj.device)))


def rollout_end_workspace(N, device):
    import torch

    return torch.empty(int(lib().mgn_rollout_end_workspace_bytes(N)), dtype=torch.uint8, device=device)


def rollout_end(out, y, x, type_index, masks, out_start, last, last_prev, preds, cursor, loss, sq, ws=None):
    """Step s = cursor of a resident rollout, after the forward (mgn_rollout_end): pred = y where the node type
    x[:, type_index] is neither NORMAL nor OUTFLOW, else out; last = pred, last_prev = pred - x[:, out columns]
    (None: not kept), preds[s] = pred (None: not kept), loss[s] = masked_mse(y, pred, node type, masks),
    sq[s] = Σ (pred - y)², cursor += 1. out, y, last, last_prev: contiguous fp32 [N, d]; preds [capacity, N, d];
    loss, sq [capacity]. Everything in place on the current stream; ws: rollout_end_workspace(N, device) or None
    (allocated here)."""
    import torch

    require_device(out)
    dev = out.device
    if out.dim() != 2:
        raise ValueError("rollout_end: out must be an fp32 [N, d] tensor")
    N, d = out.shape
    for name, t in (("out", out), ("y", y), ("last", last), ("last_prev", last_prev)):
        if t is not None:
            _rollout_2d("rollout_end", name, t, N, dev, d)
            if not t.is_contiguous():
                raise ValueError(f"rollout_end: {name} must be contiguous")
    _rollout_2d("rollout_end", "x", x, N, dev)
    if loss.dtype != torch.float32 or sq.dtype != torch.float32 or loss.dim() != 1 or sq.shape != loss.shape or \
            loss.device != dev or sq.device != dev or not loss.is_contiguous() or not sq.is_contiguous():
        raise ValueError("rollout_end: loss and sq must be contiguous fp32 [capacity] tensors on out's device")
    capacity = loss.numel()
    if preds is not None and (preds.dtype != torch.float32 or tuple(preds.shape) != (capacity, N, d) or
                              preds.device != dev or not preds.is_contiguous()):
        raise ValueError(f"rollout_end: preds must be a contiguous fp32 [{capacity}, {N}, {d}] tensor on {dev}")
    if cursor.dtype != torch.int32 or cursor.numel() != 1 or cursor.device != dev:
        raise ValueError("rollout_end: cursor must be an int32 tensor of one element on out's device")
    if any(not 0 <= int(m) < 32 for m in masks):
        raise ValueError("rollout_end: loss mask node types must lie in [0, 32)")
    tmask = 0
    for m in masks:
        tmask |= 1 << int(m)
    if ws is None:
        ws = rollout_end_workspace(N, dev)
    check(lib().mgn_rollout_end(ptr(out), ptr(y), ptr(x), N, x.stride(0), int(type_index), tmask, int(out_start), d,
                                ptr(last), ptr(last_prev), ptr(preds), capacity, ptr(cursor), ptr(loss), ptr(sq),
                                ptr(ws), ws.numel(), stream_ptr(dev)))


def gated_mlp_row_tile():
    """Rows of one workgroup tile of the gated-MLP kernels (mgn_gated_mlp_row_tile)."""
    return int(lib().mgn_gated_mlp_row_tile())


def gated_mlp_blocks(rows, max_blocks=0):
    """Workgroups of the gated-MLP row-tile kernels for `rows` rows: min(tiles, a fixed cap, max_blocks when
    > 0); workgroup b takes the tiles b, b + blocks, ... (mgn_gated_mlp_blocks)."""
    return int(lib().mgn_gated_mlp_blocks(int(rows), int(max_blocks)))


def gated_mlp_desc(hidden, dtype, w1, b1, w2, b2, w3, b3, scale_a, scale_b, max_blocks=0):
    """mgn_gated_mlp over the fp32 master parameters (tensors, raw addresses or None); max_blocks > 0 caps the
    row-tile kernels' grid."""
    return GatedMlp(int(hidden), 3 * int(hidden), int(dtype), int(hidden), int(max_blocks), 0, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                    ptr(w3), ptr(b3), ptr(scale_a), ptr(scale_b))
