"""Drop-in EncodeProcessDecode and EncodeTransformDecode (reference graphphysics/models/processors.py:27-137,
140-277) on libmgn.

Constructor, attributes (.K, .d, .temperature, .hidden_size, .only_processor, .use_diagonal) and
state_dict keys (nodes_encoder.*, edges_encoder.*, decode_module.*, processor_list.{i}.*) match the
reference, and modules are created in the reference's order so torch.manual_seed gives the same
initial weights. forward(graph) runs encoders, the MP GraphNetBlocks and the decoder as one
autograd node on HIP kernels (gfx950). Its decoder is part of the fused engine plan, so the GMM
decoder heads are out of scope there (num_mixture_components must be 0); EncodeTransformDecode
builds the diagonal mixture head (DiagonalGMMHead) when num_mixture_components > 0.

Extra (optional) keyword: compute_dtype — torch.float32 (exact-fp32 MFMA, default) or
torch.bfloat16 (bf16 storage, fp32 accumulation); also settable via GRAPHPHYSICS_MGN_DTYPE.

EncodeTransformDecode (configs with "type": "transformer") is the reference's DGL branch: nodes_encoder,
Transformer blocks whose attention is masked by the mesh adjacency, decode_module; it reads no
edge_attr. The attention core runs on libmgn's graph-attention kernels; with dense="libmgn" (opt-in) the
dense half of every block, x + gated_mlp(norm2(x)), runs on libmgn's fused gated-MLP kernels. The
attention-side projections, the encoder and the decoder are torch ops.
"""
import torch
import torch.nn as nn

from graphphysics import _native as nat
from graphphysics.models import _engine
from graphphysics.models.layers import (ATTENTION_HEADS, ATTENTION_MAX_HIDDEN, DiagonalGMMHead, GraphNetBlock,
                                        Transformer, _autocast, build_mlp, check_dense, default_compute_dtype)


class EncodeProcessDecode(nn.Module):
    def __init__(self, message_passing_num: int, node_input_size: int, edge_input_size: int,
                 output_size: int, hidden_size: int = 128, only_processor: bool = False,
                 num_mixture_components: int = 0, temperature: float = None,
                 use_diagonal: bool = True, compute_dtype: torch.dtype = None):
        super().__init__()
        if num_mixture_components != 0:
            raise NotImplementedError("GMM decoder heads on EncodeProcessDecode are not implemented: its decoder is "
                                      "part of the fused engine plan (EncodeTransformDecode has the diagonal head)")
        self.only_processor = only_processor
        self.hidden_size = hidden_size
        self.use_diagonal = use_diagonal
        self.d = output_size
        self.K = num_mixture_components
        self.temperature = temperature
        self.message_passing_num = message_passing_num
        if not self.only_processor:
            self.nodes_encoder = build_mlp(node_input_size, hidden_size, hidden_size)
            self.edges_encoder = build_mlp(edge_input_size, hidden_size, hidden_size)
            self.decode_module = build_mlp(hidden_size, hidden_size, output_size, layer_norm=False)
        self.processor_list = nn.ModuleList(
            [GraphNetBlock(hidden_size=hidden_size) for _ in range(message_passing_num)])
        self.compute_dtype = compute_dtype or default_compute_dtype()
        self._plan = None
        _engine.flatten_parameters(self)

    # parameters live in one flat fp32 buffer; re-home them after .to()/.cuda()/.float()
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        _engine.flatten_parameters(self)
        self._plan = None
        for blk in self.processor_list:
            blk._plan = None
        return out

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        return self

    def _get_plan(self):
        if self._plan is None:
            mlps = [] if self.only_processor else [self.nodes_encoder, self.edges_encoder,
                                                   self.decode_module]
            # encoders read the raw features (columns not padded); the decoder reads the processor's
            # (zero-padded) hidden state: one hidden-wide block, so its input gradient has the padded width
            kblocks = [] if self.only_processor else [0, 0, 1]
            for blk in self.processor_list:
                mlps += [blk.edge_block, blk.node_block]
                kblocks += [3, 2]  # [e ‖ x_i ‖ x_j], [x ‖ aggr]: hidden-wide blocks
            self._plan = _engine.ModelPlan(self, mlps, kblocks)
        return self._plan

    def forward(self, graph) -> torch.Tensor:
        x, edge_attr, edge_index = graph.x, graph.edge_attr, graph.edge_index
        nat.require_device(x)
        topo = _engine.get_topology(edge_index, x.size(0))
        plan = self._get_plan()
        return _engine.EPDFunction.apply(plan, nat.mgn_dtype(self.compute_dtype), self.only_processor,
                                         torch.is_grad_enabled(), x, edge_attr, topo, *plan.params)


class EncodeTransformDecode(nn.Module):
    """Reference processors.py:140-277 (constructor, attributes, state_dict keys nodes_encoder.*,
    decode_module.*, processor_list.{i}.{attention.{q,k,v}_proj, attention.proj, norm1, norm2,
    gated_mlp}.*; modules created in the reference's order). forward(graph) reads graph.x and
    graph.edge_index (the adjacency the reference wraps in a DGL sparse matrix). On HIP tensors the
    attention core runs on libmgn (no fallback); on CPU tensors as a torch composition.

    compute_dtype (keyword / set_compute_dtype): torch.float32 — everything fp32; torch.bfloat16 — the
    Linear layers run as under torch.autocast(bfloat16), q, k, v, y and their gradients are bf16 for the
    kernels, norms, residuals and softmax are fp32, master weights and gradients fp32.

    dense (keyword / set_dense): "torch" (default) or "libmgn" — who runs x + gated_mlp(norm2(x)) of every
    block (layers.Transformer); parameters, state_dict keys and the flat buffer are the same either way.

    num_mixture_components = K > 0 (with use_diagonal=True and a temperature): decode_module is a
    DiagonalGMMHead and forward returns the mixture parameters [N, K(2·output_size+1)] in fp32 (its two
    Linears under the same autocast as the rest); train it with utils.loss.masked_gmm_nll, sample it with
    models.simulator.sample_gmm_diagonal (Simulator.forward does in evaluation mode). NotImplementedError:
    temperature=None (the reference builds such a model, but its first loss or sample fails on
    tensor * None) and use_diagonal=False (the reference's own training and evaluation paths always use
    the diagonal loss and sampler, so its full-covariance head cannot be trained there either)."""

    def __init__(self, message_passing_num: int, node_input_size: int, output_size: int, hidden_size: int = 128,
                 num_heads: int = 4, only_processor: bool = False, use_proj_bias: bool = True,
                 use_separate_proj_weight: bool = True, num_mixture_components: int = 0,
                 temperature: float = None, use_diagonal: bool = True, compute_dtype: torch.dtype = None,
                 dense: str = "torch"):
        super().__init__()
        self.dense = check_dense(dense)
        if num_mixture_components < 0:
            raise ValueError(f"num_mixture_components={num_mixture_components} must be >= 0")
        if num_mixture_components > 0 and temperature is None:
            raise NotImplementedError("a mixture head needs a temperature: the reference builds the model with "
                                      "temperature=None, but its loss and its sampler then fail on tensor * None")
        if num_mixture_components > 0 and not use_diagonal:
            raise NotImplementedError("the full-covariance GMMHead (use_diagonal=False) is not implemented: the "
                                      "reference trains and samples every mixture model with the diagonal loss "
                                      "and sampler, which do not fit its parameter layout")
        if num_heads not in ATTENTION_HEADS or not 1 <= hidden_size <= ATTENTION_MAX_HIDDEN \
                or hidden_size % num_heads != 0:
            raise ValueError(f"EncodeTransformDecode(hidden_size={hidden_size}, num_heads={num_heads}): libmgn's "
                             f"graph attention supports num_heads in {ATTENTION_HEADS}, hidden_size <= "
                             f"{ATTENTION_MAX_HIDDEN} and hidden_size divisible by num_heads")
        self.hidden_size = hidden_size
        self.only_processor = only_processor
        self.use_diagonal = use_diagonal
        self.d = output_size
        self.K = num_mixture_components
        self.temperature = temperature
        self.message_passing_num = message_passing_num
        self.compute_dtype = compute_dtype or default_compute_dtype()
        if not self.only_processor:
            self.nodes_encoder = build_mlp(node_input_size, hidden_size, hidden_size)
            if num_mixture_components == 0:
                self.decode_module = build_mlp(hidden_size, hidden_size, output_size, layer_norm=False)
            else:
                self.decode_module = DiagonalGMMHead(hidden_size, output_size, num_mixture_components, temperature)
        self.processor_list = nn.ModuleList(
            [Transformer(input_dim=hidden_size, output_dim=hidden_size, num_heads=num_heads,
                         use_proj_bias=use_proj_bias, use_separate_proj_weight=use_separate_proj_weight,
                         compute_dtype=self.compute_dtype, dense=self.dense)
             for _ in range(message_passing_num)])
        self._named = None
        _engine.flatten_parameters(self)

    # parameters live in one flat fp32 buffer (a shared q/k/v weight once); re-home them after .to()/.cuda()
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        _engine.flatten_parameters(self)
        self._named = None
        return out

    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        for blk in self.processor_list:
            blk.set_compute_dtype(dtype)
        return self

    def set_dense(self, dense):
        self.dense = check_dense(dense)
        for blk in self.processor_list:
            blk.set_dense(dense)
        return self

    def _run(self, graph) -> torch.Tensor:
        x, edge_index = graph.x, graph.edge_index
        with _autocast(self.compute_dtype, x):
            if not self.only_processor:
                x = self.nodes_encoder(x)
            for block in self.processor_list:
                x = block(x, edge_index)
            if not self.only_processor:
                x = self.decode_module(x)
        return x.to(graph.x.dtype) if x.dtype != graph.x.dtype else x

    def forward(self, graph, _flat: bool = True) -> torch.Tensor:
        if self._named is None:
            self._named = list(self.named_parameters())
        if not (_flat and torch.is_grad_enabled() and any(p.requires_grad for _, p in self._named)):
            return self._run(graph)
        # the parameters pass through one identity node whose backward lays their gradients out in one
        # flat buffer (module.parameters() order), as EncodeProcessDecode's backward does
        vals = _engine.FlatGradFunction.apply(*(p for _, p in self._named))
        return torch.func.functional_call(self, {n: v for (n, _), v in zip(self._named, vals)}, (graph,),
                                          {"_flat": False})
