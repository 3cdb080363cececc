"""Drop-in counterparts of reference graphphysics/models/layers.py for the MGN path.

Same class names, constructor signatures, attributes and state_dict keys as the reference
(RMSNorm layers.py:18-74, build_mlp 77-113, GatedMLP / build_gated_mlp 198-262, Normalizer 265-392,
scaled_dot_product_attention / Attention / Transformer 395-627, GraphNetBlock 630-746), so
reference checkpoints load unchanged. GraphNetBlock.forward runs on libmgn (HIP, gfx950); there
is no CPU fallback. The transformer family's attention core (the reference's DGL sparse branch) runs
on libmgn's graph-attention kernels on a HIP tensor and as a torch composition
(sparse_attention_torch) on a CPU tensor. The block's dense half, x + gated_mlp(norm2(x)), runs on libmgn's fused gated-MLP kernels
(mgn_gated_mlp_*) when the block is built with dense="libmgn" (opt-in; the default "torch" is a composition
of torch ops); the attention-side projections (norm1, q/k/v, proj) are torch ops. DiagonalGMMHead (157-195) is the mixture-density decoder of
EncodeTransformDecode: two Linears (torch ops); its loss and sampler run on libmgn (utils/loss.py
masked_gmm_nll, models/simulator.py sample_gmm_diagonal). The full-covariance GMMHead is out of scope.
"""
import os
from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from graphphysics import _native as nat
from graphphysics.models import _engine


def default_compute_dtype():
    """fp32 (exact-fp32 MFMA, parity path) unless GRAPHPHYSICS_MGN_DTYPE=bf16."""
    v = os.environ.get("GRAPHPHYSICS_MGN_DTYPE", "fp32").lower()
    return torch.bfloat16 if v in ("bf16", "bfloat16") else torch.float32


class RMSNorm(nn.Module):
    """y = scale * x / (||x||_2 * d^-1/2 + eps)  (reference layers.py:49-74). As a stand-alone
    module it evaluates with torch ops; inside build_mlp blocks it is fused into the kernels."""

    def __init__(self, d: int, p: float = -1.0, eps: float = 1e-8, bias: bool = False):
        super().__init__()
        self.d, self.p, self.eps, self.bias = d, p, eps, bias
        self.scale = nn.Parameter(torch.ones(d))
        if self.bias:
            self.offset = nn.Parameter(torch.zeros(d))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype in (torch.bfloat16, torch.float16):
            # norms are fp32 (the output already was: scale is fp32): a bf16 Linear output under autocast is
            # normalised in fp32 on every device, as CUDA autocast's norm policy does on a HIP device
            x = x.float()
        if self.p < 0.0 or self.p > 1.0:
            nrm, dx = x.norm(2, dim=-1, keepdim=True), self.d
        else:
            k = int(self.d * self.p)
            nrm, dx = x[..., :k].norm(2, dim=-1, keepdim=True), k
        y = x / (nrm * dx ** (-0.5) + self.eps)
        return self.scale * y + self.offset if self.bias else self.scale * y


def build_mlp(in_size: int, hidden_size: int, out_size: int, nb_of_layers: int = 4,
              layer_norm: bool = True) -> nn.Module:
    """Linear, ReLU × (L-1), Linear, [RMSNorm] — parameter order/keys as reference layers.py:77-113."""
    assert nb_of_layers >= 2, "The MLP must have at least 2 layers (input and output)."
    mods = [nn.Linear(in_size, hidden_size), nn.ReLU()]
    for _ in range(nb_of_layers - 2):
        mods += [nn.Linear(hidden_size, hidden_size), nn.ReLU()]
    mods.append(nn.Linear(hidden_size, out_size))
    if layer_norm:
        mods.append(RMSNorm(out_size))
    return nn.Sequential(*mods)


class DiagonalGMMHead(nn.Module):
    """Parameters of a K-component Gaussian mixture with diagonal covariances (reference
    layers.py:157-195): forward(x [N, input_dim]) -> [N, K(2d+1)], component k = [logit, d means,
    d log-stds]. `temperature` scales the standard deviations in the loss and the sampler. Keys
    pre_proj.{weight,bias}, proj.{weight,bias}, created in the reference's order."""

    def __init__(self, input_dim: int, d: int, num_components: int, temperature: float = 1.0):
        super().__init__()
        self.d = d
        self.K = num_components
        self.temperature = temperature
        self.per_component = 2 * d + 1
        self.pre_proj = nn.Linear(input_dim, input_dim)
        self.proj = nn.Linear(input_dim, self.K * self.per_component)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(self.pre_proj(x))


class Normalizer(nn.Module):
    """Online feature normaliser (reference layers.py:265-392), same buffers and semantics.

    Differences that do not change results: the `num_accumulations < max_accumulations` test is
    evaluated on device (no host sync per call), and, when `process_group` is set (graph-sharded
    data parallel), the batch statistics are all-reduced before they are accumulated so every rank
    holds the statistics of the global batch."""

    def __init__(self, size: int, max_accumulations: int = 10 ** 5, std_epsilon: float = 1e-8,
                 name: str = "Normalizer", device: Optional[Union[str, torch.device]] = "cuda"):
        super().__init__()
        self.name = name
        self.device = device
        self._max_accumulations = max_accumulations
        self._std_epsilon = torch.tensor(std_epsilon, dtype=torch.float32, requires_grad=False,
                                         device=device)
        self.register_buffer("_acc_count", torch.tensor(0.0, device=device))
        self.register_buffer("_num_accumulations", torch.tensor(0.0, device=device))
        self.register_buffer("_acc_sum", torch.zeros((1, size), dtype=torch.float32, device=device))
        self.register_buffer("_acc_sum_squared",
                             torch.zeros((1, size), dtype=torch.float32, device=device))
        self.process_group = None
        self._pending = None  # (sum, sum_sq, count) of the global batch, set by set_pending()
        self._pending_packed = None  # the same three as one [2*size + 1] tensor (views above)
        self._pending_fresh = False  # refreshed for the next accumulating forward (one-shot)
        self._eps_cache = None

    def batch_statistics(self, d: torch.Tensor):
        """(Σ rows, Σ rows², row count) of one local batch (no exchange)."""
        if d.is_cuda and d.dim() == 2 and 1 <= d.shape[1] <= 32:
            from graphphysics import _native as nat  # batch statistics in one native pass

            s, s2 = nat.column_stats(d.float())
        else:
            s = torch.sum(d, dim=0, keepdim=True)
            s2 = torch.sum(d ** 2, dim=0, keepdim=True)
        return s, s2, torch.full((), float(d.shape[0]), device=d.device)

    def set_pending(self, s, s2, cnt):
        """Statistics (already summed over ranks) that the next accumulating forward uses instead of
        computing and exchanging its own: lets a data-parallel step exchange them before a replayed
        hipGraph. The buffers are static, so a captured forward reads each step's values."""
        if self._pending is None:
            k = s.numel()
            packed = torch.empty(2 * k + 1, dtype=torch.float32, device=s.device)
            self._pending_packed = packed
            self._pending = (packed[:k].view_as(s), packed[k:2 * k].view_as(s2), packed[2 * k])
        self._pending[0].copy_(s)
        self._pending[1].copy_(s2)
        self._pending[2].copy_(cnt.reshape(()))
        self._pending_fresh = True

    def bind_pending(self, packed_view: torch.Tensor):
        """Keep the pending statistics in `packed_view` (float32 [2*size + 1], e.g. a slice of one
        buffer several normalizers share so that a single all-reduce updates them all in place)."""
        k = self._acc_sum.numel()
        self._pending_packed = packed_view
        self._pending = (packed_view[:k].view_as(self._acc_sum), packed_view[k:2 * k].view_as(self._acc_sum_squared),
                         packed_view[2 * k])

    def mark_pending_fresh(self):
        """The bound pending buffer now holds this step's (exchanged) statistics."""
        self._pending_fresh = True

    def clear_pending(self):
        self._pending = None
        self._pending_packed = None
        self._pending_fresh = False

    def _consume_pending(self):
        """Pending statistics feed exactly ONE accumulating forward: a second forward without a new
        exchange would re-add the previous batch's statistics (a hipGraph replay re-reads the bound
        buffer, which its owner refreshes before every replay)."""
        if self._pending is None or (self._pending[0].is_cuda and torch.cuda.is_current_stream_capturing()):
            return
        if not self._pending_fresh:
            raise RuntimeError(f"{self.name}: pending batch statistics were already consumed; exchange "
                               "them (Simulator.exchange_statistics) before every training forward")
        self._pending_fresh = False

    def _eps(self) -> float:
        t = self._std_epsilon
        if self._eps_cache is None or self._eps_cache[0] is not t:
            self._eps_cache = (t, float(t))
        return self._eps_cache[1]

    def _native_ok(self, d: torch.Tensor, accumulate: bool) -> bool:
        if not (d.is_cuda and d.dim() == 2 and 1 <= d.shape[1] <= 32 and not d.requires_grad):
            return False
        if accumulate and self.process_group is not None and self._pending is None:
            return False  # statistics exchanged inside _accumulate: torch path
        bufs = (self._acc_sum, self._acc_sum_squared, self._acc_count, self._num_accumulations)
        return all(b.dtype == torch.float32 and b.is_contiguous() and b.device == d.device for b in bufs)

    def forward(self, batched_data: torch.Tensor, accumulate: bool = True) -> torch.Tensor:
        if accumulate:
            self._consume_pending()
        if self._native_ok(batched_data, accumulate):
            from graphphysics import _native as nat  # one native pass: statistics, _accumulate, normalise

            return nat.normalizer_forward(batched_data.detach(), accumulate,
                                          self._pending_packed if accumulate else None, self._acc_sum,
                                          self._acc_sum_squared, self._acc_count, self._num_accumulations,
                                          float(self._max_accumulations), self._eps())
        if accumulate:
            self._accumulate(batched_data.detach())
        return (batched_data - self._mean()) / self._std_with_epsilon()

    def inverse(self, normalized_batch_data: torch.Tensor) -> torch.Tensor:
        return normalized_batch_data * self._std_with_epsilon() + self._mean()

    def _accumulate(self, d: torch.Tensor):
        if self._pending is not None:
            s, s2, cnt = self._pending
        else:
            s, s2, cnt = self.batch_statistics(d)
        if self.process_group is not None and self._pending is None:
            import torch.distributed as dist

            packed = torch.cat([s.reshape(-1), s2.reshape(-1), cnt.reshape(1)])
            dist.all_reduce(packed, group=self.process_group)
            k = s.numel()
            s, s2, cnt = packed[:k].view_as(s), packed[k:2 * k].view_as(s2), packed[2 * k]
        live = self._num_accumulations < self._max_accumulations
        zero = torch.zeros((), device=d.device)
        self._acc_sum += torch.where(live, s, zero)
        self._acc_sum_squared += torch.where(live, s2, zero)
        self._acc_count += torch.where(live, cnt, zero)
        self._num_accumulations += live.float()

    def _mean(self) -> torch.Tensor:
        return self._acc_sum / self._acc_count.clamp(min=1.0)  # = torch.max(count, 1.0)

    def _std_with_epsilon(self) -> torch.Tensor:
        var = self._acc_sum_squared / self._acc_count.clamp(min=1.0) - self._mean() ** 2
        std = torch.sqrt(torch.clamp(var, min=0.0))
        return torch.max(std, self._std_epsilon.to(std.device))

    def get_variable(self) -> Dict[str, Any]:
        return {
            "_max_accumulations": self._max_accumulations,
            "_std_epsilon": self._std_epsilon,
            "_acc_count": self._acc_count,
            "_num_accumulations": self._num_accumulations,
            "_acc_sum": self._acc_sum,
            "_acc_sum_squared": self._acc_sum_squared,
            "name": self.name,
        }


# --------------------------------------------------------------------------- transformer family
ATTENTION_HEADS = (1, 2, 4, 8)  # mgn_graph_attention_* (include/mgn.h)
ATTENTION_MAX_HIDDEN = 256
DENSE_MODES = ("torch", "libmgn")  # who runs x + gated_mlp(norm2(x)) of a Transformer block


def check_dense(dense):
    if dense not in DENSE_MODES:
        raise ValueError(f"dense={dense!r}: must be one of {DENSE_MODES}")
    return dense


class GatedMLP(nn.Module):
    """GELU(linear1(x)) ⊙ linear2(x) (reference layers.py:198-233)."""

    def __init__(self, in_size: int, hidden_size: int, expansion_factor: int):
        super().__init__()
        self.linear1 = nn.Linear(in_size, expansion_factor * hidden_size)
        self.linear2 = nn.Linear(in_size, expansion_factor * hidden_size)
        self.activation = nn.GELU()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.activation(self.linear1(x)) * self.linear2(x)


def build_gated_mlp(in_size: int, hidden_size: int, out_size: int, expansion_factor: int = 3) -> nn.Module:
    """RMSNorm, GatedMLP, Linear — keys {0.scale, 1.linear1/2.*, 2.*} as reference layers.py:236-262."""
    return nn.Sequential(RMSNorm(in_size),
                         GatedMLP(in_size=in_size, hidden_size=hidden_size, expansion_factor=expansion_factor),
                         nn.Linear(hidden_size * expansion_factor, out_size))


def _edge_scores(q, k, edge_index, heads):
    """s[e, b] = Σ_d (q[row_e, dH+b] / sqrt(H)) k[col_e, dH+b]: heads interleaved (feature c -> head c % H)
    and the reference's 1/sqrt(num_heads) scale (layers.py:411, k.size(-1) of the reshaped k)."""
    N, h = q.shape
    row, col = edge_index[0].long(), edge_index[1].long()
    q3 = (q / heads ** 0.5).reshape(N, h // heads, heads)
    return (q3[row] * k.reshape(N, h // heads, heads)[col]).sum(1), row, col


def sparse_attention_weights(q, k, edge_index, heads):
    """[E, H] softmax weights in the caller's edge order (DGL's attn.val): the softmax runs over the
    out-edges of each source node (row), per head; duplicate edges are separate entries."""
    s, row, _ = _edge_scores(q, k, edge_index, heads)
    N = q.shape[0]
    idx = row[:, None].expand(-1, heads)
    m = torch.full((N, heads), float("-inf"), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, idx, s.detach(), "amax")  # the shift cancels: no gradient through it
    w = torch.exp(s - m[row])
    den = torch.zeros((N, heads), dtype=s.dtype, device=s.device).index_add(0, row, w)
    return w / den[row]


def sparse_attention_torch(q, k, v, edge_index, heads):
    """Adjacency-masked multi-head attention as a differentiable composition of torch ops, on any
    device and dtype: y[i, dH+b] = Σ_{e: row_e = i} p[e, b] v[col_e, dH+b] with p =
    sparse_attention_weights (0 for a node without out-edges). The CPU path of Attention, the truth
    the libmgn kernels are tested against and the baseline they are timed against."""
    N, h = q.shape
    p = sparse_attention_weights(q, k, edge_index, heads)
    row, col = edge_index[0].long(), edge_index[1].long()
    msg = p[:, None, :] * v.reshape(N, h // heads, heads)[col]
    y = torch.zeros((N, h // heads, heads), dtype=msg.dtype, device=msg.device).index_add(0, row, msg)
    return y.reshape(N, h)


def graph_attention(q, k, v, edge_index, heads):
    """sparse_attention_torch on libmgn's HIP kernels (mgn_graph_attention_forward / _backward):
    q, k, v [N, h] fp32 or bf16 HIP tensors, possibly column slices of one [N, 3h] buffer."""
    nat.require_device(q)
    topo = _engine.get_topology(edge_index, q.size(0))
    return _engine.GraphAttentionFunction.apply(topo, heads, q, k, v)


def scaled_dot_product_attention(q, k, v, att_mask=None, return_attention: bool = False):
    """Reference layers.py:424-457 on q, k, v of shape (N, head_dim, num_heads). att_mask: an
    edge_index [2, E] (in place of the reference's DGL SparseMatrix) or None (the reference's dense
    branch, as written). The attention weights are the [E, H] values of DGL's attn."""
    if att_mask is None:
        attn = torch.softmax((q / k.size(-1) ** 0.5) @ k.transpose(-2, -1), dim=-1)
        y = attn @ v
        return (y, attn) if return_attention else y
    N, heads = q.shape[0], q.shape[-1]
    q2, k2, v2 = q.reshape(N, -1), k.reshape(N, -1), v.reshape(N, -1)
    if q.is_cuda:
        y = graph_attention(q2, k2, v2, att_mask, heads)
    elif q.dtype in (torch.bfloat16, torch.float16):
        # as the kernels: q, k, v and y stored in the low-precision type, scores, softmax and sums in fp32
        y = sparse_attention_torch(q2.float(), k2.float(), v2.float(), att_mask, heads).to(q.dtype)
    else:
        y = sparse_attention_torch(q2, k2, v2, att_mask, heads)
    y = y.reshape(q.shape)
    if return_attention:
        return y, sparse_attention_weights(q2.float() if q.dtype != torch.float64 else q2,
                                           k2.float() if k.dtype != torch.float64 else k2, att_mask, heads)
    return y


def _autocast(module_dtype, x):
    """bf16 compute: the Linear layers run as under torch.autocast(bfloat16); norms, residuals and the
    attention's softmax stay fp32 (their inputs are promoted)."""
    if module_dtype == torch.bfloat16:
        return torch.autocast(device_type=x.device.type, dtype=torch.bfloat16)
    import contextlib

    return contextlib.nullcontext()


class Attention(nn.Module):
    """Multi-head attention masked by the mesh adjacency (reference layers.py:460-545, DGL branch).

    forward(x [N, input_dim], adj, return_attention=False): adj is an edge_index [2, E] tensor (the
    reference's dglsp.spmatrix(indices=edge_index)). On a HIP tensor the attention core runs on
    libmgn (graph_attention; no fallback), on a CPU tensor as sparse_attention_torch."""

    def __init__(self, input_dim=512, output_dim=512, num_heads=4, use_proj_bias: bool = True,
                 use_separate_proj_weight: bool = True, compute_dtype: torch.dtype = None):
        super().__init__()
        if num_heads not in ATTENTION_HEADS or not 1 <= output_dim <= ATTENTION_MAX_HIDDEN \
                or output_dim % num_heads != 0:
            raise ValueError(f"Attention(output_dim={output_dim}, num_heads={num_heads}): libmgn's graph attention "
                             f"supports num_heads in {ATTENTION_HEADS}, output_dim <= {ATTENTION_MAX_HIDDEN} and "
                             "output_dim divisible by num_heads")
        self.hidden_size = output_dim
        self.num_heads = num_heads
        self.head_dim = output_dim // num_heads
        self.q_proj = nn.Linear(input_dim, output_dim, bias=use_proj_bias)
        self.k_proj = nn.Linear(input_dim, output_dim, bias=use_proj_bias)
        self.v_proj = nn.Linear(input_dim, output_dim, bias=use_proj_bias)
        self.proj = nn.Linear(output_dim, output_dim, bias=use_proj_bias)
        if not use_separate_proj_weight:
            with torch.no_grad():
                self.k_proj.weight = self.q_proj.weight
                self.v_proj.weight = self.q_proj.weight
        self.compute_dtype = compute_dtype or default_compute_dtype()

    def forward(self, x: torch.Tensor, adj, return_attention: bool = False):
        N, h, H = x.size(0), self.hidden_size, self.num_heads
        with _autocast(self.compute_dtype, x):
            if adj is not None and x.is_cuda:
                # one GEMM for the three projections; the kernels read q, k, v as column slices of its output
                w = torch.cat([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight])
                b = torch.cat([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]) \
                    if self.q_proj.bias is not None else None
                qkv = nn.functional.linear(x, w, b)
                topo = _engine.get_topology(adj, N)
                y = _engine.GraphAttentionFunction.apply(topo, H, qkv, None, None)
                attn = sparse_attention_weights(qkv[:, :h], qkv[:, h:2 * h], adj, H) if return_attention else None
            else:
                q, k, v = self.q_proj(x), self.k_proj(x), self.v_proj(x)
                q, k, v = (t.reshape(N, self.head_dim, H) for t in (q, k, v))
                if return_attention:
                    y, attn = scaled_dot_product_attention(q, k, v, adj, return_attention=True)
                else:
                    y, attn = scaled_dot_product_attention(q, k, v, adj), None
            out = self.proj(y.reshape(N, -1))
        return (out, attn) if return_attention else out


class Transformer(nn.Module):
    """x = x + attention(norm1(x), adj); x = x + gated_mlp(norm2(x)) (reference layers.py:548-627; the
    gated MLP starts with an RMSNorm of its own, so its input is normalised twice; `activation` is
    constructed and never used, as in the reference). adj: an edge_index [2, E] tensor.

    dense (keyword / set_dense): "torch" (default) — the second line is a composition of torch ops;
    "libmgn" — on a HIP tensor it is one _engine.GatedMLPFunction (the fused gated-MLP kernels, in the
    module's compute_dtype, no fallback), on a CPU tensor the torch composition, as the attention."""

    def __init__(self, input_dim: int, output_dim: int, num_heads: int, activation_layer: torch.nn.Module = nn.ReLU,
                 use_proj_bias: bool = True, use_separate_proj_weight: bool = True,
                 compute_dtype: torch.dtype = None, dense: str = "torch"):
        super().__init__()
        self.dense = check_dense(dense)
        self.compute_dtype = compute_dtype or default_compute_dtype()
        self.attention = Attention(input_dim=input_dim, output_dim=output_dim, num_heads=num_heads,
                                   use_proj_bias=use_proj_bias, use_separate_proj_weight=use_separate_proj_weight,
                                   compute_dtype=self.compute_dtype)
        self.activation = activation_layer()
        self.norm1, self.norm2 = RMSNorm(output_dim), RMSNorm(output_dim)
        self.gated_mlp = build_gated_mlp(in_size=output_dim, hidden_size=output_dim, out_size=output_dim)
        self.use_adjacency = True  # the reference's HAS_DGL_SPARSE: always the sparse branch here

    def set_compute_dtype(self, dtype):
        self.compute_dtype = self.attention.compute_dtype = dtype
        return self

    def set_dense(self, dense):
        self.dense = check_dense(dense)
        return self

    def _dense_half(self, x):
        """x + gated_mlp(norm2(x)) on libmgn: one autograd node over the fp32 master parameters."""
        g = self.gated_mlp
        return _engine.GatedMLPFunction.apply(
            nat.mgn_dtype(self.compute_dtype), torch.is_grad_enabled(), x, self.norm2.scale, g[0].scale,
            g[1].linear1.weight, g[1].linear1.bias, g[1].linear2.weight, g[1].linear2.bias, g[2].weight, g[2].bias)

    def forward(self, x: torch.Tensor, adj, return_attention: bool = False):
        attn = None
        with _autocast(self.compute_dtype, x):
            if return_attention:
                x_, attn = self.attention(self.norm1(x), adj, return_attention)
                x = x + x_
            else:
                x = x + self.attention(self.norm1(x), adj, return_attention)
            if self.dense == "libmgn" and x.is_cuda:
                x = self._dense_half(x)
            else:
                x = x + self.gated_mlp(self.norm2(x))
        return (x, attn) if return_attention else x


class GraphNetBlock(nn.Module):
    """MeshGraphNet processor block (reference layers.py:630-746), fused on MI355X.

    forward(x [N,h], edge_index [2,E], edge_attr [E,h]) -> (x', e') with
      m  = edge_block([e ‖ x[col] ‖ x[row]]),  aggr_i = Σ_{col_k = i} m_k,
      x' = x + node_block([x ‖ aggr]),          e' = e + m
    (row = edge_index[0] = source, col = edge_index[1] = target; e' in the caller's edge order).
    """

    def __init__(self, hidden_size: int, nb_of_layers: int = 4, layer_norm: bool = True):
        super().__init__()
        self.edge_block = build_mlp(3 * hidden_size, hidden_size, hidden_size, nb_of_layers, layer_norm)
        self.node_block = build_mlp(2 * hidden_size, hidden_size, hidden_size, nb_of_layers, layer_norm)
        self.compute_dtype = default_compute_dtype()
        self._plan = None

    def _get_plan(self):
        if self._plan is None:
            self._plan = _engine.ModelPlan(self, [self.edge_block, self.node_block], [3, 2])
        return self._plan

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor,
                size: int = None) -> Tuple[torch.Tensor, torch.Tensor]:
        nat.require_device(x)
        topo = _engine.get_topology(edge_index, x.size(0))
        plan = self._get_plan()
        return _engine.BlockFunction.apply(plan, nat.mgn_dtype(self.compute_dtype), torch.is_grad_enabled(), x,
                                           edge_attr, topo, *plan.params)
