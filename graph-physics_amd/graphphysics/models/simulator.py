"""Drop-in Simulator (reference graphphysics/models/simulator.py:128-405) for the MGN path.

Same constructor, attributes and forward contract: forward(inputs) ->
(network_output, target_delta_normalized, outputs-or-None). The per-step preamble (target delta,
one-hot node type, three online Normalizers) is O(N+E) element-wise torch work on the device; the
Normalizers never synchronise with the host. The wrapped model is the libmgn
EncodeProcessDecode or EncodeTransformDecode. With a mixture head (model.K != 0) the evaluation
forward draws one sample per node (sample_gmm_diagonal, reference simulator.py:13-57) on libmgn.
"""
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

from graphphysics.models.layers import Normalizer
from graphphysics.utils.data import Data
from graphphysics.utils.nodetype import NodeType


def sample_gmm_diagonal(network_output: torch.Tensor, d: int, K: int, temperature: float = 1.0,
                        u: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One draw per node from the diagonal mixture network_output [N, K(2d+1)] describes (reference
    simulator.py:13-57) -> [N, d]. Deterministic given its noise: with a = softmax(logit), the component
    is the smallest k whose running sum of a exceeds u[n] (the last one catches the rest), and the sample
    is mean_k + temperature · exp(log_std_k) · z[n]. u [N] ~ U[0, 1) and z [N, d] ~ N(0, 1) default to
    torch.rand / torch.randn on the output's device: ordinary torch calls, so inside a captured hipGraph
    the generator advances with every replay.

    The distribution is the reference's; the draws are not: the reference picks the component with
    torch.multinomial, which consumes the random stream differently, so the same seed gives other samples.
    No data-dependent shapes, no Python loop over components, no host synchronisation. A HIP fp32 input
    (1 <= K <= 16, 1 <= d <= 8) runs libmgn's mgn_gmm_sample_diag; anything else a torch composition of
    the same rule (cumsum, comparison, gather)."""
    from graphphysics.utils.loss import GMM_MAX_COMPONENTS, GMM_MAX_DIM

    N = network_output.shape[0]
    if network_output.dim() != 2 or network_output.shape[1] != K * (2 * d + 1):
        raise ValueError(f"sample_gmm_diagonal: network_output {tuple(network_output.shape)} does not hold K={K} "
                         f"components of 2·{d}+1 parameters")
    dev, dt = network_output.device, network_output.dtype
    u = torch.rand(N, device=dev, dtype=dt) if u is None else u.to(dev, dt).reshape(N)
    z = torch.randn(N, d, device=dev, dtype=dt) if z is None else z.to(dev, dt).reshape(N, d)
    if network_output.is_cuda and dt == torch.float32 and 1 <= K <= GMM_MAX_COMPONENTS and 1 <= d <= GMM_MAX_DIM:
        from graphphysics import _native as nat

        net, u, z = network_output.detach().contiguous(), u.contiguous(), z.contiguous()
        out = torch.empty(N, d, dtype=dt, device=dev)
        nat.check(nat.lib().mgn_gmm_sample_diag(nat.ptr(net), N, d, K, float(temperature), nat.ptr(u), nat.ptr(z),
                                                nat.ptr(out), nat.stream_ptr(dev)))
        return out
    return sample_gmm_diagonal_torch(network_output, d, K, temperature, u, z)


def sample_gmm_diagonal_torch(network_output, d, K, temperature, u, z):
    """sample_gmm_diagonal's rule as a torch composition on any device and dtype, given its noise."""
    N = network_output.shape[0]
    net = network_output.reshape(N, K, 2 * d + 1)
    cdf = torch.cumsum(torch.softmax(net[..., 0], dim=-1), dim=-1)
    comp = (cdf <= u[:, None]).sum(dim=-1).clamp(max=K - 1)  # the first k with cdf_k > u; none: the last
    chosen = torch.gather(net, 1, comp[:, None, None].expand(N, 1, 2 * d + 1)).squeeze(1)
    return chosen[:, 1:1 + d] + torch.exp(chosen[:, 1 + d:]) * temperature * z


class Simulator(nn.Module):
    def __init__(self, node_input_size: int, edge_input_size: int, output_size: int,
                 feature_index_start: int, feature_index_end: int, output_index_start: int,
                 output_index_end: int, node_type_index: int, model: nn.Module,
                 device: torch.device, model_dir: str = "checkpoint/simulator.pth"):
        super().__init__()
        self.node_input_size = node_input_size
        self.edge_input_size = edge_input_size if edge_input_size > 0 else None
        self.output_size = output_size
        self.feature_index_start, self.feature_index_end = feature_index_start, feature_index_end
        self.node_type_index = node_type_index
        self.output_index_start, self.output_index_end = output_index_start, output_index_end
        self.model_dir = model_dir
        self.model = model.to(device)
        self._output_normalizer = Normalizer(size=output_size, name="output_normalizer", device=device)
        self._node_normalizer = Normalizer(size=node_input_size, name="node_normalizer", device=device)
        self._edge_normalizer = (Normalizer(size=edge_input_size, name="edge_normalizer", device=device)
                                 if self.edge_input_size is not None else None)
        self.device = device

    # ---- data-parallel hook: all-reduce batch statistics across graph shards
    def set_process_group(self, group):
        for n in (self._output_normalizer, self._node_normalizer, self._edge_normalizer):
            if n is not None:
                n.process_group = group
                if group is None:  # leaving data-parallel mode: no exchanged statistics linger
                    n.clear_pending()

    def normalizers(self):
        return [n for n in (self._output_normalizer, self._node_normalizer, self._edge_normalizer)
                if n is not None]

    @torch.no_grad()
    def exchange_statistics(self, inputs, group=None, loss_masks=None):
        """Data-parallel prologue for a replayed step: the batch statistics of all three normalizers
        (the same inputs the training forward accumulates) in ONE packed all-reduce over `group`,
        parked with Normalizer.set_pending() for the next forward. They depend only on the batch, so
        exchanging them before the (captured) forward is exact.

        loss_masks (node types of the masked L2 loss): the batch's masked-node count rides in the
        same all-reduce (one extra float); returns the GLOBAL count as a 1-element device tensor at a
        stable address (a captured loss reads the current batch's count from it), else None."""
        import torch.distributed as dist

        from graphphysics.utils.loss import _prepare_mask_for_loss

        def local_count(dst):
            if loss_masks is None:
                dst.zero_()
                return
            nt = inputs.x[:, self.node_type_index]
            dst.copy_(_prepare_mask_for_loss(nt[:, None], nt, list(loss_masks)).sum(dtype=torch.float32).reshape(1))

        if self._fused_preamble_ok(inputs, False):
            # one libmgn pass writes every normalizer's {Σx, Σx², count} into one buffer the
            # normalizers' pending statistics are views of (+ the loss count): one all-reduce, no copies
            from graphphysics import _native as nat

            norms = self.normalizers()
            sizes = [2 * n._acc_sum.numel() + 1 for n in norms]
            buf = getattr(self, "_stats_buf", None)
            if buf is None or buf.numel() != sum(sizes) + 1 or buf.device != inputs.x.device or \
                    any(n._pending_packed is None for n in norms):
                buf = torch.zeros(sum(sizes) + 1, dtype=torch.float32, device=inputs.x.device)
                o = 0
                for n, k in zip(norms, sizes):
                    n.bind_pending(buf[o:o + k])
                    o += k
                self._stats_buf = buf
            nat.simulator_statistics(inputs.x, inputs.y,
                                     inputs.edge_attr if self._edge_normalizer is not None else None,
                                     (self.feature_index_start, self.feature_index_end),
                                     (self.output_index_start, self.output_index_end), self.node_type_index,
                                     NodeType.SIZE, buf[:-1])
            local_count(buf[-1:])
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(buf, group=group)
            for n in norms:
                n.mark_pending_fresh()
            return buf[-1:] if loss_masks is not None else None
        delta = inputs.y - self._get_pre_target(inputs)
        nf = self._build_node_features(inputs, self._get_one_hot_type(inputs))
        srcs = [(self._output_normalizer, delta), (self._node_normalizer, nf)]
        if self._edge_normalizer is not None:
            srcs.append((self._edge_normalizer, inputs.edge_attr))
        stats = [n.batch_statistics(d) for n, d in srcs]
        cnt = torch.zeros(1, dtype=torch.float32, device=inputs.x.device)
        local_count(cnt)
        packed = torch.cat([t.reshape(-1).float() for st in stats for t in st] + [cnt])
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(packed, group=group)
        o = 0
        for (n, _), (s, s2, _) in zip(srcs, stats):
            k = s.numel()
            n.set_pending(packed[o:o + k].view_as(s), packed[o + k:o + 2 * k].view_as(s2), packed[o + 2 * k])
            o += 2 * k + 1
        if loss_masks is None:
            return None
        # a stable address for callers that capture the loss (the packed tensor is new each call)
        cb = getattr(self, "_count_buf", None)
        if cb is None or cb.device != packed.device:
            cb = self._count_buf = torch.zeros(1, dtype=torch.float32, device=packed.device)
        cb.copy_(packed[-1:])
        return cb

    def _get_pre_target(self, inputs) -> torch.Tensor:
        return inputs.x[:, self.output_index_start:self.output_index_end]

    def _get_target_normalized(self, inputs, is_training: bool = True) -> torch.Tensor:
        delta = inputs.y - self._get_pre_target(inputs)
        return self._output_normalizer(delta, is_training)

    def _get_one_hot_type(self, inputs) -> torch.Tensor:
        node_type = inputs.x[:, self.node_type_index]
        return torch.nn.functional.one_hot(torch.squeeze(node_type.long()), NodeType.SIZE)

    def _build_node_features(self, inputs, one_hot_type: torch.Tensor) -> torch.Tensor:
        feats = inputs.x[:, self.feature_index_start:self.feature_index_end]
        return torch.cat([feats, one_hot_type], dim=1)

    def _fused_preamble_ok(self, inputs, accumulate: bool) -> bool:
        """The three Normalizer.forward calls run as one libmgn preamble (mgn_simulator_preamble)
        when every input is a row-major fp32 HIP tensor and every normalizer takes its native path."""
        if not os.environ.get("MGN_FUSED_PREAMBLE", "1") != "0":
            return False
        x, y, ea = inputs.x, getattr(inputs, "y", None), inputs.edge_attr
        ts = [x, y] + ([ea] if self._edge_normalizer is not None else [])
        if any(t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1
               or t.requires_grad for t in ts):
            return False
        if y.shape[0] != x.shape[0] or y.shape[1] < self.output_index_end - self.output_index_start:
            return False
        dummy = x[:1, :1]
        return all(n._native_ok(dummy, accumulate) for n in self.normalizers())

    def _build_input_graph(self, inputs, is_training: bool) -> Tuple[Data, torch.Tensor]:
        if self._fused_preamble_ok(inputs, is_training):
            from graphphysics import _native as nat

            if is_training:
                for n in self.normalizers():
                    n._consume_pending()
            tdn, nfn, ea = nat.simulator_preamble(
                inputs.x, inputs.y, inputs.edge_attr, (self.feature_index_start, self.feature_index_end),
                (self.output_index_start, self.output_index_end), self.node_type_index, NodeType.SIZE,
                is_training, self._output_normalizer, self._node_normalizer, self._edge_normalizer)
            if ea is None:
                ea = inputs.edge_attr
            graph = Data(x=nfn, pos=getattr(inputs, "pos", None), edge_attr=ea, edge_index=inputs.edge_index)
            return graph, tdn
        tdn = self._get_target_normalized(inputs, is_training)
        nf = self._build_node_features(inputs, self._get_one_hot_type(inputs))
        nfn = self._node_normalizer(nf, is_training)
        ea = (self._edge_normalizer(inputs.edge_attr, is_training) if self._edge_normalizer is not None
              else inputs.edge_attr)
        graph = Data(x=nfn, pos=getattr(inputs, "pos", None), edge_attr=ea, edge_index=inputs.edge_index)
        return graph, tdn

    def _build_outputs(self, inputs, network_output: torch.Tensor) -> torch.Tensor:
        return self._get_pre_target(inputs) + self._output_normalizer.inverse(network_output)

    def forward(self, inputs) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        if inputs.x.is_cuda:  # a validation error flagged by an earlier launch (no host sync)
            from graphphysics import _native as nat

            nat.poll_errors(inputs.x.device)
        graph, tdn = self._build_input_graph(inputs=inputs, is_training=self.training)
        net = self.model(graph)
        if self.training:
            return net, tdn, None
        if self.model.K != 0:  # one sample per node from the mixture the head describes
            net = sample_gmm_diagonal(net, d=self.model.d, K=self.model.K, temperature=self.model.temperature)
        return net, tdn, self._build_outputs(inputs=inputs, network_output=net)

    def freeze_all(self) -> None:
        for p in self.model.parameters():
            p.requires_grad = False

    def load_checkpoint(self, ckpdir: Optional[str] = None) -> None:
        ckpdir = ckpdir or self.model_dir
        ck = torch.load(ckpdir, map_location=self.device, weights_only=True)
        self.load_state_dict(ck["model"])
        for key in ("_output_normalizer", "_node_normalizer", "_edge_normalizer"):
            st, nrm = ck.get(key, {}), getattr(self, key, None)
            if nrm is not None and st:
                for k, v in st.items():
                    cur = getattr(nrm, k, None)
                    if isinstance(cur, torch.Tensor) and isinstance(v, torch.Tensor) and cur.shape == v.shape:
                        # in place: captured TrainStep / rollout graphs keep reading these buffers
                        with torch.no_grad():
                            cur.copy_(v.to(cur.device, cur.dtype))
                    else:
                        setattr(nrm, k, v)

    def save_checkpoint(self, savedir: Optional[str] = None) -> None:
        savedir = savedir or self.model_dir
        os.makedirs(os.path.dirname(savedir) or ".", exist_ok=True)
        torch.save({
            "model": self.state_dict(),
            "_output_normalizer": self._output_normalizer.get_variable(),
            "_node_normalizer": self._node_normalizer.get_variable(),
            "_edge_normalizer": (self._edge_normalizer.get_variable() if self._edge_normalizer
                                 else None),
        }, savedir)
