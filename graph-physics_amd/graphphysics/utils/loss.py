"""Masked L2 loss (reference graphphysics/utils/loss.py:10-65) and the negative log-likelihood of the
diagonal Gaussian-mixture head (reference utils/loss.py:111-199): the reference's classes, and their
capture-safe forms masked_mse / masked_gmm_nll (no boolean indexing, no host synchronisation; on HIP
fp32 tensors one libmgn launch each way)."""
import math

import torch
import torch.nn.functional as F
from torch.nn.modules.loss import _Loss

from graphphysics.utils.nodetype import NodeType


def _prepare_mask_for_loss(network_output, node_type, masks, selected_indexes=None):
    mask = node_type == masks[0]
    for m in masks[1:]:
        mask = torch.logical_or(mask, node_type == m)
    if selected_indexes is not None:
        n = network_output.shape[0]
        keep = ~torch.isin(torch.arange(n, device=network_output.device),
                           selected_indexes.to(network_output.device))
        mask = torch.logical_and(keep, mask)
    return mask


class L2Loss(_Loss):
    @property
    def __name__(self):
        return "MSE"

    def forward(self, target, network_output, node_type, masks: list, selected_indexes=None):
        mask = _prepare_mask_for_loss(network_output, node_type, masks, selected_indexes)
        return torch.mean(((network_output - target) ** 2)[mask])


class _NativeMaskedMSE(torch.autograd.Function):
    """masked_mse on libmgn (mgn_masked_mse / mgn_masked_mse_backward): one launch each way."""

    @staticmethod
    def forward(ctx, out, target, node_type, type_mask, count):
        from graphphysics import _native as nat

        out_c, tgt_c = out.detach().contiguous(), target.detach().float().contiguous()
        rows, cols = out_c.shape
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        cnt = torch.empty((), dtype=torch.float32, device=out.device)
        ws = torch.empty(int(nat.lib().mgn_masked_mse_workspace_bytes(rows)), dtype=torch.uint8, device=out.device)
        nat.check(nat.lib().mgn_masked_mse(nat.ptr(out_c), nat.ptr(tgt_c), rows, cols, nat.ptr(node_type),
                                           node_type.stride(0), type_mask, nat.ptr(count), nat.ptr(loss),
                                           nat.ptr(cnt), nat.ptr(ws), ws.numel(), nat.stream_ptr(out.device)))
        ctx.save_for_backward(out_c, tgt_c, node_type, cnt)
        ctx.type_mask = type_mask
        return loss

    @staticmethod
    def backward(ctx, gloss):
        from graphphysics import _native as nat

        out_c, tgt_c, node_type, cnt = ctx.saved_tensors
        rows, cols = out_c.shape
        g = torch.empty_like(out_c)
        gl = gloss.detach().float().contiguous()
        nat.check(nat.lib().mgn_masked_mse_backward(nat.ptr(out_c), nat.ptr(tgt_c), rows, cols, nat.ptr(node_type),
                                                    node_type.stride(0), ctx.type_mask, nat.ptr(cnt), nat.ptr(gl),
                                                    nat.ptr(g), nat.stream_ptr(out_c.device)))
        return g, None, None, None, None


def _native_loss_ok(target, network_output, node_type, masks, count, target_cols=None):
    """target_cols: the target's column count when it is not the output's (the mixture loss)."""
    rows, cols = network_output.shape if network_output.dim() == 2 else (None, None)
    return (network_output.is_cuda and network_output.dim() == 2 and network_output.dtype == torch.float32
            and tuple(target.shape) == (rows, target_cols or cols) and node_type.dim() == 1
            and node_type.shape[0] == rows
            and node_type.dtype == torch.float32 and node_type.device == network_output.device
            and all(0 <= int(m) < 32 for m in masks) and not target.requires_grad
            and (count is None or (count.dtype == torch.float32 and count.numel() == 1)))


def masked_mse(target, network_output, node_type, masks, count=None):
    """Same value as L2Loss without boolean indexing (no data-dependent shapes, no host sync, so it
    can live inside a captured hipGraph): Σ mask·err² / (Σ mask · n_out). `count` overrides the
    denominator's mask count (data-parallel global count). CUDA fp32: one native launch each way."""
    if _native_loss_ok(target, network_output, node_type, masks, count):
        tmask = 0
        for m in masks:
            tmask |= 1 << int(m)
        return _NativeMaskedMSE.apply(network_output, target, node_type, tmask,
                                      count.reshape(()) if count is not None else None)
    m = _prepare_mask_for_loss(network_output, node_type, masks).to(network_output.dtype)
    err = ((network_output - target) ** 2).sum(dim=1)
    cnt = m.sum() if count is None else count
    return (err * m).sum() / (cnt * network_output.shape[1])


GMM_MAX_COMPONENTS, GMM_MAX_DIM = 16, 8  # libmgn's mgn_gmm_* range (include/mgn.h)


def _gmm_row_log_prob(target, network_output, d, K, temperature):
    """log p(target | mixture) per row [M]: the reference's expression (utils/loss.py:159-196) term for
    term, its three epsilons included."""
    net = network_output.reshape(network_output.shape[0], K, 2 * d + 1)
    alpha = F.softmax(net[..., 0], dim=-1)
    means, log_std = net[..., 1:1 + d], net[..., 1 + d:1 + 2 * d]
    diff = target.unsqueeze(1) - means
    std = torch.exp(log_std) * temperature
    var = std ** 2
    log_component = -0.5 * (2.0 * torch.log(std + 1e-12) + (diff ** 2) / (var + 1e-12) + math.log(2.0 * math.pi))
    log_mixture = torch.log(alpha + 1e-12) + torch.sum(log_component, dim=-1)
    return torch.logsumexp(log_mixture, dim=-1)


class DiagonalGaussianMixtureNLLLoss(_Loss):
    """Reference utils/loss.py:111-199: −mean over the masked nodes of log Σ_k a_k N(target | mean_k,
    diag((temperature · exp(log_std_k))²)); network_output [N, K(2d+1)], component k = [logit, means,
    log-stds]. A torch composition on the tensors' device (boolean indexing: not capturable —
    masked_gmm_nll is the form TrainStep records)."""

    def __init__(self, d: int, K: int, temperature: float = 1.0, **kwargs):
        super().__init__(**kwargs)
        self.d, self.K, self.temperature = d, K, temperature
        self.per_comp = 2 * d + 1

    @property
    def __name__(self):
        return "GaussianMixtureNLLLossDiag"

    def forward(self, target, network_output, node_type, masks: list, selected_indexes=None):
        mask = _prepare_mask_for_loss(network_output, node_type, masks, selected_indexes)
        target, network_output = target[mask], network_output[mask]
        if target.shape[0] == 0:
            return torch.tensor(0.0, device=network_output.device, requires_grad=True)
        return -torch.mean(_gmm_row_log_prob(target, network_output, self.d, self.K, self.temperature))


class _NativeMaskedGMMNLL(torch.autograd.Function):
    """masked_gmm_nll on libmgn (mgn_gmm_nll_diag / mgn_gmm_nll_diag_backward): one launch each way (plus
    the single-wave final pass of the loss); the backward recomputes the rows, nothing per row is saved."""

    @staticmethod
    def forward(ctx, out, target, node_type, type_mask, count, d, K, temperature):
        from graphphysics import _native as nat

        out_c, tgt_c = out.detach().contiguous(), target.detach().float().contiguous()
        rows = out_c.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        cnt = torch.empty((), dtype=torch.float32, device=out.device)
        ws = torch.empty(int(nat.lib().mgn_gmm_nll_workspace_bytes(rows)), dtype=torch.uint8, device=out.device)
        nat.check(nat.lib().mgn_gmm_nll_diag(nat.ptr(out_c), nat.ptr(tgt_c), rows, d, K, temperature,
                                             nat.ptr(node_type), node_type.stride(0), type_mask, nat.ptr(count),
                                             nat.ptr(loss), nat.ptr(cnt), nat.ptr(ws), ws.numel(),
                                             nat.stream_ptr(out.device)))
        ctx.save_for_backward(out_c, tgt_c, node_type, cnt)
        ctx.args = (type_mask, d, K, temperature)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        from graphphysics import _native as nat

        out_c, tgt_c, node_type, cnt = ctx.saved_tensors
        type_mask, d, K, temperature = ctx.args
        g = torch.empty_like(out_c)
        gl = gloss.detach().float().contiguous()
        nat.check(nat.lib().mgn_gmm_nll_diag_backward(nat.ptr(out_c), nat.ptr(tgt_c), out_c.shape[0], d, K,
                                                      temperature, nat.ptr(node_type), node_type.stride(0),
                                                      type_mask, nat.ptr(cnt), nat.ptr(gl), nat.ptr(g),
                                                      nat.stream_ptr(out_c.device)))
        return g, None, None, None, None, None, None, None


def masked_gmm_nll(target, network_output, node_type, masks, d, K, temperature, count=None):
    """Same value as DiagonalGaussianMixtureNLLLoss(d, K, temperature) without boolean indexing (no
    data-dependent shapes, no host sync, so it can live inside a captured hipGraph): −Σ mask·L / Σ mask,
    and 0 — with zero gradients — when no node is masked in, as the reference's empty-mask return.
    `count` overrides the denominator (data-parallel global count). HIP fp32 (the conditions of
    masked_mse, 1 <= K <= 16 and 1 <= d <= 8): one native launch each way; anything else: a torch
    composition whose masked-out rows are replaced by zeros before the expression, so that they
    contribute neither a value nor a NaN gradient."""
    if network_output.dim() != 2 or network_output.shape[1] != K * (2 * d + 1) or target.shape != (
            network_output.shape[0], d):
        raise ValueError(f"masked_gmm_nll: network_output {tuple(network_output.shape)} / target "
                         f"{tuple(target.shape)} do not match K={K} components of 2·{d}+1 parameters")
    if _native_loss_ok(target, network_output, node_type, masks, count, target_cols=d) \
            and 1 <= K <= GMM_MAX_COMPONENTS and 1 <= d <= GMM_MAX_DIM:
        tmask = 0
        for m in masks:
            tmask |= 1 << int(m)
        return _NativeMaskedGMMNLL.apply(network_output, target, node_type, tmask,
                                         count.reshape(()) if count is not None else None, int(d), int(K),
                                         float(temperature))
    return masked_gmm_nll_torch(target, network_output, node_type, masks, d, K, temperature, count)


def masked_gmm_nll_torch(target, network_output, node_type, masks, d, K, temperature, count=None):
    """masked_gmm_nll as a torch composition on any device and dtype (what it runs where the native path does
    not apply; tools/bench_gmm.py times the kernels against it)."""
    mask = _prepare_mask_for_loss(network_output, node_type, masks)
    keep = mask[:, None]
    logp = _gmm_row_log_prob(torch.where(keep, target, torch.zeros_like(target)),
                             torch.where(keep, network_output, torch.zeros_like(network_output)), d, K, temperature)
    cnt = mask.sum().to(network_output.dtype) if count is None else count.reshape(()).to(network_output.dtype)
    total = -torch.where(mask, logp, torch.zeros_like(logp)).sum()
    return torch.where(cnt != 0, total / torch.where(cnt != 0, cnt, torch.ones_like(cnt)), torch.zeros_like(total))


__all__ = ["L2Loss", "DiagonalGaussianMixtureNLLLoss", "NodeType", "_prepare_mask_for_loss", "masked_mse",
           "masked_gmm_nll"]
