"""Loader of tests/golden/gmm_golden.npz (written by tests/golden/make_gmm_golden.py from the reference's own
DiagonalGaussianMixtureNLLLoss / DiagonalGMMHead / EncodeTransformDecode in fp64), the model of its model
case, and the fp64 / fp32 evaluations of the mixture formulas that test_gmm_cpu.py and test_gmm_gpu.py
compare against."""
import functools
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_CASES = ["a", "b", "c", "d", "e"]


@functools.lru_cache(maxsize=None)
def _arrays():
    z = np.load(os.path.join(GOLDEN, "gmm_golden.npz"))
    out = {}
    for k in z.files:
        if k.endswith("@lo"):
            continue
        if k.endswith("@hi"):  # fp64 value = float32 head + float32 tail (make_gmm_golden.put64)
            out[k[:-3]] = z[k].astype(np.float64) + z[k[:-3] + "@lo"].astype(np.float64)
        else:
            out[k] = z[k]
    return out


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def loss_case(tag):
    """{net [N, K(2d+1)], target [N, d], node_type [N], loss (0-dim), grad: fp64 tensors; masks: list of int;
    d, K: int; temperature: float}."""
    a = _arrays()
    c = {k: _t(a[f"{tag}::{k}"]) for k in ("net", "target", "node_type", "grad")}
    c["loss"] = _t(a[f"{tag}::loss"]).reshape(())
    c["masks"] = [int(m) for m in a[f"{tag}::masks"]]
    c["d"], c["K"] = (int(v) for v in a[f"{tag}::meta"])
    c["temperature"] = float(a[f"{tag}::temperature"][0])
    return c


@functools.lru_cache(maxsize=None)
def model_case():
    """{x [23, 7], target [23, 2], node_type [23], y [23, 15], nll (0-dim): fp64 tensors; edge_index int64
    [2, 90]; masks; w / g / init: {key: fp64 tensor}}."""
    a = _arrays()
    t = np.load(os.path.join(GOLDEN, "transformer_golden.npz"))
    c = {"x": _t(t["a::x"]), "edge_index": torch.from_numpy(t["a::edge_index"].astype(np.int64))}
    c.update({k: _t(a[f"m::{k}"]) for k in ("target", "node_type", "y")})
    c["nll"] = _t(a["m::nll"]).reshape(())
    c["masks"] = [int(m) for m in a["m::masks"]]
    for kind in ("w", "g", "init"):
        pre = f"m::{kind}::"
        c[kind] = {k[len(pre):]: _t(v) for k, v in a.items() if k.startswith(pre)}
    return c


def make_model(compute_dtype=torch.float32):
    from graphphysics.models.processors import EncodeTransformDecode

    return EncodeTransformDecode(2, 7, 2, hidden_size=24, num_heads=2, num_mixture_components=3, temperature=0.5,
                                 compute_dtype=compute_dtype)


def loaded_model(dtype=torch.float64, compute_dtype=torch.float32, device="cpu"):
    m = make_model(compute_dtype)
    m.load_state_dict({k: v.float() for k, v in model_case()["w"].items()}, strict=True)  # fp16-exact values
    return m.to(dtype).to(device)


def model_forward_backward(m, dtype, device="cpu"):
    """(y, nll, {key: parameter gradient}) of the mixture NLL over the fixture's masks."""
    from graphphysics.utils.data import Data
    from graphphysics.utils.loss import masked_gmm_nll

    c = model_case()
    for p in m.parameters():
        p.grad = None
    y = m(Data(x=c["x"].to(dtype).to(device), edge_index=c["edge_index"].to(device)))
    nll = masked_gmm_nll(c["target"].to(dtype).to(device), y, c["node_type"].to(dtype).to(device), c["masks"],
                         m.d, m.K, m.temperature)
    nll.backward()
    return y.detach(), nll.detach(), {k: p.grad.detach() for k, p in m.named_parameters()}


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def grad_err(key, got):
    """rel-L2 error of a parameter gradient of the model case. k_proj.bias: its true gradient is exactly 0 (a
    constant added to every key cancels in the softmax), so its error is measured against the norm of the
    q_proj.bias gradient of the same layer (as tests/_transformer_fixture.grad_err)."""
    ref = model_case()["g"][key]
    if key.endswith("k_proj.bias"):
        scale = model_case()["g"][key.replace("k_proj", "q_proj")].norm()
        return float((got.detach().double().cpu() - ref).norm() / scale)
    return relerr(got, ref)


# ----------------------------------------------------------------------------- the formulas, written out
def row_mask(node_type, masks):
    m = torch.zeros_like(node_type, dtype=torch.bool)
    for t in masks:
        m |= node_type == t
    return m


def nll_formula(net, target, mask, d, K, temperature, count=None, grad_loss=None):
    """(loss, d loss / d net · grad_loss) of the masked mixture NLL in the dtype of `net`, written out from
    its definition with torch ops and autograd: a = softmax(logit), s = temperature · exp(log_std),
    lc_k = Σ_j −½(2 log(s + 1e-12) + diff² / (s² + 1e-12) + log 2π), L = logsumexp_k(log(a_k + 1e-12) + lc_k),
    loss = −Σ m L / c with c = count or Σ m (0 when c = 0). Masked-out rows never enter the expression."""
    net = net.detach().clone().requires_grad_(True)
    p = net.reshape(net.shape[0], K, 2 * d + 1)
    a = torch.softmax(p[..., 0], dim=-1)
    s = torch.exp(p[..., 1 + d:]) * temperature
    diff = target[:, None, :] - p[..., 1:1 + d]
    lc = (-0.5 * (2.0 * torch.log(s + 1e-12) + diff ** 2 / (s ** 2 + 1e-12) + math.log(2.0 * math.pi))).sum(-1)
    L = torch.logsumexp(torch.log(a + 1e-12) + lc, dim=-1)
    c = float(mask.sum()) if count is None else float(count)
    if c == 0 or not mask.any():
        return torch.zeros((), dtype=net.dtype), torch.zeros_like(net)
    loss = -(L[mask].sum()) / c
    (g,) = torch.autograd.grad(loss, net, torch.ones_like(loss) * (1.0 if grad_loss is None else float(grad_loss)))
    return loss.detach(), g


def sample_formula(net, d, K, temperature, u, z):
    """(component [N], sample [N, d], cdf [N, K]) of the inverse-CDF rule in the dtype of `net`: the smallest k
    whose running sum of softmax(logit) exceeds u, the last component when none does."""
    p = net.reshape(net.shape[0], K, 2 * d + 1)
    cdf = torch.cumsum(torch.softmax(p[..., 0], dim=-1), dim=-1)
    over = cdf > u[:, None]
    comp = torch.where(over.any(dim=1), over.to(torch.int64).argmax(dim=1), torch.full_like(u, K - 1, dtype=torch.int64))
    sel = p[torch.arange(net.shape[0]), comp]
    return comp, sel[:, 1:1 + d] + temperature * torch.exp(sel[:, 1 + d:]) * z, cdf
