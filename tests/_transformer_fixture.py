"""Loader of tests/golden/transformer_golden*.npz (written by tests/golden/make_transformer_golden.py
from the reference's own Attention / Transformer / EncodeTransformDecode in fp64) and builders of the
drop-in modules for its four cases. Shared by test_transformer_cpu.py and test_transformer_gpu.py."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _arrays():
    out = {}
    for name in ("transformer_golden.npz", "transformer_golden_c.npz"):
        z = np.load(os.path.join(GOLDEN, name))
        raw = {k: z[k] for k in z.files}
        for k, v in raw.items():
            if k.endswith("@lo"):
                continue
            if k.endswith("@hi"):  # fp64 value = float32 head + int16 tail (make_transformer_golden.put64)
                hi = v.astype(np.float64)
                unit = float(np.abs(v).max()) * 2.0 ** -23 / 65534 if v.size else 0.0
                out[k[:-3]] = hi + raw[k[:-3] + "@lo"].astype(np.float64) * unit
            else:
                out[k] = v
    return out


@functools.lru_cache(maxsize=None)
def case(tag):
    """{x, gy, y, gx: fp64 tensors, edge_index: int64 [2, E], w / g / init: {key: fp64 tensor}}."""
    a = _arrays()
    c = {k: torch.from_numpy(np.asarray(a[f"{tag}::{k}"], dtype=np.float64)) for k in ("x", "gy", "y", "gx")}
    c["edge_index"] = torch.from_numpy(a[f"{tag}::edge_index"].astype(np.int64))
    for kind in ("w", "g", "init"):
        pre = f"{tag}::{kind}::"
        c[kind] = {k[len(pre):]: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in a.items()
                   if k.startswith(pre)}
    return c


def make(tag, compute_dtype=torch.float32):
    """The drop-in module of a fixture case with default init (consumes the RNG as the reference)."""
    from graphphysics.models.layers import Attention, Transformer
    from graphphysics.models.processors import EncodeTransformDecode

    if tag == "a":
        return EncodeTransformDecode(3, 7, 2, hidden_size=24, num_heads=2, compute_dtype=compute_dtype)
    if tag == "b":
        return EncodeTransformDecode(3, 7, 2, hidden_size=24, num_heads=2, use_separate_proj_weight=False,
                                     compute_dtype=compute_dtype)
    if tag == "c":
        return Transformer(64, 64, 4, compute_dtype=compute_dtype)
    return Attention(32, 32, 1, compute_dtype=compute_dtype)


def loaded(tag, dtype=torch.float64, compute_dtype=torch.float32, device="cpu"):
    """The module with the fixture's weights (strict load), in `dtype` on `device`."""
    m = make(tag, compute_dtype)
    m.load_state_dict({k: v.float() for k, v in case(tag)["w"].items()}, strict=True)  # fp16-exact values
    return m.to(dtype).to(device)


def run(tag, m, x, edge_index):
    from graphphysics.utils.data import Data

    return m(Data(x=x, edge_index=edge_index)) if tag in ("a", "b") else m(x, edge_index)


def forward_backward(tag, m, dtype, device="cpu"):
    """(y, gx, {key: parameter gradient}) of (y * gy).sum() on the fixture's inputs."""
    c = case(tag)
    x = c["x"].to(dtype).to(device).clone().requires_grad_(True)  # a fresh leaf: case() is cached
    ei = c["edge_index"].to(device)
    for p in m.parameters():
        p.grad = None
    y = run(tag, m, x, ei)
    (y * c["gy"].to(y.dtype).to(device)).sum().backward()
    return y.detach(), x.grad.detach(), {k: p.grad.detach() for k, p in m.named_parameters()}


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def grad_err(tag, key, got):
    """rel-L2 error of a parameter gradient against the fixture. k_proj.bias is the exception: a constant
    added to every key shifts all scores of a source node alike and cancels in the softmax, so its true
    gradient is exactly 0 and the fixture holds only fp64 rounding noise (~1e-17); its error is
    measured against the norm of the q_proj.bias gradient of the same layer instead."""
    ref = case(tag)["g"][key]
    if key.endswith("k_proj.bias"):
        scale = case(tag)["g"][key.replace("k_proj", "q_proj")].norm()
        return float((got.detach().double().cpu() - ref).norm() / scale)
    return relerr(got, ref)
