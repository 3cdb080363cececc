"""Golden vectors of the reference's diagonal mixture-density head: runs the REFERENCE's own
DiagonalGaussianMixtureNLLLoss (graphphysics/utils/loss.py:111-199), DiagonalGMMHead (models/layers.py:157-195)
and EncodeTransformDecode (models/processors.py:140-277, DGL branch) in fp64 on the CPU over the stand-ins
in tests/golden/_stubs and writes tests/golden/gmm_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_gmm_golden.py

Storage as make_transformer_golden.py: inputs and weights are rounded to fp16-representable values BEFORE
the reference runs and are stored as float16 (exact); fp64 results are a float32 head <key>@hi plus a tail
<key>@lo — here a float32 too (value = hi + lo, relative error below 2^-47: the tests ask for 1e-12, which
the int16 tail of the transformer fixture does not reach); tests/_gmm_fixture.py decodes both. The loss
runs with float64 as torch's default dtype, so that the reference's torch.tensor(2π) constant is fp64 like
everything else.

Loss cases (prefix <tag>::): net [N, K(2d+1)], target [N, d], node_type [N], masks, meta = [d, K],
temperature, loss, and grad = d loss / d net.
  a  N=37  d=3 K=3 temperature 0.7, masks [0, 5]
  b  N=5   d=1 K=1 temperature 1
  c  N=300 d=2 K=5 temperature 2.5
  d  N=64  d=3 K=3 temperature 1, the corner: logits from {-80, 0, 80}, log-stds from {-14, -6, 0, 4}, a
     third of the targets 1e3 standard deviations from a component's mean: the +1e-12 terms matter and whole
     components underflow. The generator asserts that the reference's fp32 evaluation of it is finite.
  e  N=11  d=3 K=3: no node of a masked type — loss 0, gradient 0
Model case (prefix m::): EncodeTransformDecode(2, 7, 2, hidden_size=24, num_heads=2,
num_mixture_components=3, temperature=0.5) on the 23-node graph (x, edge_index) of the transformer
fixture's case a: state dict (w::), init checksums under torch.manual_seed(0) (init:: = [sum, sum of
squares], fp32 init), the output y, the NLL over masks [0, 5] of y against target, and every parameter
gradient of that loss (g::).
"""
import os

import numpy as np
import torch

from graphphysics.models.processors import EncodeTransformDecode  # noqa: E402  (reference code)
from graphphysics.utils.loss import DiagonalGaussianMixtureNLLLoss  # noqa: E402
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))


def f16(a):
    """Round to fp16-representable values (kept in fp64)."""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def put64(out, key, a):
    a = np.asarray(a, dtype=np.float64)
    hi = a.astype(np.float32)
    out[key + "@hi"], out[key + "@lo"] = hi, (a - hi.astype(np.float64)).astype(np.float32)


def reference_nll(net, target, node_type, masks, d, K, temperature, dtype=torch.float64):
    """(loss, d loss / d net) of the reference's class in `dtype`."""
    torch.set_default_dtype(dtype)
    try:
        n = torch.from_numpy(net).to(dtype).requires_grad_(True)
        loss = DiagonalGaussianMixtureNLLLoss(d=d, K=K, temperature=temperature)(
            torch.from_numpy(target).to(dtype), n, torch.from_numpy(node_type).to(dtype), list(masks))
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grad = n.grad if n.grad is not None else torch.zeros_like(n)  # empty mask: a constant 0
    return loss.detach(), grad.detach()


def loss_case(out, tag, net, target, node_type, masks, d, K, temperature):
    net, target = f16(net), f16(target)
    node_type = np.asarray(node_type, dtype=np.float64)
    loss, grad = reference_nll(net, target, node_type, masks, d, K, temperature)
    out[f"{tag}::net"], out[f"{tag}::target"] = net.astype(np.float16), target.astype(np.float16)
    out[f"{tag}::node_type"] = node_type.astype(np.int8)
    out[f"{tag}::masks"] = np.asarray(masks, dtype=np.int8)
    out[f"{tag}::meta"] = np.asarray([d, K], dtype=np.int16)
    out[f"{tag}::temperature"] = np.asarray([temperature], dtype=np.float64)
    put64(out, f"{tag}::loss", loss.numpy().reshape(1))
    put64(out, f"{tag}::grad", grad.numpy())
    print(tag, "loss", float(loss), "max |grad|", float(grad.abs().max()))
    return net, target, node_type


def random_case(rng, n, d, K):
    """net with logits and means ~ N(0, 1), log-stds ~ N(-0.5, 0.5²); targets near a random component."""
    net = rng.standard_normal((n, K, 2 * d + 1))
    net[..., 1 + d:] = -0.5 + 0.5 * net[..., 1 + d:]
    pick = rng.integers(0, K, n)
    target = net[np.arange(n), pick, 1:1 + d] + 1.5 * rng.standard_normal((n, d))
    return net.reshape(n, -1), target, rng.integers(0, 7, n)


def corner_case(rng, n=64, d=3, K=3):
    net = rng.standard_normal((n, K, 2 * d + 1))
    net[..., 0] = rng.choice([-80.0, 0.0, 80.0], (n, K))
    net[..., 1 + d:] = rng.choice([-14.0, -6.0, 0.0, 4.0], (n, K, d))
    pick = rng.integers(0, K, n)
    mean, std = net[np.arange(n), pick, 1:1 + d], np.exp(net[np.arange(n), pick, 1 + d:])
    far = np.where(np.arange(n) % 3 == 0, 1e3, 1.0)[:, None]  # every third row: 1e3 standard deviations away
    target = mean + far * std * rng.choice([-1.0, 1.0], (n, d))
    return net.reshape(n, -1), target, rng.integers(0, 7, n)


def model_case(out, rng):
    z = np.load(os.path.join(HERE, "transformer_golden.npz"))
    x, ei = z["a::x"].astype(np.float64), z["a::edge_index"].astype(np.int64)
    n = x.shape[0]

    def make():
        return EncodeTransformDecode(2, 7, 2, hidden_size=24, num_heads=2, num_mixture_components=3, temperature=0.5)

    torch.manual_seed(0)
    for k, v in make().state_dict().items():
        v = v.double()
        out[f"m::init::{k}"] = np.array([v.sum().item(), (v * v).sum().item()])
    torch.manual_seed(4321)
    model = make().double()
    with torch.no_grad():  # non-trivial norm scales and biases
        for k, p in model.named_parameters():
            if k.endswith("scale"):
                p.add_(0.2 * torch.randn_like(p))
            elif k.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
        for p in model.parameters():
            p.copy_(p.half().double())
    target = f16(rng.standard_normal((n, 2)))
    node_type = np.concatenate([[0, 5, 0, 4, 6, 0], rng.integers(0, 7, n - 6)]).astype(np.float64)
    y = model(Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei)))
    torch.set_default_dtype(torch.float64)
    try:
        nll = DiagonalGaussianMixtureNLLLoss(d=model.d, K=model.K, temperature=model.temperature)(
            torch.from_numpy(target), y, torch.from_numpy(node_type), [0, 5])
        nll.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out["m::target"], out["m::node_type"] = target.astype(np.float16), node_type.astype(np.int8)
    out["m::masks"] = np.asarray([0, 5], dtype=np.int8)
    put64(out, "m::y", y.detach().numpy())
    put64(out, "m::nll", nll.detach().numpy().reshape(1))
    for k, v in model.state_dict().items():
        assert np.array_equal(f16(v.numpy()), v.numpy())
        out[f"m::w::{k}"] = v.numpy().astype(np.float16)
    for k, p in model.named_parameters():
        put64(out, f"m::g::{k}", p.grad.numpy())
    print("m nll", float(nll.detach()), "y", tuple(y.shape))


def main():
    rng = np.random.default_rng(20250311)
    out = {}
    loss_case(out, "a", *random_case(rng, 37, 3, 3), [0, 5], 3, 3, 0.7)
    net, target, _ = random_case(rng, 5, 1, 1)
    loss_case(out, "b", net, target, [0, 5, 2, 0, 1], [0, 5], 1, 1, 1.0)
    loss_case(out, "c", *random_case(rng, 300, 2, 5), [0, 5], 2, 5, 2.5)
    net, target, nt = loss_case(out, "d", *corner_case(rng), [0, 5], 3, 3, 1.0)
    l32, g32 = reference_nll(net, target, nt, [0, 5], 3, 3, 1.0, torch.float32)
    assert torch.isfinite(l32) and torch.isfinite(g32).all(), "case d: the reference's fp32 evaluation is not finite"
    net, target, _ = random_case(rng, 11, 3, 3)
    loss_case(out, "e", net, target, rng.choice([1, 2, 3, 4, 6], 11), [0, 5], 3, 3, 1.0)
    assert float(out["e::loss@hi"][0]) == 0.0 and not out["e::grad@hi"].any()
    model_case(out, rng)
    path = os.path.join(HERE, "gmm_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
