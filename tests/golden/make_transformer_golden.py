"""Golden vectors of the reference's transformer family: runs the REFERENCE's own Attention,
Transformer and EncodeTransformDecode (graphphysics/models/layers.py:395-627, processors.py:140-277,
DGL branch) in fp64 over the stand-in for dgl.sparse in tests/golden/_stubs/dgl and writes
tests/golden/transformer_golden.npz (cases a, b, d) and tests/golden/transformer_golden_c.npz (case c:
its 53k parameters and their fp64 gradients do not fit one committed file beside the others). Run where
the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_transformer_golden.py

Cases (key prefix): inputs, edge_index, the full state_dict (w::<key>), the checksums of the default
init under torch.manual_seed(0) (init::<key> = [sum, sum of squares], fp32 init), the output y, the
input gradient gx and every parameter gradient (g::<key>) of (y * gy).sum().
Storage: weights and inputs are rounded to fp16-representable values BEFORE the reference runs and are
stored as float16 (exact); fp64 results are stored as a float32 head <key>@hi plus an int16 tail <key>@lo
(value = hi + lo · max|hi| · 2^-23 / 65534: absolute error below 2^-39 of the tensor's largest entry, far
inside the 1e-10 the tests ask for) — tests/_transformer_fixture.py decodes both.
  a  EncodeTransformDecode(3, 7, 2, hidden_size=24, num_heads=2): 23 nodes, 90 random edges with
     6 duplicates, one node without out-edges
  b  the same with use_separate_proj_weight=False
  c  one Transformer(64, 64, 4) block on the degree-corner graph: 150 nodes, out-degrees 0, 1, 2, 15,
     16, 17, 63, 64, 65, 130 on the first ten nodes, 0-12 on the rest, one node the target of 200
     edges, edge order shuffled
  d  one Attention(32, 32, 1) on the 23-node graph, its input scaled so that the scores reach ±60
"""
import os

import numpy as np
import torch

from graphphysics.models import layers as L  # noqa: E402  (reference code)
from graphphysics.models.processors import EncodeTransformDecode  # noqa: E402
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
assert L.HAS_DGL_SPARSE, "run with tests/golden/_stubs on PYTHONPATH (dgl.sparse stand-in)"


def small_graph(rng):
    """23 nodes, 90 edges: 84 random + 6 duplicates; node 5 has no out-edge."""
    n = 23
    row = rng.integers(0, n - 1, 84)
    row = np.where(row >= 5, row + 1, row)  # never 5
    col = rng.integers(0, n, 84)
    dup = rng.choice(84, 6, replace=False)
    row, col = np.concatenate([row, row[dup]]), np.concatenate([col, col[dup]])
    perm = rng.permutation(90)
    return n, np.stack([row[perm], col[perm]]).astype(np.int64)


def corner_graph(rng):
    n = 150
    deg = np.concatenate([[0, 1, 2, 15, 16, 17, 63, 64, 65, 130], rng.integers(0, 13, n - 10)])
    row = np.repeat(np.arange(n), deg)
    col = rng.integers(0, n, row.size)
    hot = rng.choice(row.size, 200, replace=False)
    col[hot] = 77  # in-degree skew: one node is the target of (at least) 200 edges
    perm = rng.permutation(row.size)
    return n, np.stack([row[perm], col[perm]]).astype(np.int64)


def f16(a):
    """Round to fp16-representable values (kept in fp64)."""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def put64(out, key, a):
    a = np.asarray(a, dtype=np.float64)
    hi = a.astype(np.float32)
    unit = float(np.abs(hi).max()) * 2.0 ** -23 / 65534 if a.size else 0.0
    lo = np.rint((a - hi.astype(np.float64)) / unit) if unit > 0 else np.zeros_like(a)
    assert np.abs(lo).max(initial=0) <= 32767
    out[key + "@hi"], out[key + "@lo"] = hi, lo.astype(np.int16)


def record(out, tag, make, run, x, gy, ei):
    torch.manual_seed(0)
    m32 = make()
    for k, v in m32.state_dict().items():
        v = v.double()
        out[f"{tag}::init::{k}"] = np.array([v.sum().item(), (v * v).sum().item()])
    torch.manual_seed(1234 + len(tag))
    model = make().double()
    with torch.no_grad():  # non-trivial norm scales and biases
        for k, p in model.named_parameters():
            if k.endswith("scale"):
                p.add_(0.2 * torch.randn_like(p))
            elif k.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
        for p in model.parameters():
            p.copy_(p.half().double())
    x, gy = f16(x), f16(gy)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    y = run(model, xt, torch.from_numpy(ei))
    (y * torch.from_numpy(gy).double()).sum().backward()
    out[f"{tag}::x"], out[f"{tag}::gy"] = x.astype(np.float16), gy.astype(np.float16)
    out[f"{tag}::edge_index"] = ei.astype(np.int16)
    put64(out, f"{tag}::y", y.detach().numpy())
    put64(out, f"{tag}::gx", xt.grad.numpy())
    for k, v in model.state_dict().items():
        assert np.array_equal(f16(v.numpy()), v.numpy())
        out[f"{tag}::w::{k}"] = v.numpy().astype(np.float16)
    for k, p in model.named_parameters():
        put64(out, f"{tag}::g::{k}", p.grad.numpy())
    return model


def main():
    rng = np.random.default_rng(20240607)
    out = {}
    n, ei = small_graph(rng)
    nc, eic = corner_graph(rng)
    x = rng.standard_normal((n, 7))
    gy = rng.standard_normal((n, 2))

    def run_model(m, xt, e):
        return m(Data(x=xt, edge_index=e))

    record(out, "a", lambda: EncodeTransformDecode(3, 7, 2, hidden_size=24, num_heads=2), run_model, x, gy, ei)
    record(out, "b", lambda: EncodeTransformDecode(3, 7, 2, hidden_size=24, num_heads=2,
                                                   use_separate_proj_weight=False), run_model, x, gy, ei)

    def run_block(m, xt, e):
        import dgl.sparse as dglsp

        return m(xt, dglsp.spmatrix(indices=e, shape=(xt.shape[0], xt.shape[0])))

    record(out, "c", lambda: L.Transformer(64, 64, 4), run_block, rng.standard_normal((nc, 64)),
           rng.standard_normal((nc, 64)), eic)
    xd = rng.standard_normal((n, 32))
    md = record(out, "d", lambda: L.Attention(32, 32, 1), run_block, xd, rng.standard_normal((n, 32)), ei)
    # rescale d's input so that the largest |score| is 60 (scores are quadratic in x up to the biases), re-record
    with torch.no_grad():
        for _ in range(30):
            xt = torch.from_numpy(f16(xd)).double()
            q, k = md.q_proj(xt), md.k_proj(xt)
            s = (q[ei[0]] * k[ei[1]]).sum(1).abs().max().item()  # H = 1: scale 1/sqrt(1)
            if abs(s - 60.0) < 0.5:
                break
            xd = xd * (60.0 / s) ** 0.5
    out["d::score_max"] = np.array([s])
    torch.manual_seed(1234 + 1)
    record(out, "d", lambda: L.Attention(32, 32, 1), run_block, xd, out["d::gy"].astype(np.float64), ei)
    for name, keep in (("transformer_golden.npz", lambda k: not k.startswith("c::")),
                       ("transformer_golden_c.npz", lambda k: k.startswith("c::"))):
        path = os.path.join(HERE, name)
        part = {k: v for k, v in out.items() if keep(k)}
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path), "bytes;", len(part), "arrays")
    print("d score max", s)


if __name__ == "__main__":
    main()
