"""Transformer family on the GPU: libmgn's graph-attention kernels (mgn_graph_attention_forward /
_backward) against the fp64 torch composition, exact bookkeeping of the edge lists, determinism, the
whole model against the reference's fp64 fixtures, and a captured training step.

Bounds: fp32 — the suite's assert_vs_truth rule (no further from fp64 than max(1e-5, 2x the fp32 CPU
composition)); bf16 — inputs rounded to bf16 first, no further from fp64 than max(1e-2, 2x the same
computation in bf16 on the CPU); fp32 gradients of whole models — rel-L2 <= 1e-3."""
import functools

import numpy as np
import pytest
import torch

import _transformer_fixture as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(64, 4), (128, 4), (256, 8), (16, 8), (24, 2), (32, 1)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _graph(name):
    """'corner': 150 nodes, out-degrees 0, 1, 2, 15, 16, 17, 63, 64, 65, 130, ..., one node the target of
    200 edges, shuffled; 'small': 23 nodes, 90 edges with duplicates, one node without out-edges."""
    ei = F.case("c" if name == "corner" else "a")["edge_index"]
    return (150 if name == "corner" else 23), ei


def _attention(q, k, v, gy, ei, H):
    """(y, dq, dk, dv) of the torch composition on the given tensors' device / dtype."""
    from graphphysics.models.layers import sparse_attention_torch

    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    y = sparse_attention_torch(q, k, v, ei, H)
    return (y.detach(),) + torch.autograd.grad((y * gy).sum(), (q, k, v))


@functools.lru_cache(maxsize=None)
def _reference(graph, h, H, bf16):
    """Inputs and the CPU references of one case, computed once: fp64 truth and the same composition
    in fp32 (or, bf16 case: on bf16 tensors)."""
    n, ei = _graph(graph)
    g = torch.Generator().manual_seed(1000 * h + H)
    q, k, v, gy = (torch.randn(n, h, generator=g) for _ in range(4))
    if bf16:
        q, k, v, gy = (t.bfloat16().float() for t in (q, k, v, gy))
    truth = _attention(q.double(), k.double(), v.double(), gy.double(), ei, H)
    low = torch.bfloat16 if bf16 else torch.float32
    ref = _attention(q.to(low), k.to(low), v.to(low), gy.to(low), ei, H)
    return (q, k, v, gy), truth, ref


def _kernel(q, k, v, gy, ei, H, packed):
    """(y, dq, dk, dv) of libmgn's kernels; packed: q, k, v are column slices of one [N, 3h] buffer."""
    from graphphysics.models.layers import graph_attention

    h = q.shape[1]
    if packed:
        buf = torch.cat([q, k, v], dim=1).to(DEV).requires_grad_(True)
        y = graph_attention(buf[:, :h], buf[:, h:2 * h], buf[:, 2 * h:], ei, H)
        (gb,) = torch.autograd.grad((y * gy.to(DEV)).sum(), (buf,))
        return y.detach(), gb[:, :h], gb[:, h:2 * h], gb[:, 2 * h:]
    q, k, v = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    y = graph_attention(q, k, v, ei, H)
    return (y.detach(),) + torch.autograd.grad((y * gy.to(DEV)).sum(), (q, k, v))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,H", SHAPES)
@pytest.mark.parametrize("graph", ["corner", "small"])
def test_kernel_matches_fp64_composition(graph, h, H, bf16):
    (q, k, v, gy), truth, ref = _reference(graph, h, H, bf16)
    _, ei = _graph(graph)
    eid = ei.to(DEV)
    dt = torch.bfloat16 if bf16 else torch.float32
    floor = 1e-2 if bf16 else 1e-5
    for packed in (True, False):
        got = _kernel(q.to(dt), k.to(dt), v.to(dt), gy.to(dt), eid, H, packed)
        for name, a, r, t in zip(("y", "dq", "dk", "dv"), got, ref, truth):
            assert a.dtype == dt and torch.isfinite(a).all()
            e_got, e_ref = F.relerr(a, t), F.relerr(r, t)
            print(f"{graph} h={h} H={H} {dt} packed={packed} {name}: kernel {e_got:.2e} reference {e_ref:.2e}")
            assert e_got <= max(floor, 2 * e_ref), f"{name}: kernel {e_got:.2e} vs fp64, CPU composition {e_ref:.2e}"


@pytest.mark.parametrize("h,H", [(64, 4), (24, 2), (256, 8)])
@pytest.mark.parametrize("graph", ["corner", "small"])
def test_uniform_weights_give_the_exact_neighbour_mean(graph, h, H):
    """k = 0: every weight of a node is 1/degree, so y[i] is the mean of v[col] over its out-edges (0 for
    degree 0); a dropped, doubled or misfiled edge moves a node by O(1/degree)."""
    from graphphysics.models.layers import graph_attention

    n, ei = _graph(graph)
    g = torch.Generator().manual_seed(7)
    q, v = torch.randn(n, h, generator=g), torch.randn(n, h, generator=g)
    row, col = ei
    deg = torch.zeros(n, dtype=torch.float64).index_add(0, row, torch.ones(row.numel(), dtype=torch.float64))
    mean = torch.zeros(n, h, dtype=torch.float64).index_add(0, row, v.double()[col]) / deg.clamp(min=1)[:, None]
    y = graph_attention(q.to(DEV), torch.zeros(n, h, device=DEV), v.to(DEV), ei.to(DEV), H).cpu().double()
    assert (deg == 0).any() and (y[deg == 0] == 0).all()
    err = (y - mean).norm(dim=1)[deg > 0] / mean.norm(dim=1)[deg > 0]
    assert err.max() <= 1e-6, err.max()
    # every row of v the same vector c: y[i] = c wherever there is an out-edge
    c = torch.randn(h, generator=g)
    k = torch.randn(n, h, generator=g)
    y = graph_attention(q.to(DEV), k.to(DEV), c.expand(n, h).contiguous().to(DEV), ei.to(DEV), H).cpu().double()
    err = (y - c.double()).norm(dim=1)[deg > 0] / c.double().norm()
    assert err.max() <= 1e-6 and (y[deg == 0] == 0).all(), err.max()


def test_large_scores_case_d():
    """Scores of about ±60 (fixture d): finite, and within the fp32 bound of the reference's fp64."""
    c = F.case("d")
    y32, gx32, g32 = F.forward_backward("d", F.loaded("d", torch.float32), torch.float32)
    y, gx, g = F.forward_backward("d", F.loaded("d", torch.float32, device=DEV), torch.float32, DEV)
    for name, a, r, t in [("y", y, y32, c["y"]), ("gx", gx, gx32, c["gx"])] + \
            [(k, g[k], g32[k], None) for k in g]:
        assert torch.isfinite(a).all(), name
        e_got, e_ref = (F.relerr(a, t), F.relerr(r, t)) if t is not None else \
            (F.grad_err("d", name, a), F.grad_err("d", name, r))
        print(f"d {name}: GPU {e_got:.2e} CPU fp32 {e_ref:.2e}")
        assert e_got <= max(1e-5, 2 * e_ref), f"{name}: GPU {e_got:.2e} vs fp64, CPU fp32 {e_ref:.2e}"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_two_launches_are_bitwise_equal(bf16):
    (q, k, v, gy), _, _ = _reference("corner", 64, 4, bf16)
    _, ei = _graph("corner")
    dt = torch.bfloat16 if bf16 else torch.float32
    a = _kernel(q.to(dt), k.to(dt), v.to(dt), gy.to(dt), ei.to(DEV), 4, True)
    b = _kernel(q.to(dt), k.to(dt), v.to(dt), gy.to(dt), ei.to(DEV), 4, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_whole_model_fp32_vs_reference_fixture(tag):
    c = F.case(tag)
    y32, gx32, _ = F.forward_backward(tag, F.loaded(tag, torch.float32), torch.float32)
    y, gx, g = F.forward_backward(tag, F.loaded(tag, torch.float32, device=DEV), torch.float32, DEV)
    e_got, e_ref = F.relerr(y, c["y"]), F.relerr(y32, c["y"])
    print(f"{tag} y: GPU {e_got:.2e} CPU fp32 {e_ref:.2e}")
    assert e_got <= max(1e-5, 2 * e_ref), f"forward: GPU {e_got:.2e} vs fp64, CPU fp32 {e_ref:.2e}"
    errs = {"gx": F.relerr(gx, c["gx"])}
    errs.update({k: F.grad_err(tag, k, v) for k, v in g.items()})
    print(f"{tag} gradients: max rel-L2 {max(errs.values()):.2e}")
    assert max(errs.values()) <= 1e-3, {k: e for k, e in errs.items() if e > 1e-3}


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_whole_model_bf16_vs_reference_fixture(tag):
    c = F.case(tag)
    yc, gxc, gc = F.forward_backward(tag, F.loaded(tag, torch.float32, torch.bfloat16), torch.float32)
    y, gx, g = F.forward_backward(tag, F.loaded(tag, torch.float32, torch.bfloat16, DEV), torch.float32, DEV)
    for name, a, r, t in [("y", y, yc, c["y"]), ("gx", gx, gxc, c["gx"])] + [(k, g[k], gc[k], None) for k in g]:
        e_got, e_ref = (F.relerr(a, t), F.relerr(r, t)) if t is not None else \
            (F.grad_err(tag, name, a), F.grad_err(tag, name, r))
        print(f"{tag} bf16 {name}: GPU {e_got:.2e} CPU bf16 autocast {e_ref:.2e}")
        assert e_got <= max(1e-2, 2 * e_ref), f"{name}: GPU {e_got:.2e} vs fp64, CPU bf16 autocast {e_ref:.2e}"


def test_empty_edge_set():
    """E = 0: the attention output is 0, so a block is x + proj(0) + gated_mlp(norm2(.)), forward and
    backward, without an error."""
    from graphphysics.models.layers import Transformer

    torch.manual_seed(3)
    blk = Transformer(64, 64, 4, compute_dtype=torch.float32)
    x = torch.randn(37, 64)
    ei = torch.zeros((2, 0), dtype=torch.int64)
    res = []
    for dev in ("cpu", DEV):
        m = blk.to(dev)
        xd = x.to(dev).clone().requires_grad_(True)
        y = m(xd, ei.to(dev))
        y.square().sum().backward()
        res.append((y.detach().cpu(), xd.grad.cpu(), [p.grad.cpu().clone() for p in m.parameters()]))
        m.zero_grad()
    blk = blk.to("cpu")
    with torch.no_grad():
        x1 = x + blk.attention.proj.bias
        want = x1 + blk.gated_mlp(blk.norm2(x1))
    torch.testing.assert_close(res[1][0], want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(res[1][1], res[0][1], rtol=1e-4, atol=1e-5)
    for a, b in zip(res[1][2], res[0][2]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


def _train_setup():
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    b = meshes.cylinder_batch(1, jitter=0.01)
    data = Data(edge_attr=None, **{k: torch.from_numpy(b[k]).to(DEV) for k in ("x", "y", "edge_index")})
    torch.manual_seed(0)
    m = EncodeTransformDecode(2, 11, 2, hidden_size=64, num_heads=4, compute_dtype=torch.float32)
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100)
    return sim, opt, sch, data


def test_captured_training_step_equals_eager_and_learns():
    """Simulator(edge_input_size=0) on EncodeTransformDecode, a batch without edge_attr: three captured
    TrainStep steps equal three eager ones (compared as test_captured_step_equals_eager_step), the
    fused AdamW updates one flat buffer, and the loss falls over 20 steps."""
    from graphphysics.training.optim import _flat_span
    from graphphysics.training.step import TrainStep

    res = []
    for graph in (False, True):
        sim, opt, sch, data = _train_setup()
        st = TrainStep(sim, opt, sch, data, graph=graph)
        losses = [float(st().item()) for _ in range(3)]
        torch.cuda.synchronize()
        ps = [p for p in opt.param_groups[0]["params"] if p.grad is not None]
        assert len(ps) == len(list(sim.parameters()))
        fp, fg = _flat_span(ps), _flat_span([p.grad for p in ps])
        assert fp is not None and fg is not None and fp.numel() == fg.numel() == sim.model._flat_params.numel()
        res.append((losses, [p.detach().clone() for p in sim.parameters()],
                    [b.detach().clone() for b in sim.buffers()], opt.param_groups[0]["step_count"], sch.last_epoch,
                    opt.param_groups[0]["lr"]))
        if not graph:
            more = [float(st().item()) for _ in range(17)]
            assert all(np.isfinite(losses + more)) and more[-1] < losses[0], (losses, more)
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
    for a, b in zip(res[0][1], res[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(res[0][2], res[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    assert res[0][3:] == res[1][3:] and res[1][3] == 3


def test_rollout_captured_equals_eager_with_a_transformer_model():
    """training/rollout.py on a Simulator without edge features: four autoregressive steps, replayed
    from a hipGraph and eager, give the same predictions."""
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    sim, _, _, data = _train_setup()
    sim.eval()
    frames = [Data(x=data.x.clone(), y=data.y.clone(), edge_index=data.edge_index, edge_attr=None) for _ in range(4)]
    preds = [Rollout(sim, 2, graph=graph).rollout(frames) for graph in (False, True)]
    torch.cuda.synchronize()
    assert preds[0].shape[:2] == (4, data.x.shape[0]) and torch.isfinite(preds[0]).all()
    torch.testing.assert_close(preds[1], preds[0], rtol=1e-5, atol=1e-6)
