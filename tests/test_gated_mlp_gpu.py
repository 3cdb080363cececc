"""The fused gated-MLP kernels (mgn_gated_mlp_forward / _backward, dense="libmgn") on the GPU.

Truth: the torch composition x + m.gated_mlp(m.norm2(x)) in fp64 on the CPU. Yardstick: the same composition
in fp32 on the CPU (fp32 kernels) or under torch.autocast("cpu", bfloat16) (bf16 kernels). Bound, the suite's
rule: rel-L2 error vs fp64 <= max(floor, 2 x the yardstick's error), floor 1e-5 (fp32) / 1e-2 (bf16), for y,
dx and each of the eight parameter gradients. Weights and inputs are rounded to bf16-exact values first.

Row counts come from the tile size and grid rule _native exposes: 1, T-1, T+1, 257 at every hidden size. More
row tiles than the launch has workgroups, so that the tile loop iterates and carries its state from tile to
tile, are reached two ways: with the default grid at T * (the grid's cap) + 1 rows at h = 16, and, at one h per
kernel width and more (16, 24, 64, 128, 256), with the descriptor's max_blocks = 2 at 4T + 1 rows (workgroup 0
takes tiles 0, 2, 4, workgroup 1 tiles 1, 3). An odd h (23) and an x whose base is one float off a 16-byte
boundary cover the kernels' scalar row loads."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _transformer_fixture as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HIDDEN = [16, 24, 64, 128, 256]
KEYS = ["norm2.scale", "gated_mlp.0.scale", "gated_mlp.1.linear1.weight", "gated_mlp.1.linear1.bias",
        "gated_mlp.1.linear2.weight", "gated_mlp.1.linear2.bias", "gated_mlp.2.weight", "gated_mlp.2.bias"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _bf16_exact(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _block(h, seed=0):
    """A Transformer block (fp32, CPU) with bf16-exact parameters and non-trivial norm scales."""
    from graphphysics.models.layers import Transformer

    torch.manual_seed(seed)
    m = Transformer(h, h, 1, compute_dtype=torch.float32, dense="libmgn")
    with torch.no_grad():
        m.norm2.scale.copy_(1 + 0.3 * torch.randn(h))
        m.gated_mlp[0].scale.copy_(1 + 0.3 * torch.randn(h))
        for p in m.parameters():
            p.copy_(_bf16_exact(p))
    return m


def _params(m):
    d = dict(m.named_parameters())
    return [d[k] for k in KEYS]


def _compose(m, x, gy, autocast=False):
    """(y, dx, the eight parameter gradients) of the torch composition on the CPU in m's dtype."""
    import contextlib

    x = x.clone().requires_grad_(True)
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        y = x + m.gated_mlp(m.norm2(x))
    if gy is None:
        return [y.detach()]
    g = torch.autograd.grad(y, [x] + _params(m), gy.to(y.dtype))
    return [y.detach()] + [t.detach() for t in g]


def _kernel(m, x, gy, dtype):
    """The same through Transformer._dense_half on the GPU."""
    import copy

    md = copy.deepcopy(m).float().to(DEV).set_compute_dtype(dtype)
    xd = x.float().to(DEV).requires_grad_(True)
    y = md._dense_half(xd)
    if gy is None:
        return [y.detach()]
    g = torch.autograd.grad(y, [xd] + _params(md), gy.float().to(DEV))
    torch.cuda.synchronize()
    return [y.detach()] + [t.detach() for t in g]


@functools.lru_cache(maxsize=None)
def _case(h, rows, seed=0):
    """Inputs and the CPU results (fp64 truth, fp32 and bf16-autocast yardsticks), computed once."""
    import copy

    m = _block(h, seed)
    g = torch.Generator().manual_seed(100 + seed)
    x = _bf16_exact(torch.randn(rows, h, generator=g))
    gy = _bf16_exact(torch.randn(rows, h, generator=g))
    truth = _compose(copy.deepcopy(m).double(), x.double(), gy.double())
    y32 = _compose(m, x, gy)
    ybf = _compose(m, x, gy, autocast=True)
    return m, x, gy, truth, y32, ybf


def _check(got, truth, yard, floor, what):
    names = ["y", "dx"] + KEYS
    bad = {}
    for n, a, t, r in zip(names, got, truth, yard):
        assert torch.isfinite(a).all(), f"{what} {n}: not finite"
        e_got, e_ref = F.relerr(a, t), F.relerr(r, t)
        print(f"{what} {n}: GPU {e_got:.2e} yardstick {e_ref:.2e}")
        if not e_got <= max(floor, 2 * e_ref):
            bad[n] = (e_got, e_ref)
    assert not bad, f"{what}: (GPU error, yardstick error) vs fp64 {bad}"


def _row_counts():
    from graphphysics import _native as nat

    T = nat.gated_mlp_row_tile()
    return T, [1, T - 1, T + 1, 257]


def _many_tiles():
    """A row count with more tiles than the launch has workgroups."""
    from graphphysics import _native as nat

    T = nat.gated_mlp_row_tile()
    cap = nat.gated_mlp_blocks(1 << 40)  # the default grid's cap
    rows = T * cap + 1
    assert -(-rows // T) > nat.gated_mlp_blocks(rows)
    return rows


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ri", range(4))
@pytest.mark.parametrize("h", HIDDEN)
def test_op_vs_fp64_composition(h, ri, bf16):
    rows = _row_counts()[1][ri]
    m, x, gy, truth, y32, ybf = _case(h, rows)
    got = _kernel(m, x, gy, torch.bfloat16 if bf16 else torch.float32)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"h={h} rows={rows}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_op_with_more_tiles_than_workgroups(bf16):
    rows = _many_tiles()
    m, x, gy, truth, y32, ybf = _case(16, rows)
    got = _kernel(m, x, gy, torch.bfloat16 if bf16 else torch.float32)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"h=16 rows={rows}")


def _c_interface(m, x, gy, bf16, pad=0, max_blocks=0, offset=0):
    """(y, dx, the eight gradients) through mgn_gated_mlp_forward / _backward directly: x, y and dy in buffers
    with row stride h + pad (the padding pre-filled, y's checked afterwards), x's base `offset` floats into its
    buffer, the row-tile kernels' grid capped at max_blocks workgroups."""
    from graphphysics import _native as nat

    rows, h = x.shape
    ps = [p.detach().to(DEV).contiguous() for p in _params(m)]
    sa, sb, w1, b1, w2, b2, w3, b3 = ps
    desc = nat.gated_mlp_desc(h, nat.MGN_BF16 if bf16 else nat.MGN_F32, w1, b1, w2, b2, w3, b3, sa, sb,
                              max_blocks=max_blocks)
    L = nat.lib()
    ld = h + pad
    xbuf = torch.full((rows * ld + offset,), 7.0, device=DEV)
    xb = xbuf[offset:].view(rows, ld)
    xb[:, :h] = x.to(DEV)
    gb = torch.full((rows, ld), 5.0, device=DEV)
    gb[:, :h] = gy.to(DEV)
    yb = torch.full((rows, ld), -3.0, device=DEV)
    saved = torch.empty(int(L.mgn_gated_mlp_saved_bytes(ctypes.byref(desc), rows)), dtype=torch.uint8, device=DEV)
    st = nat.stream_ptr(DEV)
    nat.check(L.mgn_gated_mlp_forward(ctypes.byref(desc), nat.ptr(xb), ld, rows, nat.ptr(yb), ld, nat.ptr(saved), st))
    wsb = int(L.mgn_gated_mlp_backward_workspace_bytes(ctypes.byref(desc), rows))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dx = torch.empty((rows, h), device=DEV)
    G = torch.empty(sum(p.numel() for p in ps), device=DEV)
    nat.check(L.mgn_gated_mlp_backward(ctypes.byref(desc), nat.ptr(xb), ld, rows, nat.ptr(saved), nat.ptr(gb), ld,
                                       nat.ptr(dx), nat.ptr(G), nat.ptr(ws), wsb, st))
    torch.cuda.synchronize()
    assert torch.equal(yb[:, h:], torch.full((rows, pad), -3.0, device=DEV)), "y written past hidden"
    got, o = [yb[:, :h], dx], 0
    for p in ps:
        got.append(G[o:o + p.numel()].view(p.shape))
        o += p.numel()
    return got


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_strided_x_y_dy(bf16):
    """ld > h for x, y and dy, through the C interface (the autograd node always allocates a dense y)."""
    h, rows = 24, _row_counts()[0] + 1
    m, x, gy, truth, y32, ybf = _case(h, rows)
    got = _c_interface(m, x, gy, bf16, pad=8)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"strided h={h} rows={rows}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", HIDDEN)
def test_tile_loop_at_every_kernel_width(h, bf16):
    """Two workgroups over five row tiles (max_blocks = 2, 4T + 1 rows): each workgroup runs its tile loop more
    than once — restaging the weights after the previous tile's readers, carrying the scale gradients'
    column sums — at every kernel width."""
    from graphphysics import _native as nat

    T = _row_counts()[0]
    rows = 4 * T + 1
    assert nat.gated_mlp_blocks(rows, 2) == 2 < -(-rows // T)
    m, x, gy, truth, y32, ybf = _case(h, rows)
    got = _c_interface(m, x, gy, bf16, max_blocks=2)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"max_blocks=2 h={h} rows={rows}")
    # y and dx are per-row results: the grid does not change a bit of them
    ref = _c_interface(m, x, gy, bf16)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_odd_hidden_size(bf16):
    """h = 23: no row of x, dy or a weight starts on a 16-byte boundary, every row load is scalar."""
    rows = _row_counts()[0] + 1
    m, x, gy, truth, y32, ybf = _case(23, rows)
    got = _kernel(m, x, gy, torch.bfloat16 if bf16 else torch.float32)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"h=23 rows={rows}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_x_off_a_16_byte_boundary(bf16):
    """h = 64 with x's base one float past a 16-byte boundary: the scalar path of the x row loads at a hidden
    size that otherwise takes the 16-byte one; the same bits as the aligned call."""
    rows = _row_counts()[0] + 1
    m, x, gy, truth, y32, ybf = _case(64, rows)
    got = _c_interface(m, x, gy, bf16, offset=1)
    _check(got, truth, ybf if bf16 else y32, 1e-2 if bf16 else 1e-5, f"unaligned x h=64 rows={rows}")
    for a, b in zip(got, _c_interface(m, x, gy, bf16)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", [16, 64, 256])
def test_every_chunk_of_the_expanded_dimension_is_used_once(h, bf16):
    """W1 = 0, b1 = linspace(0.5, 2, 3h), W2 = 0, b2 = 1, W3 = 1, b3 = 0: every y[r, i] - x[r, i] is
    Σ_j GELU(b1_j); a dropped or doubled 16-column chunk moves it by at least 16 / 3h."""
    m = _block(h)
    g = m.gated_mlp
    b1 = torch.linspace(0.5, 2, 3 * h)
    with torch.no_grad():
        g[1].linear1.weight.zero_()
        g[1].linear1.bias.copy_(b1)
        g[1].linear2.weight.zero_()
        g[1].linear2.bias.fill_(1.0)
        g[2].weight.fill_(1.0)
        g[2].bias.zero_()
    want = float(torch.nn.functional.gelu(b1.double()).sum())
    x = _bf16_exact(torch.randn(70, h, generator=torch.Generator().manual_seed(5)))
    y = _kernel(m, x, None, torch.bfloat16 if bf16 else torch.float32)[0].cpu().double()
    err = float(((y - x.double()) - want).abs().max() / want)
    print(f"h={h} {'bf16' if bf16 else 'fp32'}: max relative error of the chunk sum {err:.2e}")
    assert err <= (2e-3 if bf16 else 1e-5)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", [24, 64, 256])
def test_every_row_and_column_is_routed(h, bf16):
    """W1 = 0, b1 = c, b2 = 0, W2[j, :] = unit vector (j mod h), W3[i, j] = [j mod h = i]:
    y = x + 3 GELU(c) n with n the double RMSNorm; a misfiled column is an O(1) error."""
    import copy

    m = _block(h)
    g = m.gated_mlp
    c = 0.75
    j = torch.arange(3 * h)
    with torch.no_grad():
        g[1].linear1.weight.zero_()
        g[1].linear1.bias.fill_(c)
        g[1].linear2.weight.zero_()
        g[1].linear2.weight[j, j % h] = 1.0
        g[1].linear2.bias.zero_()
        g[2].weight.zero_()
        g[2].weight[j % h, j] = 1.0
        g[2].bias.zero_()
    rows = _row_counts()[0] + 7
    x = _bf16_exact(torch.randn(rows, h, generator=torch.Generator().manual_seed(6)))
    md = copy.deepcopy(m).double()
    with torch.no_grad():
        n = md.gated_mlp[0](md.norm2(x.double()))
        truth = x.double() + 3 * torch.nn.functional.gelu(torch.tensor(c, dtype=torch.float64)) * n
    assert F.relerr(_compose(md, x.double(), None)[0], truth) < 1e-12
    yard = _compose(m, x, None, autocast=bf16)
    got = _kernel(m, x, None, torch.bfloat16 if bf16 else torch.float32)
    _check(got, [truth], yard, 1e-2 if bf16 else 1e-5, f"routing h={h}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_zero_rows_forward(bf16):
    """All-zero rows of x: n = 0, y = b3 + W3 (GELU(b1) ⊙ b2), finite and within the bound (forward only)."""
    import copy

    h, rows = 64, _row_counts()[0] + 3
    m = _block(h)
    x = _bf16_exact(torch.randn(rows, h, generator=torch.Generator().manual_seed(7)))
    x[::3] = 0
    x[-1] = 0
    truth = _compose(copy.deepcopy(m).double(), x.double(), None)
    got = _kernel(m, x, None, torch.bfloat16 if bf16 else torch.float32)
    _check(got, truth, _compose(m, x, None, autocast=bf16), 1e-2 if bf16 else 1e-5, "zero rows")
    g = m.gated_mlp
    with torch.no_grad():
        want = g[2].bias.double() + g[2].weight.double() @ (torch.nn.functional.gelu(g[1].linear1.bias.double())
                                                            * g[1].linear2.bias.double())
    assert F.relerr(got[0][0], want) <= (1e-2 if bf16 else 1e-5)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_two_launches_are_bitwise_equal(bf16):
    m, x, gy = _block(64), None, None
    g = torch.Generator().manual_seed(8)
    x, gy = torch.randn(1100, 64, generator=g), torch.randn(1100, 64, generator=g)  # several tiles and row slabs
    dt = torch.bfloat16 if bf16 else torch.float32
    a, b = _kernel(m, x, gy, dt), _kernel(m, x, gy, dt)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_inference_forward_equals_training_forward(bf16):
    import copy

    m = _block(24)
    dt = torch.bfloat16 if bf16 else torch.float32
    x = torch.randn(131, 24, generator=torch.Generator().manual_seed(9))
    y_train = _kernel(m, x, None, dt)[0]
    md = copy.deepcopy(m).to(DEV).set_compute_dtype(dt)
    with torch.no_grad():
        y_inf = md._dense_half(x.to(DEV))
    assert torch.equal(y_inf, y_train)


def test_autograd_node_checks_versions_and_runs_twice():
    """x and the parameters are saved through save_for_backward: a retained graph gives the same gradients a
    second time, and a backward after an in-place change of x is refused (the backward recomputes from x)."""
    import copy

    m = copy.deepcopy(_block(24)).to(DEV)
    x0 = torch.randn(70, 24, generator=torch.Generator().manual_seed(11)).to(DEV)
    gy = torch.ones(70, 24, device=DEV)
    x = x0.clone().requires_grad_(True)
    y = m._dense_half(x)
    a = torch.autograd.grad(y, [x] + _params(m), gy, retain_graph=True)
    b = torch.autograd.grad(y, [x] + _params(m), gy)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    xl = x0.clone().requires_grad_(True)
    xc = xl * 1.0
    y = m._dense_half(xc)
    xc.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_whole_model_fp32_vs_reference_fixture(tag):
    c = F.case(tag)
    y32, gx32, _ = F.forward_backward(tag, F.loaded(tag, torch.float32), torch.float32)
    m = F.loaded(tag, torch.float32, device=DEV).set_dense("libmgn")
    y, gx, g = F.forward_backward(tag, m, torch.float32, DEV)
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
    m = F.loaded(tag, torch.float32, torch.bfloat16, DEV).set_dense("libmgn")
    y, gx, g = F.forward_backward(tag, m, torch.float32, DEV)
    for name, a, r, t in [("y", y, yc, c["y"]), ("gx", gx, gxc, c["gx"])] + [(k, g[k], gc[k], None) for k in g]:
        e_got, e_ref = (F.relerr(a, t), F.relerr(r, t)) if t is not None else \
            (F.grad_err(tag, name, a), F.grad_err(tag, name, r))
        print(f"{tag} bf16 {name}: GPU {e_got:.2e} CPU bf16 autocast {e_ref:.2e}")
        assert e_got <= max(1e-2, 2 * e_ref), f"{name}: GPU {e_got:.2e} vs fp64, CPU bf16 autocast {e_ref:.2e}"


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
    m = EncodeTransformDecode(2, 11, 2, hidden_size=64, num_heads=4, compute_dtype=torch.float32, dense="libmgn")
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100)
    return sim, opt, sch, data


def test_captured_training_step_equals_eager_and_learns():
    """Three captured TrainStep steps of a dense="libmgn" model equal three eager ones, at the tolerances of
    test_transformer_gpu's test of the same name, and the loss falls over 30 steps. A forward that read stale
    weights after AdamW would part from the eager run at the second step."""
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
        more = [float(st().item()) for _ in range(27)]
        assert all(np.isfinite(losses + more)) and more[-1] < losses[0], (graph, losses, more)
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
    for a, b in zip(res[0][1], res[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(res[0][2], res[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    assert res[0][3:] == res[1][3:] and res[1][3] == 3


def test_rollout_captured_equals_eager():
    """A captured Rollout of a dense="libmgn" model equals the eager one
    (test_rollout_captured_equals_eager_with_a_transformer_model's tolerances)."""
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    sim, _, _, data = _train_setup()
    sim.eval()
    frames = [Data(x=data.x.clone(), y=data.y.clone(), edge_index=data.edge_index, edge_attr=None) for _ in range(4)]
    preds = [Rollout(sim, 2, graph=graph).rollout(frames) for graph in (False, True)]
    torch.cuda.synchronize()
    assert preds[0].shape[:2] == (4, data.x.shape[0]) and torch.isfinite(preds[0]).all()
    torch.testing.assert_close(preds[1], preds[0], rtol=1e-5, atol=1e-6)
