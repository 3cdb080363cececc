"""Mixture-density head on the GPU: libmgn's mgn_gmm_nll_diag / _backward / mgn_gmm_sample_diag against an fp64
evaluation of the formulas written out in tests/_gmm_fixture.py, determinism, the empty mask, the whole model
against the reference's fp64 fixture, and captured training / rollout with a mixture model.

Bound of the kernel tests (not chosen in advance): the same formula evaluated with PyTorch fp32 ops on the same
inputs (CPU) has a measured error against fp64; the kernel may be 2x as far (the suite's usual margin over a
same-precision torch evaluation) plus an absolute floor of 1e-6 of the gradient's largest entry (for the loss:
of the loss itself, about 8 fp32 ulps — what a fixed-order fp32 sum over the rows may lose). Errors are the
largest absolute difference over the entries."""
import functools

import numpy as np
import pytest
import torch

import _gmm_fixture as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MASKS = [0, 5]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _native_nll(net, target, node_type, masks, d, K, T, count=None, grad_loss=None, strided=True):
    """(loss, gradient) of masked_gmm_nll on the device; the node types are a strided column of a wider x."""
    from graphphysics.utils.loss import masked_gmm_nll

    rows = net.shape[0]
    if strided:
        x = torch.zeros(rows, 5, device=DEV)
        x[:, 2] = node_type.float().to(DEV)
        nt = x[:, 2]
        assert nt.stride(0) == 5
    else:
        nt = node_type.float().to(DEV)
    n = net.float().to(DEV).requires_grad_(True)
    cnt = torch.tensor([count], dtype=torch.float32, device=DEV) if count is not None else None
    loss = masked_gmm_nll(target.float().to(DEV), n, nt, masks, d, K, T, count=cnt)
    assert type(loss.grad_fn).__name__.startswith("_NativeMaskedGMMNLL"), "the native path must run"
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), n.grad.cpu().double()


def _check(label, got, truth, ref32, count_factor=1.0, grad_loss=1.0):
    """got, truth, ref32: (loss, grad); truth and ref32 are evaluated for count = Σ mask and grad_loss = 1.
    count_factor = Σ mask / count scales loss and gradient, grad_loss the gradient: exact factors in fp64, and the
    fp32 evaluation's error scales by their magnitude."""
    (lk, gk), (l64, g64), (l32, g32) = got, truth, ref32
    assert torch.isfinite(lk) and torch.isfinite(gk).all(), label
    sl, sg = count_factor, count_factor * abs(grad_loss)
    e_l, r_l = float((lk - l64 * count_factor).abs()), float((l32.double() - l64).abs()) * sl
    e_g = float((gk - g64 * count_factor * grad_loss).abs().max())
    r_g = float((g32.double() - g64).abs().max()) * sg
    gmax, lmag = float(g64.abs().max()) * sg, float(l64.abs()) * sl
    print(f"{label}: loss kernel {e_l:.3e} torch-fp32 {r_l:.3e} (|loss| {lmag:.3e}); gradient kernel {e_g:.3e} "
          f"torch-fp32 {r_g:.3e} (max |g| {gmax:.3e})")
    assert e_l <= 2 * r_l + 1e-6 * lmag, f"{label} loss: kernel {e_l:.3e} vs fp64, torch fp32 {r_l:.3e}"
    assert e_g <= 2 * r_g + 1e-6 * gmax, f"{label} gradient: kernel {e_g:.3e} vs fp64, torch fp32 {r_g:.3e}"


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_kernel_matches_fp64_on_the_fixture_cases(tag):
    """Truth: the reference's own fp64 loss and gradient (fixture). Measured on an MI355X (largest absolute
    error, kernel / torch fp32 on the CPU):
      a  loss 1.3e-06 / 1.3e-06 (|loss| 17.1)     gradient 5.4e-06 / 5.4e-06 (max |g| 10.9)
      b  loss 1.9e-07 / 1.9e-07 (|loss| 3.68)     gradient 9.8e-08 / 2.0e-07 (max |g| 6.0)
      c  loss 3.5e-07 / 1.2e-07 (|loss| 4.06)     gradient 1.1e-08 / 8.7e-09 (max |g| 0.030)
      d  loss 8.1e-02 / 1.8e-02 (|loss| 5.9e+05)  gradient 2.07 / 1.95 (max |g| 2.9e+07)"""
    c = G.loss_case(tag)
    d, K, T = c["d"], c["K"], c["temperature"]
    mask = G.row_mask(c["node_type"], c["masks"])
    ref32 = G.nll_formula(c["net"].float(), c["target"].float(), mask, d, K, T)
    assert torch.isfinite(ref32[0]) and torch.isfinite(ref32[1]).all()  # the generator keeps case d finite in fp32
    got = _native_nll(c["net"], c["target"], c["node_type"], c["masks"], d, K, T)
    _check(f"fixture {tag}", got, (c["loss"], c["grad"]), ref32)


@functools.lru_cache(maxsize=None)
def _random_case(rows, K, d):
    """Inputs and the CPU evaluations (fp64 truth, fp32 torch) of one random case, computed once. Logits and
    means ~ N(0, 1), log-stds ~ N(-0.5, 0.5²), targets 1.5 standard normals from a random component's mean."""
    g = torch.Generator().manual_seed(100000 * K + 1000 * d + rows % 997)
    net = torch.randn(rows, K, 2 * d + 1, generator=g)
    net[..., 1 + d:] = -0.5 + 0.5 * net[..., 1 + d:]
    pick = torch.randint(0, K, (rows,), generator=g)
    target = net[torch.arange(rows), pick, 1:1 + d] + 1.5 * torch.randn(rows, d, generator=g)
    node_type = torch.randint(0, 7, (rows,), generator=g).float()
    if rows == 1:
        node_type[0] = 5.0
    net = net.reshape(rows, -1)
    T = 0.5 + 0.25 * (K % 3)
    mask = G.row_mask(node_type, MASKS)
    truth = G.nll_formula(net.double(), target.double(), mask, d, K, T)
    ref32 = G.nll_formula(net, target, mask, d, K, T)
    return net, target, node_type, T, float(mask.sum()), truth, ref32


@pytest.mark.parametrize("K,d", [(1, 1), (3, 3), (5, 2), (16, 8)])
@pytest.mark.parametrize("rows", [1, 257, 16411])
def test_kernel_matches_fp64_on_random_inputs(rows, K, d):
    """rows: one thread; one block plus one row; more blocks than the partial-sum grid (64) with a ragged tail.
    Node types are a strided column; with and without an explicit count, with and without grad_loss. Measured
    on an MI355X (largest absolute error, kernel / torch fp32 on the CPU, count = Σ mask, grad_loss = 1;
    loss | gradient, with |loss| and max |g| in brackets):
      rows     (K, d) = (1, 1)                   (3, 3)                         (5, 2)                         (16, 8)
      1      6.1e-09/6.1e-09 [1.26]          7.2e-08/7.2e-08 [12.2]         4.7e-07/4.7e-07 [8.74]         6.0e-06/1.7e-06 [38.5]
             4.0e-08/4.0e-08 [0.71]          2.2e-06/2.2e-06 [12.5]         1.6e-06/1.5e-06 [5.07]         1.7e-06/5.5e-06 [43.6]
      257    1.1e-07/1.1e-07 [7.15]          1.7e-06/2.1e-06 [42.7]         3.0e-08/3.0e-08 [5.58]         2.7e-06/4.9e-06 [37.7]
             1.2e-07/1.4e-07 [1.35]          3.0e-06/1.4e-05 [5.03]         3.3e-07/3.0e-07 [0.40]         1.6e-06/1.5e-06 [1.25]
      16411  1.3e-07/1.3e-07 [9.31]          1.7e-06/1.7e-06 [32.5]         3.3e-07/6.3e-07 [5.84]         1.1e-06/2.8e-06 [38.5]
             3.5e-08/3.9e-08 [0.44]          9.1e-07/9.1e-07 [0.24]         3.6e-08/3.8e-08 [0.023]        2.4e-07/1.9e-07 [0.037]"""
    net, target, node_type, T, n, truth, ref32 = _random_case(rows, K, d)
    for count, gl in ((None, None), (2.5 * n + 3.0, None), (None, 0.37), (max(n - 1.0, 1.0), -3.0)):
        fl = n / count if count is not None else 1.0
        got = _native_nll(net, target, node_type, MASKS, d, K, T, count=count, grad_loss=gl)
        _check(f"rows={rows} K={K} d={d} count={count} grad_loss={gl}", got, truth, ref32, fl,
               gl if gl is not None else 1.0)


def test_contiguous_node_types_equal_the_strided_column():
    net, target, node_type, T, *_ = _random_case(257, 3, 3)
    a = _native_nll(net, target, node_type, MASKS, 3, 3, T, strided=True)
    b = _native_nll(net, target, node_type, MASKS, 3, 3, T, strided=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_two_launches_are_bitwise_equal():
    net, target, node_type, T, *_ = _random_case(16411, 3, 3)
    a = _native_nll(net, target, node_type, MASKS, 3, 3, T)
    b = _native_nll(net, target, node_type, MASKS, 3, 3, T)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_mask_gives_zero_loss_and_zero_gradient():
    """Fixture case e and a larger random case no node type of which is masked in: 0, zeros, no NaN — also with
    an explicit count of 0, and with rows whose parameters are not finite."""
    c = G.loss_case("e")
    loss, g = _native_nll(c["net"], c["target"], c["node_type"], c["masks"], c["d"], c["K"], c["temperature"])
    assert float(loss) == 0.0 and not g.any() and tuple(g.shape) == tuple(c["net"].shape)
    net, target, node_type, T, *_ = _random_case(16411, 5, 2)
    net = net.clone()
    net[7] = float("nan")
    net[300] = float("inf")
    for masks, count in (([7, 8], None), (MASKS, 0.0)):
        loss, g = _native_nll(net, target, node_type, masks, 2, 5, T, count=count)
        assert float(loss) == 0.0 and not g.any()


# ----------------------------------------------------------------------------- sampler
@functools.lru_cache(maxsize=None)
def _sampler_case(rows, K):
    """fp32 parameters, u, z and the fp64 rule's (component, sample) plus the fp32 torch evaluation's sample. u is
    uniform, except where it lies within 1e-4 of a boundary of the fp64 CDF: there it moves to the middle of the
    row's widest component (an fp32 running sum of at most 16 terms is off by about 1e-6)."""
    d = 8 if K == 16 else 3
    g = torch.Generator().manual_seed(77 * K + rows % 997)
    net = torch.randn(rows, K, 2 * d + 1, generator=g)
    net[..., 0] *= 2.0
    net = net.reshape(rows, -1)
    u = torch.rand(rows, generator=g)
    z = torch.randn(rows, d, generator=g)
    cdf = torch.cumsum(torch.softmax(net.double().reshape(rows, K, -1)[..., 0], dim=-1), dim=-1)
    lo = torch.cat([torch.zeros(rows, 1, dtype=torch.float64), cdf[:, :-1]], dim=1)
    width = cdf - lo
    wide = width.argmax(dim=1, keepdim=True)
    mid = (lo.gather(1, wide) + 0.5 * width.gather(1, wide)).squeeze(1).float()
    inner = cdf[:, :-1]  # the last boundary decides nothing: the last component catches the rest
    close = ((inner - u.double()[:, None]).abs() < 1e-4).any(dim=1) if K > 1 else torch.zeros(rows, dtype=torch.bool)
    u = torch.where(close, mid, u)
    if K > 1:
        assert float((inner - u.double()[:, None]).abs().min()) >= 1e-4
    comp, want, _ = G.sample_formula(net.double(), d, K, 0.8, u.double(), z.double())
    comp32, ref32, _ = G.sample_formula(net, d, K, 0.8, u, z)
    assert torch.equal(comp, comp32)
    return d, net, u, z, comp, want, ref32


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("rows", [1, 257, 16411])
def test_sampler_picks_the_fp64_component_in_every_row(rows, K):
    """Every row uses the component of the fp64 rule; the values at the bound of the kernel tests. Measured on an
    MI355X (largest absolute error, kernel / torch fp32 on the CPU, largest |out| 2.4 to 91): rows 1: 3.4e-07 /
    3.4e-07, 1.2e-07 / 1.2e-07, 1.5e-07 / 3.2e-07 for K = 1, 3, 16; rows 257: 1.6e-06 / 1.6e-06, 8.8e-07 / 9.9e-07,
    1.3e-06 / 1.3e-06; rows 16411: 4.1e-06 / 3.6e-06, 4.0e-06 / 4.5e-06, 6.0e-06 / 6.0e-06."""
    from graphphysics.models.simulator import sample_gmm_diagonal

    d, net, u, z, comp, want, ref32 = _sampler_case(rows, K)
    got = sample_gmm_diagonal(net.to(DEV), d, K, 0.8, u=u.to(DEV), z=z.to(DEV))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, d)
    got = got.cpu().double()
    # which component a row used: the one whose sample is nearest (components are distinct random draws)
    p = net.double().reshape(rows, K, 2 * d + 1)
    every = p[..., 1:1 + d] + 0.8 * torch.exp(p[..., 1 + d:]) * z.double()[:, None, :]
    used = (every - got[:, None, :]).abs().amax(dim=2).argmin(dim=1)
    assert torch.equal(used, comp), f"{int((used != comp).sum())} rows picked another component"
    if rows > 1 and K > 1:
        assert len(set(comp.tolist())) == K
    e_got, e_ref = float((got - want).abs().max()), float((ref32.double() - want).abs().max())
    print(f"sampler rows={rows} K={K}: kernel {e_got:.3e} torch-fp32 {e_ref:.3e} (max |out| {float(want.abs().max()):.3e})")
    assert e_got <= 2 * e_ref + 1e-6 * float(want.abs().max())


def test_sampler_default_noise_advances():
    from graphphysics.models.simulator import sample_gmm_diagonal

    d, net, *_ = _sampler_case(257, 3)
    torch.manual_seed(3)
    a = sample_gmm_diagonal(net.to(DEV), d, 3, 0.8)
    b = sample_gmm_diagonal(net.to(DEV), d, 3, 0.8)
    torch.manual_seed(3)
    a2 = sample_gmm_diagonal(net.to(DEV), d, 3, 0.8)
    assert torch.equal(a, a2) and not torch.equal(a, b) and torch.isfinite(a).all()


# ----------------------------------------------------------------------------- whole model
def test_whole_model_fp32_vs_reference_fixture():
    """Bounds of test_transformer_gpu.py's whole-model test: the output (and here the NLL) no further from fp64
    than max(1e-5, 2x the CPU fp32 run); every parameter gradient rel-L2 <= 1e-3."""
    c = G.model_case()
    y32, nll32, _ = G.model_forward_backward(G.loaded_model(torch.float32), torch.float32)
    y, nll, g = G.model_forward_backward(G.loaded_model(torch.float32, device=DEV), torch.float32, DEV)
    assert y.dtype == torch.float32
    for name, a, r, t in (("y", y, y32, c["y"]), ("nll", nll, nll32, c["nll"])):
        e_got, e_ref = G.relerr(a, t), G.relerr(r, t)
        print(f"mixture model {name}: GPU {e_got:.2e} CPU fp32 {e_ref:.2e}")
        assert e_got <= max(1e-5, 2 * e_ref), f"{name}: GPU {e_got:.2e} vs fp64, CPU fp32 {e_ref:.2e}"
    errs = {k: G.grad_err(k, v) for k, v in g.items()}
    print(f"mixture model gradients: max rel-L2 {max(errs.values()):.2e}")
    assert max(errs.values()) <= 1e-3, {k: e for k, e in errs.items() if e > 1e-3}


def test_whole_model_bf16_vs_reference_fixture():
    """Bound of test_transformer_gpu.py's bf16 whole-model test: no further from fp64 than max(1e-2, 2x the same
    bf16 autocast run on the CPU); the output is fp32."""
    c = G.model_case()
    yc, nllc, gc = G.model_forward_backward(G.loaded_model(torch.float32, torch.bfloat16), torch.float32)
    y, nll, g = G.model_forward_backward(G.loaded_model(torch.float32, torch.bfloat16, DEV), torch.float32, DEV)
    assert y.dtype == torch.float32 and all(v.dtype == torch.float32 for v in g.values())
    for name, a, r, t in [("y", y, yc, c["y"]), ("nll", nll, nllc, c["nll"])] + [(k, g[k], gc[k], None) for k in g]:
        e_got, e_ref = (G.relerr(a, t), G.relerr(r, t)) if t is not None else (G.grad_err(name, a), G.grad_err(name, r))
        print(f"mixture model bf16 {name}: GPU {e_got:.2e} CPU bf16 autocast {e_ref:.2e}")
        assert e_got <= max(1e-2, 2 * e_ref), f"{name}: GPU {e_got:.2e} vs fp64, CPU bf16 autocast {e_ref:.2e}"


# ----------------------------------------------------------------------------- training and rollout
def _setup(K=3, temperature=0.5):
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    b = meshes.cylinder_batch(1, jitter=0.01)
    data = Data(edge_attr=None, **{k: torch.from_numpy(b[k]).to(DEV) for k in ("x", "y", "edge_index")})
    torch.manual_seed(0)
    m = EncodeTransformDecode(2, 11, 2, hidden_size=64, num_heads=4, num_mixture_components=K,
                              temperature=temperature, compute_dtype=torch.float32)
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100)
    return sim, opt, sch, data


def test_train_step_loss_is_the_mixture_nll_of_the_models_output():
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.loss import masked_gmm_nll

    sim, opt, sch, data = _setup()
    sim.train()
    got = TrainStep(sim, opt, sch, data, graph=False)._loss()
    assert type(got.grad_fn).__name__.startswith("_NativeMaskedGMMNLL")
    sim2, _, _, _ = _setup()  # the same seed: the same weights and normalizer state
    sim2.train()
    net, tdn, _ = sim2(data)
    assert tuple(net.shape) == (data.x.shape[0], 15)
    want = G.nll_formula(net.detach().cpu().double(), tdn.cpu().double(), G.row_mask(data.x[:, 2].cpu(), MASKS), 2, 3,
                         0.5)[0]
    np.testing.assert_allclose(float(got.detach()), float(want), rtol=1e-5)
    assert float(masked_gmm_nll(tdn, net, data.x[:, 2], MASKS, 2, 3, 0.5).detach()) == float(got.detach())


def test_captured_training_step_equals_eager_and_learns():
    """TrainStep on the mixture model uses masked_gmm_nll: three captured steps equal three eager ones (loss,
    parameters, normalizer buffers, AdamW moments; tolerances of test_transformer_gpu.py's captured-step test),
    parameters and gradients stay one flat span each, and the NLL falls over 30 steps on a fixed batch."""
    from graphphysics.training.optim import _flat_span
    from graphphysics.training.step import TrainStep

    res = []
    for graph in (False, True):
        sim, opt, sch, data = _setup()
        st = TrainStep(sim, opt, sch, data, graph=graph)
        losses = [float(st().item()) for _ in range(3)]
        torch.cuda.synchronize()
        ps = [p for p in opt.param_groups[0]["params"] if p.grad is not None]
        assert len(ps) == len(list(sim.parameters()))
        fp, fg = _flat_span(ps), _flat_span([p.grad for p in ps])
        assert fp is not None and fg is not None and fp.numel() == fg.numel() == sim.model._flat_params.numel()
        res.append((losses, [p.detach().clone() for p in sim.parameters()],
                    [b.detach().clone() for b in sim.buffers()],
                    [t.detach().clone() for t in opt.param_groups[0]["flat_state"]],
                    opt.param_groups[0]["step_count"], sch.last_epoch, opt.param_groups[0]["lr"]))
        if not graph:
            more = [float(st().item()) for _ in range(27)]
            assert all(np.isfinite(losses + more)) and more[-1] < losses[0], (losses, more)
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
    for a, b in zip(res[0][1], res[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(res[0][2], res[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    for a, b in zip(res[0][3], res[1][3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    assert res[0][4:] == res[1][4:] and res[1][4] == 3


def _frames(data, n=4):
    from graphphysics.utils.data import Data

    return [Data(x=data.x.clone(), y=data.y.clone(), edge_index=data.edge_index, edge_attr=None) for _ in range(n)]


def test_rollout_one_component_zero_temperature_captured_equals_eager():
    """K = 1, temperature 0: the sample is the component's mean whatever the noise, so the captured and the
    eager rollout agree at test_transformer_gpu.py's rollout tolerance."""
    from graphphysics.training.rollout import Rollout

    sim, _, _, data = _setup(K=1, temperature=0.0)
    sim.eval()
    frames = _frames(data)
    preds = [Rollout(sim, 2, graph=graph).rollout(frames) for graph in (False, True)]
    torch.cuda.synchronize()
    assert preds[0].shape == (4, data.x.shape[0], 2) and torch.isfinite(preds[0]).all()
    torch.testing.assert_close(preds[1], preds[0], rtol=1e-5, atol=1e-6)


def test_rollout_samples_inside_the_captured_graph():
    """K = 3, temperature 0.5: finite predictions, nodes outside NORMAL / OUTFLOW carry the target exactly, and
    two replays of the recorded step on the same frame and the same previous prediction differ, because the
    noise is drawn inside the graph and the generator advances with every replay."""
    from graphphysics.training.rollout import Rollout, build_mask

    sim, _, _, data = _setup(K=3, temperature=0.5)
    sim.eval()
    frames = _frames(data)
    for graph in (False, True):
        ro = Rollout(sim, 2, graph=graph)
        preds = ro.rollout(frames)
        torch.cuda.synchronize()
        assert preds.shape == (4, data.x.shape[0], 2) and torch.isfinite(preds).all()
        keep = build_mask(2, data)
        assert keep.any() and not keep.all()
        for p in preds:
            assert torch.equal(p[keep], data.y[keep])
    assert ro._graph is not None
    outs = []
    for _ in range(2):
        ro._sx.copy_(data.x)
        ro._sy.copy_(data.y)
        ro._last.copy_(preds[0])
        ro._graph.replay()
        outs.append(ro._gpred.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0][keep], outs[1][keep])
    assert not torch.equal(outs[0][~keep], outs[1][~keep])
