"""Mixture-density head without a GPU: DiagonalGaussianMixtureNLLLoss, masked_gmm_nll, DiagonalGMMHead, the
EncodeTransformDecode that carries it and sample_gmm_diagonal against fixtures written by the reference's own
code in fp64 (tests/golden/make_gmm_golden.py), and the host side of libmgn's mgn_gmm_* ABI."""
import os

import pytest
import torch

import _gmm_fixture as G


def _run(fn, c, **kw):
    net = c["net"].clone().requires_grad_(True)
    loss = fn(c["target"], net, c["node_type"], c["masks"], **kw)
    (g,) = torch.autograd.grad(loss, net, allow_unused=True)
    return loss.detach(), g if g is not None else torch.zeros_like(net)


@pytest.mark.parametrize("tag", G.LOSS_CASES)
def test_fp64_loss_and_gradient_reproduce_the_reference(tag):
    """The reference's class and the capture-safe form, loss and d loss / d network_output, to 1e-12
    relative; the empty mask (case e) gives exactly 0 and an all-zero gradient."""
    from graphphysics.utils.loss import DiagonalGaussianMixtureNLLLoss, masked_gmm_nll

    c = G.loss_case(tag)
    d, K, T = c["d"], c["K"], c["temperature"]
    cls = DiagonalGaussianMixtureNLLLoss(d, K, T)
    assert cls.__name__ == "GaussianMixtureNLLLossDiag" and cls.per_comp == 2 * d + 1
    for name, (loss, g) in (("class", _run(cls, c)),
                            ("masked", _run(lambda t, o, nt, m: masked_gmm_nll(t, o, nt, m, d, K, T), c))):
        assert loss.dim() == 0
        if tag == "e":  # (the class returns the reference's torch.tensor(0.0) there: torch's default dtype)
            assert float(loss) == 0.0 and not g.any(), name
            continue
        assert loss.dtype == torch.float64
        torch.testing.assert_close(loss, c["loss"], rtol=1e-12, atol=0, msg=f"{tag} {name} loss")
        err = G.relerr(g, c["grad"])
        print(tag, name, "gradient rel-L2", err)
        assert err <= 1e-12, (tag, name, err)
        # entry by entry too: 1e-12 of the gradient's largest entry
        assert float((g - c["grad"]).abs().max()) <= 1e-12 * float(c["grad"].abs().max())


def test_selected_indexes_are_excluded_by_the_class():
    from graphphysics.utils.loss import DiagonalGaussianMixtureNLLLoss

    c = G.loss_case("a")
    cls = DiagonalGaussianMixtureNLLLoss(c["d"], c["K"], c["temperature"])
    sel = torch.nonzero(G.row_mask(c["node_type"], c["masks"])).flatten()[:3]
    keep = G.row_mask(c["node_type"], c["masks"])
    keep[sel] = False
    want, _ = G.nll_formula(c["net"], c["target"], keep, c["d"], c["K"], c["temperature"])
    got = cls(c["target"], c["net"], c["node_type"], c["masks"], selected_indexes=sel)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0)


def test_explicit_count_scales_the_loss_as_one_over_count():
    from graphphysics.utils.loss import masked_gmm_nll

    c = G.loss_case("c")
    n = float(G.row_mask(c["node_type"], c["masks"]).sum())
    for count in (1.0, n, 3.5 * n):
        fn = lambda t, o, nt, m: masked_gmm_nll(t, o, nt, m, c["d"], c["K"], c["temperature"],  # noqa: E731
                                                count=torch.tensor([count], dtype=torch.float64))
        loss, g = _run(fn, c)
        torch.testing.assert_close(loss, c["loss"] * n / count, rtol=1e-12, atol=0)
        assert G.relerr(g, c["grad"] * n / count) <= 1e-12
    zero, g = _run(lambda t, o, nt, m: masked_gmm_nll(t, o, nt, m, c["d"], c["K"], c["temperature"],
                                                       count=torch.zeros(1, dtype=torch.float64)), c)
    assert float(zero) == 0.0 and not g.any()


def test_masked_out_rows_cannot_poison_the_capture_safe_form():
    """A NaN / inf in a row of another node type changes neither the loss nor the gradient of the rest."""
    from graphphysics.utils.loss import masked_gmm_nll

    c = dict(G.loss_case("a"))
    out = torch.nonzero(~G.row_mask(c["node_type"], c["masks"])).flatten()
    net = c["net"].clone()
    net[out[0]] = float("nan")
    net[out[1]] = float("inf")
    c["net"] = net
    loss, g = _run(lambda t, o, nt, m: masked_gmm_nll(t, o, nt, m, c["d"], c["K"], c["temperature"]), c)
    torch.testing.assert_close(loss, c["loss"], rtol=1e-12, atol=0)
    assert torch.isfinite(g).all() and G.relerr(g, c["grad"]) <= 1e-12


def test_head_keys_shapes_and_default_init_match_the_reference():
    from graphphysics.models.layers import DiagonalGMMHead

    c = G.model_case()
    torch.manual_seed(0)
    m = G.make_model()
    head = m.decode_module
    assert isinstance(head, DiagonalGMMHead)
    assert (head.d, head.K, head.temperature, head.per_component) == (2, 3, 0.5, 5)
    assert (m.d, m.K, m.temperature, m.use_diagonal) == (2, 3, 0.5, True)
    assert list(head.state_dict()) == ["pre_proj.weight", "pre_proj.bias", "proj.weight", "proj.bias"]
    assert tuple(head.proj.weight.shape) == (15, 24) and tuple(head.pre_proj.weight.shape) == (24, 24)
    sd = m.state_dict()
    assert list(sd) == list(c["w"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(c["w"][k].shape), k
        v = v.double()
        torch.testing.assert_close(torch.stack([v.sum(), (v * v).sum()]), c["init"][k], rtol=1e-12, atol=1e-12, msg=k)


def test_mixture_model_keeps_one_flat_parameter_and_gradient_span():
    from graphphysics.training.distributed import flat_grad_buffer

    m = G.loaded_model(torch.float32)
    n = sum(p.numel() for p in m.parameters())
    assert m._flat_params.numel() == n
    assert all(p.untyped_storage().data_ptr() == m._flat_params.untyped_storage().data_ptr() for p in m.parameters())
    G.model_forward_backward(m, torch.float32)
    flat = flat_grad_buffer(list(m.parameters()))
    assert flat is not None and flat.numel() == n


def test_model_case_fp64_reproduces_the_reference():
    """Output, NLL and every parameter gradient at the bound test_transformer_cpu.py uses for its cases a
    and b: 1e-10 rel-L2, after a strict weight load."""
    c = G.model_case()
    y, nll, grads = G.model_forward_backward(G.loaded_model(torch.float64), torch.float64)
    assert tuple(y.shape) == (23, 15)
    errs = {"y": G.relerr(y, c["y"]), "nll": G.relerr(nll, c["nll"])}
    assert set(grads) == set(c["g"])
    errs.update({k: G.grad_err(k, g) for k, g in grads.items()})
    print("model case max rel-L2", max(errs.values()))
    assert max(errs.values()) <= 1e-10, {k: e for k, e in errs.items() if e > 1e-10}


def test_model_case_bf16_is_autocast_with_fp32_output_and_gradients():
    c = G.model_case()
    m = G.loaded_model(torch.float32, compute_dtype=torch.bfloat16)
    y, _, grads = G.model_forward_backward(m, torch.float32)
    assert y.dtype == torch.float32 and all(g.dtype == torch.float32 for g in grads.values())
    assert 1e-5 < G.relerr(y, c["y"]) < 5e-2


@pytest.mark.parametrize("tag", ["a", "c", "d"])
def test_cpu_sampler_is_the_inverse_cdf_rule(tag):
    from graphphysics.models.simulator import sample_gmm_diagonal

    c = G.loss_case(tag)
    n, d, K, T = c["net"].shape[0], c["d"], c["K"], c["temperature"]
    g = torch.Generator().manual_seed(11)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    u[:3] = torch.tensor([0.0, 1.0 - 2.0 ** -53, 0.5])
    z = torch.randn(n, d, generator=g, dtype=torch.float64)
    comp, want, cdf = G.sample_formula(c["net"], d, K, T, u, z)
    # the rule, once more, by a plain loop
    for i in range(n):
        k = next((k for k in range(K) if cdf[i, k] > u[i]), K - 1)
        assert k == int(comp[i])
    got = sample_gmm_diagonal(c["net"], d, K, T, u=u, z=z)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, d)
    torch.testing.assert_close(got, want, rtol=1e-14, atol=0)
    assert len(set(comp.tolist())) > 1 or K == 1
    # u beyond the running sum's end: the last component catches it
    last = sample_gmm_diagonal(c["net"], d, K, T, u=torch.full((n,), 2.0, dtype=torch.float64), z=z)
    p = c["net"].reshape(n, K, 2 * d + 1)[:, K - 1]
    torch.testing.assert_close(last, p[:, 1:1 + d] + T * torch.exp(p[:, 1 + d:]) * z, rtol=1e-14, atol=0)


def test_default_noise_is_drawn_with_torch_and_follows_the_seed():
    from graphphysics.models.simulator import sample_gmm_diagonal

    c = G.loss_case("a")
    net = c["net"].float()
    torch.manual_seed(5)
    a = sample_gmm_diagonal(net, 3, 3, 0.7)
    b = sample_gmm_diagonal(net, 3, 3, 0.7)
    torch.manual_seed(5)
    a2 = sample_gmm_diagonal(net, 3, 3, 0.7)
    assert torch.equal(a, a2) and not torch.equal(a, b) and a.dtype == torch.float32


def test_simulator_evaluation_samples_then_builds_outputs():
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.utils.data import Data

    c = G.model_case()
    torch.manual_seed(1)
    m = EncodeTransformDecode(1, 11, 2, hidden_size=24, num_heads=2, num_mixture_components=3, temperature=0.5)
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, torch.device("cpu"))
    x = torch.randn(23, 5, generator=torch.Generator().manual_seed(2))
    x[:, 2] = c["node_type"].float()
    data = Data(x=x, y=torch.randn(23, 2, generator=torch.Generator().manual_seed(3)), edge_attr=None,
                edge_index=c["edge_index"])
    sim.train()
    net, tdn, out = sim(data)
    assert tuple(net.shape) == (23, 15) and out is None
    sim.eval()
    with torch.no_grad():
        net, tdn, out = sim(data)
    assert tuple(net.shape) == (23, 2) and tuple(out.shape) == (23, 2)
    torch.testing.assert_close(out, sim._build_outputs(data, net))


def test_constructor_limits():
    from graphphysics.models.processors import EncodeProcessDecode, EncodeTransformDecode

    kw = dict(hidden_size=24, num_heads=2, num_mixture_components=3)
    with pytest.raises(NotImplementedError, match="temperature"):
        EncodeTransformDecode(1, 7, 2, **kw)
    with pytest.raises(NotImplementedError, match="use_diagonal=False"):
        EncodeTransformDecode(1, 7, 2, temperature=1.0, use_diagonal=False, **kw)
    with pytest.raises(NotImplementedError, match="EncodeProcessDecode"):
        EncodeProcessDecode(1, 7, 3, 2, hidden_size=32, num_mixture_components=3, temperature=1.0)
    assert EncodeTransformDecode(1, 7, 2, temperature=1.0, **kw).K == 3
    assert EncodeTransformDecode(1, 7, 2, hidden_size=24, num_heads=2).K == 0  # the MLP decoder, as before


def test_shape_mismatch_is_an_error():
    from graphphysics.models.simulator import sample_gmm_diagonal
    from graphphysics.utils.loss import masked_gmm_nll

    c = G.loss_case("a")
    with pytest.raises(ValueError):
        masked_gmm_nll(c["target"], c["net"], c["node_type"], c["masks"], 3, 2, 1.0)
    with pytest.raises(ValueError):
        sample_gmm_diagonal(c["net"], 2, 3, 1.0)


# ----------------------------------------------------------------------------- ABI (no device)
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    return nat.load()


def test_gmm_symbols_and_abi_version(lib):
    from graphphysics import _native as nat
    from graphphysics.utils import loss as L

    assert lib.mgn_abi_version() == 17 == nat.ABI_VERSION
    for name in ("mgn_gmm_nll_workspace_bytes", "mgn_gmm_nll_diag", "mgn_gmm_nll_diag_backward", "mgn_gmm_sample_diag"):
        assert name in nat.EXPORTS and getattr(lib, name) is not None
    assert "MGN_HAS_GMM 1" in open(os.path.join(G.GOLDEN, "..", "..", "include", "mgn.h")).read()
    assert lib.mgn_gmm_nll_workspace_bytes(1) > 0
    assert {"DiagonalGaussianMixtureNLLLoss", "masked_gmm_nll"} <= set(L.__all__)


@pytest.mark.parametrize("d,K,word", [(3, 0, "K"), (3, 17, "K"), (0, 3, "d"), (9, 3, "d")])
def test_gmm_entry_points_reject_unsupported_shapes_before_any_launch(lib, d, K, word):
    # the pointers are never dereferenced: the shape check comes first
    rc = lib.mgn_gmm_nll_diag(None, None, 10, d, K, 1.0, None, 1, 1, None, None, None, None, 1 << 20, None)
    assert rc != 0 and f" {word} " in lib.mgn_last_error().decode()
    rc = lib.mgn_gmm_nll_diag_backward(None, None, 10, d, K, 1.0, None, 1, 1, None, None, None, None)
    assert rc != 0 and f" {word} " in lib.mgn_last_error().decode()
    rc = lib.mgn_gmm_sample_diag(None, 10, d, K, 1.0, None, None, None, None)
    assert rc != 0 and f" {word} " in lib.mgn_last_error().decode()
