"""Transformer family without a GPU: the drop-in GatedMLP / Attention / Transformer /
EncodeTransformDecode against fixtures written by the reference's own code in fp64
(tests/golden/make_transformer_golden.py), and the host side of libmgn's graph-attention ABI."""
import ctypes

import pytest
import torch

import _transformer_fixture as F

CASES = ["a", "b", "c", "d"]


@pytest.mark.parametrize("tag", CASES)
def test_default_init_matches_reference_rng_order(tag):
    c = F.case(tag)
    torch.manual_seed(0)
    sd = F.make(tag).state_dict()
    assert list(sd) == list(c["w"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(c["w"][k].shape), k
        v = v.double()
        got = torch.stack([v.sum(), (v * v).sum()])
        torch.testing.assert_close(got, c["init"][k], rtol=1e-12, atol=1e-12, msg=k)


@pytest.mark.parametrize("tag", CASES)
def test_fp64_cpu_path_reproduces_reference(tag):
    """Outputs, input gradients and every parameter gradient to 1e-10 rel-L2 (strict weight load)."""
    c = F.case(tag)
    m = F.loaded(tag, torch.float64)
    y, gx, grads = F.forward_backward(tag, m, torch.float64)
    errs = {"y": F.relerr(y, c["y"]), "gx": F.relerr(gx, c["gx"])}
    assert set(grads) == set(c["g"])
    errs.update({k: F.grad_err(tag, k, g) for k, g in grads.items()})
    print(tag, "max rel-L2", max(errs.values()))
    assert max(errs.values()) <= 1e-10, {k: e for k, e in errs.items() if e > 1e-10}


def test_large_scores_are_shifted_before_exp():
    """Case d reaches scores of about ±60: fp32 exp(60)² would overflow a sum without the max shift."""
    c = F.case("d")
    y, gx, _ = F.forward_backward("d", F.loaded("d", torch.float32), torch.float32)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    assert F.relerr(y, c["y"]) <= 1e-4


def test_shared_projection_weight_is_one_parameter():
    m = F.make("b")
    n_sep = sum(p.numel() for p in F.make("a").parameters())
    for blk in m.processor_list:
        att = blk.attention
        assert att.k_proj.weight is att.q_proj.weight and att.v_proj.weight is att.q_proj.weight
    params = list(m.parameters())
    assert len({id(p) for p in params}) == len(params)
    n = sum(p.numel() for p in params)
    assert n == n_sep - 3 * 2 * 24 * 24
    assert m._flat_params.numel() == n  # the shared weight once in the flat buffer
    assert all(p.untyped_storage().data_ptr() == m._flat_params.untyped_storage().data_ptr() for p in params)
    sd = m.state_dict()
    for i in range(3):
        for k in ("q_proj", "k_proj", "v_proj"):
            assert f"processor_list.{i}.attention.{k}.weight" in sd


def test_gradients_land_in_one_flat_buffer():
    from graphphysics.training.distributed import flat_grad_buffer

    for tag in ("a", "b"):
        m = F.loaded(tag, torch.float32)
        F.forward_backward(tag, m, torch.float32)
        flat = flat_grad_buffer(list(m.parameters()))
        assert flat is not None and flat.numel() == m._flat_params.numel()


def test_return_attention_weights_sum_to_one_per_source_and_head():
    c = F.case("c")
    m = F.loaded("c", torch.float64)
    ei = c["edge_index"]
    out, attn = m(c["x"], ei, return_attention=True)
    assert F.relerr(out, c["y"]) <= 1e-10
    E, H = ei.shape[1], 4
    assert tuple(attn.shape) == (E, H) and (attn > 0).all()
    sums = torch.zeros(150, H, dtype=torch.float64).index_add(0, ei[0], attn)
    has = torch.zeros(150, dtype=torch.bool)
    has[ei[0]] = True
    assert not has.all()  # the fixture has a node without out-edges
    torch.testing.assert_close(sums[has], torch.ones_like(sums[has]), rtol=0, atol=1e-12)
    assert (sums[~has] == 0).all()


def test_constructor_limits_and_mixture_heads():
    from graphphysics.models.layers import Attention
    from graphphysics.models.processors import EncodeTransformDecode

    for kw in (dict(hidden_size=24, num_heads=3), dict(hidden_size=260, num_heads=4), dict(hidden_size=20, num_heads=8)):
        with pytest.raises(ValueError, match="num_heads in .*256"):
            EncodeTransformDecode(1, 7, 2, **kw)
    with pytest.raises(ValueError):
        Attention(32, 30, 4)
    with pytest.raises(NotImplementedError):
        EncodeTransformDecode(1, 7, 2, hidden_size=24, num_heads=2, num_mixture_components=3)


def test_bf16_compute_dtype_is_autocast_with_fp32_master_gradients():
    c = F.case("a")
    m = F.loaded("a", torch.float32, compute_dtype=torch.bfloat16)
    y, gx, grads = F.forward_backward("a", m, torch.float32)
    assert y.dtype == torch.float32 and all(g.dtype == torch.float32 for g in grads.values())
    assert 1e-5 < F.relerr(y, c["y"]) < 5e-2
    m.set_compute_dtype(torch.float32)
    assert F.relerr(F.forward_backward("a", m, torch.float32)[0], c["y"]) < 1e-5


# ----------------------------------------------------------------------------- ABI (no device)
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    return nat.load()


def test_graph_attention_symbols_and_abi_version(lib):
    from graphphysics import _native as nat

    assert lib.mgn_abi_version() == 17 == nat.ABI_VERSION
    for name in ("mgn_graph_attention_workspace_bytes", "mgn_graph_attention_forward",
                 "mgn_graph_attention_backward"):
        assert name in nat.EXPORTS and getattr(lib, name) is not None
    assert "MGN_HAS_GRAPH_ATTENTION 1" in open(F.os.path.join(F.GOLDEN, "..", "..", "include", "mgn.h")).read()


@pytest.mark.parametrize("hidden,heads,word", [(24, 3, "heads"), (260, 4, "hidden"), (20, 8, "multiple")])
def test_graph_attention_rejects_unsupported_shapes_before_any_launch(lib, hidden, heads, word):
    from graphphysics import _native as nat

    topo = nat.Topology(10, 20, 0, 0, 0, 0, 0, 0)  # never dereferenced: the shape check comes first
    for dt in (nat.MGN_F32, nat.MGN_BF16):
        rc = lib.mgn_graph_attention_forward(ctypes.byref(topo), None, None, None, hidden, hidden, heads, dt, None,
                                             None, None)
        assert rc != 0 and word in lib.mgn_last_error().decode()
        rc = lib.mgn_graph_attention_backward(ctypes.byref(topo), None, None, None, None, None, None, hidden, hidden,
                                              heads, dt, None, None, None, None, 0, None)
        assert rc != 0 and word in lib.mgn_last_error().decode()


@pytest.mark.parametrize("E,H", [(0, 4), (1, 1), (90, 2), (1400000, 8)])
def test_graph_attention_workspace_holds_two_floats_per_edge_and_head(lib, E, H):
    from graphphysics import _native as nat

    topo = nat.Topology(10, E, 0, 0, 0, 0, 0, 0)
    for dt in (nat.MGN_F32, nat.MGN_BF16):
        assert lib.mgn_graph_attention_workspace_bytes(ctypes.byref(topo), 64, H, dt) >= E * 2 * H * 4
