"""dense="torch" | "libmgn" without a device: validation, the CPU path (the torch composition under either
setting), unchanged parameters and keys, and the C interface's symbols and refusals."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native

    _native.load()
    return _native


def _model(dense, **kw):
    from graphphysics.models.processors import EncodeTransformDecode

    torch.manual_seed(0)
    return EncodeTransformDecode(2, 7, 2, hidden_size=24, num_heads=2, dense=dense, **kw)


def test_dense_is_validated():
    from graphphysics.models.layers import Transformer
    from graphphysics.models.processors import EncodeTransformDecode

    for bad in ("hip", "", None, "LIBMGN"):
        with pytest.raises(ValueError):
            Transformer(16, 16, 2, dense=bad)
        with pytest.raises(ValueError):
            EncodeTransformDecode(1, 7, 2, hidden_size=16, num_heads=2, dense=bad)
        with pytest.raises(ValueError):
            Transformer(16, 16, 2).set_dense(bad)
        with pytest.raises(ValueError):
            _model("torch").set_dense(bad)
    assert Transformer(16, 16, 2).dense == "torch" and _model("torch").dense == "torch"
    m = _model("torch").set_dense("libmgn")
    assert m.dense == "libmgn" and all(b.dense == "libmgn" for b in m.processor_list)
    assert all(b.dense == "libmgn" for b in _model("libmgn").processor_list)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cpu_tensors_run_the_torch_composition(dt):
    from graphphysics.utils.data import Data

    g = torch.Generator().manual_seed(1)
    x = torch.randn(19, 7, generator=g)
    ei = torch.randint(0, 19, (2, 60), generator=g)
    gy = torch.randn(19, 2, generator=g)
    out = []
    for dense in ("torch", "libmgn"):
        m = _model(dense, compute_dtype=dt)
        xi = x.clone().requires_grad_(True)
        y = m(Data(x=xi, edge_index=ei))
        (y * gy).sum().backward()
        out.append((y.detach(), xi.grad, [p.grad for p in m.parameters()]))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert len(out[0][2]) == len(out[1][2]) > 0
    for a, b in zip(out[0][2], out[1][2]):
        assert torch.equal(a, b)


def test_state_dict_and_initial_weights_do_not_depend_on_dense():
    a, b = _model("torch"), _model("libmgn")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a._flat_params.numel() == b._flat_params.numel()
    # the eight parameters of a block's dense half are contiguous in the flat buffer, in module order
    blk = b.processor_list[0]
    g = blk.gated_mlp
    ps = [blk.norm2.scale, g[0].scale, g[1].linear1.weight, g[1].linear1.bias, g[1].linear2.weight,
          g[1].linear2.bias, g[2].weight, g[2].bias]
    for p, q in zip(ps, ps[1:]):
        assert q.data_ptr() == p.data_ptr() + 4 * p.numel()


def test_abi_and_symbols(nat):
    L = nat.lib()
    assert L.mgn_abi_version() == 17
    with open(os.path.join(ROOT, "include", "mgn.h")) as f:
        header = f.read()
    assert "#define MGN_HAS_GATED_MLP 1" in header
    for name in ("mgn_gated_mlp_saved_bytes", "mgn_gated_mlp_forward", "mgn_gated_mlp_backward_workspace_bytes",
                 "mgn_gated_mlp_backward", "mgn_gated_mlp_row_tile", "mgn_gated_mlp_blocks"):
        assert name in header and hasattr(L, name)
    T = nat.gated_mlp_row_tile()
    assert T >= 16 and nat.gated_mlp_blocks(0) == 0 and nat.gated_mlp_blocks(1) == 1
    assert nat.gated_mlp_blocks(3 * T + 1, 2) == 2 and nat.gated_mlp_blocks(T, 2) == 1
    assert nat.gated_mlp_blocks(3 * T + 1) == 4 and nat.gated_mlp_blocks(1 << 40) == nat.gated_mlp_blocks(1 << 41)


def _desc(nat, h=16, expand=None, dtype=0, max_blocks=0, **null):
    fake = 0x10000  # never dereferenced: every refusal comes before a launch
    p = {k: (None if null.get(k) else fake) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "scale_a", "scale_b")}
    return nat.GatedMlp(h, 3 * h if expand is None else expand, dtype, h, max_blocks, 0, p["w1"], p["b1"], p["w2"],
                        p["b2"], p["w3"], p["b3"], p["scale_a"], p["scale_b"])


def _fwd(nat, d, x=0x10000, ldx=None, rows=5, y=0x10000, ldy=None):
    h = d.hidden
    return nat.lib().mgn_gated_mlp_forward(ctypes.byref(d), x, h if ldx is None else ldx, rows, y,
                                           h if ldy is None else ldy, None, None)


def _bwd(nat, d, rows=5, ws=0x10000, ws_bytes=None, x=0x10000, saved=0x10000, dy=0x10000, dx=0x10000, grads=0x10000):
    L = nat.lib()
    need = int(L.mgn_gated_mlp_backward_workspace_bytes(ctypes.byref(d), rows))
    return L.mgn_gated_mlp_backward(ctypes.byref(d), x, d.hidden, rows, saved, dy, d.hidden, dx, grads, ws,
                                    need if ws_bytes is None else ws_bytes, None)


def _err(nat):
    return nat.lib().mgn_last_error().decode()


def test_refusals_without_a_device(nat):
    for h in (0, 257, -3):
        assert _fwd(nat, _desc(nat, h)) != 0 and "hidden must be in [1, 256]" in _err(nat)
        assert _bwd(nat, _desc(nat, h)) != 0 and "hidden must be in [1, 256]" in _err(nat)
    assert _fwd(nat, _desc(nat, 16, expand=32)) != 0 and "must be 3 * hidden" in _err(nat)
    assert _bwd(nat, _desc(nat, 16, expand=64)) != 0 and "must be 3 * hidden" in _err(nat)
    assert _fwd(nat, _desc(nat, 16, dtype=2)) != 0 and "dtype must be MGN_F32 or MGN_BF16" in _err(nat)
    assert _bwd(nat, _desc(nat, 16, dtype=-1)) != 0 and "dtype must be MGN_F32 or MGN_BF16" in _err(nat)
    assert _fwd(nat, _desc(nat, 16, max_blocks=-1)) != 0 and "max_blocks must be >= 0" in _err(nat)
    assert _bwd(nat, _desc(nat, 16, max_blocks=-1)) != 0 and "max_blocks must be >= 0" in _err(nat)
    for k in ("w1", "b1", "w2", "b2", "w3", "b3", "scale_a", "scale_b"):
        assert _fwd(nat, _desc(nat, **{k: True})) != 0 and "NULL parameter pointer" in _err(nat)
        assert _bwd(nat, _desc(nat, **{k: True})) != 0 and "NULL parameter pointer" in _err(nat)
    assert nat.lib().mgn_gated_mlp_forward(None, 0x10000, 16, 5, 0x10000, 16, None, None) != 0
    assert "descriptor is NULL" in _err(nat)
    d = _desc(nat)
    assert _fwd(nat, d, x=None) != 0 and "NULL tensor" in _err(nat)
    assert _fwd(nat, d, y=None) != 0 and "NULL tensor" in _err(nat)
    assert _fwd(nat, d, ldx=15) != 0 and "must be >= hidden" in _err(nat)
    assert _fwd(nat, d, ldy=8) != 0 and "must be >= hidden" in _err(nat)
    assert _fwd(nat, d, rows=-1) != 0 and "rows must be >= 0" in _err(nat)
    for k in ("x", "saved", "dy", "dx", "grads"):
        assert _bwd(nat, d, **{k: None}) != 0 and "NULL tensor" in _err(nat)
    assert _bwd(nat, d, ws=None) != 0 and "NULL workspace" in _err(nat)
    need = int(nat.lib().mgn_gated_mlp_backward_workspace_bytes(ctypes.byref(d), 5))
    assert need > 0
    assert _bwd(nat, d, ws_bytes=need - 1) != 0 and "workspace too small" in _err(nat)
    # rows == 0: a no-op that returns 0, with nothing to read or write
    assert _fwd(nat, d, rows=0, x=None, y=None) == 0
    assert _bwd(nat, d, rows=0, ws=None, ws_bytes=0, x=None, saved=None, dy=None, dx=None, grads=None) == 0


def test_workspace_is_bounded_at_hidden_256(nat):
    """The partial weight-gradient slabs do not grow with the row count past their cap: beyond it the
    workspace grows only by the per-row operands."""
    d = _desc(nat, 256)
    L = nat.lib()
    w = [int(L.mgn_gated_mlp_backward_workspace_bytes(ctypes.byref(d), r)) for r in (1 << 16, 1 << 17, 1 << 18)]
    assert w[2] - w[1] == 2 * (w[1] - w[0])
    per_row = (w[1] - w[0]) / (1 << 16)
    assert w[0] - per_row * (1 << 16) < 64 * (1 << 20)  # slabs and column sums: under 64 MiB
