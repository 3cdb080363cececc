"""The node side of a block's data gradients, through mgn_node_grad (include/mgn.h): the chained kernel
(chain16_node_grad_kernel: one wave per 16-node tile, W0bᵀ ‖ W0cᵀ in LDS; bf16, h = 128) against the generic
node_grad_kernel and against references that use neither.

  dP_i[v] = Σ dZ0[k]            k in [col_ptr[v], col_ptr[v+1])       fp32, in edge order, then bf16
  dP_j[v] = Σ dZ0[row_perm[k]]  k in [row_ptr[v], row_ptr[v+1])
  dx      = dx_part + dP_i·W0b + dP_j·W0c

* impl 2 (chained) and impl 1 (generic) write the same bits of dx and dP8, on the corner graph of
  tests/_impulse.py, on a graph built here for the gather's group bookkeeping (N = 16·19 + 5, isolated nodes,
  degrees of exactly one group, of 2 groups + 3, of 1) and on N = 7, in both dx layouts, on the default grid and
  with a CU cap of 1 (one workgroup: a wave walks several tiles and reuses its LDS scratch);
* dP8 equals a CPU emulation (sequential fp32 adds in edge order, then bf16) bit for bit, rows [N, RP) are zero,
  rows >= N of a sentinel-filled dx are untouched, and dx is within one bf16 rounding of the fp64 value from the
  bf16 operands plus the fp32 accumulation bound: |dx − ref| <= 2⁻⁸ |ref| + 2·256·2⁻²⁴ Σ|a_k b_k| per element.

Inputs: random bf16 dZ0, dx_part and W0 from a fixed seed. Every graph has a few hundred nodes at most.
"""
import ctypes
import functools

import pytest
import torch

import _impulse as I

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 128
GROUP = 8  # edge rows per round trip of both kernels' gathers (node_grad_kernel SG, MGN_NG_SG)
SENTINEL = -12288.0  # bf16-exact, far outside the results' range


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


# --------------------------------------------------------------------------- graphs
BUILT_N = 16 * 19 + 5
ISOLATED = (3, 17, 200)
NODE_GROUP, NODE_LONG, NODE_ONE = 5, 40, 100  # degrees GROUP, 2 GROUP + 3, 1 (in and out)


def built_graph(seed=7):
    g = torch.Generator().manual_seed(seed)
    n = BUILT_N
    special = set(ISOLATED) | {NODE_GROUP, NODE_LONG, NODE_ONE}
    others = torch.tensor([v for v in range(n) if v not in special])

    def pick(k):
        return others[torch.randint(0, others.numel(), (k,), generator=g)]

    src, dst = [pick(4 * n)], [pick(4 * n)]
    for v, d in ((NODE_GROUP, GROUP), (NODE_LONG, 2 * GROUP + 3), (NODE_ONE, 1)):
        src += [pick(d), torch.full((d,), v)]  # d in-edges, d out-edges
        dst += [torch.full((d,), v), pick(d)]
    src += [torch.tensor([n - 1, 1])]  # the last node (ragged tile) has an out-edge and an in-edge
    dst += [torch.tensor([0, n - 1])]
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    return n, ei[:, torch.randperm(ei.shape[1], generator=g)]


def tiny_graph(seed=5):
    g = torch.Generator().manual_seed(seed)
    return 7, torch.randint(0, 7, (2, 20), generator=g)


GRAPHS = {"corner": I.corner_graph, "built": built_graph, "n7": tiny_graph}


def test_built_graph_has_the_degrees_it_is_built_for():
    n, ei = built_graph()
    outd, ind = torch.bincount(ei[0], minlength=n), torch.bincount(ei[1], minlength=n)
    assert n % 16 == 5
    for v in ISOLATED:
        assert int(ind[v]) == 0 and int(outd[v]) == 0
    for v, d in ((NODE_GROUP, GROUP), (NODE_LONG, 2 * GROUP + 3), (NODE_ONE, 1)):
        assert int(ind[v]) == d and int(outd[v]) == d
    assert int(ind[n - 1]) >= 1 and int(outd[n - 1]) >= 1


# --------------------------------------------------------------------------- one problem per graph
class Problem:
    """The topology, the packed W0 and the operands of one graph (device), with CPU copies for the references."""

    def __init__(self, name):
        from graphphysics import _native as nat
        from graphphysics.models._engine import GraphTopology

        self.n, ei = GRAPHS[name]()
        self.topo = GraphTopology(ei.to(DEV), self.n)
        self.e = int(ei.shape[1])
        self.rp = (self.n + 63) // 64 * 64
        g = torch.Generator().manual_seed(1234)
        self.dz0 = torch.randn(self.e, H, generator=g).to(torch.bfloat16)
        self.dx_part = torch.randn(self.n, H, generator=g).to(torch.bfloat16)
        self.w0 = (0.1 * torch.randn(H, 3 * H, generator=g)).to(torch.bfloat16)  # nn.Linear weight [out, in]
        L = nat.lib()
        elems = int(L.mgn_linear_pack_elems(H, 3 * H, nat.MGN_BF16))
        self.w32 = self.w0.float().to(DEV).contiguous()
        self.pack = torch.zeros(2 * elems, dtype=torch.bfloat16, device=DEV)
        job = nat.PackJob(self.w32.data_ptr(), self.pack.data_ptr(), self.pack.data_ptr() + 2 * elems, H, 3 * H,
                          nat.MGN_BF16, 0, 0, 0, 0, 0)
        jobs = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(DEV)
        nat.check(L.mgn_pack_weights(nat.ptr(jobs), 1, H * 3 * H, nat.stream_ptr(DEV)))
        self.mlp = nat.Mlp()
        m = self.mlp
        m.n_layers, m.in_dim, m.hidden, m.out_dim, m.has_norm, m.dtype = 4, 3 * H, H, H, 1, nat.MGN_BF16
        m.wpack, m.wtpack = self.pack.data_ptr(), self.pack.data_ptr() + 2 * elems
        self.dz0_d, self.dx_part_d = self.dz0.to(DEV), self.dx_part.to(DEV)
        torch.cuda.synchronize()
        nat.check_errors(DEV)
        self.col_ptr = self.topo.col_ptr.cpu().tolist()
        self.row_ptr = self.topo.row_ptr.cpu().tolist()
        self.row_perm = self.topo.row_perm.cpu().tolist()


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(name)


@functools.lru_cache(maxsize=None)
def run(name, pair, cap, impl):
    """(dx [RP, H] sentinel-filled before the call, dP8 flat [2 RP H] NaN-filled before it), on the CPU."""
    from graphphysics import _native as nat

    p = problem(name)
    dx = torch.full((p.rp, H), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dp8 = torch.full((2 * p.rp * H,), float("nan"), dtype=torch.bfloat16, device=DEV)
    nat.node_grad(p.topo.struct, p.mlp, p.dz0_d, p.dx_part_d, dp8, dx, dx_pair=pair, impl=impl, data_cus=cap)
    torch.cuda.synchronize()
    return dx.cpu(), dp8.cpu()


def bits(t):
    return t.contiguous().view(torch.int16)


def unpair(dx):
    """Row-major columns of pair-layout rows (feature 16t + 4g + r sits at 32(t>>1) + 8g + 4(t&1) + r)."""
    col = torch.empty(H, dtype=torch.long)
    for t in range(8):
        for g in range(4):
            for r in range(4):
                col[16 * t + 4 * g + r] = 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r
    return dx[:, col]


def rows_of_r8(dp8, rp):
    """[2, RP, H] from R8 [2][RP/8][H][8] (element (m, c) at ((m/8) H + c) 8 + m % 8)."""
    return dp8.view(2, rp // 8, H, 8).permute(0, 1, 3, 2).reshape(2, rp, H)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dP [2, N, H] bf16 from sequential fp32 adds in edge order, dx fp64, Σ|a_k b_k| fp64), computed once."""
    p = problem(name)
    z = p.dz0.float()
    dp = torch.zeros(2, p.n, H, dtype=torch.float32)
    for v in range(p.n):
        acc = torch.zeros(H, dtype=torch.float32)
        for k in range(p.col_ptr[v], p.col_ptr[v + 1]):
            acc = acc + z[k]
        dp[0, v] = acc
        acc = torch.zeros(H, dtype=torch.float32)
        for k in range(p.row_ptr[v], p.row_ptr[v + 1]):
            acc = acc + z[p.row_perm[k]]
        dp[1, v] = acc
    dp = dp.to(torch.bfloat16)
    w = p.w0.double()
    wb, wc = w[:, H:2 * H], w[:, 2 * H:]
    a = dp.double()
    dx = p.dx_part.double() + a[0] @ wb + a[1] @ wc
    mag = a[0].abs() @ wb.abs() + a[1].abs() @ wc.abs()
    return dp, dx, mag


CASES = [(name, pair, cap) for name in GRAPHS for pair in (False, True) for cap in (0, 1)]
IDS = [f"{n}-{'pair' if p else 'rows'}-{'cap1' if c else 'grid'}" for n, p, c in CASES]


# --------------------------------------------------------------------------- check 1
@pytest.mark.parametrize("name,pair,cap", CASES, ids=IDS)
def test_chained_equals_generic_bit_for_bit(name, pair, cap):
    from graphphysics import _native as nat

    dx_g, dp_g = run(name, pair, cap, nat.NODE_GRAD_GENERIC)
    dx_c, dp_c = run(name, pair, cap, nat.NODE_GRAD_CHAINED)
    n = problem(name).n
    assert torch.equal(bits(dp_c), bits(dp_g)), "dP8 differs from the generic kernel's"
    assert torch.equal(bits(dx_c[:n]), bits(dx_g[:n])), "dx differs from the generic kernel's"


# --------------------------------------------------------------------------- check 2
@pytest.mark.parametrize("impl", [1, 2], ids=["generic", "chained"])
@pytest.mark.parametrize("name,pair,cap", CASES, ids=IDS)
def test_against_independent_references(name, pair, cap, impl):
    p = problem(name)
    dx, dp8 = run(name, pair, cap, impl)
    dp_ref, dx_ref, mag = reference(name)
    dp = rows_of_r8(dp8, p.rp)
    assert torch.equal(bits(dp[:, :p.n]), bits(dp_ref)), "dP8 is not the sequential fp32 sum in edge order"
    assert bool((bits(dp[:, p.n:]) == 0).all()), "rows [N, RP) of dP8 must be zero"
    assert bool((dx[p.n:].float() == torch.tensor(SENTINEL, dtype=torch.bfloat16).float()).all()), \
        "rows >= N of dx were written"
    got = (unpair(dx[:p.n]) if pair else dx[:p.n]).double()
    assert bool(torch.isfinite(got).all())
    bound = 2.0 ** -8 * dx_ref.abs() + 2 * 256 * 2.0 ** -24 * mag
    over = (got - dx_ref).abs() - bound
    assert float(over.max()) <= 0.0, f"dx off by {float(over.max()):.3e} beyond the bound at {int(over.argmax())}"


def test_auto_writes_the_same_bits_and_the_chained_kernel_is_refused_where_it_does_not_apply():
    """impl 0 (the kernel the block backward would launch at this size) gives the same bits, as either kernel
    does; impl 2 on an fp32 MLP is an error, not a fallback."""
    from graphphysics import _native as nat

    dx_a, dp_a = run("n7", False, 0, nat.NODE_GRAD_AUTO)
    dx_c, dp_c = run("n7", False, 0, nat.NODE_GRAD_CHAINED)
    assert torch.equal(bits(dx_a[:7]), bits(dx_c[:7])) and torch.equal(bits(dp_a), bits(dp_c))
    p = problem("n7")
    m = nat.Mlp()
    m.n_layers, m.in_dim, m.hidden, m.out_dim, m.has_norm, m.dtype = 4, 3 * H, H, H, 1, nat.MGN_F32
    m.wpack, m.wtpack = p.mlp.wpack, p.mlp.wtpack
    buf = torch.zeros(2 * p.rp * H, dtype=torch.float32, device=DEV)
    rc = nat.lib().mgn_node_grad(ctypes.byref(p.topo.struct), ctypes.byref(m), nat.ptr(buf), nat.ptr(buf),
                                 nat.ptr(buf), nat.ptr(buf), 0, 2, None, nat.stream_ptr(DEV))
    assert rc != 0 and b"chained node_grad" in nat.lib().mgn_last_error()
