"""Impulse-response checks of the GraphNetBlock backward (test infrastructure).

The backward of a block (reference layers.py:667-746: edge MLP on [e ‖ x[col] ‖ x[row]], sum over col, node MLP
on [x ‖ aggr], two residuals) is LINEAR in the upstream gradient. With that gradient non-zero in one row only,
the input gradients may be non-zero only in the rows the graph predicts, and every other row is exactly 0.0 in
any number format (0 x ReLU mask = 0, the RMSNorm backward of a zero row is zero):

  impulse on e_out[k]:  dx ≠ 0 only on {src(k), dst(k)},          de ≠ 0 only on {k};
  impulse on x_out[v]:  dx ≠ 0 only on {v} ∪ src(in-edges of v),  de ≠ 0 only on the in-edges of v.

A contribution dropped or filed under another node is a support error (bit-exact criterion); one added twice is
a 100 % value error on a row that holds a single term.

This module holds what the CPU and the GPU tests share: the graphs (built for the tile bookkeeping of the
target-sorted edge order), models whose ReLU branches cannot flip under bf16 rounding (a single-row gradient
moves by 10-70 % on ONE flipped unit, which would drown the value check), the impulse positions, the predicted
supports, and the oracle (oracle/mgn_oracle.py) evaluated once per precision and differentiated per impulse.
"""
import torch

from oracle import mgn_oracle as O

LISTED_DEGREES = [0, 1, 15, 16, 17, 0, 31, 32, 33, 100, 2, 0, 64, 5]  # in-degrees of nodes 0..13
HUB = 20            # source of 130 re-sourced edges: out-edges in (nearly) every 16-row tile
CORNER_NODES = 101
CORNER_SEED = 3     # test_edge_agg_gpu's seed; the random bulk (randint(0, 8) per node) then gives E = 602
PATH_NODES = 60     # stack_graph: nodes 101..160


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


# --------------------------------------------------------------------------- graphs
def corner_graph(seed=CORNER_SEED):
    """(n, edge_index): 101 nodes, the listed in-degrees on nodes 0..13 (0, 1, one below / at / above one and
    two 16-row tiles, 64, 100), a random bulk of in-degree < 8, random sources, 130 random edges re-sourced to
    node HUB, a self-loop (first in-edge of node 4), a parallel pair (the first two in-edges of node 3 share
    their source), shuffled (the library sorts by target itself). Built as tests/test_edge_agg_gpu.py's
    _corner_graph. E = 602: no multiple of 16, 32 or 64, and more than three 192-row workgroup passes."""
    g = torch.Generator().manual_seed(seed)
    n = CORNER_NODES
    degs = LISTED_DEGREES + torch.randint(0, 8, (n - len(LISTED_DEGREES),), generator=g).tolist()
    dst = torch.cat([torch.full((d,), v, dtype=torch.long) for v, d in enumerate(degs)])
    e = dst.numel()
    src = torch.randint(0, n, (e,), generator=g)
    src[torch.randperm(e, generator=g)[:130]] = HUB
    first = torch.cumsum(torch.tensor([0] + degs), 0)
    src[first[4]] = 4                      # self-loop 4 -> 4
    src[first[3] + 1] = src[first[3]]      # parallel pair into node 3
    perm = torch.randperm(e, generator=g)
    return n, torch.stack([src[perm], dst[perm]])


def stack_graph(seed=CORNER_SEED):
    """The corner graph plus a disjoint bidirectional path on nodes 101..160 (its last link doubled: E = 722,
    a ragged last tile again), shuffled: the backward of b blocks spreads an impulse deep in the path over
    exactly 2b + 1 nodes, while the corner component (a hub, in-degrees up to 100) saturates — so the support
    assertion keeps its power on a stack."""
    n0, ei = corner_graph(seed)
    a = torch.arange(n0, n0 + PATH_NODES - 1)
    path = torch.cat([torch.stack([a, a + 1]), torch.stack([a + 1, a])], dim=1)
    path = torch.cat([path, path[:, [PATH_NODES - 2, 2 * PATH_NODES - 3]]], dim=1)
    ei = torch.cat([ei, path], dim=1)
    g = torch.Generator().manual_seed(seed + 1)
    return n0 + PATH_NODES, ei[:, torch.randperm(ei.shape[1], generator=g)]


# --------------------------------------------------------------------------- robust models
AGG_FACTOR = 1.0 / 32
"""The further factor on the aggregate columns of the node MLP's first Linear (an aggregate sums up to 100
unit-RMS messages). With 1/16 the smallest node layer-0 |pre-activation| on these graphs is 0.013 (h = 100),
0.08 (h = 128) and 0.04 (second block of the h = 32 stack): below the 0.25 margin the value checks rest on. With
1/32 it is >= 0.9 at every size and in every block (tests/test_block_impulse_cpu.py pins >= 0.25)."""


def _make_robust(block, h):
    with torch.no_grad():
        for name, seq in (("edge", block.edge_block), ("node", block.node_block)):
            for i in (0, 2, 4):  # the three hidden Linears
                seq[i].weight.mul_(0.25)
                seq[i].bias.copy_(2.0 - 4.0 * (torch.arange(seq[i].bias.numel()) % 2).float())
            if name == "node":
                seq[0].weight[:, h:2 * h].mul_(AGG_FACTOR)
            seq[7].scale.copy_(1.0 + 0.125 * (torch.arange(h) % 3).float())
        for p in block.parameters():
            p.copy_(bf16_exact(p))


def robust_block(h, seed=0):
    """A GraphNetBlock (default init under `seed`) whose hidden pre-activations stay clear of 0: hidden
    weights x 0.25, hidden biases ±2 alternating by unit, aggregate columns of the node MLP's first Linear a
    further x AGG_FACTOR, RMSNorm scales 1 + 0.125 (j % 3), every parameter a bf16-exact value."""
    from graphphysics.models.layers import GraphNetBlock

    torch.manual_seed(seed)
    blk = GraphNetBlock(h)
    _make_robust(blk, h)
    return blk


def robust_stack(mp, h, seed=0):
    """An only_processor EncodeProcessDecode of `mp` robust blocks."""
    from graphphysics.models.processors import EncodeProcessDecode

    torch.manual_seed(seed)
    m = EncodeProcessDecode(mp, h, h, h, h, only_processor=True)
    for blk in m.processor_list:
        _make_robust(blk, h)
    return m


def inputs(n, e, h, seed=1):
    """x [n, h], e [e, h]: randn rounded to bf16 (every path reads the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    return bf16_exact(torch.randn(n, h, generator=g)), bf16_exact(torch.randn(e, h, generator=g))


def impulse_vector(kind, idx, h):
    """The upstream gradient's one non-zero row: bf16-exact, random, a function of the position alone."""
    g = torch.Generator().manual_seed(100003 * (1 if kind == "edge" else 2) + idx)
    return bf16_exact(torch.randn(h, generator=g))


# --------------------------------------------------------------------------- positions, supports
def impulse_positions(ei, n):
    """(edge ids, node ids) in the CALLER's numbering. Edges by their position p in the target-sorted order the
    library works in (argsort(dst, stable)): both ends of every 16-row tile, the 32 / 64 / 192-row step
    boundaries, the last (ragged) tile and the one before it, the first and last in-edge of every
    listed-degree node (segments ending exactly on a tile among them), the hub's first and last out-edge, a
    self-loop, both copies of a parallel pair. Nodes: the listed degrees, the hub, tile-boundary ids, the last."""
    src, dst = ei[0], ei[1]
    e = ei.shape[1]
    order = torch.argsort(dst, stable=True)
    ps = {p for p in range(e) if p % 16 in (0, 15)}
    ps |= {p for p in (31, 32, 63, 64, 191, 192, 193) if p < e}
    ps |= set(range(max(e - 17, 0), e))
    col_ptr = torch.searchsorted(dst[order].contiguous(), torch.arange(n + 1))
    for v in range(len(LISTED_DEGREES)):
        lo, hi = int(col_ptr[v]), int(col_ptr[v + 1])
        if hi > lo:
            ps |= {lo, hi - 1}
    out = (src[order] == HUB).nonzero().flatten()
    ps |= {int(out[0]), int(out[-1])}
    eids = {int(order[p]) for p in ps}
    loops = (src == dst).nonzero().flatten()
    assert loops.numel() >= 1, "the graph has no self-loop"
    eids.add(int(loops[0]))
    key = src * n + dst
    _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    par = (cnt[inv] >= 2).nonzero().flatten()
    assert par.numel() >= 2, "the graph has no parallel edges"
    k0 = int(par[0])
    eids |= {k0, int((key == key[k0]).nonzero().flatten()[1])}
    return sorted(eids), _nodes(n)


def _nodes(n):
    return list(range(len(LISTED_DEGREES))) + [HUB, 15, 16, 63, 64, n - 1]


def stack_nodes(ei, n):
    """Node impulses for stack_graph: impulse_positions' nodes (n - 1 is the path's end), nodes deep in the
    path and at its start, and the targets of the edges at both ends of every 16-row tile and in the last 17
    positions of the target-sorted order — the last block's edge-MLP gradients of such an impulse are the
    outer products of that node's in-edge rows (everything farther is ~1e7 times smaller), so the row coverage
    of the edge weight-gradient kernels is checked at every tile boundary on the stack as well."""
    e = ei.shape[1]
    dst = ei[1][torch.argsort(ei[1], stable=True)]
    ends = {int(dst[p]) for p in range(e) if p % 16 in (0, 15) or p >= e - 17}
    base = _nodes(n) + [CORNER_NODES, CORNER_NODES + 1, CORNER_NODES + 29, CORNER_NODES + 30, n - 2]
    return base + sorted(ends - set(base))


def predicted_support(ei, kind, idx):
    """(rows of dx, rows of de) that may be — and, with half of all units open, are — non-zero for one block."""
    src, dst = ei[0], ei[1]
    if kind == "edge":
        return sorted({int(src[idx]), int(dst[idx])}), [idx]
    ins = (dst == idx).nonzero().flatten()
    return sorted({idx} | set(src[ins].tolist())), ins.tolist()


def nonzero_rows(t):
    return (t != 0).any(dim=1).nonzero().flatten().tolist()


# --------------------------------------------------------------------------- the oracle, per impulse
class OracleRun:
    """One forward of the oracle (block: mp=None; stack: encode_process_decode(..., only_processor), which
    composes graph_net_block mp times as processors.py does) in `mode` — "fp64", "fp32" or "autocast" (bf16, as
    the suite's bf16 yardstick) — kept for one backward per impulse. record: the hidden pre-activations."""

    def __init__(self, params, x, e, ei, mode, mp=None):
        dt = torch.float64 if mode == "fp64" else torch.float32
        self.p = {k: v.detach().to(dt).requires_grad_(True) for k, v in params.items()}
        self.x = x.detach().clone().to(dt).requires_grad_(True)  # a copy: the caller's x stays a plain tensor
        self.e = e.detach().clone().to(dt).requires_grad_(True)
        self.record = {}
        self.dt = dt
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=mode == "autocast"):
            if mp is None:
                self.x_out, self.e_out = O.graph_net_block(self.x, ei, self.e, self.p, record=self.record)
            else:
                self.x_out = O.encode_process_decode(self.x, ei, self.e, self.p, mp, only_processor=True,
                                                     record=self.record)
                self.e_out = None

    def grads(self, kind, idx, vec):
        """{"dx", "de", parameter keys...} for the upstream gradient `vec` in row idx of e_out / x_out."""
        out = self.e_out if kind == "edge" else self.x_out
        up = torch.zeros(out.shape, dtype=out.dtype)
        up[idx] = vec.to(out.dtype)
        keys = list(self.p)
        gs = torch.autograd.grad([out], [self.x, self.e] + [self.p[k] for k in keys], [up], retain_graph=True,
                                 allow_unused=True)
        gs = [torch.zeros_like(t) if g_ is None else g_
              for g_, t in zip(gs, [self.x, self.e] + [self.p[k] for k in keys])]
        return dict(zip(["dx", "de"] + keys, gs))


def relerr_rows(got, ref, rows=None):
    """rel-L2 over `rows` (a parameter gradient: the whole tensor)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    return float((got - ref).norm() / (ref.norm() + 1e-300))


# --------------------------------------------------------------------------- the assertions
def assert_support(grads, want_dx, want_de, what):
    """The non-zero rows of dx and de are exactly the wanted ones (both directions), and everything is finite."""
    for key, want in (("dx", want_dx), ("de", want_de)):
        assert bool(torch.isfinite(grads[key]).all()), f"{what}: {key} not finite"
        got = nonzero_rows(grads[key].detach().cpu())
        assert got == sorted(want), (f"{what}: non-zero rows of {key}: missing {sorted(set(want) - set(got))}, "
                                     f"unexpected {sorted(set(got) - set(want))}")


def hop_groups(ei, n, v, rows_dx, rows_de):
    """{name: (key, rows)}: the support rows of a node impulse at v by their distance from v along in-edges — a
    node's dx row by its own distance d >= 1 ("dx_hop{d}"), an edge's de row by the distance of its target
    ("de_hop{d}"). Each hop over an edge scales the gradient by the edge MLP's small Jacobian (~1e-7 here), and
    row v itself holds the residual's identity term, so a rel-L2 over the whole support only sees the nearest
    rows: the values are checked group by group as well."""
    src, dst = ei[0], ei[1]
    dist = torch.full((n,), -1, dtype=torch.long)
    dist[v] = 0
    frontier, d = torch.tensor([v]), 0
    while frontier.numel():
        d += 1
        nxt = torch.unique(src[torch.isin(dst, frontier)])
        frontier = nxt[dist[nxt] < 0]
        dist[frontier] = d
    out = {}
    for r in rows_dx:
        if int(dist[r]) >= 1:
            out.setdefault(f"dx_hop{int(dist[r])}", ("dx", []))[1].append(r)
    for k in rows_de:
        out.setdefault(f"de_hop{int(dist[dst[k]])}", ("de", []))[1].append(k)
    return out


def value_errors(got, ref64, yard, rows_dx, rows_de, groups=None):
    """{key: (rel-L2 of `got` vs fp64, rel-L2 of the yardstick evaluation vs fp64)}: dx and de on their support
    rows, every parameter gradient whole, and each of `groups` (hop_groups) on its rows."""
    out = {}
    for k in ref64:
        rows = rows_dx if k == "dx" else rows_de if k == "de" else None
        out[k] = (relerr_rows(got[k], ref64[k], rows), relerr_rows(yard[k], ref64[k], rows))
    for name, (k, rows) in (groups or {}).items():
        out[name] = (relerr_rows(got[k], ref64[k], rows), relerr_rows(yard[k], ref64[k], rows))
    return out


def assert_values(errs, floor, what):
    """The suite's rules: fp32 within max(1e-5, 2 x the fp32 CPU oracle's error), bf16 within max(1e-2, 2 x
    the autocast oracle's error), each rel-L2 against fp64 (floor = 1e-5 / 1e-2)."""
    for k, (e_got, e_yard) in errs.items():
        assert e_got <= max(floor, 2 * e_yard), f"{what} {k}: {e_got:.3e} vs fp64, yardstick {e_yard:.3e}"
