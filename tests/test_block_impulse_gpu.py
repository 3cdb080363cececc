"""Impulse responses of the GraphNetBlock backward on the GPU (tests/_impulse.py has the method).

One upstream-gradient row is non-zero per forward + backward. The rows of dx / de that come back non-zero must
be exactly the rows the graph predicts — a contribution of one edge dropped, or filed under another node
(node_grad's two segment sums by target and by source, the edge backward's gather of the node MLP's aggregate
gradient, a tile's ragged end, a pair-layout hand-off), changes that SET, and the criterion is bit-exact in
bf16 as in fp32. On those rows the values — single terms, so a doubled or missing one is an error of ~1 —
and every parameter gradient are held against the fp64 oracle with the suite's rules: fp32 within
max(1e-5, 2 x the fp32 CPU oracle's error), bf16 within max(1e-2, 2 x the autocast oracle's error). That rule
applies to a single row because the models' ReLU branches cannot flip (tests/test_block_impulse_cpu.py measures
the margins and that the predicted supports are the oracle's, without a GPU).

Single block: GraphNetBlock called directly (row-major in and out, mgn_block_backward) at every kernel width,
two padded sizes and both dtypes, on the corner graph (E = 602: ragged last tile, segments ending on a 16-row
tile, a source with out-edges in most tiles, a self-loop, parallel edges). Stack: an only_processor
EncodeProcessDecode on the engine's default switches (pair-layout hand-offs, deferred reduction, chained
projections, NULL for the last block's de), with recomputed edge inputs, with the edge-side sums, and in fp32.
"""
import functools

import pytest
import torch

import _impulse as I

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

BLOCK_CASES = [(torch.float32, 16), (torch.float32, 32), (torch.float32, 64), (torch.float32, 128),
               (torch.float32, 256), (torch.float32, 24), (torch.bfloat16, 64), (torch.bfloat16, 128),
               (torch.bfloat16, 256), (torch.bfloat16, 100)]
# (dtype, mp, h, _engine.REW, MGN_EDGE_AGG)
STACK_CASES = [(torch.bfloat16, 3, 128, "auto", None), (torch.bfloat16, 3, 128, "1", None),
               (torch.bfloat16, 3, 128, "auto", "1"), (torch.bfloat16, 3, 128, "auto", "bwd"),
               (torch.float32, 3, 128, "auto", None), (torch.float32, 2, 32, "auto", None)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _floor(dtype):
    return 1e-5 if dtype == torch.float32 else 1e-2


def _yard(dtype):
    return "fp32" if dtype == torch.float32 else "autocast"


def _collect(module, xd, ed):
    g = {"dx": xd.grad.detach().cpu(), "de": ed.grad.detach().cpu()}
    g.update({k: p.grad.detach().cpu() for k, p in module.named_parameters()})
    xd.grad = ed.grad = None
    module.zero_grad(set_to_none=True)
    return g


@functools.lru_cache(maxsize=None)
def _block_records(dtype, h):
    """Every impulse of the corner graph through one GraphNetBlock, one forward + backward each (the backward
    drops its saves). Kept per impulse: the non-zero rows, finiteness, whether the node MLP's parameter
    gradients are all exactly 0, the shapes, and the value errors (kernel, yardstick) against fp64."""
    n, ei = I.corner_graph()
    blk = I.robust_block(h)
    params = {k: v.detach().clone() for k, v in blk.named_parameters()}
    x, e = I.inputs(n, ei.shape[1], h)
    ref = I.OracleRun(params, x, e, ei, "fp64")
    yard = I.OracleRun(params, x, e, ei, _yard(dtype))
    blk.compute_dtype = dtype
    blk = blk.to(DEV)
    xd, ed, eid = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True), ei.to(DEV)
    eids, nodes = I.impulse_positions(ei, n)
    recs = []
    for kind, ids in (("edge", eids), ("node", nodes)):
        for i in ids:
            vec = I.impulse_vector(kind, i, h)
            x2, e2 = blk(xd, eid, ed)
            upx, upe = torch.zeros_like(x2), torch.zeros_like(e2)
            (upe if kind == "edge" else upx)[i] = vec.to(DEV)
            torch.autograd.backward([x2, e2], [upx, upe])
            torch.cuda.synchronize()
            g = _collect(blk, xd, ed)
            want_dx, want_de = I.predicted_support(ei, kind, i)
            recs.append(dict(
                kind=kind, idx=i, want=(want_dx, want_de), got=(I.nonzero_rows(g["dx"]), I.nonzero_rows(g["de"])),
                finite=all(bool(torch.isfinite(v).all()) for v in g.values()),
                shapes_ok=g["dx"].shape == (n, h) and g["de"].shape == (ei.shape[1], h)
                and all(g[k].shape == v.shape for k, v in params.items()),
                node_params_zero=not any(bool(v.any()) for k, v in g.items() if k.startswith("node_block")),
                errs=I.value_errors(g, ref.grads(kind, i, vec), yard.grads(kind, i, vec), want_dx, want_de,
                                    I.hop_groups(ei, n, i, want_dx, want_de) if kind == "node" else None)))
    return recs


def _worst(recs, kind):
    """{key: (worst kernel error, worst yardstick error)} over the impulses of one kind."""
    out = {}
    for r in recs:
        if r["kind"] == kind:
            for k, (a, b) in r["errs"].items():
                pa, pb = out.get(k, (0.0, 0.0))
                out[k] = (max(pa, a), max(pb, b))
    return out


def _report(tag, recs):
    for kind in ("edge", "node"):
        w = _worst(recs, kind)
        if w:
            data = {k: w[k] for k in sorted(w) if k.startswith(("dx", "de"))}
            par = [v for k, v in w.items() if k not in data]
            print(f"\n{tag} {kind} impulses: worst rel-L2 vs fp64 (kernel, yardstick) "
                  + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in data.items())
                  + f", parameters {max(a for a, _ in par):.2e} / {max(b for _, b in par):.2e}")


@pytest.mark.parametrize("dtype,h", BLOCK_CASES)
def test_block_impulse_support(dtype, h):
    """The non-zero rows of dx and de are exactly the predicted ones, for every position; an edge impulse
    leaves every node-MLP parameter gradient exactly 0; everything is finite. h = 24 and 100 run zero-padded to
    32 / 128: the results have the caller's width, and a leak from the padded columns (an RMSNorm over the
    padded width, a padded weight row that is not zero) would show in test_block_impulse_values."""
    for r in _block_records(dtype, h):
        what = f"{r['kind']} impulse {r['idx']}"
        assert r["finite"], what
        assert r["shapes_ok"], what
        for key, got, want in zip(("dx", "de"), r["got"], r["want"]):
            assert got == sorted(want), (f"{what}: non-zero rows of {key}: missing {sorted(set(want) - set(got))}, "
                                         f"unexpected {sorted(set(got) - set(want))}")
        if r["kind"] == "edge":
            assert r["node_params_zero"], what


@pytest.mark.parametrize("dtype,h", BLOCK_CASES)
def test_block_impulse_values(dtype, h):
    """The same runs: dx and de on their support rows and every parameter gradient (for an edge impulse the
    edge MLP's are one row's outer products, the node MLP's zero) against the fp64 oracle, within
    max(1e-5, 2 x fp32 CPU oracle) / max(1e-2, 2 x autocast oracle). For a node impulse dx is also measured
    without the node's own row (dx_hop1: the sum by source; row v holds the residual's identity term, ~1e7
    times the terms that arrive over edges)."""
    recs = _block_records(dtype, h)
    _report(f"block {str(dtype)[6:]} h={h}", recs)
    for r in recs:
        I.assert_values(r["errs"], _floor(dtype), f"{r['kind']} impulse {r['idx']}")


def _stack_run(model, xd, ed, eid, v, vec):
    from graphphysics.utils.data import Data

    y = model(Data(x=xd, edge_index=eid, edge_attr=ed))
    up = torch.zeros_like(y)
    up[v] = vec.to(DEV)
    y.backward(up)
    torch.cuda.synchronize()
    return _collect(model, xd, ed)


def _stack_setup(dtype, mp, h):
    n, ei = I.stack_graph()
    m = I.robust_stack(mp, h)
    params = {k: v.detach().clone() for k, v in m.named_parameters()}
    x, e = I.inputs(n, ei.shape[1], h)
    m = m.set_compute_dtype(dtype).to(DEV)
    xd, ed, eid = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True), ei.to(DEV)
    return n, ei, m, params, x, e, xd, ed, eid


@pytest.mark.parametrize("dtype,mp,h,rew,eagg", STACK_CASES)
def test_stack_impulse_support_and_values(dtype, mp, h, rew, eagg, monkeypatch):
    """Node impulses on the output of a stack: the non-zero rows of gx and gea equal the fp64 oracle's (an
    impulse deep in the path component reaches 2 mp + 1 nodes, the in-degree-0 nodes only themselves), the
    values on them — whole, and per distance from the impulse (_impulse.hop_groups: every hop over an edge
    shrinks the gradient by ~1e7, so the whole-support figure sees the nearest rows only) — and every
    parameter gradient are within the single-block bounds. The impulse nodes include the target of every
    tile-boundary edge (_impulse.stack_nodes): the last block's edge-MLP gradients are then those in-edge rows'
    outer products, on the saved-input ring and on the recomputing launch (REW = "1")."""
    import ctypes

    from graphphysics import _native as nat
    from graphphysics.models import _engine

    if eagg is None:
        monkeypatch.delenv("MGN_EDGE_AGG", raising=False)
    else:
        monkeypatch.setenv("MGN_EDGE_AGG", eagg)
    n, ei, m, params, x, e, xd, ed, eid = _stack_setup(dtype, mp, h)
    ref = I.OracleRun(params, x, e, ei, "fp64", mp=mp)
    yard = I.OracleRun(params, x, e, ei, _yard(dtype), mp=mp)
    recs, seen = [], {}
    rew0, _engine.REW = _engine.REW, rew
    _engine.INSPECT = lambda st: seen.update(rew=bool(st["rew"]))
    try:
        for v in I.stack_nodes(ei, n):
            vec = I.impulse_vector("node", v, h)
            g = _stack_run(m, xd, ed, eid, v, vec)
            _engine.INSPECT = None
            g64 = ref.grads("node", v, vec)
            want_dx, want_de = I.nonzero_rows(g64["dx"]), I.nonzero_rows(g64["de"])
            for k, t in g.items():
                assert bool(torch.isfinite(t).all()), (v, k)
            I.assert_support(g, want_dx, want_de, f"node impulse {v}")
            recs.append(dict(kind="node", idx=v,
                             errs=I.value_errors(g, g64, yard.grads("node", v, vec), want_dx, want_de,
                                                 I.hop_groups(ei, n, v, want_dx, want_de))))
    finally:
        _engine.REW, _engine.INSPECT = rew0, None
    # the switches took effect: recomputed edge inputs, the forward's edge-side sums (scratch in use)
    assert seen["rew"] == (rew == "1")
    if dtype == torch.bfloat16:
        pw = m._get_plan().packed(DEV, nat.MGN_BF16)
        sb = nat.lib().mgn_block_forward_scratch_bytes(ctypes.byref(_engine.get_topology(eid, n).struct),
                                                       ctypes.byref(pw.descs[0]), ctypes.byref(pw.descs[1]))
        assert (sb > 0) == (eagg == "1"), (eagg, sb)
    _report(f"stack {str(dtype)[6:]} mp={mp} h={h} REW={rew} MGN_EDGE_AGG={eagg}", recs)
    for r in recs:
        I.assert_values(r["errs"], _floor(dtype), f"node impulse {r['idx']}")


def test_stack_impulse_is_bitwise_reproducible(monkeypatch):
    """Two runs of one impulse (bf16 h = 128 stack, default switches): every gradient bit for bit."""
    monkeypatch.delenv("MGN_EDGE_AGG", raising=False)
    n, ei, m, params, x, e, xd, ed, eid = _stack_setup(torch.bfloat16, 3, 128)
    v = 9  # in-degree 100, the hub among its sources
    vec = I.impulse_vector("node", v, 128)
    a = _stack_run(m, xd, ed, eid, v, vec)
    b = _stack_run(m, xd, ed, eid, v, vec)
    for k in a:
        assert torch.equal(a[k], b[k]), k
