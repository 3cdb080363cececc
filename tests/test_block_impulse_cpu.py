"""The preconditions tests/test_block_impulse_gpu.py rests on, measured with the oracle alone (no GPU): the GPU
tests compare supports and single-row values, and never measure these themselves.

* for every impulse position the fp64 oracle's non-zero rows are exactly the graph-predicted ones, and so are
  the rows under torch.autocast("cpu", bfloat16) (no predicted row is zero by accident, none underflows);
* for an edge impulse (zero upstream gradient on x_out) every node-MLP parameter gradient is exactly 0, in fp64
  and under autocast;
* the robust models (_impulse.robust_block / robust_stack) keep every hidden pre-activation at |z| >= 0.25 in
  fp64 at every size the GPU tests use, with 40-60 % of each layer's units open — a bf16 rounding of the
  layer's inputs moves z by ~2^-8 |z| terms, far from flipping a unit, so the suite's "2 x autocast" rule
  applies to a single row;
* on the stack at least a third of the node impulses have a support of fewer than half of the rows (else the
  support assertion would have no power there).
"""
import pytest
import torch

import _impulse as I

BLOCK_SIZES = [16, 32, 64, 128, 256, 24, 100]  # every h of test_block_impulse_gpu's single-block cases
STACKS = [(3, 128), (2, 32)]                   # its stacks


def _block_runs(h, modes):
    n, ei = I.corner_graph()
    blk = I.robust_block(h)
    x, e = I.inputs(n, ei.shape[1], h)
    return n, ei, [I.OracleRun(dict(blk.named_parameters()), x, e, ei, m) for m in modes]


def test_corner_graph_is_the_graph_the_positions_assume():
    n, ei = I.corner_graph()
    assert (n, ei.shape[1]) == (101, 602)
    deg = torch.bincount(ei[1], minlength=n)
    assert deg[: len(I.LISTED_DEGREES)].tolist() == I.LISTED_DEGREES
    assert int((ei[0] == I.HUB).sum()) >= 130
    order = torch.argsort(ei[1], stable=True)
    tiles = {int(p) // 16 for p in (ei[0][order] == I.HUB).nonzero().flatten()}
    assert len(tiles) >= 30, "the hub's out-edges should sit in most of the 38 tiles"
    assert bool((ei[0] == ei[1]).any())
    assert torch.unique(ei[0] * n + ei[1]).numel() < ei.shape[1]  # parallel edges
    eids, nodes = I.impulse_positions(ei, n)
    assert len(set(eids)) == len(eids) and len(eids) >= 100 and len(nodes) == 20
    ns, es = I.stack_graph()
    assert (ns, es.shape[1]) == (161, 722)


@pytest.mark.parametrize("h", BLOCK_SIZES)
def test_oracle_supports_equal_graph_prediction(h):
    """Every position, fp64 and autocast; node-MLP parameter gradients exactly 0 for edge impulses."""
    n, ei, runs = _block_runs(h, ("fp64", "autocast"))
    eids, nodes = I.impulse_positions(ei, n)
    for kind, ids in (("edge", eids), ("node", nodes)):
        for i in ids:
            want_dx, want_de = I.predicted_support(ei, kind, i)
            vec = I.impulse_vector(kind, i, h)
            for run, mode in zip(runs, ("fp64", "autocast")):
                g = run.grads(kind, i, vec)
                I.assert_support(g, want_dx, want_de, f"{mode} {kind} {i}")
                if kind == "edge":
                    for k, v in g.items():
                        if k.startswith("node_block"):
                            assert not bool(v.any()), (mode, i, k)


@pytest.mark.parametrize("h", BLOCK_SIZES)
def test_robust_block_margins(h):
    _, _, (run,) = _block_runs(h, ("fp64",))
    _check_margins(run.record, 6)


@pytest.mark.parametrize("mp,h", STACKS)
def test_robust_stack_margins_and_support_power(mp, h):
    n, ei = I.stack_graph()
    m = I.robust_stack(mp, h)
    x, e = I.inputs(n, ei.shape[1], h)
    run = I.OracleRun(dict(m.named_parameters()), x, e, ei, "fp64", mp=mp)
    _check_margins(run.record, 6 * mp)
    nodes = I.stack_nodes(ei, n)
    small = 0
    for v in nodes:
        g = run.grads("node", v, I.impulse_vector("node", v, h))
        rows_x, rows_e = I.nonzero_rows(g["dx"]), I.nonzero_rows(g["de"])
        assert v in rows_x
        small += len(rows_x) < n / 2 and len(rows_e) < ei.shape[1] / 2
        if v == I.CORNER_NODES + 30:  # deep in the path: 2b + 1 nodes after b blocks
            assert rows_x == list(range(v - mp, v + mp + 1))
    assert 3 * small >= len(nodes), (small, len(nodes))


def _check_margins(record, layers):
    seen = 0
    for prefix, zs in record.items():
        for i, z in enumerate(zs):
            seen += 1
            assert float(z.abs().min()) >= 0.25, (prefix, i, float(z.abs().min()))
            assert 0.4 <= float((z > 0).double().mean()) <= 0.6, (prefix, i, float((z > 0).double().mean()))
    assert seen == layers
