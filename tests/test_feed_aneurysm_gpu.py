"""Aneurysm features in the resident feed on the GPU: libmgn's mgn_feed_inflow_stats and mgn_feed_batch_aneurysm
against the same rules written as torch ops (dataset.resident.inflow_stats_torch / fill_aneurysm_torch, evaluated
on the CPU) and against the reference's own build_features -> add_noise (tests/golden/aneurysm_feed_golden.npz),
their argument checks, and TrainStep(feed=...) on a small tetrahedral grid.

The fill copies fp32 values, subtracts and adds one rounded product: every comparison of it is bit equality. The
statistics: min and max are exact; the mean is an fp64 sum of the distinct values in ascending order, held to
|got − m| <= 2^-24·|m| + n·2^-53·Σ|v| against math.fsum (the final rounding to fp32, plus the worst case of n fp64
additions), and it is the torch rule's bits too, because that rule adds the same values in the same order.

Shapes: graphs of 1, 70 and 600 nodes (spans that cross a wave and a 256-thread block): graph 0 has no inflow node,
in graph 1 every node is inflow (no masked zero) and one carries the wall flag, graph 2 has 200 inflow nodes — 601
values, more than one 512-element sorting stage — with repeats across nodes and components and a node at
pos = (0, 0, z); one further graph has a value set of exactly the capacity."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
U24, U53 = 2.0 ** -24, 2.0 ** -53
SIZES, T = [1, 70, 600], 4
RANGES = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)]  # coarse-aneurysm.json
SCALES = [10.0, 10.0, 1.0, 10.0, 10.0, 1.0]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _offsets(sizes):
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    return gp


def _graph(n, kind, F, g):
    """CPU (traj [T, n, F], pos [n, 3]) of one graph. kind: "none" (no node on the face y == 0), "all" (every node
    inflow, node 0 with the wall flag), "mixed" (the first 200 nodes inflow, node 200 at (0, 0, z), 20 outflow
    nodes, 40 wall nodes off the face; the first 60 inflow rows hold multiples of 2^-6 in [-1, 1], so their
    accelerations repeat across nodes and components) or an int m (the first m nodes inflow)."""
    traj = torch.randn(T, n, F, generator=g)
    traj[:, :, 3] = 0.0
    pos = torch.randn(n, 3, generator=g)
    pos[:, 1] = pos[:, 1].abs() + 0.5
    if kind == "all":
        pos[:, 1], pos[:, 0] = 0.0, -pos[:, 0].abs() - 0.5
        traj[:, 0, 3] = 1.0
    elif kind == "mixed":
        pos[:200, 1], pos[:200, 0] = 0.0, -pos[:200, 0].abs() - 0.5
        pos[200, 1], pos[200, 0] = 0.0, 0.0
        pos[201:221, 1], pos[201:221, 0] = 0.0, pos[201:221, 0].abs() + 0.5
        traj[:, 221:261, 3] = 1.0
        traj[:, 5, 3] = 1.0  # a wall node on the inflow face
        traj[:, :60, 0:3] = torch.randint(-64, 65, (T, 60, 3), generator=g).float() / 64.0
        traj[2, 7, 0:3] = traj[1, 7, 0:3]  # an inflow node at rest between frames 1 and 2
    elif isinstance(kind, int):
        pos[:kind, 1], pos[:kind, 0] = 0.0, -pos[:kind, 0].abs() - 0.5
    return traj, pos


@pytest.fixture(scope="module", params=[4, 6], ids=["F4", "F6"])
def case(request):
    """The batch of the three graphs on the CPU, and the kernel's statistics table of it (computed once)."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    F = request.param
    g = torch.Generator().manual_seed(100 + F)
    parts = [_graph(n, kind, F, g) for n, kind in zip(SIZES, ("none", "all", "mixed"))]
    traj = torch.cat([p[0] for p in parts], dim=1).contiguous()
    pos = torch.cat([p[1] for p in parts], dim=0).contiguous()
    gp = _offsets(SIZES)
    cpu = ResidentTrajectories(traj, gp, (0, 3), F + 9, aneurysm={"pos": pos})  # the torch rules' table
    dev = ResidentTrajectories(traj.to(DEV), gp, (0, 3), F + 9, aneurysm={"pos": pos.to(DEV)})  # the kernel's
    torch.cuda.synchronize()
    assert cpu.inflow_ptr.tolist() == [0, 0, 70, 270] and dev._max_values == 601
    assert nat.MGN_FEED_INFLOW_CAPACITY >= 4096
    return dict(F=F, traj=traj, pos=pos, gp=gp, parts=parts, cpu=cpu, dev=dev, stats=dev.inflow_stats.cpu())


def _fsum_bound_check(got, cur, nxt, mask):
    d = (nxt[:, 0:3] - cur[:, 0:3])[mask].reshape(-1).tolist()
    if not bool(mask.all()):
        d.append(0.0)
    distinct = sorted(set(float(v) + 0.0 for v in d))
    n = len(distinct)
    m = math.fsum(distinct) / n
    err, bound = abs(float(got[0]) - m), U24 * abs(m) + n * U53 * math.fsum(abs(v) for v in distinct)
    print(f"n = {n} distinct of {len(d)}: mean {float(got[0])!r}, fsum mean {m!r}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(got[1]) == distinct[0] and float(got[2]) == distinct[-1]
    return n, len(d)


def test_stats_equal_the_torch_rule(case):
    from graphphysics import _native as nat

    traj, gp, stats, cpu = case["traj"], case["gp"], case["stats"], case["cpu"]
    assert tuple(stats.shape) == (T - 1, 3, 3)
    mask = cpu.node_type == 4
    for t in range(T - 1):
        assert torch.equal(stats[t, 0], torch.zeros(3))  # no inflow node
        for b in (1, 2):
            rows = slice(gp[b], gp[b + 1])
            n, total = _fsum_bound_check(stats[t, b], traj[t, rows], traj[t + 1, rows], mask[rows])
            assert total == (210 if b == 1 else 601)
            if b == 2:
                assert n < 590  # repeats were dropped
        assert torch.equal(stats[t, :, 1:], cpu.inflow_stats[t, :, 1:])  # min and max: bit for bit
    assert bool(mask[gp[1]:gp[2]].all()) and float(case["traj"][0, gp[1], 3]) == 1.0  # a wall node that is INFLOW
    assert float(cpu.node_type[gp[2] + 200]) == 5.0 and float(cpu.node_type[gp[2] + 5]) == 4.0
    assert torch.equal(stats, cpu.inflow_stats)  # the mean too: the torch rule adds the same values in the same order
    # a second launch: identical bits
    again = torch.full_like(case["dev"].inflow_stats, SENTINEL)
    dev = case["dev"]
    nat.feed_inflow_stats(dev.traj, dev.graph_ptr, dev.inflow_ptr, dev.inflow_rows, dev._max_values, again)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), stats)


def test_stats_do_not_depend_on_the_place_in_the_batch(case):
    """Graph 2's data placed first in the batch, and alone in a batch of one: the same bits."""
    from graphphysics.dataset.resident import ResidentTrajectories

    F, parts, stats = case["F"], case["parts"], case["stats"]
    order = [2, 0, 1]
    traj = torch.cat([parts[i][0] for i in order], dim=1).contiguous().to(DEV)
    pos = torch.cat([parts[i][1] for i in order], dim=0).contiguous().to(DEV)
    feed = ResidentTrajectories(traj, _offsets([SIZES[i] for i in order]), (0, 3), F + 9, aneurysm={"pos": pos})
    alone = ResidentTrajectories(parts[2][0].contiguous().to(DEV), [0, SIZES[2]], (0, 3), F + 9,
                                 aneurysm={"pos": parts[2][1].contiguous().to(DEV)})
    torch.cuda.synchronize()
    assert torch.equal(feed.inflow_stats.cpu()[:, 0], stats[:, 2])
    assert torch.equal(feed.inflow_stats.cpu()[:, 1:], stats[:, 0:2])
    assert torch.equal(alone.inflow_stats.cpu()[:, 0], stats[:, 2])


def test_a_value_set_of_exactly_the_capacity():
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    cap = nat.MGN_FEED_INFLOW_CAPACITY
    m = (cap - 1) // 3
    assert 3 * m + 1 == cap, "the capacity is not of the form 3·M + 1: choose the graph otherwise"
    n = m + 5
    g = torch.Generator().manual_seed(7)
    traj, pos = _graph(n, m, 4, g)
    traj[:, : m // 2, 0:3] = torch.randint(-64, 65, (T, m // 2, 3), generator=g).float() / 64.0
    cpu = ResidentTrajectories(traj.contiguous(), [0, n], (0, 3), 13, aneurysm={"pos": pos})
    dev = ResidentTrajectories(traj.contiguous().to(DEV), [0, n], (0, 3), 13, aneurysm={"pos": pos.to(DEV)})
    torch.cuda.synchronize()
    assert dev._max_values == cap
    stats = dev.inflow_stats.cpu()
    mask = cpu.node_type == 4
    for t in range(T - 1):
        _, total = _fsum_bound_check(stats[t, 0], traj[t], traj[t + 1], mask)
        assert total == cap
    assert torch.equal(stats, cpu.inflow_stats)


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noise"])
def test_fill_equals_the_torch_rule_bit_for_bit(case, noisy):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import fill_aneurysm_torch

    F, traj, pos, gp, dev, stats = case["F"], case["traj"], case["pos"], case["gp"], case["dev"], case["stats"]
    N, Fx = traj.shape[1], F + 10
    keep_traj, keep_pos = dev.traj.clone(), dev.pos.clone()
    ranges = RANGES if noisy else []
    scales = torch.tensor(SCALES) if noisy else None
    z = torch.randn(N, 6, generator=torch.Generator().manual_seed(5)) if noisy else None
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    for frames, ldx in (([1, 1, 1], Fx), ([T - 2] * 3, Fx + 3), ([2, 1, 2], Fx)):
        fr = torch.tensor(frames, dtype=torch.int32)
        wx, wy = fill_aneurysm_torch(traj, gp, fr, pos, case["cpu"].node_type, stats, (0, 3), ranges, scales, z)
        x = torch.full((N, ldx), SENTINEL, device=DEV)
        y = torch.full((N, 3), SENTINEL, device=DEV)
        nat.feed_batch_aneurysm(dev.traj, dev.graph_ptr, fr.to(DEV), (0, 3), dev.pos, dev.node_type, dev.inflow_stats,
                                ranges, d(scales), d(z), x, y)
        torch.cuda.synchronize()
        x, y = x.cpu(), y.cpu()
        assert torch.equal(x[:, :Fx], wx) and torch.equal(y, wy)
        assert bool((x[:, Fx:] == SENTINEL).all())
        # the rule itself, independent of fill_aneurysm_torch
        for b, f in enumerate(frames):
            rows = slice(gp[b], gp[b + 1])
            assert torch.equal(y[rows], traj[f + 1, rows, 0:3])
            assert torch.equal(x[rows, F + 3:F + 6], pos[rows])
            assert torch.equal(x[rows, F + 6:F + 9], stats[f, b].expand(gp[b + 1] - gp[b], 3))
            assert torch.equal(x[rows, 3], traj[f, rows, 3])
            other = case["cpu"].node_type[rows] != 0
            assert torch.equal(x[rows, F:F + 3][other], (traj[f, rows, 0:3] - traj[f - 1, rows, 0:3])[other])
            if noisy and int((~other).sum()):
                assert not torch.equal(x[rows, 0:3][~other], traj[f, rows, 0:3][~other])
        assert torch.equal(x[:, F + 9], case["cpu"].node_type)
    assert torch.equal(dev.traj, keep_traj) and torch.equal(dev.pos, keep_pos)


def test_reference_fixture_through_the_kernels():
    """tests/golden/aneurysm_feed_golden.npz: every column of the reference's x but the mean bit for bit, the mean
    within 2^-24·|m_ref| + 2^-24·Σ|v| (test_feed_aneurysm_cpu.py)."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    zf = np.load(os.path.join(G, "aneurysm_feed_golden.npz"))
    gold = {k: torch.from_numpy(zf[k]) if zf[k].ndim else zf[k] for k in zf.files}
    traj = torch.stack([gold["prev_frame"], gold["frame"], gold["next_frame"]]).contiguous().to(DEV)
    N, F = traj.shape[1], traj.shape[2]
    noise = {"noise_index_start": [int(r[0]) for r in zf["ranges"]], "noise_index_end": [int(r[1]) for r in zf["ranges"]],
             "noise_scale": [float(v) for v in zf["scales"]], "node_type_index": F + 9}
    feed = ResidentTrajectories(traj, [0, N], (0, 3), F + 9, noise=noise, frames=[1],
                                aneurysm={"pos": gold["pos"].to(DEV).contiguous()})
    assert torch.equal(feed.node_type.cpu(), gold["node_type"])
    x, y = torch.full((N, F + 10), SENTINEL, device=DEV), torch.full((N, 3), SENTINEL, device=DEV)
    nat.feed_batch_aneurysm(traj, feed.graph_ptr, feed.frame, (0, 3), feed.pos, feed.node_type, feed.inflow_stats,
                            feed.ranges, feed.scales, gold["z"].to(DEV), x, y)
    torch.cuda.synchronize()
    x, want = x.cpu(), gold["x_out"]
    cols = [c for c in range(F + 10) if c != F + 6]
    assert torch.equal(x[:, cols], want[:, cols])
    assert torch.equal(y.cpu(), gold["next_frame"][:, 0:3])
    m, m_ref = x[:, F + 6], float(want[0, F + 6])
    distinct = gold["distinct"].tolist()
    assert bool((m == m[0]).all())
    assert abs(float(m[0]) - m_ref) <= U24 * abs(m_ref) + U24 * math.fsum(abs(v) for v in distinct)
    n = len(distinct)
    exact = math.fsum(distinct) / n
    assert abs(float(m[0]) - exact) <= U24 * abs(exact) + n * U53 * math.fsum(abs(v) for v in distinct)


# ------------------------------------------------------------------------------------------------ raw calls
def _raw_fill(**over):
    """mgn_feed_batch_aneurysm called directly with valid arguments for a [4, 10, 5] trajectory, except `over`.
    Returns (status, message, x): x is pre-filled with a sentinel."""
    from graphphysics import _native as nat

    Tn, N, F = 4, 10, 5
    a = {"traj": torch.zeros(Tn, N, F, device=DEV), "T": Tn, "N": N, "F": F,
         "graph_ptr": torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV), "B": 2,
         "frame": torch.tensor([1, 2], dtype=torch.int32, device=DEV), "y_start": 0, "y_end": 3,
         "pos": torch.ones(N, 3, device=DEV), "node_type": torch.zeros(N, device=DEV),
         "stats": torch.full((Tn - 1, 2, 3), 2.0, device=DEV), "n": 2, "start": [0, 5], "end": [3, 8],
         "scales": torch.ones(8, device=DEV), "z": torch.zeros(N, 8, device=DEV), "ldz": 8,
         "x": torch.full((N, 17), SENTINEL, device=DEV), "ldx": 17, "y": torch.full((N, 3), SENTINEL, device=DEV),
         "ldy": 3}
    a.update(over)
    rg = nat.FeedRanges8()
    rg.n = a["n"]
    for i, (s, e) in enumerate(zip(a["start"], a["end"])):
        rg.start[i], rg.end[i] = s, e
    rc = nat.lib().mgn_feed_batch_aneurysm(nat.ptr(a["traj"]), a["T"], a["N"], a["F"], nat.ptr(a["graph_ptr"]), a["B"],
                                           nat.ptr(a["frame"]), a["y_start"], a["y_end"], nat.ptr(a["pos"]),
                                           nat.ptr(a["node_type"]), nat.ptr(a["stats"]), rg, nat.ptr(a["scales"]),
                                           nat.ptr(a["z"]), a["ldz"], nat.ptr(a["x"]), a["ldx"], nat.ptr(a["y"]),
                                           a["ldy"], nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), a["x"]


BAD_FILL = {
    "T<3": dict(T=2), "F<4": dict(F=3), "range_end>F+10": dict(end=[3, 16]), "range_start<0": dict(start=[-1, 5]),
    "range_reversed": dict(start=[3, 5], end=[0, 8]), "ranges_overlap": dict(start=[0, 2], end=[3, 8]),
    "range_holds_type": dict(start=[0, 13], end=[3, 15]), "range_is_type": dict(start=[0, 14], end=[3, 15]),
    "y_end>F": dict(y_end=6), "y_reversed": dict(y_start=3, y_end=2), "n>8": dict(n=9), "n<0": dict(n=-1),
    "ldx<F+10": dict(ldx=14), "ldy<width": dict(ldy=2), "ldz<width": dict(ldz=5), "traj_null": dict(traj=None),
    "pos_null": dict(pos=None), "node_type_null": dict(node_type=None), "stats_null": dict(stats=None),
    "frame_null": dict(frame=None), "graph_ptr_null": dict(graph_ptr=None), "x_null": dict(x=None),
    "y_null": dict(y=None), "scales_null": dict(scales=None), "N<0": dict(N=-1), "B<0": dict(B=-1),
}


@pytest.mark.parametrize("name", list(BAD_FILL))
def test_bad_fill_arguments_are_refused_before_any_launch(name):
    rc, msg, x = _raw_fill(**BAD_FILL[name])
    assert rc != 0 and "feed_batch_aneurysm" in msg, (rc, msg)
    assert x is None or bool((x == SENTINEL).all())


def test_the_valid_raw_fill_runs_and_no_nodes_is_success_without_a_launch():
    rc, _, x = _raw_fill()
    assert rc == 0 and bool((x[:, 15:] == SENTINEL).all())
    want = torch.tensor([0.0] * 8 + [1.0] * 3 + [2.0] * 3 + [0.0], device=DEV)
    assert torch.equal(x[:, :15], want.expand(10, 15))
    for over in (dict(N=0), dict(B=0), dict(N=0, traj=None, x=None)):
        rc, msg, x = _raw_fill(**over)
        assert rc == 0, msg
        assert x is None or bool((x == SENTINEL).all())


def _raw_stats(**over):
    """mgn_feed_inflow_stats called directly with valid arguments for a [3, 10, 4] trajectory, except `over`."""
    from graphphysics import _native as nat

    Tn, N, F = 3, 10, 4
    traj = torch.zeros(Tn, N, F, device=DEV)
    traj[1, :, 0:3] = torch.arange(30.0, device=DEV).reshape(10, 3)
    a = {"traj": traj, "T": Tn, "N": N, "F": F, "graph_ptr": torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV),
         "B": 2, "inflow_ptr": torch.tensor([0, 2, 2], dtype=torch.int32, device=DEV),
         "inflow_rows": torch.tensor([1, 3], dtype=torch.int32, device=DEV), "max_values": 7,
         "stats": torch.full((Tn - 1, 2, 3), SENTINEL, device=DEV)}
    a.update(over)
    rc = nat.lib().mgn_feed_inflow_stats(nat.ptr(a["traj"]), a["T"], a["N"], a["F"], nat.ptr(a["graph_ptr"]), a["B"],
                                         nat.ptr(a["inflow_ptr"]), nat.ptr(a["inflow_rows"]), a["max_values"],
                                         nat.ptr(a["stats"]), nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), a["stats"]


BAD_STATS = {
    "T<2": dict(T=1), "F<4": dict(F=3), "N<0": dict(N=-1), "B<0": dict(B=-1), "max_values<0": dict(max_values=-1),
    "over_capacity": dict(max_values=None), "traj_null": dict(traj=None),
    "graph_ptr_null": dict(graph_ptr=None), "inflow_ptr_null": dict(inflow_ptr=None),
    "inflow_rows_null": dict(inflow_rows=None), "stats_null": dict(stats=None),
}


@pytest.mark.parametrize("name", list(BAD_STATS))
def test_bad_stats_arguments_are_refused_before_any_launch(name):
    from graphphysics import _native as nat

    over = dict(BAD_STATS[name])
    if name == "over_capacity":
        over["max_values"] = nat.MGN_FEED_INFLOW_CAPACITY + 1
    rc, msg, stats = _raw_stats(**over)
    assert rc != 0 and "feed_inflow_stats" in msg, (rc, msg)
    assert stats is None or bool((stats == SENTINEL).all())


def test_the_valid_raw_stats_call_runs_and_no_nodes_is_success_without_a_launch():
    rc, _, stats = _raw_stats()
    assert rc == 0
    # frame 0 -> 1: rows 1 and 3 of graph 0 gain (3, 4, 5) and (9, 10, 11), plus the masked zero; graph 1: no inflow
    want0 = torch.tensor([[(0 + 3 + 4 + 5 + 9 + 10 + 11) / 7, 0.0, 11.0], [0.0, 0.0, 0.0]], device=DEV)
    want1 = torch.tensor([[-(3 + 4 + 5 + 9 + 10 + 11) / 7, -11.0, 0.0], [0.0, 0.0, 0.0]], device=DEV)
    assert torch.equal(stats[0], want0) and torch.equal(stats[1], want1)
    for over in (dict(N=0), dict(B=0)):
        rc, msg, stats = _raw_stats(**over)
        assert rc == 0 and bool((stats == SENTINEL).all()), msg


# ------------------------------------------------------------------------------------------------ TrainStep(feed=...)
T_GRID, B_GRID = 5, 2
FRAMES = ([1, 2], [3, 1], [2, 2])
SEEDS = (11, 12, 13)


@pytest.fixture(scope="module")
def grid():
    """Two copies of meshes.tet_grid(11, 6, 5) (330 nodes each): the plane y = 0 is the inflow (x < 0) and outflow
    (x >= 0, with nodes at x = 0) face, the plane z = 0 carries the wall flag. T = 5 random frames [velocity, wall
    flag]; the second graph's velocities are 1.5 times the first's. Returns (traj [5, 660, 4] on the device, node
    offsets, pos [660, 3], edge_index [2, E], edge_attr [E, 4])."""
    from graphphysics.utils import meshes

    p, cells = meshes.tet_grid(11, 6, 5, 0.25, origin=(-1.25, 0.0, 0.0))
    n = p.shape[0]
    ei1 = meshes.tetra_to_edge_index(cells, n)
    ea1 = meshes.edge_features(p, ei1)
    g = torch.Generator().manual_seed(3)
    v = 0.1 * torch.randn(T_GRID, n, 3, generator=g)
    wall = torch.from_numpy((p[:, 2] == 0).astype(np.float32))[None, :, None].expand(T_GRID, n, 1)
    traj = torch.cat([torch.cat([v, wall], dim=2), torch.cat([1.5 * v, wall], dim=2)], dim=1).contiguous().to(DEV)
    pos = torch.from_numpy(np.concatenate([p, p], 0)).contiguous().to(DEV)
    ei1 = torch.as_tensor(np.asarray(ei1), dtype=torch.int64)
    ei = torch.cat([ei1, ei1 + n], dim=1).contiguous().to(DEV)
    ea = torch.from_numpy(np.concatenate([ea1, ea1], 0)).contiguous().to(DEV)
    assert n == 330 and int((pos[:, 1] == 0).sum()) == 2 * 55
    return traj, [0, n, 2 * n], pos, ei, ea


def _grid_setup():
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    torch.manual_seed(0)
    model = EncodeProcessDecode(2, 13 + 9, 4, 3, 32, compute_dtype=torch.float32)
    sim = Simulator(13 + 9, 4, 3, 0, 13, 0, 3, 13, model, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def _grid_feed(grid, frames):
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp, pos, ei, ea = grid
    noise = {"noise_index_start": [s for s, _ in RANGES], "noise_index_end": [e for _, e in RANGES],
             "noise_scale": [0.01 * s for s in SCALES], "node_type_index": 13}
    return ResidentTrajectories(traj, gp, (0, 3), 13, noise=noise, frames=frames, aneurysm={"pos": pos})


def test_captured_fed_step_equals_the_host_loop_bit_for_bit(grid):
    """Three captured fed steps on explicit frames, the normals fixed by re-seeding ahead of each step, against
    three captured steps on batches the host loop builds from the same frames and normals: per graph a Data of the
    frame through external.aneurysm.build_features (which shares the mean rule, so x is identical), then the noise
    rule. Losses and parameters are compared bit for bit. Then drawn frames: replays fill different batches."""
    from graphphysics.external.aneurysm import build_features
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    traj, gp, pos, ei, ea = grid
    keep, keep_pos = traj.clone(), pos.clone()
    N = traj.shape[1]

    feed = _grid_feed(grid, [1, 1])
    assert int((feed.node_type == 4).sum()) == 2 * 25 and int((feed.node_type == 5).sum()) == 2 * 30
    sim, opt, sch = _grid_setup()
    batch = Data(x=torch.zeros(N, 14, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=ea.clone())
    step = TrainStep(sim, opt, sch, batch, graph=True, feed=feed)
    step.capture()  # the warm-up steps draw too: record first, so every seeded step below is one replay
    fed = dict(losses=[], z=[], x=[])
    for fr, seed in zip(FRAMES, SEEDS):
        feed.set_frames(fr)
        torch.manual_seed(seed)
        fed["losses"].append(step().clone())
        fed["z"].append(feed.z.clone())
        fed["x"].append(step.batch.x.clone())
    torch.cuda.synchronize()
    assert step.graph is not None and opt.param_groups[0]["step_count"] == 3
    fed_params = [p.detach().clone() for p in sim.parameters()]
    assert len({float(v) for v in fed["losses"]}) == 3  # three different batches

    sim2, opt2, sch2 = _grid_setup()
    host, losses = None, []
    normal = (feed.node_type == 0)[:, None]
    for i, fr in enumerate(FRAMES):
        xs, ys = [], []
        for b, f in enumerate(fr):
            rows = slice(gp[b], gp[b + 1])
            d = build_features(Data(x=traj[f, rows].clone(), y=traj[f + 1, rows, 0:3].clone(), pos=pos[rows],
                                    previous_data=traj[f - 1, rows, 0:3].clone()))
            xs.append(d.x)
            ys.append(d.y)
        x, y = torch.cat(xs), torch.cat(ys)
        zc = 0
        for k, (s, e) in enumerate(feed.ranges):
            x[:, s:e] = torch.where(normal, x[:, s:e] + fed["z"][i][:, zc:zc + e - s] * feed.scales[k], x[:, s:e])
            zc += e - s
        assert torch.equal(x, fed["x"][i])
        b = Data(x=x, y=y, edge_index=ei, edge_attr=ea.clone())
        if host is None:
            host = TrainStep(sim2, opt2, sch2, b, graph=True)
        else:
            host.batch = b
        losses.append(host().clone())
    torch.cuda.synchronize()
    print("losses fed", [float(v) for v in fed["losses"]], "host loop", [float(v) for v in losses])
    for a, b in zip(fed["losses"], losses):
        assert torch.equal(a, b)
    for a, b in zip(fed_params, sim2.parameters()):
        assert torch.equal(a, b.detach())

    # drawn frames: the step is recorded anew with the draw inside, and every replay fills another batch
    feed.set_frames("random")
    torch.manual_seed(1)
    seen = []
    for _ in range(6):
        assert np.isfinite(float(step().item()))
        seen.append((feed.frame.clone(), step.batch.x.clone()))
        assert int(feed.frame.min()) >= 1 and int(feed.frame.max()) <= T_GRID - 2
    for (fa, xa), (fb, xb) in zip(seen, seen[1:]):
        assert not torch.equal(xa, xb)
    assert len({tuple(f.tolist()) for f, _ in seen}) > 1  # 6 draws of 2 frames out of 3 each
    assert torch.equal(traj, keep) and torch.equal(pos, keep_pos)
