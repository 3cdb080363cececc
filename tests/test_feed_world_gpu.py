"""World positions in the resident feed on the GPU: libmgn's mgn_feed_batch_world and
mgn_feed_world_edge_features against the same rules written as torch ops (dataset.resident.fill_world_torch /
world_edge_features_torch, evaluated on the CPU: IEEE division and square root) and against the reference's own
pipeline (tests/golden/world_feed_golden.npz), their argument checks, and TrainStep(feed=...) on a small plate.

The kernels copy fp32 values, subtract, add one rounded product, divide a sum by a count and take a correctly
rounded square root of a term-by-term sum, so wherever the obstacle sum is exact (values that are multiples of
2^-8: any summation order gives the same sum) every comparison is bit equality (torch.equal)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
NORM_RTOL = 5 * 2.0 ** -24  # the reference's torch.norm against the term-by-term form (test_feed_world_cpu.py)


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


def _case(sizes, F, T, all_obstacle=None, dyadic=True, seed=0):
    """CPU [T, N, F] frames (the last column the node type: NORMAL 0, OBSTACLE 1, HANDLE 3 mixed, the first node
    of every graph an OBSTACLE; graph `all_obstacle` entirely), node offsets. dyadic: multiples of 2^-8 in
    [-1, 1], so every displacement and every sum of fewer than 2^13 of them is exact in fp32."""
    g = torch.Generator().manual_seed(seed + 31 * F + T + 7 * len(sizes) + sum(sizes))
    N, gp = sum(sizes), _offsets(sizes)
    if dyadic:
        traj = torch.randint(-256, 257, (T, N, F), generator=g).float() / 256.0
    else:
        traj = torch.randn(T, N, F, generator=g)
    types = torch.tensor([0.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, (N,), generator=g)]
    for b, s in enumerate(sizes):
        if s:
            types[gp[b]] = 1.0
        if b == all_obstacle:
            types[gp[b]:gp[b + 1]] = 1.0
    traj[:, :, F - 1] = types
    return traj.contiguous(), gp


def _edges(N, seed=0):
    """[2, E] int64 on the CPU: random pairs, a self-loop, and the first edge repeated twice."""
    g = torch.Generator().manual_seed(seed + N)
    ei = torch.randint(0, N, (2, 3 * N + 5), generator=g)
    loop = torch.tensor([[N - 1], [N - 1]])
    return torch.cat([ei, loop, ei[:, :1], ei[:, :1]], dim=1)


def _run_kernels(traj, gp, frames, ranges, scales, z, ldx, ei, ld_ea):
    """Both launches on sentinel-filled buffers. Returns CPU (x, y, mean, edge_attr)."""
    from graphphysics import _native as nat

    T, N, F = traj.shape
    B = len(gp) - 1
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    x = torch.full((N, ldx), SENTINEL, device=DEV)
    y = torch.full((N, 3), SENTINEL, device=DEV)
    mean = torch.full((B, 3), SENTINEL, device=DEV)
    nat.feed_batch_world(d(traj), torch.tensor(gp, dtype=torch.int32, device=DEV),
                         torch.tensor(frames, dtype=torch.int32, device=DEV), (0, 3), F - 1, ranges, d(scales), d(z), x,
                         y, mean)
    ea = torch.full((ei.shape[1], ld_ea), SENTINEL, device=DEV)
    nat.feed_world_edge_features(ei[0].to(DEV, torch.int32).contiguous(), ei[1].to(DEV, torch.int32).contiguous(), x,
                                 ea, 4)
    torch.cuda.synchronize()
    return x.cpu(), y.cpu(), mean.cpu(), ea.cpu()


# (graph sizes, index of an all-OBSTACLE graph)
SIZES = {
    "one_node": ([1], None),
    "uneven": ([5, 64, 193], None),
    "empty_graph": ([0, 65, 7], None),  # the raw call only: the class refuses a graph without an OBSTACLE node
    "long_graph": ([1300, 3], None),  # the reduction walks a graph in several strides of its workgroup
    "all_obstacle": ([6, 70], 1),
}
# F, noisy ranges in batch layout (None: noise off); the node type sits in batch column F + 2
CONFIGS = [(4, None), (4, [(0, 3)]), (9, None), (9, [(0, 3)]), (9, [(0, 3), (7, 9)])]


@pytest.mark.parametrize("F,ranges", CONFIGS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("name", list(SIZES))
def test_kernels_equal_the_torch_rules_bit_for_bit(name, F, ranges):
    from graphphysics.dataset.resident import fill_world_torch, world_edge_features_torch

    sizes, all_obstacle = SIZES[name]
    T = 4
    traj, gp = _case(sizes, F, T, all_obstacle)
    N, B, Fx = traj.shape[1], len(sizes), F + 3
    keep = traj.clone()
    W = sum(e - s for s, e in ranges) if ranges else 0
    z = torch.randn(N, W, generator=torch.Generator().manual_seed(5)) if ranges else None
    scales = torch.tensor([0.02, 1.5][:len(ranges)]) if ranges else None
    ei = _edges(N)
    for frames, ldx, ld_ea in (([0] * B, Fx, 8), ([T - 2] * B, Fx + 2, 9),
                               ([0 if b % 2 else T - 2 for b in range(B)], Fx, 9)):
        fr = torch.tensor(frames, dtype=torch.int32)
        wx, wy, wmean = fill_world_torch(traj, gp, fr, (0, 3), F - 1, ranges or [], scales, z)
        # the premise of bit equality: the obstacle sums are exact, so their order does not matter
        for b in range(B):
            rows = slice(gp[b], gp[b + 1])
            obstacle = keep[frames[b], rows, F - 1] == 1
            d = (keep[frames[b] + 1, rows, 0:3] - keep[frames[b], rows, 0:3])[obstacle]
            assert torch.equal(d.sum(0).double(), d.double().sum(0))
            if name == "empty_graph" and b == 0:
                assert d.shape[0] == 0 and torch.equal(wmean[b], torch.zeros(3))
            if b == all_obstacle:
                assert bool(obstacle.all()) and torch.equal(wx[rows, 3:6], d)
        x, y, mean, ea = _run_kernels(traj, gp, frames, ranges or [], scales, z, ldx, ei, ld_ea)
        assert torch.equal(mean, wmean)
        assert torch.equal(x[:, :Fx], wx) and torch.equal(y, wy)
        assert bool((x[:, Fx:] == SENTINEL).all())
        want = torch.full((ei.shape[1], ld_ea), SENTINEL)
        world_edge_features_torch(wx, ei, want, 4)
        assert torch.equal(ea, want)  # the four columns, and the sentinels in [0, 4) and beyond 8
        loop = 3 * N + 5
        assert torch.equal(ea[loop, 4:8], torch.zeros(4)) and torch.equal(ea[0, 4:8], ea[-1, 4:8])
        # the rule itself, independent of fill_world_torch
        for b, f in enumerate(frames):
            rows = slice(gp[b], gp[b + 1])
            assert torch.equal(y[rows], keep[f + 1, rows, 0:3])
            assert torch.equal(x[rows, Fx - 1], keep[f, rows, F - 1])
            other = keep[f, rows, F - 1] != 0
            assert torch.equal(x[rows, 0:3][other], keep[f, rows, 0:3][other])
            if ranges and int((~other).sum()):
                assert not torch.equal(x[rows, 0:3][~other], keep[f, rows, 0:3][~other])
    assert torch.equal(traj, keep)


def test_no_edges_and_no_nodes_are_success_without_a_launch():
    from graphphysics import _native as nat

    x = torch.zeros(4, 7, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    nat.feed_world_edge_features(none, none, x, torch.zeros(0, 8, device=DEV), 4)
    traj = torch.zeros(3, 0, 4, device=DEV)
    gp, fr = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    mean = torch.full((1, 3), SENTINEL, device=DEV)
    nat.feed_batch_world(traj, gp, fr, (0, 3), 3, [], None, None, torch.zeros(0, 7, device=DEV),
                         torch.zeros(0, 3, device=DEV), mean)
    torch.cuda.synchronize()
    assert bool((mean == SENTINEL).all())


def _ulp(v):
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32))).double()


def test_random_data_mean_is_as_close_to_fp64_as_torch_fp32():
    """Random normal frames: the obstacle sum is no longer exact, so its order shows. The mean-derived values
    (obstacle_mean, and columns [3, 6) of the rows that are not OBSTACLE) are compared with the fp64 mean.

    The error of a graph's mean is that of its 3-vector, max |mean - fp64 mean| over the components: the bound is
    twice that error of torch's own fp32 sum(0) / M on the same data, and not less than 1 ulp of the largest
    component. Component by component the comparison would be one of two rounding errors that are each, by
    chance, anywhere between 0 and their bound — torch's is 0.2 ulp on one component here, where no fp32
    summation order can promise 1 ulp — so every component is instead held to the bound that holds for ANY
    order of an fp32 sum, |fl(sum) - sum| <= gamma(M - 1) * sum |d_i| with gamma(n) = n u / (1 - n u),
    u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), plus the two roundings of the
    division, 2 u |mean|. Measured on an MI355X (graph: M, kernel / torch max error in units of 1e-8):
    0: 162, 0.77 / 1.71; 1: 294, 1.09 / 1.35; 2: 15, 3.28 / 2.98 — and component 2 of graph 2 alone, 3.28 (2.2 ulp)
    against torch's 0.30 (0.2 ulp): held component by component to twice torch's error, this case fails there.
    Everything that does not depend on the mean is bit-equal."""
    from graphphysics.dataset.resident import fill_world_torch, world_edge_features_torch

    sizes, F, T = [700, 1301, 40], 9, 3
    traj, gp = _case(sizes, F, T, dyadic=False)
    N, B, Fx = traj.shape[1], len(sizes), F + 3
    frames, ranges = [0, 1, 1], [(0, 3), (7, 9)]
    z = torch.randn(N, 5, generator=torch.Generator().manual_seed(9))
    scales = torch.tensor([0.02, 1.5])
    ei = _edges(N)
    x, y, mean, ea = _run_kernels(traj, gp, frames, ranges, scales, z, Fx, ei, 8)
    wx, wy, wmean = fill_world_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), (0, 3), F - 1, ranges, scales, z)
    u = 2.0 ** -24
    for b, f in enumerate(frames):
        rows = slice(gp[b], gp[b + 1])
        obstacle = traj[f, rows, F - 1] == 1
        d = (traj[f + 1, rows, 0:3] - traj[f, rows, 0:3])[obstacle]
        M = d.shape[0]
        m64 = d.double().sum(0) / M
        err, err_torch = (mean[b].double() - m64).abs(), (wmean[b].double() - m64).abs()
        any_order = ((M - 1) * u / (1 - (M - 1) * u)) * d.double().abs().sum(0) / M + 2 * u * m64.abs()
        bound = max(2 * float(err_torch.max()), float(_ulp(m64.float()).max()))
        print(f"graph {b}: M = {M}, |kernel - fp64| = {err.tolist()}, |torch - fp64| = {err_torch.tolist()}, "
              f"bound = {bound}, any-order bound = {any_order.tolist()}")
        assert bool((err <= any_order).all())
        assert float(err.max()) <= bound
        others = x[rows, 3:6][~obstacle]
        assert torch.equal(others, mean[b].expand_as(others))  # the rows carry the mean the kernel wrote
    quiet = [c for c in range(Fx) if c not in (3, 4, 5)]
    assert torch.equal(x[:, quiet], wx[:, quiet]) and torch.equal(y, wy)
    obstacle = torch.cat([traj[f, gp[b]:gp[b + 1], F - 1] == 1 for b, f in enumerate(frames)])
    assert torch.equal(x[obstacle], wx[obstacle])
    want = torch.full((ei.shape[1], 8), SENTINEL)
    world_edge_features_torch(wx, ei, want, 4)  # reads columns [0, 3) only
    assert torch.equal(ea, want)


def test_reference_fixture_through_the_kernels():
    """tests/golden/world_feed_golden.npz: the reference's x and its relative world positions bit for bit, its
    torch.norm column at 5·2^-24 relative, the pre-filled edge_attr columns untouched."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    z = np.load(os.path.join(G, "world_feed_golden.npz"))
    gold = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k] for k in z.files}
    gold["k"] = k = int(z["node_type_index"])
    traj = torch.stack([gold["frame"], gold["next_frame"]]).contiguous().to(DEV)
    noise = {"noise_index_start": [int(r[0]) for r in z["ranges"]], "noise_index_end": [int(r[1]) for r in z["ranges"]],
             "noise_scale": [float(v) for v in z["scales"]], "node_type_index": k + 3}
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": k + 3,
          "edge_index": gold["edge_index"].to(DEV), "edge_attr_start": 4}
    feed = ResidentTrajectories(traj, [0, traj.shape[1]], (0, 3), k, noise=noise, frames=[0], world_pos=wp)
    N, E = traj.shape[1], gold["edge_index"].shape[1]
    x, y = torch.full((N, 8), SENTINEL, device=DEV), torch.full((N, 3), SENTINEL, device=DEV)
    ea = torch.full((E, 8), SENTINEL, device=DEV)
    ea[:, :4] = gold["edge_attr_in"].to(DEV)
    nat.feed_batch_world(traj, feed.graph_ptr, feed.frame, (0, 3), gold["k"], feed.ranges, feed.scales,
                         gold["z"].to(DEV), x, y, feed.obstacle_mean)
    nat.feed_world_edge_features(feed.senders, feed.receivers, x, ea, 4)
    torch.cuda.synchronize()
    want = gold["edge_attr_out"]
    assert torch.equal(x.cpu(), gold["x_out"])
    assert torch.equal(y.cpu(), gold["next_frame"][:, 0:3])
    assert torch.equal(feed.obstacle_mean.cpu()[0], gold["obstacle_mean"])
    assert torch.equal(ea.cpu()[:, :7], want[:, :7])
    torch.testing.assert_close(ea.cpu()[:, 7], want[:, 7], rtol=NORM_RTOL, atol=0)


def test_two_fills_with_the_same_frames_and_normals_give_identical_bits():
    """Random (not dyadic) data, so a reduction whose order varied would show: the class's fill, then the same
    launches again from the frames and normals that fill left in feed.frame / feed.z, twice."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.utils.data import Data

    sizes, F = [1300, 500, 77], 5
    traj, gp = _case(sizes, F, 5, dyadic=False)
    N = traj.shape[1]
    ei = _edges(N).to(DEV)
    noise = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.01, "node_type_index": F + 2}
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": F + 2, "edge_index": ei,
          "edge_attr_start": 4}
    feed = ResidentTrajectories(traj.to(DEV), gp, (0, 3), F - 1, noise=noise, world_pos=wp)
    b = Data(x=torch.zeros(N, F + 3, device=DEV), y=torch.zeros(N, 3, device=DEV),
             edge_attr=torch.zeros(ei.shape[1], 8, device=DEV), edge_index=ei)
    feed.fill(b)
    first = (b.x.clone(), b.y.clone(), b.edge_attr.clone(), feed.obstacle_mean.clone())
    assert int(feed.frame.min()) >= 0 and int(feed.frame.max()) <= 3
    for _ in range(2):
        x, y = torch.full_like(b.x, SENTINEL), torch.full_like(b.y, SENTINEL)
        ea, mean = torch.zeros_like(b.edge_attr), torch.full_like(feed.obstacle_mean, SENTINEL)
        nat.feed_batch_world(feed.traj, feed.graph_ptr, feed.frame, (0, 3), F - 1, feed.ranges, feed.scales, feed.z,
                             x, y, mean)
        nat.feed_world_edge_features(feed.senders, feed.receivers, x, ea, 4)
        for got, want in zip((x, y, ea, mean), first):
            assert torch.equal(got, want)


def _raw_world(**over):
    """mgn_feed_batch_world called directly with valid arguments for a [3, 10, 6] trajectory, except `over`.
    Returns (status, message, x, mean): x and mean are pre-filled with a sentinel."""
    from graphphysics import _native as nat

    T, N, F = 3, 10, 6
    traj = torch.zeros(T, N, F, device=DEV)
    traj[:, 0, 5] = traj[:, 4, 5] = 1.0
    a = {"traj": traj, "T": T, "N": N, "F": F, "graph_ptr": torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV),
         "B": 2, "frame": torch.tensor([0, 1], dtype=torch.int32, device=DEV), "y_start": 0, "y_end": 3,
         "type_index": 5, "n": 2, "start": [0, 6], "end": [3, 8], "scales": torch.ones(4, device=DEV),
         "z": torch.zeros(N, 8, device=DEV), "ldz": 8, "x": torch.full((N, 11), SENTINEL, device=DEV), "ldx": 11,
         "y": torch.full((N, 3), SENTINEL, device=DEV), "ldy": 3, "mean": torch.full((2, 3), SENTINEL, device=DEV)}
    a.update(over)
    rg = nat.FeedRanges()
    rg.n = a["n"]
    for i, (s, e) in enumerate(zip(a["start"], a["end"])):
        rg.start[i], rg.end[i] = s, e
    rc = nat.lib().mgn_feed_batch_world(nat.ptr(a["traj"]), a["T"], a["N"], a["F"], nat.ptr(a["graph_ptr"]), a["B"],
                                        nat.ptr(a["frame"]), a["y_start"], a["y_end"], a["type_index"], rg,
                                        nat.ptr(a["scales"]), nat.ptr(a["z"]), a["ldz"], nat.ptr(a["x"]), a["ldx"],
                                        nat.ptr(a["y"]), a["ldy"], nat.ptr(a["mean"]), nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), a["x"], a["mean"]


BAD_WORLD = {
    "T<2": dict(T=1), "F<4": dict(F=3), "range_end>F+3": dict(end=[3, 10]), "range_start<0": dict(start=[-1, 6]),
    "range_reversed": dict(start=[3, 6], end=[0, 8]), "ranges_overlap": dict(start=[0, 2], end=[3, 8]),
    "range_holds_type": dict(start=[0, 7], end=[3, 9]), "range_is_type": dict(start=[0, 8], end=[3, 9]),
    "y_end>F": dict(y_end=7), "y_start!=0": dict(y_start=1, y_end=4), "y_end<3": dict(y_end=2),
    "type_index=F": dict(type_index=6), "type_index<3": dict(type_index=2), "type_index<0": dict(type_index=-1),
    "n>4": dict(n=5), "n<0": dict(n=-1), "ldx<F+3": dict(ldx=8), "ldy<width": dict(ldy=2), "ldz<width": dict(ldz=4),
    "mean_null": dict(mean=None), "mean_null_no_nodes": dict(mean=None, N=0),
}


@pytest.mark.parametrize("name", list(BAD_WORLD))
def test_bad_world_arguments_are_refused_before_any_launch(name):
    rc, msg, x, mean = _raw_world(**BAD_WORLD[name])
    assert rc != 0 and "feed_batch_world" in msg, (rc, msg)
    assert bool((x == SENTINEL).all()) and (mean is None or bool((mean == SENTINEL).all()))


def test_the_valid_raw_world_call_runs():
    rc, _, x, mean = _raw_world()
    assert rc == 0 and bool((x[:, 9:] == SENTINEL).all()) and bool((mean == 0).all())
    assert bool((x[:, 8] == torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 0, 0], device=DEV)).all())
    assert bool((x[:, :8] == 0).all())


def _raw_edges(**over):
    from graphphysics import _native as nat

    a = {"senders": torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV),
         "receivers": torch.tensor([1, 2, 2], dtype=torch.int32, device=DEV), "E": 3,
         "x": torch.arange(12.0, device=DEV).reshape(3, 4), "ldx": 4,
         "ea": torch.full((3, 8), SENTINEL, device=DEV), "ld_ea": 8, "start": 4}
    a.update(over)
    rc = nat.lib().mgn_feed_world_edge_features(nat.ptr(a["senders"]), nat.ptr(a["receivers"]), a["E"],
                                                nat.ptr(a["x"]), a["ldx"], nat.ptr(a["ea"]), a["ld_ea"], a["start"],
                                                nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), a["ea"]


BAD_EDGES = {"ld_ea<start+4": dict(ld_ea=7), "start<0": dict(start=-1), "start_too_big": dict(start=5),
             "ldx<3": dict(ldx=2), "E<0": dict(E=-1), "senders_null": dict(senders=None),
             "receivers_null": dict(receivers=None), "x_null": dict(x=None)}


@pytest.mark.parametrize("name", list(BAD_EDGES))
def test_bad_edge_arguments_are_refused_before_any_launch(name):
    rc, msg, ea = _raw_edges(**BAD_EDGES[name])
    assert rc != 0 and "feed_world_edge_features" in msg, (rc, msg)
    assert bool((ea == SENTINEL).all())


def test_the_valid_raw_edge_call_runs():
    rc, _, ea = _raw_edges()
    assert rc == 0 and bool((ea[:, :4] == SENTINEL).all())
    norm = float(torch.sqrt(torch.tensor(48.0)))
    want = torch.tensor([[-4.0, -4, -4, norm], [-4.0, -4, -4, norm], [0.0, 0, 0, 0]], device=DEV)
    assert torch.equal(ea[:, 4:], want)


# ----------------------------------------------------------------------------- TrainStep(feed=...)
NOISE = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.003, "node_type_index": 6}
T_PLATE, B_PLATE = 4, 2


@pytest.fixture(scope="module")
def plate():
    """A small DeformingPlate-shaped batch: plate_sample(nx=6, ny=4, nz=2) twice, T = 4 frames interpolated
    between its x and y (the second graph moves 1.5 times as far), the static edges and mesh edge features of
    plate_graph. The frames are rounded to multiples of 2^-12: every obstacle sum is then exact, so a batch built
    by the torch rules on the device is the feed's batch bit for bit, whatever order either sums in.
    Returns (traj [4, N, 4] on the device, node offsets, edge_index [2, E], clean edge_attr [E, 8])."""
    from graphphysics.utils import meshes

    kw = dict(nx=6, ny=4, nz=2)
    s = meshes.plate_sample(seed=0, **kw)
    g, _ = meshes.plate_graph(DEV, seed=0, **kw)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
    graphs = []
    for amp in (1.0, 1.5):
        frames = []
        for f in range(T_PLATE):
            w = x0[:, 0:3] + (amp * f / (T_PLATE - 1)) * (y0 - x0[:, 0:3])
            frames.append(torch.cat([torch.round(w * 4096.0) / 4096.0, x0[:, 3:4]], dim=1))
        graphs.append(torch.stack(frames))
    traj = torch.cat(graphs, dim=1).contiguous().to(DEV)
    ei = torch.cat([g.edge_index, g.edge_index + n], dim=1).contiguous()
    ea = torch.cat([g.edge_attr, g.edge_attr], dim=0).contiguous()
    assert traj.shape == (T_PLATE, B_PLATE * n, 4) and ea.shape[1] == 8
    return traj, [0, n, 2 * n], ei, ea


def _plate_setup():
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    torch.manual_seed(0)
    sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, EncodeProcessDecode(2, 15, 8, 3, 32, compute_dtype=torch.float32), DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def _plate_batch(plate):
    from graphphysics.utils.data import Data

    traj, gp, ei, ea = plate
    N = traj.shape[1]
    return Data(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=ea.clone())


def _plate_feed(plate):
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp, ei, ea = plate
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6, "edge_index": ei,
          "edge_attr_start": 4}
    return ResidentTrajectories(traj, gp, (0, 3), 3, noise=NOISE, frames=[0, 0], world_pos=wp)


FRAMES = ([0, 2], [2, 1], [1, 1])
SEEDS = (11, 12, 13)


def _run_fed(plate, graph):
    """Three steps on explicit frames. The default generator is re-seeded before each step, and the fill's
    normal_ is the step's first draw, so the eager and the captured step draw the same normals (asserted by the
    caller on the recorded z)."""
    from graphphysics.training.step import TrainStep

    feed = _plate_feed(plate)
    sim, opt, sch = _plate_setup()
    step = TrainStep(sim, opt, sch, _plate_batch(plate), graph=graph, feed=feed)
    if graph:
        step.capture()  # the warm-up steps draw too: record first, so every seeded step below is one replay
    losses, zs, xs, eas = [], [], [], []
    for fr, seed in zip(FRAMES, SEEDS):
        feed.set_frames(fr)
        torch.manual_seed(seed)
        losses.append(float(step().item()))
        zs.append(feed.z.clone())
        xs.append(step.batch.x.clone())
        eas.append(step.batch.edge_attr.clone())
    torch.cuda.synchronize()
    return dict(losses=losses, z=zs, x=xs, ea=eas, params=[p.detach().clone() for p in sim.parameters()],
                buffers=[b.detach().clone() for b in sim.buffers()], step=step, feed=feed,
                count=opt.param_groups[0]["step_count"])


def test_captured_fed_plate_step_equals_eager_and_the_host_loop(plate):
    """Mirrors test_feed_gpu.py::test_captured_fed_step_equals_eager_and_the_host_loop, with noise and the edge
    side: captured == eager at that test's tolerances on the same frames and normals; a plain captured TrainStep
    handed, by assignment, the batches the torch rules build from those frames and normals gives the same
    losses; then two replays with drawn frames train on different batches; edge_attr[:, :4] never changes."""
    from graphphysics.dataset.resident import fill_world_torch, world_edge_features_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    traj, gp, ei, clean_ea = plate
    keep, keep_ea = traj.clone(), clean_ea.clone()
    eager, cap = _run_fed(plate, False), _run_fed(plate, True)
    assert cap["step"].graph is not None and cap["count"] == 3 and eager["count"] == 3
    for a, b in zip(eager["z"], cap["z"]):
        assert torch.equal(a, b)  # the same normals, so the same batches
    for k in ("x", "ea"):
        for a, b in zip(eager[k], cap[k]):
            assert torch.equal(a, b)
    np.testing.assert_allclose(eager["losses"], cap["losses"], rtol=1e-6)
    for a, b in zip(eager["params"], cap["params"]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(eager["buffers"], cap["buffers"]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    assert len(set(cap["losses"])) == 3  # three different batches
    for ea in cap["ea"]:
        assert torch.equal(ea[:, :4], clean_ea[:, :4])
    assert not torch.equal(cap["ea"][0][:, 4:], cap["ea"][1][:, 4:])

    # the host loop the feed replaces, from the same frames and normals: the torch rules on the CPU (IEEE division
    # and square root; the plate's obstacle sums are exact), so its batches are the feed's bit for bit
    feed = cap["feed"]
    sim, opt, sch = _plate_setup()
    step, losses = None, []
    for i, fr in enumerate(FRAMES):
        x, y, _ = fill_world_torch(traj.cpu(), gp, torch.tensor(fr, dtype=torch.int32), (0, 3), 3, feed.ranges,
                                   feed.scales.cpu(), cap["z"][i].cpu())
        ea = world_edge_features_torch(x, ei.cpu(), clean_ea.cpu(), 4)
        x, y, ea = x.to(DEV), y.to(DEV), ea.to(DEV)
        assert torch.equal(x, cap["x"][i]) and torch.equal(ea, cap["ea"][i])
        b = Data(x=x, y=y, edge_index=ei, edge_attr=ea)
        if step is None:
            step = TrainStep(sim, opt, sch, b, graph=True)
        else:
            step.batch = b
        losses.append(float(step().item()))
    np.testing.assert_allclose(losses, cap["losses"], rtol=1e-6)

    # drawn frames: the step is recorded anew with the draw inside, and every replay fills another batch
    step = cap["step"]
    feed.set_frames("random")
    torch.manual_seed(1)
    seen = []
    for _ in range(6):
        assert np.isfinite(float(step().item()))
        seen.append((feed.frame.clone(), feed.z.clone(), step.batch.x.clone(), step.batch.edge_attr.clone()))
        assert torch.equal(step.batch.edge_attr[:, :4], clean_ea[:, :4])
        assert int(feed.frame.min()) >= 0 and int(feed.frame.max()) <= T_PLATE - 2
    for (fa, za, xa, ea_a), (fb, zb, xb, ea_b) in zip(seen, seen[1:]):
        assert not torch.equal(za, zb) and not torch.equal(xa, xb) and not torch.equal(ea_a[:, 4:], ea_b[:, 4:])
    assert len({tuple(f.tolist()) for f, _, _, _ in seen}) > 1  # 6 draws of 2 frames out of 3 each
    assert torch.equal(traj, keep) and torch.equal(clean_ea, keep_ea)
