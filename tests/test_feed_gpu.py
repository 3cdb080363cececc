"""Resident trajectories on the GPU: libmgn's mgn_feed_batch against the same rule written as torch ops
(dataset.resident.fill_torch) and against the reference's own add_noise (tests/golden/feed_golden.npz), its
argument checks, the frame draws, and TrainStep(feed=...): eager, captured, data-parallel, transformer.

The kernel copies fp32 values and adds one rounded product to them (the torch composition's expression), so
every comparison of x and y is bit equality (torch.equal), not a tolerance."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _case(sizes, F, T, seed=0):
    """Random [T, N, F] frames on the device (the last column: node types 0, 4, 5, 6 mixed, about half NORMAL),
    node offsets, and frames that include 0 and T-2 and differ between graphs."""
    g = torch.Generator().manual_seed(seed + 31 * F + T)
    N, B = sum(sizes), len(sizes)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, F - 1] = torch.tensor([0.0, 0.0, 4.0, 5.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    frames = [0 if b == 0 else T - 2 if b == 1 else b % (T - 1) for b in range(B)]
    if B == 1:
        frames = [T - 2]
    return traj.to(DEV), gp, frames


# (graph sizes, F, T, noisy ranges, y_columns, width of x)
SHAPES = {
    "one_node": ([1], 3, 2, [(0, 2)], (0, 2), 5),
    "uneven": ([1, 64, 193], 3, 6, [(0, 2)], (0, 2), 3),
    "empty_graphs": ([0, 65, 0, 7], 6, 3, [(0, 2), (3, 5)], (1, 3), 8),
    "cylinder": ([1923] * 8, 3, 6, [(0, 2)], (0, 2), 3),
    "wide": ([100, 29], 24, 4, [(10, 17), (0, 3), (20, 23), (4, 5)], (5, 9), 32),
}


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_fill_torch_bit_for_bit(name, noise):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import fill_torch

    sizes, F, T, ranges, ycols, ldx = SHAPES[name]
    traj, gp, frames = _case(sizes, F, T)
    N, nti = traj.shape[1], F - 1
    keep = traj.clone()
    gp_d = torch.tensor(gp, dtype=torch.int32, device=DEV)
    fr_d = torch.tensor(frames, dtype=torch.int32, device=DEV)
    W = sum(e - s for s, e in ranges)
    g = torch.Generator().manual_seed(5)
    z = torch.randn(N, W, generator=g).to(DEV) if noise else None
    scales = torch.tensor([0.02, 0.5, 1.5, 3e-3][:len(ranges)], device=DEV)
    x = torch.full((N, ldx), SENTINEL, device=DEV)
    y = torch.full((N, ycols[1] - ycols[0]), SENTINEL, device=DEV)
    nat.feed_batch(traj, gp_d, fr_d, ycols, nti, ranges, scales, z, x, y)
    wx, wy = fill_torch(traj, gp, fr_d, ycols, nti, ranges, scales, z)
    torch.cuda.synchronize()
    assert torch.equal(x[:, :F], wx) and torch.equal(y, wy)
    assert bool((x[:, F:] == SENTINEL).all())
    assert torch.equal(traj, keep)
    # the rule itself, independent of fill_torch: graph by graph, from the clean frames
    for b, f in enumerate(frames):
        rows = slice(gp[b], gp[b + 1])
        assert torch.equal(y[rows], keep[f + 1, rows, ycols[0]:ycols[1]])
        quiet = [c for c in range(F) if not (noise and any(s <= c < e for s, e in ranges))]
        assert torch.equal(x[rows][:, quiet], keep[f, rows][:, quiet])
        if noise and gp[b + 1] > gp[b]:
            normal = keep[f, rows, nti] == 0
            s, e = ranges[0]
            assert torch.equal(x[rows, s:e][~normal], keep[f, rows, s:e][~normal])
            if int(normal.sum()):
                assert not torch.equal(x[rows, s:e][normal], keep[f, rows, s:e][normal])


def test_no_nodes_is_success_without_a_launch():
    from graphphysics import _native as nat

    traj = torch.zeros(3, 0, 3, device=DEV)
    x, y = torch.zeros(0, 3, device=DEV), torch.zeros(0, 2, device=DEV)
    gp, fr = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    nat.feed_batch(traj, gp, fr, (0, 2), 2, [(0, 2)], torch.ones(1, device=DEV), torch.zeros(0, 2, device=DEV), x, y)
    torch.cuda.synchronize()


def test_reference_fixture_through_the_kernel():
    """One graph, T = 2, frame 0, traj[0] = the fixture's x_in, z the normals the reference drew: x is the
    reference's add_noise output bit for bit, plain and with the curriculum scales of t = 0.25."""
    from graphphysics.dataset.resident import ResidentTrajectories

    z = np.load(os.path.join(G, "feed_golden.npz"))
    x_in = torch.from_numpy(z["x_in"])
    N, F = x_in.shape
    nti = int(z["node_type_index"])
    traj = torch.stack([x_in, x_in * 2.0]).to(DEV)
    noise = {"noise_index_start": [int(r[0]) for r in z["ranges"]], "noise_index_end": [int(r[1]) for r in z["ranges"]],
             "noise_scale": [float(s) for s in z["scales"]], "node_type_index": nti}
    feed = ResidentTrajectories(traj, [0, N], (0, 2), nti, noise=noise, frames=[0])
    from graphphysics import _native as nat

    for key, t in (("x_out", None), ("x_out_t", float(z["t"]))):
        feed.set_noise_t(t)
        x, y = torch.full((N, F), SENTINEL, device=DEV), torch.full((N, 2), SENTINEL, device=DEV)
        nat.feed_batch(traj, feed.graph_ptr, feed.frame, (0, 2), nti, feed.ranges, feed.scales,
                       torch.from_numpy(z["z"]).to(DEV), x, y)
        assert torch.equal(x.cpu(), torch.from_numpy(z[key])), key
        assert torch.equal(y.cpu(), (x_in * 2.0)[:, 0:2])


def _raw_call(**over):
    """mgn_feed_batch called directly with valid arguments for a [3, 10, 6] trajectory, except `over`. Returns
    (status, message, x): x is pre-filled with a sentinel."""
    from graphphysics import _native as nat

    T, N, F = 3, 10, 6
    a = {"traj": torch.zeros(T, N, F, device=DEV), "T": T, "N": N, "F": F,
         "graph_ptr": torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV), "B": 2,
         "frame": torch.tensor([0, 1], dtype=torch.int32, device=DEV), "y_start": 0, "y_end": 2, "type_index": 5,
         "n": 2, "start": [0, 3], "end": [2, 5], "scales": torch.ones(4, device=DEV),
         "z": torch.zeros(N, 8, device=DEV), "ldz": 8, "x": torch.full((N, 8), SENTINEL, device=DEV), "ldx": 8,
         "y": torch.full((N, 2), SENTINEL, device=DEV), "ldy": 2}
    a.update(over)
    rg = nat.FeedRanges()
    rg.n = a["n"]
    for i, (s, e) in enumerate(zip(a["start"], a["end"])):
        rg.start[i], rg.end[i] = s, e
    rc = nat.lib().mgn_feed_batch(nat.ptr(a["traj"]), a["T"], a["N"], a["F"], nat.ptr(a["graph_ptr"]), a["B"],
                                  nat.ptr(a["frame"]), a["y_start"], a["y_end"], a["type_index"], rg,
                                  nat.ptr(a["scales"]), nat.ptr(a["z"]), a["ldz"], nat.ptr(a["x"]), a["ldx"],
                                  nat.ptr(a["y"]), a["ldy"], nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), a["x"]


BAD = {
    "T<2": dict(T=1), "F<1": dict(F=0), "range_end>F": dict(end=[2, 7]), "range_start<0": dict(start=[-1, 3]),
    "range_reversed": dict(start=[2, 3], end=[0, 5]), "ranges_overlap": dict(start=[0, 1], end=[2, 5]),
    "y_end>F": dict(y_end=7), "y_start<0": dict(y_start=-1), "y_reversed": dict(y_start=3, y_end=2),
    "type_index=F": dict(type_index=6), "type_index<0": dict(type_index=-1), "n>4": dict(n=5), "n<0": dict(n=-1),
    "ldx<F": dict(ldx=5), "ldy<width": dict(ldy=1), "ldz<width": dict(ldz=3),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(name):
    rc, msg, x = _raw_call(**BAD[name])
    assert rc != 0 and "feed_batch" in msg, (rc, msg)
    assert bool((x == SENTINEL).all())


def test_the_valid_raw_call_runs():
    rc, _, x = _raw_call()
    assert rc == 0 and bool((x[:, :6] == 0).all()) and bool((x[:, 6:] == SENTINEL).all())


def test_random_frames_cover_the_frames_that_have_a_successor():
    """200 fills at B = 8, T = 6: every index in [0, 4]; each of the five values occurs (missing one has
    probability below 5 * 0.8^1600)."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.utils.data import Data

    traj, gp, _ = _case([3] * 8, 3, 6)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    b = Data(x=torch.zeros(24, 3, device=DEV), y=torch.zeros(24, 2, device=DEV))
    ptr = feed.frame.data_ptr()
    seen = []
    for _ in range(200):
        feed.fill(b)
        seen.append(feed.frame.clone())
    seen = torch.stack(seen).cpu()
    assert feed.frame.data_ptr() == ptr and feed.frame.dtype == torch.int32
    assert int(seen.min()) >= 0 and int(seen.max()) <= 4
    assert sorted(set(seen.flatten().tolist())) == [0, 1, 2, 3, 4]
    assert len({tuple(r) for r in seen.tolist()}) > 100  # the draws advance, graphs draw independently


# ----------------------------------------------------------------------------- TrainStep(feed=...)
NOISE = {"noise_index_start": 0, "noise_index_end": 2, "noise_scale": 0.02, "node_type_index": 2}


def _cylinder(batch=2):
    """(Data of cylinder_batch(batch), traj [6, N, 3] of the mesh's 6 velocity frames + node types, node offsets)."""
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    m = meshes.load_cylinder_mesh()
    b = meshes.cylinder_batch(batch, jitter=0.01, mesh=m)
    data = Data(**{k: torch.from_numpy(b[k]).to(DEV) for k in ("x", "y", "edge_index", "edge_attr")})
    vel, nt = m["velocity"].astype(np.float32), m["node_type"].astype(np.float32)
    one = np.concatenate([vel, np.broadcast_to(nt[None, :, None], (vel.shape[0], nt.shape[0], 1))], axis=2)
    traj = torch.from_numpy(np.ascontiguousarray(np.concatenate([one] * batch, axis=1))).to(DEV)
    n = nt.shape[0]
    assert traj.shape == (6, batch * n, 3)
    return data, traj, [i * n for i in range(batch + 1)]


def _epd_setup(mp=2):
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    torch.manual_seed(0)
    sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(mp, 11, 3, 2, 32, compute_dtype=torch.float32), DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def test_captured_step_consumes_the_feed():
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch
    from graphphysics.training.step import TrainStep

    data, traj, gp = _cylinder()
    keep = traj.clone()
    feed = ResidentTrajectories(traj, gp, (0, 2), 2, noise=NOISE)
    sim, opt, sch = _epd_setup()
    step = TrainStep(sim, opt, sch, data, graph=True, feed=feed)
    normal = traj[0, :, 2] == 0
    xs, zs, losses = [], [], []
    for _ in range(3):
        losses.append(float(step().item()))
        assert step.graph is not None
        wx, wy = fill_torch(traj, gp, feed.frame, (0, 2), 2, feed.ranges, feed.scales, feed.z)
        assert torch.equal(step.batch.x, wx) and torch.equal(step.batch.y, wy)
        assert int(feed.frame.min()) >= 0 and int(feed.frame.max()) <= 4
        xs.append(step.batch.x.clone())
        zs.append(feed.z.clone())
    assert all(np.isfinite(losses))
    for a, b, za, zb in ((xs[0], xs[1], zs[0], zs[1]), (xs[1], xs[2], zs[1], zs[2])):
        assert not torch.equal(za, zb)  # the generator advanced inside the graph
        assert not torch.equal(a[normal][:, :2], b[normal][:, :2])
        assert torch.equal(a[:, 2], b[:, 2])
    # rows of other types carry the clean values of whichever frame was drawn
    last = feed.frame.long()[torch.repeat_interleave(torch.arange(2, device=DEV), gp[1])]
    assert torch.equal(step.batch.x[~normal], keep[last, torch.arange(gp[2], device=DEV)][~normal])
    assert torch.equal(traj, keep)
    assert step.batch.x is not data.x  # the caller's tensors are not the recorded ones


FRAMES = ([0, 3], [4, 1], [2, 2])


def _run_fed(graph, data_parallel=None, mp=2, frames=FRAMES):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.step import TrainStep

    data, traj, gp = _cylinder()
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    sim, opt, sch = _epd_setup(mp)
    step = TrainStep(sim, opt, sch, data, graph=graph, feed=feed, data_parallel=data_parallel)
    losses = []
    for fr in frames:
        feed.set_frames(fr)
        losses.append(float(step().item()))
    torch.cuda.synchronize()
    return (losses, [p.detach().clone() for p in sim.parameters()], [b.detach().clone() for b in sim.buffers()],
            [t.detach().clone() for t in opt.param_groups[0]["flat_state"]], opt.param_groups[0]["step_count"],
            sch.last_epoch, opt.param_groups[0]["lr"])


def test_captured_fed_step_equals_eager_and_the_host_loop():
    """Explicit frames, changed before each of 3 steps, noise off: captured == eager at the tolerances of
    test_gpu_parity.py::test_captured_step_equals_eager_step; and a plain captured TrainStep handed the same three
    batches by assignment gives the same losses: the feed is the host loop it replaces."""
    from graphphysics.dataset.resident import fill_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    res = [_run_fed(False), _run_fed(True)]
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
    for a, b in zip(res[0][1], res[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(res[0][2], res[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    for a, b in zip(res[0][3], res[1][3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    assert res[0][4:] == res[1][4:] and res[1][4] == 3
    assert len(set(res[1][0])) == 3  # three different batches

    data, traj, gp = _cylinder()
    sim, opt, sch = _epd_setup()
    step, losses = None, []
    for fr in FRAMES:
        x, y = fill_torch(traj, gp, torch.tensor(fr, dtype=torch.int32, device=DEV), (0, 2), 2, [], None, None)
        b = Data(x=x, y=y, edge_index=data.edge_index, edge_attr=data.edge_attr)
        if step is None:
            step = TrainStep(sim, opt, sch, b, graph=True)
        else:
            step.batch = b
        losses.append(float(step().item()))
    np.testing.assert_allclose(losses, res[1][0], rtol=1e-6)


def test_data_parallel_prologue_sees_the_fed_batch():
    """One rank, data_parallel=True (the statistics exchange before the replay), as
    test_gpu_parity.py::test_captured_data_parallel_step_matches_captured_step and at its tolerances: with the
    same explicit frames it equals the single-process captured step, so the statistics and the masked-node
    count were taken from the fed batch, not from the batch the step was constructed with."""
    import torch.distributed as dist

    frames = FRAMES + ([1, 0],)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29900 + os.getpid() % 200))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        dp = _run_fed(True, data_parallel=True, mp=3, frames=frames)
    finally:
        dist.destroy_process_group()
    one = _run_fed(True, mp=3, frames=frames)
    np.testing.assert_allclose(dp[0], one[0], rtol=1e-6)
    for a, c in zip(dp[1], one[1]):
        torch.testing.assert_close(a, c, rtol=1e-6, atol=1e-7)


def test_transformer_trains_from_the_feed():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    data, traj, gp = _cylinder(1)
    data = Data(x=data.x, y=data.y, edge_index=data.edge_index, edge_attr=None)
    torch.manual_seed(0)
    m = EncodeTransformDecode(2, 11, 2, hidden_size=64, num_heads=4, compute_dtype=torch.float32)
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2, noise=NOISE)
    step = TrainStep(sim, opt, sch, data, graph=True, feed=feed)
    losses = [float(step().item()) for _ in range(3)]
    assert step.graph is not None and all(np.isfinite(losses)), losses
    assert step.batch.edge_attr is None and not torch.equal(feed.z, torch.zeros_like(feed.z))
