"""Per-frame world edges on the GPU: libmgn's mgn_world_topology_build against the reference's own add_world_edges
(tests/golden/world_edges_golden.npz) through GraphTopology(reference edge_index), and against the same rule as
torch ops (dataset.resident.world_topology_torch) on seeded random graphs; the capacity bit; graph attention on the
bound dynamic topology; a captured TrainStep(feed=dynamic_edges feed) and the captured resident rollout against the
per-frame host loop (add_world_edges per graph, a fresh topology, an eager step).

The build is integer work plus one fp64 comparison per candidate pair, stated term by term, so its arrays are
compared entry for entry; the attention kernels are deterministic and read a topology only through those arrays,
so their outputs on the dynamic topology and on a host-built one are compared with torch.equal."""
import pytest
import torch

import _world_edges as WE
from _world_edges import K, N1

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


@pytest.fixture(scope="module")
def gold():
    return WE.load_golden()


def _build(pos, types, gp, mesh, radius, W):
    """DynamicTopology over the case, built once from pos [N, 3] / types [N] (CPU tensors): the x the kernel reads is
    a batch row [pos ‖ junk ‖ type], so both strides are exercised."""
    from graphphysics.models._engine import DynamicTopology

    N = pos.shape[0]
    x = torch.full((N, 7), -5.0)
    x[:, 0:3], x[:, 6] = pos, types
    x = x.to(DEV)
    topo = DynamicTopology(mesh, gp, N, radius, W, DEV)
    topo.build(x, x[:, 6])
    return topo


def _assert_topology_equals(topo, ei, N):
    """The first num_edges entries of the per-edge arrays, both pointer arrays, num_edges and the live columns of
    edge_index, against GraphTopology(ei) and a plain stable-sort restatement."""
    from graphphysics import _native as nat
    from graphphysics.models._engine import GraphTopology

    E = int(topo.num_edges_dev.item())
    nat.check_errors(DEV)
    assert E == ei.shape[1]
    assert torch.equal(topo.edge_index[:, :E].cpu(), ei)
    ref = GraphTopology(ei.to(DEV), N)
    nat.check_errors(DEV)
    want = WE.stable_arrays(ei, N)
    for k in WE.ARRAYS:
        n = N + 1 if k.endswith("_ptr") else E
        got = getattr(topo, k)[:n].cpu()
        assert torch.equal(got, getattr(ref, k)[:n].cpu()), k
        assert torch.equal(got, want[k]), k
    assert topo.num_edges == topo.num_mesh_edges + N * topo.max_neighbors and topo.struct.num_edges == topo.num_edges


@pytest.mark.parametrize("W", [10, 16])
def test_raw_build_equals_the_reference_on_every_frame(gold, W):
    traj, gp, mesh = WE.plate(gold)
    for frames in ((0, 0), (1, 1), (2, 2), (3, 3), (3, 2)):
        pos = torch.cat([traj[frames[0], :N1, 0:3], traj[frames[1], N1:, 0:3]])
        topo = _build(pos, traj[0, :, K], gp, mesh, gold["plate_radius"], W)
        _assert_topology_equals(topo, WE.ref_edge_index(gold, frames), 2 * N1)
        assert int(topo.num_edges_dev.item()) == WE.ref_counts(gold, frames)


def test_raw_build_on_the_hand_made_graph(gold):
    topo = _build(gold["hand_pos"], gold["hand_type"], [0, 12], gold["hand_mesh"], gold["hand_radius"], 2)
    _assert_topology_equals(topo, gold["hand_ei"], 12)


RANDOM = [dict(sizes=[1]), dict(sizes=[63]), dict(sizes=[64]), dict(sizes=[65]), dict(sizes=[255]), dict(sizes=[256]),
          dict(sizes=[257]), dict(sizes=[300]), dict(sizes=[1100], radius=0.0625),
          dict(sizes=[40, 0, 50]), dict(sizes=[70, 30, 33], no_obstacle=0, all_obstacle=1),
          dict(sizes=[0, 129, 0])]


@pytest.mark.parametrize("case", RANDOM, ids=lambda c: "-".join(map(str, c["sizes"])))
def test_raw_build_equals_the_torch_rule_on_random_graphs(case):
    """N = 1, 63, 64, 65 (a wave, its last lane, the first lane of a second), 255, 256, 257 and 300 (the same for a
    workgroup of the search), 1100 (more than one candidate tile of 1024), empty graphs, a graph without OBSTACLE
    nodes and one made only of them; max_neighbors is the
    largest world degree of the case, so one node's degree equals it exactly; then once more with room to spare."""
    from graphphysics.dataset.resident import world_topology_torch

    pos, types, gp, mesh, radius = WE.random_case(seed=sum(case["sizes"]), **case)
    N = pos.shape[0]
    ei, _ = world_topology_torch(pos, types, gp, mesh, radius)
    mkey, key = mesh[0] * N + mesh[1], ei[0] * N + ei[1]
    world = ei[:, ~torch.isin(key, mkey)]
    deg = int(torch.bincount(world[0], minlength=N).max()) if world.shape[1] else 0
    if N >= 63:
        assert deg >= 2, "the case has no contacts to speak of"
    for W in (max(deg, 1), deg + 3):
        topo = _build(pos, types, gp, mesh, radius, W)
        _assert_topology_equals(topo, ei, N)
    if sum(1 for s in case["sizes"] if s) > 1:  # a search across the batch would have linked two graphs
        whole, _ = world_topology_torch(pos, types, [0, N], mesh, radius)
        assert whole.shape[1] > ei.shape[1]


def test_no_nodes_is_success_without_a_launch():
    topo = _build(torch.zeros(0, 3), torch.zeros(0), [0], torch.zeros(2, 0, dtype=torch.int64), 0.03, 4)
    torch.cuda.synchronize()
    assert int(topo.num_edges_dev.item()) == 0 and topo.num_edges == 0


def test_overflow_sets_the_bit_skips_adamw_and_raises(gold):
    """max_neighbors = 9 on frame 3 (largest world in-degree 10): the build flags MGN_ERR_WORLD_CAPACITY, an AdamW
    step issued meanwhile leaves the parameters alone, the next poll raises the capacity ValueError and clears the
    word; every index the build wrote is inside its array."""
    from graphphysics import _native as nat
    from graphphysics.training.optim import FusedAdamW

    traj, gp, mesh = WE.plate(gold)
    nat.check_errors(DEV)
    p = torch.nn.Parameter(torch.ones(64, device=DEV))
    opt = FusedAdamW([p], lr=0.1)
    pos = torch.cat([traj[3, :N1, 0:3], traj[3, N1:, 0:3]])
    topo = _build(pos, traj[0, :, K], gp, mesh, gold["plate_radius"], 9)
    p.grad = torch.ones_like(p)
    opt.step()
    torch.cuda.synchronize()
    ew = nat.error_word(DEV)
    assert int(ew.dev.item()) & nat.ERR_WORLD_CAPACITY
    assert torch.equal(p.detach(), torch.ones_like(p))
    N, E_cap = 2 * N1, topo.num_edges
    E = int(topo.num_edges_dev.item())
    assert 0 <= E <= E_cap
    for k in ("csc_src", "csc_dst"):
        a = getattr(topo, k)
        assert int(a.min()) >= 0 and int(a.max()) < N, k
    for k in ("csc_eid", "row_perm"):
        a = getattr(topo, k)
        assert int(a.min()) >= 0 and int(a.max()) < E_cap, k
    for k in ("col_ptr", "row_ptr"):
        a = getattr(topo, k)
        assert int(a.min()) >= 0 and int(a.max()) <= E_cap and bool((a[1:] >= a[:-1]).all()), k
    assert int(topo.edge_index.min()) >= 0 and int(topo.edge_index.max()) < N
    ew.arm()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="max_neighbors") as info:
        nat.poll_errors(DEV)
    assert info.value.mgn_skipped_updates == 1
    assert int(ew.dev.item()) == 0
    nat.check_errors(DEV)
    opt.step()  # the word is clear: the update runs
    torch.cuda.synchronize()
    assert not torch.equal(p.detach(), torch.ones_like(p))


@pytest.mark.parametrize("hidden,heads", [(64, 4), (16, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attention_on_the_bound_topology_equals_the_host_built_one(gold, hidden, heads, dtype):
    """GraphAttentionFunction through get_topology on the feed's bound tensor (frame 3 of both graphs) and on
    GraphTopology(reference edge_index): y, dq, dk, dv are equal bit for bit."""
    from graphphysics.models import _engine
    from graphphysics.models._engine import GraphAttentionFunction, GraphTopology

    traj, gp, mesh = WE.plate(gold, DEV)
    feed = WE.dyn_feed(traj, gp, mesh, W=16, frames=[3, 3])
    batch = _Batch(x=torch.zeros(2 * N1, 7, device=DEV), y=torch.zeros(2 * N1, 3, device=DEV),
                   edge_index=feed.edge_index, edge_attr=None)
    feed.fill(batch)
    ei = WE.ref_edge_index(gold, (3, 3)).to(DEV)
    topos = (_engine.get_topology(feed.edge_index, 2 * N1), GraphTopology(ei, 2 * N1))
    assert topos[0] is feed.topology and int(feed.num_edges_dev.item()) == ei.shape[1]
    g = torch.Generator().manual_seed(hidden + heads)
    q0, k0, v0, gy = (torch.randn(2 * N1, hidden, generator=g).to(DEV, dtype) for _ in range(4))
    outs = []
    for topo in topos:
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        y = GraphAttentionFunction.apply(topo, heads, q, k, v)
        y.backward(gy)
        outs.append((y.detach(), q.grad, k.grad, v.grad))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    assert float(outs[0][0].float().abs().max()) > 0


NOISE = {"noise_index_start": [0], "noise_index_end": [3], "noise_scale": [0.002], "node_type_index": K + 3}
STEPS = (((0, 0), 21), ((3, 2), 22), ((1, 3), 23))  # (frames, seed of the step's normals)


def _opt(sim):
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def test_captured_fed_step_equals_the_host_loop_and_is_recorded_once(gold):
    """TrainStep(feed=dynamic_edges feed) with noise, explicit frames, explicit normals: one recording, a replay per
    step at frames (0, 0), (3, 2), (1, 3); the loss of every step and all parameters afterwards equal, bit for bit,
    those of an identical model stepped eagerly through the host loop (the batch by the torch rules from the same
    normals, add_world_edges per graph on that x, a fresh topology). With a zero noise scale the replays' edge counts
    are the fixture's."""
    from graphphysics.dataset.resident import fill_world_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    traj, gp, mesh = WE.plate(gold, DEV)
    N = 2 * N1
    feed = WE.dyn_feed(traj, gp, mesh, W=16, noise=NOISE, frames=[0, 0])
    sim = WE.plate_transformer(DEV)
    opt, sch = _opt(sim)
    batch = Data(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=feed.edge_index,
                 edge_attr=None)
    step = TrainStep(sim, opt, sch, batch, graph=True, feed=feed)
    step.capture()
    graph = step.graph
    losses, zs, xs, counts = [], [], [], []
    for frames, seed in STEPS:
        feed.set_frames(list(frames))
        torch.manual_seed(seed)
        losses.append(step().clone())
        zs.append(feed.z.clone())
        xs.append(step.batch.x.clone())
        counts.append(int(feed.num_edges_dev.item()))
        assert step.graph is graph  # never re-recorded
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in sim.parameters()]

    host = WE.plate_transformer(DEV)
    hopt, hsch = _opt(host)
    hstep, hlosses = None, []
    for i, (frames, _) in enumerate(STEPS):
        x, y, _ = fill_world_torch(traj.cpu(), gp, torch.tensor(frames, dtype=torch.int32), (0, 3), K, feed.ranges,
                                   feed.scales.cpu(), zs[i].cpu())
        assert torch.equal(x.to(DEV), xs[i])
        ei = WE.host_edges(x, gp, mesh)
        assert ei.shape[1] == counts[i], (i, ei.shape[1], counts[i])
        b = Data(x=x.to(DEV), y=y.to(DEV), edge_index=ei.to(DEV), edge_attr=None)
        if hstep is None:
            hstep = TrainStep(host, hopt, hsch, b, graph=False)
        else:
            hstep.batch = b
        hlosses.append(hstep().clone())
    torch.cuda.synchronize()
    print("losses captured", [float(v) for v in losses], "host loop", [float(v) for v in hlosses])
    print("max |param difference|", max(float((a - b.detach()).abs().max()) for a, b in zip(params, host.parameters())))
    assert len(set(counts)) > 1
    for a, b in zip(losses, hlosses):
        assert torch.equal(a, b)
    for a, b in zip(params, host.parameters()):
        assert torch.equal(a, b.detach())

    # a zero noise scale: the fixture's counts, still the same recording
    feed.set_noise_t(1.0)
    for frames in ((0, 0), (3, 2)):
        feed.set_frames(list(frames))
        step()
        assert step.graph is graph
        assert int(feed.num_edges_dev.item()) == WE.ref_counts(gold, frames)
        assert torch.equal(feed.current_edge_index().cpu(), WE.ref_edge_index(gold, frames))


@pytest.mark.parametrize("mode", ["frame", "prediction"])
def test_captured_resident_rollout_equals_the_host_loop(gold, mode):
    """Three steps from frame 0, one recording: predictions, losses and squared errors equal the per-frame host
    loop's bit for bit; in "frame" mode the steps' edge counts are the fixture's."""
    from graphphysics import _native as nat
    from graphphysics.training.rollout import Rollout

    traj, gp, mesh = WE.plate(gold, DEV)
    N = 2 * N1
    sim = WE.plate_transformer(DEV).eval()
    want, old, counts, xs = WE.rollout_host_loop(sim, traj.cpu(), gp, mesh, [0, 0], 3, mode, DEV)
    feed = WE.dyn_feed(traj, gp, mesh, W=16)
    ro = Rollout(sim, K + 3, graph=True, feed=feed, world_edges=mode)
    batch = _Batch(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=feed.edge_index,
                   edge_attr=None, pos=None)
    got = ro.rollout_resident(batch, 0, 3)
    torch.cuda.synchronize()
    assert ro.resident_records == 1
    print("max |prediction difference|", float((got - want).abs().max()))
    assert torch.equal(got, want)
    assert torch.equal(torch.stack(ro.losses), torch.stack(old.losses))
    # the squared errors: mgn_rollout_end's own fixed-order sum over the host loop's predictions and targets
    last, cursor = torch.zeros(N, 3, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, sq = torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    for s in range(3):
        nat.rollout_end(old.outputs[s].contiguous(), old.targets[s].contiguous(), xs[s].to(DEV), K + 3, ro.masks, 0,
                        last, None, None, cursor, loss, sq)
    assert torch.equal(ro._res_sq[0], sq) and torch.equal(torch.stack(ro.losses), loss)
    assert abs(ro.all_rollout_rmse() - old.all_rollout_rmse()) <= 1e-6 * old.all_rollout_rmse()
    assert ro.resident_num_edges.tolist() == counts
    if mode == "frame":
        assert counts == [WE.ref_counts(gold, (s, s)) for s in range(3)]
    # a second trajectory from other frames: the same recording
    want2, _, counts2, _ = WE.rollout_host_loop(sim, traj.cpu(), gp, mesh, [1, 0], 2, mode, DEV)
    assert torch.equal(ro.rollout_resident(batch, [1, 0], 2), want2) and ro.resident_records == 1
    assert ro.resident_num_edges.tolist() == counts2
