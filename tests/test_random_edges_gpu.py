"""Random long-range edges on the GPU: libmgn's mgn_random_topology_build against the rule as torch ops
(dataset.resident.random_topology_torch, itself checked against a literal walk in test_random_edges_cpu.py), entry for
entry; the switch; graph attention on a rebuilt topology with a stale tail; a captured TrainStep(feed=random_edges
feed) and the captured resident rollout against the per-step host loop (the torch rule, a fresh host-built topology, an
eager step).

The build is integer work, so its arrays are compared entry for entry; the attention kernels are deterministic and read
a topology only through those arrays, so outputs on the rebuilt topology and on a host-built one are compared with
torch.equal."""
import pytest
import torch

import _world_edges as WE
import test_random_edges_cpu as RC

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


def _topology(gp, mesh, cp, W):
    from graphphysics.models._engine import RandomTopology

    return RandomTopology(mesh, gp, gp[-1], cp, W, DEV)


def _on(enabled=True):
    return torch.tensor([1 if enabled else 0], dtype=torch.int32, device=DEV)


def _assert_equals_rule(topo, pairs, gp, cp, mesh, W, enabled=True):
    """edge_index[:, :E], the first E entries of the per-edge arrays, both pointer arrays and num_edges_dev against
    random_topology_torch of the same pairs; returns E."""
    from graphphysics.dataset.resident import random_topology_torch

    N = gp[-1]
    ei, want = random_topology_torch(pairs.cpu(), gp, mesh, W, enabled, cand_ptr=cp)
    E = int(topo.num_edges_dev.item())
    assert E == ei.shape[1]
    assert torch.equal(topo.edge_index[:, :E].cpu(), ei)
    for k in WE.ARRAYS:
        n = N + 1 if k.endswith("_ptr") else E
        assert torch.equal(getattr(topo, k)[:n].cpu(), want[k]), k
    assert topo.num_edges == mesh.shape[1] + N * W and topo.struct.num_edges == topo.num_edges
    return E


def _draw(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2 ** 31 - 1, (C, 2), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)


def _cand(gp, mesh, ratio):
    from graphphysics.dataset.resident import random_candidate_ptr

    return random_candidate_ptr(gp, mesh, ratio)


# ---------------------------------------------------------------------------------------------- the raw build
def test_one_node():
    none = torch.zeros(2, 0, dtype=torch.int64)
    topo = _topology([0, 1], none, [0, 0], 4)
    topo.build(torch.zeros(0, 2, dtype=torch.int32, device=DEV), _on())
    assert _assert_equals_rule(topo, torch.zeros(0, 2, dtype=torch.int32), [0, 1], [0, 0], none, 4) == 0
    # candidates on a graph of one node are all self-pairs
    topo = _topology([0, 1], none, [0, 3], 4)
    pairs = _draw(3, 1)
    topo.build(pairs, _on())
    assert _assert_equals_rule(topo, pairs, [0, 1], [0, 3], none, 4) == 0


@pytest.mark.parametrize("W", [1, 2, 16, 64])
def test_uneven_graphs_equal_the_torch_rule(W):
    """Graphs of 1, 0, 300 and 5 nodes at ratio 1.0: a graph boundary inside a workgroup, a node range across two
    workgroups, about four candidate endpoints per node, so lists of 1 and 2 overflow (fewer edges than at 64)."""
    gp, mesh = RC.uneven_case()
    cp = _cand(gp, mesh, 1.0)
    assert cp[:3] == [0, 0, 0] and cp[3] > 500 and cp[4] > cp[3]
    topo, full = _topology(gp, mesh, cp, W), _topology(gp, mesh, cp, 64)
    for seed in (1, 2):
        pairs = _draw(cp[-1], seed)
        topo.build(pairs, _on())
        E = _assert_equals_rule(topo, pairs, gp, cp, mesh, W)
        full.build(pairs, _on())
        E_full = int(full.num_edges_dev.item())
        assert E_full > mesh.shape[1] + cp[-1]
        assert E < E_full if W <= 2 else E == E_full
        deg = torch.bincount(topo.edge_index[0, :E], minlength=gp[-1]) - torch.bincount(mesh[0], minlength=gp[-1]).to(DEV)
        assert int(deg.max()) <= W and int(deg.min()) >= 0
        if W <= 2:
            assert int(deg.max()) == W


def test_grid_with_more_candidates_than_one_tile():
    """A triangulated 27 × 26 grid at ratio 1.0: about 2,000 candidates, one LDS tile of 1024 and a partial one; and
    two builds from the same pairs are bitwise equal in every array, tails included."""
    mesh = RC.grid_mesh(27, 26)
    gp = [0, 702]
    cp = _cand(gp, mesh, 1.0)
    assert 1024 < cp[-1] < 2 * 1024
    topo = _topology(gp, mesh, cp, 16)
    pairs = _draw(cp[-1], 3)
    topo.build(pairs, _on())
    E = _assert_equals_rule(topo, pairs, gp, cp, mesh, 16)
    assert E > mesh.shape[1] + 1.8 * cp[-1]
    names = WE.ARRAYS + ("edge_index", "num_edges_dev")
    first = {k: getattr(topo, k).clone() for k in names}
    topo.build(pairs, _on())
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(topo, k), first[k]), k
    other = _topology(gp, mesh, cp, 16)  # and in another object, whose arrays start from zeros
    other.build(pairs, _on())
    for k in names:
        live = k == "edge_index" or (k in WE.ARRAYS and not k.endswith("_ptr"))  # [.., :E]; the others whole
        a, b = getattr(other, k), first[k]
        assert torch.equal(a[..., :E], b[..., :E]) if live else torch.equal(a, b), k


@pytest.mark.parametrize("kind", ["one node", "all repeats", "all mesh edges", "one pair both ways"])
def test_adversarial_pairs(kind):
    """All candidates of the large graph on one node (it overflows its 16 entries and flags the rest, which removes them
    at their other endpoints), one pair repeated throughout, mesh edges only, one pair in both orders."""
    gp, mesh = RC.uneven_case()
    cp = _cand(gp, mesh, 1.0)
    lo, n = gp[2], gp[3] - gp[2]
    pairs = _draw(cp[-1], 4).cpu()
    big = slice(cp[2], cp[3])
    C_big = cp[3] - cp[2]
    if kind == "one node":
        pairs[big, 0] = 17
        pairs[big.start:big.stop:2] = pairs[big.start:big.stop:2].flip(1)  # on either side
    elif kind == "all repeats":
        pairs[big] = torch.tensor([3 + n, 250])  # 3 through a wrap
    elif kind == "all mesh edges":
        inside = mesh[:, (mesh[0] >= lo) & (mesh[0] < lo + n)] - lo
        pairs[big] = inside[:, torch.arange(C_big) % inside.shape[1]].t().int()
    else:
        pairs[big] = torch.tensor([5, 9])
        pairs[big.start + 1:big.stop:2] = torch.tensor([9, 5])
    pairs = pairs.to(DEV)
    topo = _topology(gp, mesh, cp, 16)
    topo.build(pairs, _on())
    E = _assert_equals_rule(topo, pairs, gp, cp, mesh, 16)
    ei = topo.edge_index[:, :E].cpu()
    inside = (ei[0] >= lo) & (ei[0] < lo + n)
    new_big = int(inside.sum()) - int(((mesh[0] >= lo) & (mesh[0] < lo + n)).sum())
    if kind == "one node":
        assert new_big == 2 * 16 and int((ei[0] == lo + 17).sum()) == int((mesh[0] == lo + 17).sum()) + 16
    elif kind == "all mesh edges":
        assert new_big == 0
    else:
        assert new_big in (0, 2)  # 0 when the pair happens to be a mesh edge


# ---------------------------------------------------------------------------------------------- the switch, the tail
def test_switched_off_gives_the_host_topology_of_the_mesh():
    from graphphysics import _native as nat
    from graphphysics.models._engine import GraphTopology

    gp, mesh = RC.uneven_case()
    feed = RC.plain_feed(gp, mesh, 1.0, 16, DEV)
    batch = RC.batch_of(feed, DEV)
    torch.manual_seed(0)
    feed.fill(batch)
    assert int(feed.num_edges_dev.item()) > mesh.shape[1]
    feed.set_random_edges(False)
    feed.build_random_edges()
    E = _assert_equals_rule(feed.topology, feed.pairs, gp, feed.cand_ptr.tolist(), mesh, 16, enabled=False)
    assert E == mesh.shape[1] and torch.equal(feed.current_edge_index().cpu(), mesh)
    ref = GraphTopology(mesh.to(DEV), gp[-1])
    nat.check_errors(DEV)
    for k in WE.ARRAYS:
        n = gp[-1] + 1 if k.endswith("_ptr") else E
        assert torch.equal(getattr(feed.topology, k)[:n], getattr(ref, k)[:n]), k
    feed.fill(batch)  # a fill draws but still builds the mesh
    assert int(feed.num_edges_dev.item()) == E
    feed.set_random_edges(True)
    feed.fill(batch)
    assert int(feed.num_edges_dev.item()) > E


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_stale_tail_is_never_read_by_attention(dtype):
    """A build with many edges, then one with fewer (other pairs at a smaller live count, then the mesh alone): graph
    attention through the bound topology equals, bit for bit, attention on a host-built topology of the same
    edge_index — y, dq, dk, dv."""
    from graphphysics.models import _engine
    from graphphysics.models._engine import GraphAttentionFunction, GraphTopology

    gp, mesh = RC.uneven_case()
    N = gp[-1]
    feed = RC.plain_feed(gp, mesh, 1.0, 16, DEV)
    feed.set_pairs(_draw(feed.pairs.shape[0], 5).cpu())
    feed.build_random_edges()
    many = int(feed.num_edges_dev.item())
    g = torch.Generator().manual_seed(9)
    q0, k0, v0, gy = (torch.randn(N, 32, generator=g).to(DEV, dtype) for _ in range(4))
    fewer = _draw(feed.pairs.shape[0], 6).cpu()
    fewer[40:] = fewer[39]  # most candidates repeat one pair
    for pairs, enabled in ((fewer, True), (fewer, False)):
        feed.set_pairs(pairs)
        feed.set_random_edges(enabled)
        feed.build_random_edges()
        E = int(feed.num_edges_dev.item())
        assert mesh.shape[1] <= E < many - 100
        ei = feed.current_edge_index().clone()
        topos = (_engine.get_topology(feed.edge_index, N), GraphTopology(ei, N))
        assert topos[0] is feed.topology
        outs = []
        for topo in topos:
            q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
            y = GraphAttentionFunction.apply(topo, 2, q, k, v)
            y.backward(gy)
            outs.append((y.detach(), q.grad, k.grad, v.grad))
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
        assert float(outs[0][0].float().abs().max()) > 0


def test_captured_resident_rollout_switched_off_equals_the_plain_feed():
    """feed.set_random_edges(False); feed.build_random_edges(): the captured resident rollout on the feed's bound
    edge_index equals, bit for bit, the one on a plain feed with the mesh edge_index. The rollout never rebuilds."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    gold = WE.load_golden()
    traj, gp, mesh = WE.plate(gold, DEV)
    N = traj.shape[1]
    sim = WE.plate_transformer(DEV).eval()
    feed = ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=WE.world_pos(),
                                random_edges={"edge_index": mesh, "ratio": 0.5, "max_new": 8})
    plain = ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=WE.world_pos())

    def run(f, ei):
        ro = Rollout(sim, WE.K + 3, graph=True, feed=f, world_edges="off")
        b = _Batch(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=None,
                   pos=None)
        out = ro.rollout_resident(b, 0, 3)
        return out, torch.stack(ro.losses), ro

    want, want_loss, _ = run(plain, mesh.to(DEV))
    feed.set_pairs(_draw(feed.pairs.shape[0], 8).cpu())
    feed.build_random_edges()
    on_count = int(feed.num_edges_dev.item())
    on, _, _ = run(feed, feed.edge_index)
    assert int(feed.num_edges_dev.item()) == on_count > mesh.shape[1]  # no rebuild inside the rollout
    assert not torch.equal(on, want)
    feed.set_random_edges(False)
    feed.build_random_edges()
    got, got_loss, ro = run(feed, feed.edge_index)
    torch.cuda.synchronize()
    assert ro.resident_records == 1
    assert torch.equal(got, want) and torch.equal(got_loss, want_loss)


# ---------------------------------------------------------------------------------------------- the captured step
def _sim(node_in, type_index, seed=0):
    """The smallest transformer that exercises the path: EncodeTransformDecode(2, ..., hidden_size=32, num_heads=2)."""
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    torch.manual_seed(seed)
    model = EncodeTransformDecode(2, node_in + 9, 3, hidden_size=32, num_heads=2, compute_dtype=torch.float32)
    sim = Simulator(node_in + 9, 0, 3, 0, node_in, 0, 3, type_index, model, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def _data(feed):
    from graphphysics.utils.data import Data

    return Data(x=torch.zeros(feed.N, feed.Fx, device=DEV), y=torch.zeros(feed.N, 3, device=DEV),
                edge_index=feed.edge_index, edge_attr=None)


def _same(sims, losses):
    for other in losses[1:]:
        for a, b in zip(losses[0], other):
            assert bool(torch.isfinite(a)) and torch.equal(a, b)
    for other in sims[1:]:
        for a, b in zip(sims[0].parameters(), other.parameters()):
            assert torch.equal(a.detach(), b.detach())


def test_captured_step_draws_new_edges_on_every_replay():
    from graphphysics.dataset.resident import random_topology_torch
    from graphphysics.training.step import TrainStep

    gp, mesh = RC.uneven_case()
    feed = RC.plain_feed(gp, mesh, 0.5, 16, DEV, T=4)
    sim, opt, sch = _sim(3, 3)
    step = TrainStep(sim, opt, sch, _data(feed), graph=True, feed=feed)
    step.capture()
    graph = step.graph
    torch.manual_seed(11)
    seen = []
    for _ in range(3):
        assert bool(torch.isfinite(step()))
        assert step.graph is graph
        pairs = feed.pairs.clone()
        want, _ = random_topology_torch(pairs.cpu(), gp, mesh, 16, cand_ptr=feed.cand_ptr.tolist())
        assert torch.equal(feed.current_edge_index().cpu(), want) and want.shape[1] > mesh.shape[1]
        seen.append((pairs, want))
    for (pa, ea), (pb, eb) in zip(seen, seen[1:]):
        assert not torch.equal(pa, pb) and (ea.shape != eb.shape or not torch.equal(ea, eb))
    # switched off without a new recording: the mesh
    feed.set_random_edges(False)
    step()
    assert step.graph is graph and torch.equal(feed.current_edge_index().cpu(), mesh)
    # explicit pairs are another recording (the draw is not part of it)
    feed.set_random_edges(True)
    feed.set_pairs(seen[0][0].cpu())
    step()
    assert step.graph is not graph and torch.equal(feed.current_edge_index().cpu(), seen[0][1])


def test_captured_equals_eager_equals_the_host_loop():
    """Three steps with explicit pairs and frames changed before each: the captured step with the feed, the eager step
    with an identical feed, and the host loop — fill_torch, random_topology_torch, a NEW edge_index tensor and so a
    fresh host-built topology, an eager step — give the same losses and parameters, bit for bit."""
    from graphphysics.dataset.resident import fill_torch, random_topology_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    gp, mesh = RC.uneven_case()
    feeds = [RC.plain_feed(gp, mesh, 0.5, 16, DEV, T=4, frames=[0, 0, 0, 0]) for _ in range(2)]
    C = feeds[0].pairs.shape[0]
    plan = [([0, 0, 0, 0], _draw(C, 21).cpu()), ([2, 1, 1, 0], _draw(C, 22).cpu()), ([1, 0, 2, 2], _draw(C, 23).cpu())]
    sims, losses = [], []
    for feed, graph in zip(feeds, (True, False)):
        feed.set_pairs(plan[0][1])
        sim, opt, sch = _sim(3, 3)
        step = TrainStep(sim, opt, sch, _data(feed), graph=graph, feed=feed)
        if graph:
            step.capture()
            recorded = step.graph
        out = []
        for frames, pairs in plan:
            feed.set_frames(frames)
            feed.set_pairs(pairs)
            out.append(step().clone())
        assert not graph or step.graph is recorded
        sims.append(sim)
        losses.append(out)
    sim, opt, sch = _sim(3, 3)
    traj, step, out, counts = feeds[0].traj.cpu(), None, [], []
    for frames, pairs in plan:
        x, y = fill_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), (0, 3), 3, [], None, None)
        ei, _ = random_topology_torch(pairs, gp, mesh, 16, cand_ptr=feeds[0].cand_ptr.tolist())
        counts.append(ei.shape[1])
        b = Data(x=x.to(DEV), y=y.to(DEV), edge_index=ei.to(DEV), edge_attr=None)
        if step is None:
            step = TrainStep(sim, opt, sch, b, graph=False)
        else:
            step.batch = b
        out.append(step().clone())
    torch.cuda.synchronize()
    print("losses captured", [float(v) for v in losses[0]], "eager", [float(v) for v in losses[1]],
          "host loop", [float(v) for v in out], "edges", counts)
    assert len(set(counts)) > 1 and len({float(v) for v in out}) == 3
    _same(sims + [sim], losses + [out])


def test_captured_aneurysm_step_equals_the_host_loop():
    """The same with an aneurysm= feed (both aneurysm configs carry new_edges_ratio): the batch by fill_aneurysm_torch."""
    import _aneurysm as AN
    from graphphysics.dataset.resident import ResidentTrajectories, fill_aneurysm_torch, random_topology_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    traj, pos, gp = AN.case([40, 25], 4, 5)
    _, _, _, mesh, _ = WE.random_case(sizes=[40, 25], seed=2)
    feed = ResidentTrajectories(traj.to(DEV), gp, (0, 3), 13, aneurysm={"pos": pos.to(DEV)}, frames=[1, 1],
                                random_edges={"edge_index": mesh, "ratio": 1.0, "max_new": 4})
    C = feed.pairs.shape[0]
    plan = [([1, 2], _draw(C, 31).cpu()), ([3, 1], _draw(C, 32).cpu()), ([2, 2], _draw(C, 33).cpu())]
    feed.set_pairs(plan[0][1])
    sim, opt, sch = _sim(13, 13)
    step = TrainStep(sim, opt, sch, _data(feed), graph=True, feed=feed)
    step.capture()
    recorded, got = step.graph, []
    for frames, pairs in plan:
        feed.set_frames(frames)
        feed.set_pairs(pairs)
        got.append(step().clone())
    assert step.graph is recorded
    host, hopt, hsch = _sim(13, 13)
    hstep, out = None, []
    for frames, pairs in plan:
        x, y = fill_aneurysm_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), pos, feed.node_type.cpu(),
                                   feed.inflow_stats.cpu(), (0, 3), [], None, None)
        ei, _ = random_topology_torch(pairs, gp, mesh, 4, cand_ptr=feed.cand_ptr.tolist())
        b = Data(x=x.to(DEV), y=y.to(DEV), edge_index=ei.to(DEV), edge_attr=None)
        if hstep is None:
            hstep = TrainStep(host, hopt, hsch, b, graph=False)
        else:
            hstep.batch = b
        out.append(hstep().clone())
    torch.cuda.synchronize()
    print("losses captured", [float(v) for v in got], "host loop", [float(v) for v in out])
    _same([sim, host], [got, out])


def test_the_loss_falls_over_30_steps():
    """One fixed frame per graph, new random edges on every replay: the mean loss of the last five of 30 captured
    steps is below that of the first five."""
    from graphphysics.training.step import TrainStep

    gp, mesh = RC.uneven_case()
    feed = RC.plain_feed(gp, mesh, 0.5, 16, DEV, T=4, frames=[0, 0, 0, 0])
    sim, opt, sch = _sim(3, 3)
    step = TrainStep(sim, opt, sch, _data(feed), graph=True, feed=feed)
    torch.manual_seed(5)
    losses = [float(step()) for _ in range(30)]
    print("losses", [round(v, 4) for v in losses])
    assert all(v == v and abs(v) < float("inf") for v in losses)
    assert sum(losses[-5:]) < sum(losses[:5])


def test_a_model_with_edge_attr_is_refused_before_capture():
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    gp, mesh = RC.uneven_case()
    feed = RC.plain_feed(gp, mesh, 0.5, 16, DEV)
    model = EncodeProcessDecode(2, 3 + 9, 4, 3, 32, compute_dtype=torch.float32)
    sim = Simulator(3 + 9, 4, 3, 0, 3, 0, 3, 3, model, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3)
    batch = _data(feed)
    batch.edge_attr = torch.zeros(feed.edge_index.shape[1], 4, device=DEV)
    with pytest.raises(ValueError, match="edge_attr"):
        TrainStep(sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100), batch, graph=True, feed=feed)
    sim2, opt2, sch2 = _sim(3, 3)
    other = _data(feed)
    other.edge_index = mesh.to(DEV)
    with pytest.raises(ValueError, match="feed.edge_index"):
        TrainStep(sim2, opt2, sch2, other, graph=True, feed=feed)
