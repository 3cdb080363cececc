"""World edges and random long-range edges in one topology, on the GPU: libmgn's mgn_world_random_topology_build against
the rule as torch ops (dataset.resident.world_random_topology_torch, itself checked against a brute-force union in
test_world_random_edges_cpu.py), entry for entry; adversarial candidates; the switch against mgn_world_topology_build
and the reference's own add_world_edges; the capacity bit; a captured TrainStep and the captured resident rollout on a
feed built with dynamic_edges= and random_edges=, against the host loop and against a dynamic_edges=-only feed.

The build is integer work plus one fp64 comparison per candidate pair, so its arrays are compared entry for entry; the
model's kernels are deterministic and read a topology only through those arrays, so losses, parameters and predictions
are compared with torch.equal. No tolerance is involved anywhere."""
import pytest
import torch

import _world_edges as WE
import test_world_random_edges_cpu as WR
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


def _x(pos, types):
    """The batch rows [pos ‖ junk ‖ type] the kernel reads, so that both strides are exercised."""
    x = torch.full((pos.shape[0], 7), -5.0)
    x[:, 0:3], x[:, 6] = pos, types
    return x.to(DEV)


def _topology(c, W, R):
    from graphphysics.models._engine import WorldRandomTopology

    return WorldRandomTopology(c["mesh"], c["gp"], c["gp"][-1], c["radius"], W, c["cp"], R, DEV)


def _on(enabled=True):
    return torch.tensor([1 if enabled else 0], dtype=torch.int32, device=DEV)


def _assert_equals(topo, ei, want, N):
    """edge_index[:, :E], the first E entries of the per-edge arrays, both pointer arrays and num_edges_dev against an
    (edge_index, arrays) of the torch rule; returns E."""
    from graphphysics import _native as nat

    E = int(topo.num_edges_dev.item())
    nat.check_errors(DEV)
    assert E == ei.shape[1]
    assert torch.equal(topo.edge_index[:, :E].cpu(), ei.cpu())
    for k in WE.ARRAYS:
        n = N + 1 if k.endswith("_ptr") else E
        assert torch.equal(getattr(topo, k)[:n].cpu(), want[k].cpu()), k
    return E


def _assert_equals_rule(topo, c, pairs, W, R, enabled=True):
    from graphphysics.dataset.resident import world_random_topology_torch

    ei, want = world_random_topology_torch(c["pos"], c["types"], pairs.cpu(), c["gp"], c["mesh"], c["radius"], W, R,
                                           enabled, cand_ptr=c["cp"])
    N = c["gp"][-1]
    E = _assert_equals(topo, ei, want, N)
    assert topo.num_edges == c["mesh"].shape[1] + N * (W + R) and topo.struct.num_edges == topo.num_edges
    return E, ei


# ---------------------------------------------------------------------------------------------- the raw build
CASES = [dict(seed=1), dict(seed=2), dict(seed=3), dict(seed=4, no_obstacle=2, all_obstacle=4)]


@pytest.mark.parametrize("R", [1, 2, 16, 64])
def test_uneven_graphs_equal_the_torch_rule(R):
    """Graphs of 1, 2, 37, 300 and 5 nodes at ratio 1.0 (a graph boundary inside a workgroup, a node range across two
    workgroups), a graph without OBSTACLE nodes and one made only of them; max_neighbors is the rule's own largest world
    degree, computed on the CPU first, so one node's world list is exactly full. Lists of 1 and 2 overflow."""
    for kw in CASES:
        c = WR.case(**kw)
        N, W = c["gp"][-1], max(c["deg"], 1)
        assert c["deg"] >= 2
        topo = _topology(c, W, R)
        pairs = WR.draw(c["cp"][-1], 40 + kw["seed"], DEV)
        x = _x(c["pos"], c["types"])
        topo.build(x, x[:, 6], pairs, _on())
        E, ei = _assert_equals_rule(topo, c, pairs, W, R)
        assert E > c["ei_w"].shape[1] > c["mesh"].shape[1]
        key, wkey = ei[0] * N + ei[1], c["ei_w"][0] * N + c["ei_w"][1]
        assert bool(torch.isin(wkey, key).all())
        new = key[~torch.isin(key, wkey)]
        deg = torch.bincount(torch.div(new, N, rounding_mode="floor"), minlength=N)
        assert int(deg.max()) <= R
        if R <= 2:
            assert int(deg.max()) == R


def test_more_than_one_workgroup_tile_and_queue():
    """A graph of 700 nodes behind one of 3, ratio 1.0 on the dense random mesh: three workgroups of the search, about
    1,400 candidates (one LDS tile of 1024 and a partial one, so the register prefetch runs ahead once), and 60
    candidates on one node, whose queue of 32 is drained in the middle of the scan. Two builds are bitwise equal."""
    c = WR.case(7, sizes=[3, 700], radius=0.0625)
    N, W, R = c["gp"][-1], max(c["deg"], 1), 16
    C = c["cp"][-1]
    assert 1024 < C < 2048 and c["deg"] >= 2
    pairs = WR.draw(C, 8)
    at = c["cp"][1] + 200
    pairs[at:at + 60, 0] = 40
    pairs[at:at + 60:2] = pairs[at:at + 60:2].flip(1)
    pairs = pairs.to(DEV)
    x = _x(c["pos"], c["types"])
    topo = _topology(c, W, R)
    topo.build(x, x[:, 6], pairs, _on())
    E, ei = _assert_equals_rule(topo, c, pairs, W, R)
    assert E > c["ei_w"].shape[1] + 1.8 * C
    names = WE.ARRAYS + ("edge_index", "num_edges_dev")
    first = {k: getattr(topo, k).clone() for k in names}
    topo.build(x, x[:, 6], pairs, _on())
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(topo, k), first[k]), k


def _feed_of(c, W, R, **kw):
    """A resident feed with both over the case: two equal frames [pos ‖ type], no noise, frame 0 of every graph, so
    the fill's x carries the case's positions exactly."""
    from graphphysics.dataset.resident import ResidentTrajectories

    row = torch.cat([c["pos"], c["types"][:, None]], dim=1)
    traj = torch.stack([row, row]).contiguous().to(DEV)
    B = len(c["gp"]) - 1
    return ResidentTrajectories(traj, c["gp"], (0, 3), K, world_pos=WE.world_pos(), frames=[0] * B,
                                dynamic_edges={"edge_index": c["mesh"], "radius": c["radius"], "max_neighbors": W},
                                random_edges={"edge_index": c["mesh"], "ratio": 1.0, "max_new": R}, one_topology=True,
                                **kw)


@pytest.mark.parametrize("kind", ["all world edges", "all mesh edges", "all repeats", "one pair both ways",
                                  "self-pairs"])
def test_adversarial_pairs(kind):
    """Every candidate of the large graph is a world edge of this build (taken from step 1 of the rule: nothing is
    added, which fails when the second exclusion list is wrong), a mesh edge, a repeat of one pair, one pair in both
    orders, a self-pair."""
    c = WR.case(6, obstacles=True)
    N, W, R = c["gp"][-1], max(c["deg"], 1), 16
    feed = _feed_of(c, W, R)
    assert feed.cand_ptr.tolist() == c["cp"]
    lo, n = c["gp"][3], 300
    big = slice(c["cp"][3], c["cp"][4])
    C_big = big.stop - big.start
    pairs = WR.draw(c["cp"][-1], 9)
    pairs[:big.start] = 0  # the small graphs add nothing: self-pairs
    pairs[big.stop:] = 0
    mkey = c["mesh"][0] * N + c["mesh"][1]
    wkey = c["ei_w"][0] * N + c["ei_w"][1]
    if kind == "all world edges":
        world = c["ei_w"][:, ~torch.isin(wkey, mkey)]
        world = world[:, world[0] >= lo] - lo
        assert world.shape[1] >= 100 and int(world.max()) < n
        pairs[big] = world[:, torch.arange(C_big) % world.shape[1]].t().int()
        pairs[big.start:big.stop:3, 0] += n  # some through a wrap
    elif kind == "all mesh edges":
        inside = c["mesh"][:, (c["mesh"][0] >= lo) & (c["mesh"][0] < lo + n)] - lo
        pairs[big] = inside[:, torch.arange(C_big) % inside.shape[1]].t().int()
    elif kind == "all repeats":
        pairs[big] = torch.tensor([3 + n, 250], dtype=torch.int32)
    elif kind == "one pair both ways":
        pairs[big] = torch.tensor([5, 9], dtype=torch.int32)
        pairs[big.start + 1:big.stop:2] = torch.tensor([9, 5], dtype=torch.int32)
    else:
        pairs[big, 0] %= 100000
        pairs[big, 1] = pairs[big, 0] + n * (torch.arange(C_big, dtype=torch.int32) % 2)  # half through a wrap
    feed.set_pairs(pairs)
    batch = WR.batch_of(feed, DEV)
    feed.fill(batch)
    assert torch.equal(batch.x[:, 0:3].cpu(), c["pos"])
    E, ei = _assert_equals_rule(feed.topology, c, pairs, W, R)
    assert torch.equal(feed.current_edge_index().cpu(), ei)
    added = E - c["ei_w"].shape[1]
    if kind in ("all world edges", "all mesh edges", "self-pairs"):
        assert added == 0 and torch.equal(ei, c["ei_w"])
    else:
        assert added in (0, 2)  # 0 when the pair happens to be a mesh or world edge


# ---------------------------------------------------------------------------------------------- the switch, capacity
def test_switched_off_equals_the_world_build(gold):
    """enabled = 0: the six arrays, the live columns of edge_index and the count equal a DynamicTopology build on the
    same positions, entry for entry; on the plate fixture they are the reference's add_world_edges of frames (0, 2)."""
    from graphphysics.models._engine import DynamicTopology, WorldRandomTopology
    from graphphysics.dataset.resident import random_candidate_ptr

    def compare(both, dyn, N):
        E = int(dyn.num_edges_dev.item())
        assert int(both.num_edges_dev.item()) == E
        assert torch.equal(both.edge_index[:, :E], dyn.edge_index[:, :E])
        for k in WE.ARRAYS:
            n = N + 1 if k.endswith("_ptr") else E
            assert torch.equal(getattr(both, k)[:n], getattr(dyn, k)[:n]), k
        return E

    for kw in CASES[:2] + CASES[3:4]:
        c = WR.case(**kw)
        N, W = c["gp"][-1], max(c["deg"], 1)
        x = _x(c["pos"], c["types"])
        pairs = WR.draw(c["cp"][-1], 3, DEV)
        both = _topology(c, W, 16)
        both.build(x, x[:, 6], pairs, _on())  # a build with random edges first: the tail is stale afterwards
        assert int(both.num_edges_dev.item()) > c["ei_w"].shape[1]
        both.build(x, x[:, 6], pairs, _on(False))
        dyn = DynamicTopology(c["mesh"], c["gp"], N, c["radius"], W, DEV)
        dyn.build(x, x[:, 6])
        assert compare(both, dyn, N) == c["ei_w"].shape[1]
        _assert_equals_rule(both, c, pairs, W, 16, enabled=False)
    traj, gp, mesh = WE.plate(gold)
    pos = torch.cat([traj[0, :N1, 0:3], traj[2, N1:, 0:3]])
    x = _x(pos, traj[0, :, K])
    cp = random_candidate_ptr(gp, mesh, 0.5)
    both = WorldRandomTopology(mesh, gp, 2 * N1, gold["plate_radius"], 16, cp, 8, DEV)
    both.build(x, x[:, 6], WR.draw(cp[-1], 4, DEV), _on(False))
    dyn = DynamicTopology(mesh, gp, 2 * N1, gold["plate_radius"], 16, DEV)
    dyn.build(x, x[:, 6])
    assert compare(both, dyn, 2 * N1) == WE.ref_counts(gold, (0, 2))
    assert torch.equal(both.edge_index[:, :WE.ref_counts(gold, (0, 2))].cpu(), WE.ref_edge_index(gold, (0, 2)))


def test_over_max_neighbors_flags_and_raises_over_max_new_does_not(gold):
    """max_neighbors = 9 on frame 3 of the plate (largest world degree 10): the build flags MGN_ERR_WORLD_CAPACITY and
    the next poll raises the capacity ValueError, as for dynamic_edges=; every index written is inside its array. A node
    far over max_new = 1 raises nothing."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import random_candidate_ptr
    from graphphysics.models._engine import WorldRandomTopology

    traj, gp, mesh = WE.plate(gold)
    N = 2 * N1
    pos = torch.cat([traj[3, :N1, 0:3], traj[3, N1:, 0:3]])
    x = _x(pos, traj[0, :, K])
    cp = random_candidate_ptr(gp, mesh, 1.0)
    pairs = WR.draw(cp[-1], 5)
    pairs[:, 0] = 7  # every candidate on node 7 of its graph
    pairs = pairs.to(DEV)
    nat.check_errors(DEV)
    roomy = WorldRandomTopology(mesh, gp, N, gold["plate_radius"], 16, cp, 1, DEV)
    roomy.build(x, x[:, 6], pairs, _on())
    torch.cuda.synchronize()
    nat.check_errors(DEV)  # over max_new: candidates are dropped, no error bit
    assert int(roomy.num_edges_dev.item()) == WE.ref_counts(gold, (3, 3)) + 4  # one new pair per graph
    tight = WorldRandomTopology(mesh, gp, N, gold["plate_radius"], 9, cp, 1, DEV)
    tight.build(x, x[:, 6], pairs, _on())
    torch.cuda.synchronize()
    ew = nat.error_word(DEV)
    assert int(ew.dev.item()) & nat.ERR_WORLD_CAPACITY
    E_cap = tight.num_edges
    assert 0 <= int(tight.num_edges_dev.item()) <= E_cap
    for k in ("csc_src", "csc_dst"):
        a = getattr(tight, k)
        assert int(a.min()) >= 0 and int(a.max()) < N, k
    for k in ("csc_eid", "row_perm"):
        a = getattr(tight, k)
        assert int(a.min()) >= 0 and int(a.max()) < E_cap, k
    for k in ("col_ptr", "row_ptr"):
        a = getattr(tight, k)
        assert int(a.min()) >= 0 and int(a.max()) <= E_cap and bool((a[1:] >= a[:-1]).all()), k
    assert int(tight.edge_index.min()) >= 0 and int(tight.edge_index.max()) < N
    ew.arm()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="max_neighbors"):
        nat.poll_errors(DEV)
    assert int(ew.dev.item()) == 0
    nat.check_errors(DEV)


# ---------------------------------------------------------------------------------------------- through the step
NOISE = {"noise_index_start": [0], "noise_index_end": [3], "noise_scale": [0.002], "node_type_index": K + 3}
STEPS = (((0, 0), 21), ((3, 2), 22), ((1, 3), 23))  # (frames, seed of the step's normals and of its pairs)


def _opt(sim):
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


def _data(feed):
    from graphphysics.utils.data import Data

    return Data(x=torch.zeros(feed.N, 7, device=DEV), y=torch.zeros(feed.N, 3, device=DEV),
                edge_index=feed.edge_index, edge_attr=None)


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_fed_step_equals_the_host_loop(gold, graph):
    """TrainStep(feed=combined feed) with noise, explicit frames and explicit pairs changed before every step — one
    recording and a replay per step, or the eager step — against the host loop on an identical model: fill_world_torch
    from the step's own normals, world_random_topology_torch on device tensors, a NEW edge_index tensor and so a fresh
    host-built topology, an eager step. Losses and parameters are equal bit for bit, so captured = eager = host loop."""
    from graphphysics.dataset.resident import fill_world_torch, world_random_topology_torch
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data

    traj, gp, mesh = WE.plate(gold, DEV)
    feed = WR.combined_feed(traj, gp, mesh, noise=NOISE, frames=[0, 0])
    C = feed.pairs.shape[0]
    feed.set_pairs(WR.draw(C, STEPS[0][1]))
    sim = WE.plate_transformer(DEV)
    opt, sch = _opt(sim)
    step = TrainStep(sim, opt, sch, _data(feed), graph=graph, feed=feed)
    recorded = None
    if graph:
        step.capture()
        recorded = step.graph
    losses, zs, xs, eis = [], [], [], []
    for frames, seed in STEPS:
        feed.set_frames(list(frames))
        feed.set_pairs(WR.draw(C, seed))
        torch.manual_seed(seed)
        losses.append(step().clone())
        zs.append(feed.z.clone())
        xs.append(step.batch.x.clone())
        eis.append(feed.current_edge_index().clone())
        assert step.graph is recorded  # never re-recorded
    torch.cuda.synchronize()

    host = WE.plate_transformer(DEV)
    hopt, hsch = _opt(host)
    hstep, hlosses, counts = None, [], []
    for i, (frames, seed) in enumerate(STEPS):
        x, y, _ = fill_world_torch(traj.cpu(), gp, torch.tensor(frames, dtype=torch.int32), (0, 3), K, feed.ranges,
                                   feed.scales.cpu(), zs[i].cpu())
        x = x.to(DEV)
        assert torch.equal(x, xs[i])
        ei, _ = world_random_topology_torch(x, x[:, K + 3], WR.draw(C, seed, DEV), gp, mesh.to(DEV), 0.03, 16, 8,
                                            cand_ptr=feed._cand_list)
        assert ei.is_cuda and torch.equal(ei, eis[i])
        counts.append(ei.shape[1])
        b = Data(x=x, y=y.to(DEV), edge_index=ei.contiguous(), edge_attr=None)
        if hstep is None:
            hstep = TrainStep(host, hopt, hsch, b, graph=False)
        else:
            hstep.batch = b
        hlosses.append(hstep().clone())
    torch.cuda.synchronize()
    print("losses", [float(v) for v in losses], "host loop", [float(v) for v in hlosses], "edges", counts)
    assert len(set(counts)) > 1 and len({float(v) for v in hlosses}) == 3
    for a, b in zip(losses, hlosses):
        assert bool(torch.isfinite(a)) and torch.equal(a, b)
    for a, b in zip(sim.parameters(), host.parameters()):
        assert torch.equal(a.detach(), b.detach())


def test_drawn_pairs_differ_between_replays_and_the_world_part_follows_x(gold):
    """pairs="random": two replays of one recorded graph give different live edge_index columns; each is the rule on
    that replay's noisy x and drawn pairs, and holds exactly the world edges of that x."""
    from graphphysics.dataset.resident import world_random_topology_torch, world_topology_torch
    from graphphysics.training.step import TrainStep

    traj, gp, mesh = WE.plate(gold, DEV)
    N = 2 * N1
    feed = WR.combined_feed(traj, gp, mesh, noise=NOISE, frames=[3, 2])
    sim = WE.plate_transformer(DEV)
    opt, sch = _opt(sim)
    step = TrainStep(sim, opt, sch, _data(feed), graph=True, feed=feed)
    step.capture()
    graph = step.graph
    torch.manual_seed(31)
    seen = []
    for _ in range(2):
        assert bool(torch.isfinite(step())) and step.graph is graph
        x, pairs = step.batch.x.cpu(), feed.pairs.cpu()
        ei = feed.current_edge_index().cpu()
        want, _ = world_random_topology_torch(x, x[:, K + 3], pairs, gp, mesh, 0.03, 16, 8, cand_ptr=feed._cand_list)
        assert torch.equal(ei, want)
        world, _ = world_topology_torch(x, x[:, K + 3], gp, mesh, 0.03)
        key, wkey = ei[0] * N + ei[1], world[0] * N + world[1]
        assert bool(torch.isin(wkey, key).all()) and wkey.numel() > mesh.shape[1]
        # what is not mesh or world is random: no OBSTACLE–NORMAL pair within the radius is among it
        assert key.numel() - wkey.numel() > feed.pairs.shape[0]
        seen.append((pairs, ei))
    assert not torch.equal(seen[0][0], seen[1][0])
    assert seen[0][1].shape != seen[1][1].shape or not torch.equal(seen[0][1], seen[1][1])


def test_switched_off_step_equals_the_dynamic_feed_s(gold):
    """set_random_edges(False) after the recording, with no new one: the losses and parameters of three captured steps
    equal, bit for bit, those of a captured step on a dynamic_edges=-only feed with the same frames and normals."""
    from graphphysics.training.step import TrainStep

    traj, gp, mesh = WE.plate(gold, DEV)
    runs = []
    for both in (True, False):
        feed = WR.combined_feed(traj, gp, mesh, noise=NOISE, frames=[0, 0]) if both else \
            WE.dyn_feed(traj, gp, mesh, W=16, noise=NOISE, frames=[0, 0])
        sim = WE.plate_transformer(DEV)
        opt, sch = _opt(sim)
        step = TrainStep(sim, opt, sch, _data(feed), graph=True, feed=feed)
        if both:
            feed.set_pairs(WR.draw(feed.pairs.shape[0], 2))  # only the normals are drawn: one generator sequence
        step.capture()
        graph = step.graph
        if both:
            feed.set_random_edges(False)
        losses, zs, counts = [], [], []
        for frames, seed in STEPS:
            feed.set_frames(list(frames))
            torch.manual_seed(seed)
            losses.append(step().clone())
            zs.append(feed.z.clone())
            counts.append(int(feed.num_edges_dev.item()))
            assert step.graph is graph
        torch.cuda.synchronize()
        runs.append((sim, losses, zs, counts))
    (sim_a, loss_a, z_a, n_a), (sim_b, loss_b, z_b, n_b) = runs
    print("losses switched off", [float(v) for v in loss_a], "dynamic_edges only", [float(v) for v in loss_b], n_a)
    for a, b in zip(z_a, z_b):
        assert torch.equal(a, b)  # the same normals in both runs
    assert n_a == n_b and len(set(n_a)) > 1
    for a, b in zip(loss_a, loss_b):
        assert bool(torch.isfinite(a)) and torch.equal(a, b)
    for a, b in zip(sim_a.parameters(), sim_b.parameters()):
        assert torch.equal(a.detach(), b.detach())


@pytest.mark.parametrize("mode", ["frame", "prediction"])
def test_rollout_switched_off_equals_the_dynamic_feed_s(gold, mode):
    """rollout_resident on the combined feed, switched off, equals the dynamic_edges=-only feed's rollout bit for bit:
    predictions, losses and the steps' edge counts. Switched on, with pairs held, it attends over more edges."""
    from graphphysics.training.rollout import Rollout

    traj, gp, mesh = WE.plate(gold, DEV)
    N = 2 * N1
    sim = WE.plate_transformer(DEV).eval()

    def run(feed):
        ro = Rollout(sim, K + 3, graph=True, feed=feed, world_edges=mode)
        b = _Batch(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=feed.edge_index,
                   edge_attr=None, pos=None)
        out = ro.rollout_resident(b, 0, 3)
        torch.cuda.synchronize()
        assert ro.resident_records == 1
        return out, torch.stack(ro.losses), ro.resident_num_edges.tolist()

    want, want_loss, want_counts = run(WE.dyn_feed(traj, gp, mesh, W=16))
    feed = WR.combined_feed(traj, gp, mesh)
    feed.set_pairs(WR.draw(feed.pairs.shape[0], 6))
    on, _, on_counts = run(feed)
    assert all(a > b + feed.pairs.shape[0] for a, b in zip(on_counts, want_counts)) and not torch.equal(on, want)
    assert torch.equal(feed.pairs.cpu(), WR.draw(feed.pairs.shape[0], 6))  # the rollout draws nothing
    feed.set_random_edges(False)
    got, got_loss, got_counts = run(feed)
    assert got_counts == want_counts
    assert torch.equal(got, want) and torch.equal(got_loss, want_loss)
    if mode == "frame":
        assert got_counts == [WE.ref_counts(gold, (s, s)) for s in range(3)]


def test_a_model_with_edge_attr_is_refused_before_capture(gold):
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    traj, gp, mesh = WE.plate(gold, DEV)
    feed = WR.combined_feed(traj, gp, mesh)
    model = EncodeProcessDecode(2, 6 + 9, 4, 3, 32, compute_dtype=torch.float32)
    sim = Simulator(6 + 9, 4, 3, 0, 6, 0, 3, K + 3, model, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3)
    batch = _data(feed)
    batch.edge_attr = torch.zeros(feed.edge_index.shape[1], 4, device=DEV)
    with pytest.raises(ValueError, match="edge_attr"):
        TrainStep(sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100), batch, graph=True, feed=feed)
    sim2 = WE.plate_transformer(DEV)
    opt2, sch2 = _opt(sim2)
    other = _data(feed)
    other.edge_index = mesh.to(DEV)
    with pytest.raises(ValueError, match="feed.edge_index"):
        TrainStep(sim2, opt2, sch2, other, graph=True, feed=feed)
