"""World positions in the resident feed on the CPU (no kernels): ResidentTrajectories(world_pos=...) through its
torch path (dataset.resident.fill_world_torch / world_edge_features_torch) against the reference's own
add_obstacles_next_pos -> add_noise -> add_world_pos_features (tests/golden/world_feed_golden.npz, written by
tests/golden/make_world_feed_golden.py), the host-side validation, the rollout's refusal, the stored data staying
clean, and a feed without world_pos= staying what it was."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
# the norm column: the reference's torch.norm is another 3-term reduction than (v0·v0 + v1·v1) + v2·v2; each is
# within 2.5·2^-24 relative of the exact value
NORM_RTOL = 5 * 2.0 ** -24


class _Batch:
    def __init__(self, x, y, edge_attr=None):
        self.x, self.y, self.edge_attr = x, y, edge_attr


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(G, "world_feed_golden.npz"))
    d = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k] for k in z.files}
    d["ranges"] = [tuple(int(v) for v in r) for r in z["ranges"]]
    d["scales"] = [float(s) for s in z["scales"]]
    d["k"] = int(z["node_type_index"])
    return d


def gold_feed(gold, dev="cpu", edges=True):
    """The fixture as a feed: T = 2, one graph, frame 0, z to be written into feed.z by the caller."""
    from graphphysics.dataset.resident import ResidentTrajectories

    k = gold["k"]
    traj = torch.stack([gold["frame"], gold["next_frame"]]).contiguous().to(dev)
    noise = {"noise_index_start": [s for s, _ in gold["ranges"]], "noise_index_end": [e for _, e in gold["ranges"]],
             "noise_scale": gold["scales"], "node_type_index": k + 3}
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": k + 3}
    if edges:
        wp.update(edge_index=gold["edge_index"].to(dev), edge_attr_start=4)
    return ResidentTrajectories(traj, [0, traj.shape[1]], (0, 3), k, noise=noise, frames=[0], world_pos=wp), traj


def test_torch_rules_reproduce_the_reference_pipeline(gold):
    from graphphysics.dataset.resident import fill_world_torch, world_edge_features_torch

    feed, traj = gold_feed(gold)
    keep = traj.clone()
    x, y, mean = fill_world_torch(traj, [0, traj.shape[1]], feed.frame, (0, 3), gold["k"], feed.ranges, feed.scales,
                                  gold["z"])
    assert torch.equal(x, gold["x_out"])
    assert torch.equal(y, gold["next_frame"][:, 0:3])
    assert torch.equal(mean[0], gold["obstacle_mean"])
    E = gold["edge_index"].shape[1]
    ea = torch.full((E, 9), SENTINEL)
    ea[:, :4] = gold["edge_attr_in"]
    world_edge_features_torch(x, gold["edge_index"], ea, 4)
    want = gold["edge_attr_out"]
    assert torch.equal(ea[:, :4], gold["edge_attr_in"]) and bool((ea[:, 8] == SENTINEL).all())
    assert torch.equal(ea[:, 4:7], want[:, 4:7])
    torch.testing.assert_close(ea[:, 7], want[:, 7], rtol=NORM_RTOL, atol=0)
    assert torch.equal(traj, keep)


def test_fill_writes_the_batch_and_leaves_the_stored_data_clean(gold):
    """Three fills on CPU tensors (explicit frames, drawn normals): traj and edge_attr[:, :4] never change,
    columns beyond those written keep their sentinel, x differs between fills on the noisy columns of NORMAL rows
    only and the edge features follow it; then the rules fill runs, on the feed's own state with the fixture's
    normals written into feed.z, give the reference's x."""
    feed, traj = gold_feed(gold)
    keep = traj.clone()
    N, E = traj.shape[1], gold["edge_index"].shape[1]
    ea = torch.full((E, 8), SENTINEL)
    ea[:, :4] = gold["edge_attr_in"]
    b = _Batch(torch.full((N, 10), SENTINEL), torch.zeros(N, 3), ea)
    seen = []
    for _ in range(3):
        assert feed.fill(b) is b
        assert torch.equal(traj, keep) and torch.equal(b.edge_attr[:, :4], gold["edge_attr_in"])
        assert bool((b.x[:, 8:] == SENTINEL).all()) and not bool((b.edge_attr == SENTINEL).any())
        assert torch.equal(b.y, keep[1, :, 0:3])
        assert torch.equal(feed.obstacle_mean[0], gold["obstacle_mean"])
        seen.append((b.x.clone(), b.edge_attr.clone()))
    normal = keep[0, :, gold["k"]] == 0
    quiet = [3, 4, 5, 6]
    for (xa, ea_a), (xb, ea_b) in zip(seen, seen[1:]):
        assert torch.equal(xa[~normal], xb[~normal]) and torch.equal(xa[:, quiet], xb[:, quiet])
        assert not torch.equal(xa[normal][:, [0, 1, 2, 7]], xb[normal][:, [0, 1, 2, 7]])
        assert not torch.equal(ea_a[:, 4:], ea_b[:, 4:])  # the edge features follow the noisy x
    # the fill with the reference's normals in feed.z's place: the same rules, the reference's bits
    from graphphysics.dataset.resident import fill_world_torch

    feed.z.copy_(gold["z"])
    x, _, _ = fill_world_torch(traj, feed.graph_ptr, feed.frame, feed.y_columns, feed.node_type_index, feed.ranges,
                               feed.scales, feed.z)
    assert torch.equal(x, gold["x_out"])


def test_x_only_feed_needs_no_edge_attr(gold):
    feed, traj = gold_feed(gold, edges=False)
    N = traj.shape[1]
    b = _Batch(torch.zeros(N, 8), torch.zeros(N, 3))
    feed.fill(b)
    assert feed.senders is None and torch.equal(b.x[:, 6], traj[0, :, gold["k"]])
    obstacle = traj[0, :, gold["k"]] == 1
    assert torch.equal(b.x[~obstacle][:, 3:6], gold["obstacle_mean"].expand(int((~obstacle).sum()), 3))
    assert torch.equal(b.x[obstacle][:, 3:6], (traj[1] - traj[0])[obstacle][:, 0:3])


def _small(F=5, k=3, sizes=(4, 6), T=3):
    g = torch.Generator().manual_seed(3)
    N = sum(sizes)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, k] = 0.0
    gp = [0]
    for s in sizes:
        traj[:, gp[-1], k] = 1.0  # the first node of every graph: OBSTACLE
        gp.append(gp[-1] + s)
    return traj, gp


def test_every_refused_configuration_raises_value_error():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _small()
    N = traj.shape[1]
    ei = torch.tensor([[0, 1, 5], [1, 0, 9]])

    def make(wp=None, traj_=traj, y=(0, 3), k=3, noise=None, rotate=None, **over):
        w = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": k + 3}
        w.update(over)
        return ResidentTrajectories(traj_, gp, y, k, noise=noise, rotate=rotate, world_pos=w if wp is None else wp)

    assert make().Fx == 8 and make(edge_index=ei, edge_attr_start=4).senders.dtype == torch.int32
    with pytest.raises(ValueError, match="keys"):
        make(radius=0.03)
    with pytest.raises(ValueError, match="dict"):
        make(wp=[0, 3, 6])
    with pytest.raises(ValueError, match=r"\(0, 3\)"):
        make(world_pos_index_start=1, world_pos_index_end=4)
    with pytest.raises(ValueError, match=r"\(0, 3\)"):
        make(world_pos_index_end=2)
    with pytest.raises(ValueError, match="y_columns"):
        make(y=(1, 4))
    with pytest.raises(ValueError, match="y_columns"):
        make(y=(0, 2))
    with pytest.raises(ValueError, match="node_type_index"):
        make(node_type_index=3)
    noise = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.1, "node_type_index": 3}
    with pytest.raises(ValueError, match="node_type_index"):
        make(noise=noise)  # the frame's index: with world_pos= the noise dict is in batch layout
    assert make(noise=dict(noise, node_type_index=6)).z.shape == (N, 3)
    assert make(noise=dict(noise, noise_index_start=7, noise_index_end=8, node_type_index=6)).ranges == [(7, 8)]
    with pytest.raises(ValueError, match="outside"):
        make(noise=dict(noise, noise_index_end=9, node_type_index=6))
    with pytest.raises(ValueError, match="node type"):
        make(noise=dict(noise, noise_index_start=5, noise_index_end=7, node_type_index=6))
    no_obstacle = traj.clone()
    no_obstacle[:, gp[1], 3] = 0.0
    with pytest.raises(ValueError, match="graph 1 has no OBSTACLE"):
        make(traj_=no_obstacle)
    for bad in (torch.tensor([[0, 1], [1, N]]), torch.tensor([[-1, 1], [1, 0]]), torch.tensor([0, 1, 2]),
                torch.zeros(3, 4, dtype=torch.int64), torch.zeros(2, 4), [[0, 1], [1, 0]]):
        with pytest.raises(ValueError, match="edge_index"):
            make(edge_index=bad, edge_attr_start=4)
    with pytest.raises(ValueError, match="go together"):
        make(edge_index=ei)
    with pytest.raises(ValueError, match="go together"):
        make(edge_attr_start=4)
    with pytest.raises(ValueError, match="edge_attr_start"):
        make(edge_index=ei, edge_attr_start=-1)
    with pytest.raises(ValueError, match="rotate"):
        make(rotate={"feature_indices": [(0, 3)]})
    with pytest.raises(ValueError, match="F = 3"):
        ResidentTrajectories(traj[:, :, :3].contiguous(), gp, (0, 3), 2,
                             world_pos={"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 5})
    with pytest.raises(ValueError, match=">= 3"):
        make(k=2)


def test_fill_validates_the_batch():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _small()
    N = traj.shape[1]
    ei = torch.tensor([[0, 1, 5], [1, 0, 9]])
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6, "edge_index": ei,
          "edge_attr_start": 4}
    feed = ResidentTrajectories(traj, gp, (0, 3), 3, world_pos=wp)
    ok = lambda: _Batch(torch.zeros(N, 8), torch.zeros(N, 3), torch.zeros(3, 8))  # noqa: E731
    feed.fill(ok())
    for change in (dict(x=torch.zeros(N, 7)), dict(x=torch.zeros(N, 8, dtype=torch.float64)),
                   dict(y=torch.zeros(N, 2)), dict(edge_attr=None), dict(edge_attr=torch.zeros(3, 7)),
                   dict(edge_attr=torch.zeros(2, 8)), dict(edge_attr=torch.zeros(3, 8, dtype=torch.float64)),
                   dict(edge_attr=torch.zeros(8, 3).t())):
        b = ok()
        for key, v in change.items():
            setattr(b, key, v)
        with pytest.raises(ValueError):
            feed.fill(b)


def test_the_resident_rollout_refuses_a_world_feed():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout

    traj, gp = _small()
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6}
    world = ResidentTrajectories(traj, gp, (0, 3), 3, world_pos=wp)
    plain = ResidentTrajectories(traj, gp, (0, 3), 3)
    sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, EncodeProcessDecode(2, 15, 8, 3, 8), torch.device("cpu"))
    with pytest.raises(ValueError, match="world_pos"):
        Rollout(sim, 6, feed=world, graph=False)
    sim2 = Simulator(12, 4, 3, 0, 3, 0, 3, 3, EncodeProcessDecode(2, 12, 4, 3, 8), torch.device("cpu"))
    ro = Rollout(sim2, 3, feed=plain, graph=False)
    ro.feed = world  # a feed swapped in after construction is refused by the run itself
    with pytest.raises(ValueError, match="world_pos"):
        ro.rollout_resident(_Batch(torch.zeros(10, 5), torch.zeros(10, 3)))


def test_train_step_accepts_the_wider_batch():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.step import TrainStep

    traj, gp = _small()
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6}
    feed = ResidentTrajectories(traj, gp, (0, 3), 3, world_pos=wp)
    sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, EncodeProcessDecode(2, 15, 8, 3, 8), torch.device("cpu"))
    opt = torch.optim.AdamW(sim.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, 10)
    step = TrainStep(sim, opt, sched, _Batch(torch.zeros(10, 8), torch.zeros(10, 3)), graph=False, feed=feed)
    assert step.feed is feed
    feed.fill(step.batch)
    assert torch.equal(step.node_type, traj[0, :, 3])


def test_a_feed_without_world_pos_is_unchanged():
    """fill on the existing add_noise fixture: the same x as fill_torch with the normals fill drew, and that x is
    the reference's add_noise output when the fixture's normals are in their place; none of the new state."""
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch

    z = np.load(os.path.join(G, "feed_golden.npz"))
    x_in = torch.from_numpy(z["x_in"])
    N, F = x_in.shape
    nti = int(z["node_type_index"])
    ranges = [tuple(int(v) for v in r) for r in z["ranges"]]
    traj = torch.stack([x_in, x_in + 1.0])
    noise = {"noise_index_start": [s for s, _ in ranges], "noise_index_end": [e for _, e in ranges],
             "noise_scale": [float(s) for s in z["scales"]], "node_type_index": nti}
    feed = ResidentTrajectories(traj, [0, N], (0, 2), nti, noise=noise, frames=[0])
    assert not feed.world and feed.Fx == F and feed.obstacle_mean is None and feed.senders is None
    b = _Batch(torch.full((N, F + 1), SENTINEL), torch.zeros(N, 2))
    feed.fill(b)
    wx, wy = fill_torch(traj, [0, N], feed.frame, (0, 2), nti, feed.ranges, feed.scales, feed.z)
    assert torch.equal(b.x[:, :F], wx) and torch.equal(b.y, wy) and bool((b.x[:, F] == SENTINEL).all())
    wx, _ = fill_torch(traj, [0, N], feed.frame, (0, 2), nti, feed.ranges, feed.scales, torch.from_numpy(z["z"]))
    assert torch.equal(wx, torch.from_numpy(z["x_out"]))


def test_library_refuses_bad_arguments_without_a_device():
    """Both entry points check their arguments on the host before any device work: a nonzero status and a message,
    here with null data pointers (nothing is launched); no nodes / no edges is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    def world(T=3, N=10, F=6, B=2, ys=0, ye=3, ti=5, ranges=((0, 3), (6, 8)), n=None, ldz=8, ldx=9, ldy=3, mean=8):
        rg = nat.feed_ranges(ranges)
        if n is not None:
            rg.n = n
        rc = nat.lib().mgn_feed_batch_world(None, T, N, F, None, B, None, ys, ye, ti, rg, None, None, ldz, None, ldx,
                                            None, ldy, mean, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert world(N=0)[0] == 0 and world(B=0)[0] == 0
    for kw in (dict(T=1), dict(F=3), dict(F=0), dict(ranges=((0, 3), (7, 10))), dict(ranges=((-1, 2),)),
               dict(ranges=((2, 1),)), dict(ranges=((0, 3), (2, 5))), dict(ranges=((7, 9),)), dict(ranges=((8, 9),)),
               dict(ye=7), dict(ys=1, ye=4), dict(ye=2), dict(ti=6), dict(ti=2), dict(ti=-1), dict(n=5), dict(n=-1),
               dict(ldx=8), dict(ldy=2), dict(mean=None), dict(N=0, mean=None), dict()):  # the last: null pointers
        rc, msg = world(**kw)
        assert rc != 0 and "feed_batch_world" in msg, (kw, rc, msg)

    def edges(E=5, ldx=8, ld_ea=8, s=4, p=8):
        rc = nat.lib().mgn_feed_world_edge_features(p, p, E, p, ldx, p, ld_ea, s, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert edges(E=0)[0] == 0 and edges(E=0, p=None)[0] == 0
    for kw in (dict(ld_ea=7), dict(s=-1), dict(s=5), dict(ldx=2), dict(E=-1), dict(p=None)):
        rc, msg = edges(**kw)
        assert rc != 0 and "feed_world_edge_features" in msg, (kw, rc, msg)
