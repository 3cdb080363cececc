"""The resident rollout on Lagrangian data, on the CPU (no kernels): Rollout.rollout_resident(world_edges=...)
through its torch path (dataset.resident.rollout_begin_world_torch / world_edge_features_torch / rollout_end_torch,
graph=False) against the reference's own validation loop (tests/golden/world_rollout_golden.npz, written by
tests/golden/make_world_rollout_golden.py), against the per-frame host loop it replaces, the three edge modes, the
refusals, and the stored data staying clean. The forward is the CPU oracle's (the fixture's weights)."""
import pytest
import torch

import _plate as P
from _plate import EA_START, NORM_RTOL, SENTINEL


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def gold():
    return P.load_golden()


@pytest.fixture(scope="module")
def sim(gold):
    return P.OracleSim(gold["weights"])


def _gold_setup(gold, sim, mode, edges=True):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    traj, k, ei = gold["traj"], gold["k"], gold["edge_index"]
    N, E = traj.shape[1], ei.shape[1]
    feed = ResidentTrajectories(traj, [0, N], (0, 3), k, world_pos=P.world_pos(k, ei if edges else None))
    ea = torch.full((E, 8), SENTINEL)
    ea[:, :4] = gold["edge_attr_in"]
    batch = _Batch(x=torch.full((N, 8), SENTINEL), y=torch.zeros(N, 3), edge_index=ei, edge_attr=ea, pos=None)
    return Rollout(sim, k + 3, graph=False, feed=feed, world_edges=mode), batch


def _seen(ro, batch, steps):
    """The x and edge_attr the model saw at step steps - 1, and that run's predictions: a run of `steps` steps from
    frame 0 leaves them in the rollout's static batch."""
    pred = ro.rollout_resident(batch, 0, steps)
    return ro._res.x.clone(), ro._res.edge_attr.clone(), pred


def test_frame_mode_reproduces_the_reference_validation(gold, sim):
    """Per step: the x the reference's model saw and edge_attr[:, :7] bit for bit, the norm column at 5·2^-24
    relative, predictions within 1e-4·(1 + |ref|); val losses and the all-rollout RMSE within 1e-6 + 1e-4·ref (the
    bounds of test_rollout_gpu.py against the reference)."""
    ro, batch = _gold_setup(gold, sim, "frame")
    keep_traj, keep_ea = gold["traj"].clone(), batch.edge_attr.clone()
    S = gold["steps"]
    for s in range(S):
        x, ea, pred = _seen(ro, batch, s + 1)
        assert torch.equal(x, gold[f"x{s}"]), s
        assert torch.equal(ea[:, :7], gold[f"edge_attr{s}"][:, :7]), s
        torch.testing.assert_close(ea[:, 7], gold[f"edge_attr{s}"][:, 7], rtol=NORM_RTOL, atol=0)
        ref = gold[f"pred{s}"]
        assert bool(((pred[s] - ref).abs() <= 1e-4 * (1 + ref.abs())).all()), (s, float((pred[s] - ref).abs().max()))
    ro.clear()
    ro.rollout_resident(batch, 0, S)
    assert len(ro.losses) == S
    for a, b in zip([float(l) for l in ro.losses], gold["val_loss"].tolist()):
        assert abs(a - b) <= 1e-6 + 1e-4 * b, (a, b)
    ref_rmse = float(gold["val_all_rollout_rmse"][0])
    assert abs(ro.all_rollout_rmse() - ref_rmse) <= 1e-6 + 1e-4 * ref_rmse
    # from step 1 on the reference's edge features are NOT those of the positions its model saw
    from graphphysics.dataset.resident import world_edge_features_torch

    fed = world_edge_features_torch(gold["x1"], gold["edge_index"], gold["edge_attr1"].clone(), EA_START)
    assert not torch.equal(fed[:, 4:7], gold["edge_attr1"][:, 4:7])
    assert torch.equal(gold["traj"], keep_traj) and torch.equal(batch.edge_attr, keep_ea)


DYADIC = dict(sizes=[17, 23], F=5, T=5, k=3, starts=[0, 1], steps=3)


@pytest.fixture(scope="module")
def dyadic():
    traj, gp = P.case(DYADIC["sizes"], DYADIC["F"], DYADIC["T"], k=DYADIC["k"])
    ei = P.edges(traj.shape[1], gp)
    ea = torch.full((ei.shape[1], 9), SENTINEL)
    ea[:, :4] = torch.randint(-256, 257, (ei.shape[1], 4), generator=torch.Generator().manual_seed(4)).float() / 256.0
    return traj, gp, ei, ea[:, :8]  # a row stride of 9: a view, not a contiguous tensor


def _dyadic_rollout(dyadic, sim, mode, edges=True):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    traj, gp, ei, ea = dyadic
    k, N = DYADIC["k"], traj.shape[1]
    feed = ResidentTrajectories(traj, gp, (0, 3), k, world_pos=P.world_pos(k, ei if edges else None))
    batch = _Batch(x=torch.full((N, 9), SENTINEL), y=torch.zeros(N, 3), edge_index=ei, edge_attr=ea, pos=None)
    return Rollout(sim, k + 3, graph=False, feed=feed, world_edges=mode), batch


@pytest.mark.parametrize("mode", ["frame", "prediction", "off"])
def test_resident_rollout_equals_the_host_loop(dyadic, sim, mode):
    traj, gp, ei, ea = dyadic
    keep_traj, keep_ea = traj.clone(), ea.clone()
    starts, steps, k = DYADIC["starts"], DYADIC["steps"], DYADIC["k"]
    want, old, xs, eas = P.host_loop(sim, traj, gp, ei, ea.contiguous(), starts, steps, mode, k)
    ro, batch = _dyadic_rollout(dyadic, sim, mode)
    got = ro.rollout_resident(batch, starts, steps)
    assert got.shape == (steps, traj.shape[1], 3) and torch.equal(got, want)
    assert torch.equal(torch.stack(ro.losses), torch.stack(old.losses))
    assert abs(ro.all_rollout_rmse() - old.all_rollout_rmse()) <= 1e-6 * old.all_rollout_rmse()
    # the last step's batch as the model saw it; the column beyond F + 3 is the caller's
    assert torch.equal(ro._res.x[:, :8], xs[-1]) and bool((ro._res.x[:, 8] == SENTINEL).all())
    assert torch.equal(ro._res.edge_attr, eas[-1])
    if mode == "off":
        assert torch.equal(ro._res.edge_attr, keep_ea) and bool((ro._res.edge_attr[:, 4:] == SENTINEL).all())
    # the graphs started at different frames
    n0 = gp[1]
    assert torch.equal(ro._res.y[:n0], traj[3, :n0, 0:3]) and torch.equal(ro._res.y[n0:], traj[4, n0:, 0:3])
    # a second trajectory from other frames starts clean
    want2, _, _, _ = P.host_loop(sim, traj, gp, ei, ea.contiguous(), [2, 0], 2, mode, k)
    assert torch.equal(ro.rollout_resident(batch, [2, 0], 2), want2)
    assert torch.equal(traj, keep_traj) and torch.equal(ea, keep_ea)


def test_prediction_mode_follows_the_fed_back_positions(dyadic, sim):
    from graphphysics.dataset.resident import world_edge_features_torch

    traj, gp, ei, ea = dyadic
    k, starts = DYADIC["k"], DYADIC["starts"]
    frame, batch = _dyadic_rollout(dyadic, sim, "frame")
    pred, _ = _dyadic_rollout(dyadic, sim, "prediction")
    fx, fea, fp = _seen_from(frame, batch, starts, 1)
    px, pea, pp = _seen_from(pred, batch, starts, 1)
    assert torch.equal(fx, px) and torch.equal(fea, pea) and torch.equal(fp, pp)  # step 0: nothing fed back yet
    normal = torch.cat([traj[0, :gp[1], k], traj[1, gp[1]:, k]]) == 0
    touches = (normal[ei[0]] | normal[ei[1]]) & (ei[0] != ei[1])
    assert 0 < int(touches.sum()) < ei.shape[1] and 0 < int((~touches).sum())
    for steps in (2, 3):
        fx, fea, fp = _seen_from(frame, batch, starts, steps)
        px, pea, pp = _seen_from(pred, batch, starts, steps)
        want = world_edge_features_torch(px, ei, torch.full_like(pea, SENTINEL), EA_START)
        assert torch.equal(pea[:, 4:8], want[:, 4:8]) and torch.equal(pea[:, :4], ea[:, :4])
        # step 1 feeds back step 0's prediction, the same in both modes; its edge features differ, so from step 2
        # on the two rollouts drift apart. The fill does not.
        assert torch.equal(px[:, 0:3], fx[:, 0:3]) == (steps == 2)
        assert torch.equal(px[:, 3:], fx[:, 3:])  # displacement, node type, the other columns: the clean frame's
        differs = (pea[:, 4:8] != fea[:, 4:8]).any(dim=1)
        assert bool(differs[touches].all()) and not bool(differs[~touches].any())


def _seen_from(ro, batch, starts, steps):
    pred = ro.rollout_resident(batch, starts, steps)
    return ro._res.x[:, :8].clone(), ro._res.edge_attr.clone(), pred


def test_off_mode_works_without_an_edge_side(dyadic, sim):
    traj, gp, ei, ea = dyadic
    with_edges, batch = _dyadic_rollout(dyadic, sim, "off")
    without, _ = _dyadic_rollout(dyadic, sim, "off", edges=False)
    a = with_edges.rollout_resident(batch, 0, 2)
    b = without.rollout_resident(batch, 0, 2)
    assert torch.equal(a, b) and torch.equal(without._res.edge_attr, ea)
    assert without._res.world_clean is None and with_edges._res.obstacle_mean.shape == (2, 3)


def test_the_torch_rule_on_a_hand_built_case():
    """Previous data in batch columns (9, 12), x two columns wider than F + 3, and a graph whose step leaves the
    trajectory: nothing of it is written."""
    from graphphysics.dataset.resident import fill_world_torch, rollout_begin_world_torch

    traj, gp = P.case([4, 0, 5], 10, 4, k=5)
    N, F = traj.shape[1], 10
    keep = traj.clone()
    frame = torch.tensor([0, 0, 1], dtype=torch.int32)
    last, last_prev = torch.full((N, 3), 11.0), torch.full((N, 3), 13.0)

    def run(cursor, prev=(9, 12)):
        x, y = torch.full((N, F + 5), SENTINEL), torch.full((N, 3), SENTINEL)
        mean, wc = torch.full((3, 3), SENTINEL), torch.full((N, 3), SENTINEL)
        rollout_begin_world_torch(traj, gp, frame, torch.tensor([cursor], dtype=torch.int32), (0, 3), 5, (0, 3), prev,
                                  last, last_prev if prev else None, x, y, mean, wc)
        return x, y, mean, wc

    x, y, mean, wc = run(0)
    wx, wy, wmean = fill_world_torch(traj, gp, frame, (0, 3), 5, [], None, None)
    assert torch.equal(x[:, :F + 3], wx) and torch.equal(y, wy) and torch.equal(mean, wmean)
    assert torch.equal(wc, wx[:, 0:3]) and bool((x[:, F + 3:] == SENTINEL).all())
    assert torch.equal(mean[1], torch.zeros(3))  # the empty graph
    x, y, mean, wc = run(1)
    wx, wy, wmean = fill_world_torch(traj, gp, frame + 1, (0, 3), 5, [], None, None)
    assert torch.equal(x[:, 0:3], last) and torch.equal(x[:, 9:12], last_prev)
    assert torch.equal(x[:, 3:9], wx[:, 3:9]) and torch.equal(x[:, 12], wx[:, 12]) and torch.equal(y, wy)
    assert torch.equal(wc, wx[:, 0:3]) and torch.equal(mean, wmean)  # clean, whatever was fed back
    assert torch.equal(run(1, None)[0][:, 9:12], wx[:, 9:12])
    # cursor 2: graph 2 would read frames 3 and 4 of 4
    x, y, mean, wc = run(2)
    wx, wy, wmean = fill_world_torch(traj, gp, torch.tensor([2, 2, 2]), (0, 3), 5, [], None, None)
    assert torch.equal(x[:4, 3:9], wx[:4, 3:9]) and torch.equal(y[:4], wy[:4]) and torch.equal(mean[:2], wmean[:2])
    for t in (x[4:], y[4:], mean[2], wc[4:]):
        assert bool((t == SENTINEL).all())
    assert torch.equal(traj, keep)


def test_world_edges_refusals_and_acceptance(gold, sim):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    traj, k, ei = gold["traj"], gold["k"], gold["edge_index"]
    N, E = traj.shape[1], ei.shape[1]
    world = ResidentTrajectories(traj, [0, N], (0, 3), k, world_pos=P.world_pos(k, ei))
    bare = ResidentTrajectories(traj, [0, N], (0, 3), k, world_pos=P.world_pos(k))
    plain = ResidentTrajectories(traj, [0, N], (0, 3), k)
    kw = dict(graph=False)
    # the default still refuses a world feed, and now names the option
    with pytest.raises(ValueError, match="world_pos.*world_edges"):
        Rollout(sim, k + 3, feed=world, **kw)
    for mode in ("frame", "prediction", "off"):
        assert Rollout(sim, k + 3, feed=world, world_edges=mode, **kw).world_edges == mode
        with pytest.raises(ValueError, match="world_pos"):  # not a world feed
            Rollout(sim, k, feed=plain, world_edges=mode, **kw)
        with pytest.raises(ValueError, match="node_type_index"):  # the frame's index, not the batch's
            Rollout(sim, k, feed=world, world_edges=mode, **kw)
    Rollout(sim, k + 3, feed=bare, world_edges="off", **kw)
    for mode in ("frame", "prediction"):
        with pytest.raises(ValueError, match="edge_index"):
            Rollout(sim, k + 3, feed=bare, world_edges=mode, **kw)
    with pytest.raises(ValueError, match="world_edges"):
        Rollout(sim, k + 3, feed=world, world_edges="truth", **kw)
    # the batch
    ro = Rollout(sim, k + 3, feed=world, world_edges="frame", **kw)
    x, y, ea = torch.zeros(N, 8), torch.zeros(N, 3), torch.zeros(E, 8)
    with pytest.raises(ValueError, match="batch.x"):
        ro.rollout_resident(_Batch(x=x[:, :7], y=y, edge_index=ei, edge_attr=ea), 0, 2)
    with pytest.raises(ValueError, match="batch.edge_attr"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea[:, :7]), 0, 2)
    with pytest.raises(ValueError, match="batch.edge_attr"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=None), 0, 2)
    with pytest.raises(ValueError, match="batch.edge_attr"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea[:-1]), 0, 2)
    assert ro.losses == []
    # a mode swapped after construction is checked by the run itself
    ro.world_edges = None
    with pytest.raises(ValueError, match="world_pos"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea), 0, 2)
    # output columns against the batch width: (0, 3) fits, the previous-data columns may lie beyond the frame's F
    Rollout(sim, k + 3, feed=world, world_edges="off", use_previous_data=True, previous_data_start=3,
            previous_data_end=6, **kw)
    with pytest.raises(ValueError, match="inside"):
        Rollout(sim, k + 3, feed=world, world_edges="off", use_previous_data=True, previous_data_start=7,
                previous_data_end=10, **kw)
    with pytest.raises(ValueError, match="node_type_index"):
        Rollout(sim, k + 3, feed=world, world_edges="off", use_previous_data=True, previous_data_start=4,
                previous_data_end=7, **kw)


def test_library_refuses_bad_world_rollout_arguments_without_a_device():
    """mgn_rollout_begin_world checks its arguments on the host before any device work (null data pointers here:
    nothing is launched); no nodes is success, but not without obstacle_mean."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    def begin(T=3, N=10, F=6, B=2, ys=0, ye=3, ti=5, os_=0, oe=3, ps=3, pe=6, ldl=3, ldp=3, ldx=9, ldy=3, mean=8):
        rc = nat.lib().mgn_rollout_begin_world(None, T, N, F, None, B, None, None, ys, ye, ti, os_, oe, ps, pe, None,
                                               ldl, None, ldp, None, ldx, None, ldy, mean, None, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert begin(N=0)[0] == 0 and begin(B=0)[0] == 0
    for kw in (dict(T=1), dict(F=3), dict(F=0), dict(ye=7), dict(ys=1, ye=4), dict(ye=2), dict(ti=2), dict(ti=6),
               dict(ti=-1), dict(oe=10), dict(os_=2, oe=2), dict(os_=-1), dict(pe=10), dict(ps=5, pe=4),
               dict(ps=2, pe=5), dict(os_=6, oe=9, ps=0, pe=3), dict(ps=7, pe=9, ldp=2), dict(ps=8, pe=9), dict(ldx=8),
               dict(ldy=2), dict(ldl=2), dict(ldp=2), dict(mean=None), dict(N=0, mean=None), dict()):  # last: nulls
        rc, msg = begin(**kw)
        assert rc != 0 and "rollout_begin_world" in msg, (kw, rc, msg)
