"""The resident rollout on aneurysm data, on the CPU (no kernels): dataset.resident.rollout_begin_aneurysm_torch
against fill_aneurysm_torch, and Rollout.rollout_resident(acceleration=...) through its torch path (graph=False)
against the reference's own validation loop (tests/golden/aneurysm_rollout_golden.npz, written by
tests/golden/make_aneurysm_rollout_golden.py), against the per-frame host loop it replaces, the refusals, and the
stored data staying clean. The forward is the CPU oracle's (the fixture's weights).

Every column of x but the mean is compared bit for bit; the mean (column F + 6) is held to the bound derived in
test_feed_aneurysm_cpu.py, 2^-24·|m_ref| + 2^-24·Σ|v|. Predictions, losses and the RMSE carry test_rollout_gpu.py's
bounds against the reference."""
import pytest
import torch

import _aneurysm as A
from _aneurysm import RUNS, SENTINEL


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def gold():
    return A.load_golden()


@pytest.fixture(scope="module")
def sim(gold):
    return A.OracleSim(gold["weights"])


def _feed(traj, pos, gp=None):
    from graphphysics.dataset.resident import ResidentTrajectories

    gp = [0, traj.shape[1]] if gp is None else gp
    return ResidentTrajectories(traj, gp, (0, 3), traj.shape[2] + 9, aneurysm={"pos": pos})


# ------------------------------------------------------------------------------------------------ the torch rule
def test_the_torch_rule_on_a_hand_built_case():
    """Three graphs (one empty), F = 5, x two columns wider than F + 10: the fill of frame + s, the feedback in the
    output and the previous-data columns, and graphs whose step leaves [1, T − 2]: nothing of them is written."""
    from graphphysics.dataset.resident import fill_aneurysm_torch, rollout_begin_aneurysm_torch

    F, T = 5, 5
    traj, pos, gp = A.case([6, 0, 9], F, T)
    feed = _feed(traj, pos, gp)
    N, Fx = traj.shape[1], F + 10
    keep = (traj.clone(), pos.clone(), feed.node_type.clone(), feed.inflow_stats.clone())
    assert len({tuple(r) for r in feed.inflow_stats[:, 2].tolist()}) > 1  # the statistics follow the frame
    frame = torch.tensor([1, 1, 2], dtype=torch.int32)
    last, last_prev = torch.full((N, 3), 11.0), torch.full((N, 3), 13.0)

    def run(cursor, prev=(F, F + 3), fr=frame):
        x, y = torch.full((N, Fx + 2), SENTINEL), torch.full((N, 3), SENTINEL)
        rollout_begin_aneurysm_torch(traj, gp, fr, torch.tensor([cursor], dtype=torch.int32), (0, 3), feed.pos,
                                     feed.node_type, feed.inflow_stats, (0, 3), prev, last,
                                     last_prev if prev else None, x, y)
        return x, y

    def fill(fr):
        return fill_aneurysm_torch(traj, gp, torch.tensor(fr, dtype=torch.int32), feed.pos, feed.node_type,
                                   feed.inflow_stats, (0, 3), [], None, None)

    x, y = run(0)
    wx, wy = fill([1, 1, 2])
    assert torch.equal(x[:, :Fx], wx) and torch.equal(y, wy) and bool((x[:, Fx:] == SENTINEL).all())
    x, y = run(1)
    wx, wy = fill([2, 2, 3])
    assert torch.equal(x[:, 0:3], last) and torch.equal(x[:, F:F + 3], last_prev) and torch.equal(y, wy)
    assert torch.equal(x[:, 3:F], wx[:, 3:F]) and torch.equal(x[:, F + 3:Fx], wx[:, F + 3:Fx])
    assert bool((x[:, Fx:] == SENTINEL).all())
    x, _ = run(1, (F + 3, F + 6))  # other previous-data columns: the acceleration stays the clean frames'
    assert torch.equal(x[:, F + 3:F + 6], last_prev) and torch.equal(x[:, 3:F + 3], wx[:, 3:F + 3])
    x, _ = run(1, None)  # no previous data
    assert torch.equal(x[:, 0:3], last) and torch.equal(x[:, 3:Fx], wx[:, 3:Fx])
    # cursor 2: graph 2 would read frames 4 and 5 of 5
    x, y = run(2)
    wx, wy = fill([3, 3, 3])
    assert torch.equal(x[:6, 3:F], wx[:6, 3:F]) and torch.equal(x[:6, F + 3:Fx], wx[:6, F + 3:Fx])
    assert torch.equal(y[:6], wy[:6]) and torch.equal(x[:6, 0:3], last[:6])
    assert bool((x[6:] == SENTINEL).all()) and bool((y[6:] == SENTINEL).all())
    # frame 0 has no predecessor: graph 0 is left alone at cursor 0 and written at cursor 1
    x, y = run(0, fr=torch.tensor([0, 0, 1], dtype=torch.int32))
    assert bool((x[:6] == SENTINEL).all()) and bool((y[:6] == SENTINEL).all())
    assert torch.equal(x[6:, :Fx], fill([1, 1, 1])[0][6:])
    x, y = run(1, fr=torch.tensor([0, 0, 1], dtype=torch.int32))
    assert torch.equal(y, fill([1, 1, 2])[1]) and not bool((x[:, :Fx] == SENTINEL).any())
    for a, b in zip((traj, pos, feed.node_type, feed.inflow_stats), keep):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the fixture
def _gold_rollout(gold, sim, run, wide=0):
    from graphphysics.training.rollout import Rollout

    traj, ei = gold["traj"], gold["edge_index"]
    N, F = traj.shape[1], traj.shape[2]
    feed = _feed(traj, gold["pos"])
    batch = _Batch(x=torch.full((N, F + 10 + wide), SENTINEL), y=torch.zeros(N, 3), edge_index=ei,
                   edge_attr=gold["edge_attr"], pos=None)
    return Rollout(sim, F + 9, graph=False, feed=feed, acceleration=RUNS[run]), batch, feed


@pytest.mark.parametrize("run", list(RUNS))
def test_reproduces_the_reference_validation(gold, sim, run):
    ro, batch, feed = _gold_rollout(gold, sim, run)
    keep = (gold["traj"].clone(), gold["pos"].clone(), gold["edge_attr"].clone())

    def seen(s):  # a run of s + 1 steps from frame 1 leaves step s's batch in the rollout's static buffers
        pred = ro.rollout_resident(batch, 1, s + 1)
        return ro._res.x.clone(), pred

    ro2, _, _ = _gold_rollout(gold, sim, run)
    ro2.rollout_resident(batch, 1)  # steps: the default, T − 1 − start
    A.check_fixture(gold, run, seen, [float(l) for l in ro2.losses], ro2.all_rollout_rmse())
    assert torch.equal(gold["traj"], keep[0]) and torch.equal(feed.pos, keep[1])
    assert torch.equal(batch.edge_attr, keep[2]) and bool((batch.x == SENTINEL).all())


def test_the_two_runs_differ_from_step_1_on(gold):
    assert torch.equal(gold["prev::pred0"], gold["frame::pred0"])
    assert not torch.equal(gold["prev::pred1"], gold["frame::pred1"])


# ------------------------------------------------------------------------------------------------ the host loop
DYADIC = dict(sizes=[17, 23], F=4, T=6, starts=[1, 2], steps=3)


@pytest.fixture(scope="module")
def dyadic():
    traj, pos, gp = A.case(DYADIC["sizes"], DYADIC["F"], DYADIC["T"])
    ei = A.edges(traj.shape[1], gp)
    ea = torch.randint(-256, 257, (ei.shape[1], 4), generator=torch.Generator().manual_seed(4)).float() / 256.0
    return traj, pos, gp, ei, ea


@pytest.mark.parametrize("mode", ["frame", "prediction"])
def test_resident_rollout_equals_the_host_loop(dyadic, sim, mode):
    from graphphysics.training.rollout import Rollout

    traj, pos, gp, ei, ea = dyadic
    keep_traj = traj.clone()
    starts, steps, F, N = DYADIC["starts"], DYADIC["steps"], DYADIC["F"], traj.shape[1]
    want, old, xs = A.host_loop(sim, traj, pos, gp, ei, ea, starts, steps, mode)
    ro = Rollout(sim, F + 9, graph=False, feed=_feed(traj, pos, gp), acceleration=mode)
    assert ro.use_prev == (mode == "prediction") and ro._prev_cols == ((F, F + 3) if mode == "prediction" else None)
    batch = _Batch(x=torch.full((N, F + 11), SENTINEL), y=torch.zeros(N, 3), edge_index=ei, edge_attr=ea, pos=None)
    got = ro.rollout_resident(batch, starts, steps)
    assert got.shape == (steps, N, 3) and torch.equal(got, want)
    assert torch.equal(torch.stack(ro.losses), torch.stack(old.losses))
    assert abs(ro.all_rollout_rmse() - old.all_rollout_rmse()) <= 1e-6 * old.all_rollout_rmse()
    # the last step's batch as the model saw it; the column beyond F + 10 is the caller's
    assert torch.equal(ro._res.x[:, :F + 10], xs[-1]) and bool((ro._res.x[:, F + 10] == SENTINEL).all())
    n0 = gp[1]  # the graphs started at different frames
    assert torch.equal(ro._res.y[:n0], traj[4, :n0, 0:3]) and torch.equal(ro._res.y[n0:], traj[5, n0:, 0:3])
    # a second trajectory from other frames starts clean
    want2, _, _ = A.host_loop(sim, traj, pos, gp, ei, ea, [3, 1], 2, mode)
    assert torch.equal(ro.rollout_resident(batch, [3, 1], 2), want2)
    assert ro.resident_records == 0 and torch.equal(traj, keep_traj)


def test_switching_the_mode_is_applied_by_the_next_run(dyadic, sim):
    from graphphysics.training.rollout import Rollout

    traj, pos, gp, ei, ea = dyadic
    F, N = DYADIC["F"], traj.shape[1]
    batch = _Batch(x=torch.zeros(N, F + 10), y=torch.zeros(N, 3), edge_index=ei, edge_attr=ea, pos=None)
    ro = Rollout(sim, F + 9, graph=False, feed=_feed(traj, pos, gp), acceleration="frame")
    frame = ro.rollout_resident(batch, 1, 3)
    state = ro._res
    ro.acceleration = "prediction"
    pred = ro.rollout_resident(batch, 1, 3)
    assert ro._res is not state and ro._res.last_prev is not None  # the mode is part of the recorded key
    assert torch.equal(frame[0], pred[0]) and not torch.equal(frame[1], pred[1])
    ro.acceleration = "frame"
    assert torch.equal(ro.rollout_resident(batch, 1, 3), frame) and ro._prev_cols is None


# ------------------------------------------------------------------------------------------------ refusals
def test_acceleration_refusals_and_acceptance(gold, sim):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    traj, pos, ei = gold["traj"], gold["pos"], gold["edge_index"]
    N, F = traj.shape[1], traj.shape[2]
    feed = _feed(traj, pos)
    plain = ResidentTrajectories(traj, [0, N], (0, 3), 3)
    wide = torch.zeros(4, N, F + 10)
    wide[:, 0, F + 9] = 1.0  # an OBSTACLE node
    world = ResidentTrajectories(wide, [0, N], (0, 3), F + 9,
                                 world_pos={"world_pos_index_start": 0, "world_pos_index_end": 3,
                                            "node_type_index": F + 12})
    kw = dict(graph=False)
    # the default still refuses an aneurysm feed, and now names the option
    with pytest.raises(ValueError, match="aneurysm= is not supported yet without.*acceleration=.*later pull request"):
        Rollout(sim, F + 9, feed=feed, **kw)
    for mode in ("frame", "prediction"):
        assert Rollout(sim, F + 9, feed=feed, acceleration=mode, **kw).acceleration == mode
        with pytest.raises(ValueError, match="needs a feed built with aneurysm="):
            Rollout(sim, 3, feed=plain, acceleration=mode, **kw)
        with pytest.raises(ValueError, match="needs feed="):
            Rollout(sim, 3, acceleration=mode, **kw)
        with pytest.raises(ValueError, match=r"node_type_index 3 differs from F \+ 9 = 13"):
            Rollout(sim, 3, feed=feed, acceleration=mode, **kw)
        with pytest.raises(ValueError, match="world_edges"):
            Rollout(sim, F + 9, feed=feed, acceleration=mode, world_edges="off", **kw)
        with pytest.raises(ValueError, match="acceleration= and world_edges= do not go together"):
            Rollout(sim, F + 12, feed=world, acceleration=mode, world_edges="off", **kw)
    with pytest.raises(ValueError, match="acceleration must be None or one of"):
        Rollout(sim, F + 9, feed=feed, acceleration="truth", **kw)
    # "frame": previous data elsewhere is fine, on the acceleration columns it is not
    ro = Rollout(sim, F + 9, feed=feed, acceleration="frame", use_previous_data=True, previous_data_start=F + 3,
                 previous_data_end=F + 6, **kw)
    assert ro._prev_cols == (F + 3, F + 6)
    for ps in (F - 2, F, F + 2):
        if ps == F - 2:  # (2, 5) also overlaps the output columns; either refusal is a ValueError
            match = "intersect|overlap"
        else:
            match = "intersect"
        with pytest.raises(ValueError, match=match):
            Rollout(sim, F + 9, feed=feed, acceleration="frame", use_previous_data=True, previous_data_start=ps,
                    previous_data_end=ps + 3, **kw)
    # "prediction": the acceleration columns, given or not; nothing else
    for given in ({}, dict(use_previous_data=True, previous_data_start=F, previous_data_end=F + 3)):
        ro = Rollout(sim, F + 9, feed=feed, acceleration="prediction", **given, **kw)
        assert ro.use_prev and (ro.ps, ro.pe) == (F, F + 3) and ro._prev_cols == (F, F + 3)
    with pytest.raises(ValueError, match="previous-data columns"):
        Rollout(sim, F + 9, feed=feed, acceleration="prediction", use_previous_data=True, previous_data_start=F + 3,
                previous_data_end=F + 6, **kw)

    class _Other:  # a simulator that predicts other columns
        output_index_start, output_index_end, device, training = 1, 4, torch.device("cpu"), False

    with pytest.raises(ValueError, match=r"output columns \(0, 3\)"):
        Rollout(_Other(), F + 9, feed=feed, acceleration="prediction", **kw)
    # the column check runs against the batch width F + 10: previous-data columns may lie beyond the frame's F, not
    # beyond the row, and never on the node type
    with pytest.raises(ValueError, match="inside"):
        Rollout(sim, F + 9, feed=feed, acceleration="frame", use_previous_data=True, previous_data_start=F + 8,
                previous_data_end=F + 11, **kw)
    with pytest.raises(ValueError, match="node_type_index"):
        Rollout(sim, F + 9, feed=feed, acceleration="frame", use_previous_data=True, previous_data_start=F + 7,
                previous_data_end=F + 10, **kw)
    # the batch and the start frames
    ro = Rollout(sim, F + 9, feed=feed, acceleration="prediction", **kw)
    x, y, ea = torch.zeros(N, F + 10), torch.zeros(N, 3), gold["edge_attr"]
    with pytest.raises(ValueError, match="batch.x"):
        ro.rollout_resident(_Batch(x=x[:, :F + 9], y=y, edge_index=ei, edge_attr=ea), 1, 2)
    with pytest.raises(ValueError, match="batch.y"):
        ro.rollout_resident(_Batch(x=x, y=y[:, :2], edge_index=ei, edge_attr=ea), 1, 2)
    with pytest.raises(ValueError, match=r"frames must lie in \[1, 4\]"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea), 0, 2)
    with pytest.raises(ValueError, match="leave the trajectory"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea), 1, 5)
    with pytest.raises(ValueError, match="leave the trajectory"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea), 5)
    assert ro.losses == []
    # a mode removed after construction is refused by the run itself
    ro.acceleration = None
    with pytest.raises(ValueError, match="aneurysm= is not supported yet without"):
        ro.rollout_resident(_Batch(x=x, y=y, edge_index=ei, edge_attr=ea), 1, 2)


def test_library_refuses_bad_aneurysm_rollout_arguments_without_a_device():
    """mgn_rollout_begin_aneurysm checks its arguments on the host before any device work (null data pointers here:
    nothing is launched); no nodes is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    def begin(T=4, N=10, F=5, B=2, ys=0, ye=3, os_=0, oe=3, ps=5, pe=8, ldl=3, ldp=3, ldx=15, ldy=3):
        rc = nat.lib().mgn_rollout_begin_aneurysm(None, T, N, F, None, B, None, None, ys, ye, None, None, None, os_, oe,
                                                  ps, pe, None, ldl, None, ldp, None, ldx, None, ldy, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert begin(N=0)[0] == 0 and begin(B=0)[0] == 0
    for kw in (dict(T=2), dict(F=3), dict(F=0), dict(N=-1), dict(B=-1), dict(ye=6), dict(ys=3, ye=2), dict(ys=-1),
               dict(oe=16), dict(os_=2, oe=2), dict(os_=-1), dict(pe=16), dict(ps=6, pe=5), dict(ps=-1),
               dict(ps=2, pe=5), dict(os_=12, oe=15, ps=0, pe=0), dict(ps=12, pe=15), dict(ps=14, pe=15, ldp=1),
               dict(ldx=14), dict(ldy=2), dict(ldl=2), dict(ldp=2), dict()):  # the last: null pointers
        rc, msg = begin(**kw)
        assert rc != 0 and "rollout_begin_aneurysm" in msg, (kw, rc, msg)
