"""Resident rollout on the CPU (no kernels): Rollout.rollout_resident against the existing Rollout.rollout on the
cylinder mesh, the two torch rules (dataset.resident.rollout_begin_torch / rollout_end_torch) on a hand-built
case, and the host-side argument checks."""
import numpy as np
import pytest
import torch

CPU = torch.device("cpu")


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _cylinder():
    """(static batch of frame 0, the 5 per-frame batches of the existing path, traj [6, 1923, 3], node offsets)."""
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    m = meshes.load_cylinder_mesh()
    frames = []
    for t in range(5):
        b = meshes.cylinder_batch(1, t=t, mesh=m)
        frames.append(Data(x=torch.from_numpy(b["x"]), y=torch.from_numpy(b["y"]),
                           edge_index=torch.from_numpy(b["edge_index"]), edge_attr=None))
    vel, nt = m["velocity"].astype(np.float32), m["node_type"].astype(np.float32)
    traj = torch.from_numpy(np.ascontiguousarray(
        np.concatenate([vel, np.broadcast_to(nt[None, :, None], (vel.shape[0], nt.shape[0], 1))], axis=2)))
    assert traj.shape == (6, 1923, 3)
    f0 = frames[0]
    batch = Data(x=f0.x.clone(), y=f0.y.clone(), edge_index=f0.edge_index, edge_attr=None)
    return batch, frames, traj, [0, 1923]


def _sim():
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator

    torch.manual_seed(0)
    sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, EncodeTransformDecode(2, 11, 2, 16, num_heads=4), CPU)
    sim.eval()
    return sim


def test_resident_rollout_equals_the_existing_rollout_on_cpu():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    batch, frames, traj, gp = _cylinder()
    nt = traj[0, :, 2]
    assert [int((nt == v).sum()) for v in (0, 4, 5, 6)] == [1689, 19, 19, 196]  # the mask is not trivial
    keep = traj.clone()
    sim = _sim()
    old = Rollout(sim, 2, graph=False)
    want = old.rollout(frames)
    new = Rollout(sim, 2, graph=False, feed=ResidentTrajectories(traj, gp, (0, 2), 2))
    got = new.rollout_resident(batch, 0, 5)
    assert got.shape == (5, 1923, 2) and torch.equal(got, want)
    assert len(new.losses) == 5 and all(l.dim() == 0 for l in new.losses)
    assert torch.equal(torch.stack(new.losses), torch.stack(old.losses))
    a, b = new.all_rollout_rmse(), old.all_rollout_rmse()
    assert abs(a - b) <= 1e-6 * b
    assert torch.equal(traj, keep)
    # a second trajectory (frames 1..3) starts clean: it equals the existing path on those frames
    old2 = Rollout(sim, 2, graph=False)
    want2 = old2.rollout(frames[1:4])
    assert torch.equal(new.rollout_resident(batch, 1, 3), want2)
    assert len(new.losses) == 8 and torch.equal(torch.stack(new.losses[5:]), torch.stack(old2.losses))
    # mixed use: resident steps and stepped frames in one epoch
    both = (5 * b * b + 3 * old2.all_rollout_rmse() ** 2) / 8
    assert abs(new.all_rollout_rmse() - both ** 0.5) <= 1e-6 * both ** 0.5
    new.rollout(frames[:2])
    full = Rollout(sim, 2, graph=False)
    full.rollout(frames)
    full.rollout(frames[1:4])
    full.rollout(frames[:2])
    assert abs(new.all_rollout_rmse() - full.all_rollout_rmse()) <= 1e-6 * full.all_rollout_rmse()
    new.clear()
    assert new.losses == [] and new._res_sq == [] and new._res_count == 0
    # default steps: to the end of the trajectory; predictions not kept
    assert new.rollout_resident(batch, 2, keep_predictions=False) is None
    assert len(new.losses) == 3


def test_torch_rules_on_a_hand_built_case():
    """B = 3 with an empty middle graph, per-graph start frames, F = 7, out (1, 3), prev (4, 6), type column 6,
    x two columns wider than F."""
    from graphphysics.dataset.resident import rollout_begin_torch, rollout_end_torch
    from graphphysics.utils.loss import masked_mse

    g = torch.Generator().manual_seed(3)
    T, F, gp, frames = 6, 7, [0, 4, 4, 9], [1, 0, 2]
    N = gp[-1]
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, 6] = torch.tensor([0.0, 4.0, 5.0, 6.0, 0.0, 0.0, 6.0, 5.0, 4.0])
    keep_traj = traj.clone()
    frame = torch.tensor(frames, dtype=torch.int32)
    cursor = torch.zeros(1, dtype=torch.int32)
    x, y = torch.full((N, F + 2), -7.0), torch.full((N, 2), -7.0)
    last, last_prev = torch.full((N, 2), 11.0), torch.full((N, 2), 13.0)
    preds, loss, sq = torch.full((3, N, 2), -7.0), torch.full((3,), -7.0), torch.full((3,), -7.0)
    args = (traj, gp, frame, cursor, (1, 3), (1, 3), (4, 6), last, last_prev, x, y)

    def clean(s, plus):
        return torch.cat([keep_traj[1 + s + plus, 0:4], keep_traj[2 + s + plus, 4:9]])

    # step 0: the clean frame, nothing fed back
    rollout_begin_torch(*args)
    assert torch.equal(x[:, :F], clean(0, 0)) and torch.equal(y, clean(0, 1)[:, 1:3])
    assert bool((x[:, F:] == -7.0).all())
    out = torch.randn(N, 2, generator=g)
    pred = rollout_end_torch(out, y, x, 6, [0, 5], 1, last, last_prev, preds, cursor, loss, sq)
    normal = (traj[0, :, 6] == 0) | (traj[0, :, 6] == 5)
    assert torch.equal(pred[normal], out[normal]) and torch.equal(pred[~normal], y[~normal])
    assert torch.equal(last, pred) and torch.equal(last_prev, pred - clean(0, 0)[:, 1:3])
    assert torch.equal(preds[0], pred) and bool((preds[1:] == -7.0).all())
    assert torch.equal(loss[0], masked_mse(y, pred, x[:, 6], [0, 5])) and bool((loss[1:] == -7.0).all())
    torch.testing.assert_close(sq[0], ((out - y)[normal] ** 2).sum(), rtol=1e-6, atol=0)
    assert int(cursor) == 1
    # step 1: last / last_prev into their columns only
    keep_last, keep_prev = last.clone(), last_prev.clone()
    rollout_begin_torch(*args)
    assert torch.equal(x[:, 1:3], keep_last) and torch.equal(x[:, 4:6], keep_prev)
    c1 = clean(1, 0)
    assert torch.equal(x[:, [0, 3, 6]], c1[:, [0, 3, 6]]) and torch.equal(y, clean(1, 1)[:, 1:3])
    assert bool((x[:, F:] == -7.0).all())
    pred1 = rollout_end_torch(out, y, x, 6, [0, 5], 1, last, last_prev, preds, cursor, loss, sq)
    assert torch.equal(last_prev, pred1 - keep_last) and torch.equal(preds[1], pred1) and int(cursor) == 2
    assert torch.equal(preds[0], pred) and bool((preds[2] == -7.0).all()) and float(loss[2]) == -7.0
    # without previous data the previous-data columns carry the frame
    rollout_begin_torch(traj, gp, frame, cursor, (1, 3), (1, 3), None, last, None, x, y)
    assert torch.equal(x[:, 4:6], clean(2, 0)[:, 4:6]) and torch.equal(x[:, 1:3], pred1)
    assert torch.equal(traj, keep_traj)


def test_bad_arguments_raise_value_error():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    batch, frames, traj, gp = _cylinder()
    sim = _sim()
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    ro = Rollout(sim, 2, graph=False, feed=feed)
    for start, steps in ((0, 6), (3, 3), (5, 1), (-1, 2), ([0, 0], 2), (0, 0)):
        with pytest.raises(ValueError):
            ro.rollout_resident(batch, start, steps)
    assert ro.losses == []
    with pytest.raises(ValueError, match="feed"):
        Rollout(sim, 2, graph=False).rollout_resident(batch, 0, 2)
    # widths: the feed's target columns, the previous-data columns
    with pytest.raises(ValueError, match="width"):
        Rollout(sim, 2, graph=False, feed=ResidentTrajectories(traj, gp, (0, 1), 2))
    wide = torch.zeros(3, 4, 6)
    wide_feed = ResidentTrajectories(wide, [0, 4], (0, 2), 5)
    prev = dict(use_previous_data=True, graph=False, feed=wide_feed)
    Rollout(sim, 5, previous_data_start=2, previous_data_end=4, **prev)  # the valid layout
    with pytest.raises(ValueError, match="width"):
        Rollout(sim, 5, previous_data_start=2, previous_data_end=5, **prev)
    with pytest.raises(ValueError, match="overlap"):
        Rollout(sim, 5, previous_data_start=1, previous_data_end=3, **prev)
    with pytest.raises(ValueError, match="inside"):
        Rollout(sim, 5, previous_data_start=5, previous_data_end=7, **prev)
    # the type column inside an overwritten range
    with pytest.raises(ValueError, match="node_type_index"):
        Rollout(sim, 1, graph=False, feed=feed)
    with pytest.raises(ValueError, match="node_type_index"):
        Rollout(sim, 3, previous_data_start=2, previous_data_end=4, **prev)
    # a feed on another device than the simulator, a batch on another device than the feed
    with pytest.raises(ValueError, match="feed lives on"):
        Rollout(sim, 2, graph=False, feed=ResidentTrajectories(traj.to("meta"), gp, (0, 2), 2))
    meta = _Batch(x=batch.x.to("meta"), y=batch.y.to("meta"), edge_index=batch.edge_index, edge_attr=None)
    with pytest.raises(ValueError, match="batch.x"):
        ro.rollout_resident(meta, 0, 2)
    for x, y in ((batch.x[:-1], batch.y[:-1]), (batch.x[:, :2], batch.y), (batch.x, batch.y[:, :1]),
                 (batch.x.double(), batch.y)):
        with pytest.raises(ValueError):
            ro.rollout_resident(_Batch(x=x, y=y, edge_index=batch.edge_index, edge_attr=None), 0, 2)


def test_rollout_without_feed_behaves_as_before():
    from graphphysics.training.rollout import Rollout

    _, frames, _, _ = _cylinder()
    sim = _sim()
    ro = Rollout(sim, 2, graph=False)
    assert ro.feed is None and ro.resident_records == 0
    got = ro.rollout(frames[:3])
    # the reference's loop, restated
    last, want = None, []
    for f in frames[:3]:
        x = f.x.clone()
        if last is not None:
            x[:, 0:2] = last
        with torch.no_grad():
            _, _, pred = sim(_Batch(x=x, y=f.y, edge_index=f.edge_index, edge_attr=None, pos=None))
        mask = ~((x[:, 2] == 0) | (x[:, 2] == 5))
        pred[mask] = f.y[mask]
        last = pred
        want.append(pred)
    assert torch.equal(got, torch.stack(want))
    p, t = torch.cat(want), torch.cat([f.y for f in frames[:3]])
    assert abs(ro.all_rollout_rmse() - float(torch.sqrt(((p - t) ** 2).mean()))) <= 1e-7
    assert len(ro.losses) == 3 and len(ro.outputs) == 3


def test_library_refuses_bad_rollout_arguments_without_a_device():
    """mgn_rollout_begin / mgn_rollout_end check their arguments on the host before any device work (null
    pointers here: nothing is launched); no nodes is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    def begin(T=3, N=10, F=6, B=2, ys=0, ye=2, os_=0, oe=2, ps=3, pe=5, ldl=2, ldp=2, ldx=8, ldy=2):
        rc = nat.lib().mgn_rollout_begin(None, T, N, F, None, B, None, None, ys, ye, os_, oe, ps, pe, None, ldl, None,
                                         ldp, None, ldx, None, ldy, None)
        return rc, nat.lib().mgn_last_error().decode()

    def end(N=10, ldx=8, ti=5, os_=0, d=2, cap=4, ws=None):
        ws = nat.lib().mgn_rollout_end_workspace_bytes(N) if ws is None else ws
        rc = nat.lib().mgn_rollout_end(None, None, None, N, ldx, ti, 33, os_, d, None, None, None, cap, None, None,
                                       None, None, ws, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert begin(N=0)[0] == 0 and begin(B=0)[0] == 0 and end(N=0)[0] == 0
    assert nat.lib().mgn_rollout_end_workspace_bytes(1923) >= 3 * 64 * 4
    for kw in (dict(T=1), dict(F=0), dict(ye=7), dict(ys=3, ye=2), dict(oe=7), dict(os_=2, oe=2), dict(os_=-1),
               dict(pe=7), dict(ps=4, pe=3), dict(ps=1, pe=3), dict(ldx=5), dict(ldy=1), dict(ldl=1), dict(ldp=1),
               dict()):  # the last: valid but null pointers
        rc, msg = begin(**kw)
        assert rc != 0 and "rollout_begin" in msg, (kw, rc, msg)
    for kw in (dict(d=0), dict(os_=7), dict(os_=-1), dict(ti=8), dict(ti=-1), dict(ti=1), dict(cap=0), dict(ws=8),
               dict()):
        rc, msg = end(**kw)
        assert rc != 0 and "rollout_end" in msg, (kw, rc, msg)
