"""The resident rollout on Lagrangian data on the GPU: libmgn's mgn_rollout_begin_world against the same rule
written as torch ops (dataset.resident.rollout_begin_world_torch, evaluated on the CPU: IEEE division) and against
mgn_feed_batch_world at the same frame, its argument checks, the reference's own validation loop
(tests/golden/world_rollout_golden.npz) through the kernels, and Rollout.rollout_resident(world_edges=...) —
captured and eager — against the per-frame host loop on a small plate.

The kernel copies fp32 values, subtracts once and divides a sum by a count, so wherever the obstacle sum is exact
(values that are multiples of 2^-8: any summation order gives the same sum) every comparison is bit equality
(torch.equal); on random data it is compared with mgn_feed_batch_world, which runs the same reduction."""
import pytest
import torch

import _plate as P
from _plate import EA_START, NORM_RTOL, SENTINEL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _buffers(N, B, ldx, dev, wc=True):
    return dict(x=torch.full((N, ldx), SENTINEL, device=dev), y=torch.full((N, 3), SENTINEL, device=dev),
                mean=torch.full((B, 3), SENTINEL, device=dev),
                wc=torch.full((N, 3), SENTINEL, device=dev) if wc else None)


# (graph sizes, index of an all-OBSTACLE graph)
SIZES = {
    "one_node": ([1], None),
    "uneven": ([5, 64, 193], None),
    "empty_graph": ([0, 65, 7], None),  # the raw call only: the class refuses a graph without an OBSTACLE node
    "long_graph": ([1300, 3], None),  # the reduction walks a graph in several strides of its workgroup
    "all_obstacle": ([6, 70], 1),
}


@pytest.mark.parametrize("F", [4, 9])
@pytest.mark.parametrize("name", list(SIZES))
def test_kernel_equals_the_torch_rule_bit_for_bit(name, F):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rollout_begin_world_torch

    sizes, all_obstacle = SIZES[name]
    traj, gp = P.case(sizes, F, T, all_obstacle=all_obstacle)  # the node type in frame column F - 1
    N, B, Fx = traj.shape[1], len(sizes), F + 3
    g = torch.Generator().manual_seed(3 + N)
    last, last_prev = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    traj_d, gp_d, keep = traj.to(DEV), _i32(gp), traj.clone()
    prev_cols = (3, 6) if F == 4 else (6, 9)  # batch layout; the node type sits in batch column F + 2
    for cursor in (0, 1, 2):
        # uneven frames, graph 0 at the last step that has a successor: frame + cursor == T - 2
        frames = [(T - 2 - cursor) - (b % (T - 1 - cursor)) for b in range(B)]
        assert frames[0] + cursor == T - 2 and min(frames) >= 0
        for prev, ldx, wc in ((None, Fx, True), (prev_cols, Fx + 2, False), (prev_cols, Fx, True)):
            k, w = _buffers(N, B, ldx, DEV, wc), _buffers(N, B, ldx, "cpu", wc)
            cur = _i32([cursor])
            nat.rollout_begin_world(traj_d, gp_d, _i32(frames), cur, (0, 3), F - 1, (0, 3), prev, last.to(DEV),
                                    last_prev.to(DEV) if prev else None, k["x"], k["y"], k["mean"], k["wc"])
            rollout_begin_world_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), cursor, (0, 3), F - 1, (0, 3),
                                      prev, last, last_prev if prev else None, w["x"], w["y"], w["mean"], w["wc"])
            torch.cuda.synchronize()
            for key in ("x", "y", "mean", "wc"):  # the sentinel columns at or beyond F + 3 included
                if k[key] is not None:
                    assert torch.equal(k[key].cpu(), w[key]), (key, cursor, prev, ldx)
            assert int(cur) == cursor  # only read
            # the rule itself, independent of the torch form
            x, y = k["x"].cpu(), k["y"].cpu()
            assert bool((x[:, Fx:] == SENTINEL).all())
            for b, f in enumerate(frames):
                rows, t = slice(gp[b], gp[b + 1]), f + cursor
                assert torch.equal(y[rows], keep[t + 1, rows, 0:3])
                assert torch.equal(x[rows, Fx - 1], keep[t, rows, F - 1])
                assert torch.equal(x[rows, 0:3], last[rows] if cursor else keep[t, rows, 0:3])
                if wc:
                    assert torch.equal(k["wc"].cpu()[rows], keep[t, rows, 0:3])
                obstacle = keep[t, rows, F - 1] == 1
                d = (keep[t + 1, rows, 0:3] - keep[t, rows, 0:3])[obstacle]
                assert torch.equal(d.sum(0).double(), d.double().sum(0))  # the premise: the sums are exact
                if F == 9 or prev is None or not cursor:  # F == 4 with previous data: columns [3, 6) are fed back
                    assert torch.equal(x[rows, 3:6][obstacle], d)
                if b == all_obstacle:
                    assert bool(obstacle.all())
                if name == "empty_graph" and b == 0:
                    assert torch.equal(k["mean"].cpu()[b], torch.zeros(3))
                if prev and cursor:
                    assert torch.equal(x[rows, prev[0]:prev[1]], last_prev[rows])
    assert torch.equal(traj_d.cpu(), keep)


def test_the_same_bits_as_the_feed_at_that_frame():
    """Random normal frames: the obstacle sum is not exact, so its order shows. obstacle_mean, x and y at cursor s
    are mgn_feed_batch_world's with frame + s and no noise, bit for bit, but for the fed-back columns."""
    from graphphysics import _native as nat

    sizes, F = [700, 1301, 40], 9
    traj, gp = P.case(sizes, F, T, dyadic=False)
    N, B, Fx = traj.shape[1], len(sizes), F + 3
    traj_d, gp_d = traj.to(DEV), _i32(gp)
    last = torch.randn(N, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    frames = [0, 1, 0]
    for cursor in (0, 1):
        k, w = _buffers(N, B, Fx, DEV), _buffers(N, B, Fx, DEV)
        nat.rollout_begin_world(traj_d, gp_d, _i32(frames), _i32([cursor]), (0, 3), F - 1, (0, 3), None, last, None,
                                k["x"], k["y"], k["mean"], k["wc"])
        nat.feed_batch_world(traj_d, gp_d, _i32([f + cursor for f in frames]), (0, 3), F - 1, [], None, None, w["x"],
                             w["y"], w["mean"])
        torch.cuda.synchronize()
        assert torch.equal(k["mean"], w["mean"]) and torch.equal(k["y"], w["y"])
        assert torch.equal(k["x"][:, 3:], w["x"][:, 3:])
        assert torch.equal(k["x"][:, 0:3], last if cursor else w["x"][:, 0:3])
        assert torch.equal(k["wc"], w["x"][:, 0:3])
        again = _buffers(N, B, Fx, DEV)  # and the same bits on a second launch
        nat.rollout_begin_world(traj_d, gp_d, _i32(frames), _i32([cursor]), (0, 3), F - 1, (0, 3), None, last, None,
                                again["x"], again["y"], again["mean"], again["wc"])
        for key in ("x", "y", "mean", "wc"):
            assert torch.equal(again[key], k[key])


def test_a_step_outside_the_trajectory_writes_nothing_of_that_graph():
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rollout_begin_world_torch

    sizes, F = [6, 70], 9
    traj, gp = P.case(sizes, F, T)
    N, Fx = traj.shape[1], F + 3
    frames, cursor = [T - 2, 0], 1  # graph 0: frame + cursor == T - 1 has no successor
    last = torch.ones(N, 3)
    k, w = _buffers(N, 2, Fx, DEV), _buffers(N, 2, Fx, "cpu")
    nat.rollout_begin_world(traj.to(DEV), _i32(gp), _i32(frames), _i32([cursor]), (0, 3), F - 1, (0, 3), None,
                            last.to(DEV), None, k["x"], k["y"], k["mean"], k["wc"])
    rollout_begin_world_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), cursor, (0, 3), F - 1, (0, 3), None,
                              last, None, w["x"], w["y"], w["mean"], w["wc"])
    torch.cuda.synchronize()
    for key in ("x", "y", "wc"):
        assert bool((k[key][:6] == SENTINEL).all()), key
        assert not bool((k[key][6:] == SENTINEL).any()), key
        assert torch.equal(k[key].cpu(), w[key])
    assert bool((k["mean"][0] == SENTINEL).all()) and torch.equal(k["mean"].cpu(), w["mean"])
    assert torch.equal(k["y"][6:].cpu(), traj[2, 6:, 0:3])


def _raw(**over):
    """mgn_rollout_begin_world called directly with valid arguments for a [3, 10, 6] trajectory, except `over`.
    Returns (status, message, the buffers x / y / mean / wc pre-filled with a sentinel)."""
    from graphphysics import _native as nat

    Tr, N, F = 3, 10, 6
    traj = torch.zeros(Tr, N, F, device=DEV)
    traj[:, 0, 5] = traj[:, 4, 5] = 1.0
    a = {"traj": traj, "T": Tr, "N": N, "F": F, "graph_ptr": _i32([0, 4, 10]), "B": 2, "frame": _i32([0, 1]),
         "cursor": _i32([0]), "y_start": 0, "y_end": 3, "type_index": 5, "out_start": 0, "out_end": 3,
         "prev_start": 3, "prev_end": 6, "last": torch.ones(N, 3, device=DEV), "ld_last": 3,
         "last_prev": torch.ones(N, 3, device=DEV), "ld_prev": 3, "x": torch.full((N, 11), SENTINEL, device=DEV),
         "ldx": 11, "y": torch.full((N, 3), SENTINEL, device=DEV), "ldy": 3,
         "mean": torch.full((2, 3), SENTINEL, device=DEV), "wc": torch.full((N, 3), SENTINEL, device=DEV)}
    a.update(over)
    p = nat.ptr
    rc = nat.lib().mgn_rollout_begin_world(p(a["traj"]), a["T"], a["N"], a["F"], p(a["graph_ptr"]), a["B"], p(a["frame"]),
                                           p(a["cursor"]), a["y_start"], a["y_end"], a["type_index"], a["out_start"],
                                           a["out_end"], a["prev_start"], a["prev_end"], p(a["last"]), a["ld_last"],
                                           p(a["last_prev"]), a["ld_prev"], p(a["x"]), a["ldx"], p(a["y"]), a["ldy"],
                                           p(a["mean"]), p(a["wc"]), nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), [a[k] for k in ("x", "y", "mean", "wc")]


BAD = {
    # what mgn_rollout_begin refuses, ranges and ldx against F + 3 = 9
    "T<2": dict(T=1), "N<0": dict(N=-1), "B<0": dict(B=-1), "y_end>F": dict(y_end=7),
    "y_reversed": dict(y_start=4, y_end=3), "out_empty": dict(out_start=1, out_end=1), "out_start<0": dict(out_start=-1),
    "out_end>F+3": dict(out_end=10), "prev_end>F+3": dict(prev_start=9, prev_end=10),
    "prev_reversed": dict(prev_start=5, prev_end=4), "prev_start<0": dict(prev_start=-1),
    "ranges_overlap": dict(prev_start=2, prev_end=5), "ldx<F+3": dict(ldx=8), "ldy<width": dict(ldy=2),
    "ld_last<width": dict(ld_last=2), "ld_prev<width": dict(ld_prev=2), "traj_null": dict(traj=None),
    "cursor_null": dict(cursor=None), "x_null": dict(x=None),
    # its own
    "F<4": dict(F=3), "type_index<3": dict(type_index=2), "type_index=F": dict(type_index=6),
    "y_start!=0": dict(y_start=1, y_end=4), "y_end<3": dict(y_end=2),
    "out_holds_type": dict(out_start=6, out_end=9, prev_start=0, prev_end=0),
    "prev_holds_type": dict(prev_start=7, prev_end=9, ld_prev=2), "prev_is_type": dict(prev_start=8, prev_end=9),
    "mean_null": dict(mean=None), "mean_null_no_nodes": dict(mean=None, N=0), "last_null": dict(last=None),
    "last_prev_null": dict(last_prev=None),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(name):
    rc, msg, buffers = _raw(**BAD[name])
    assert rc != 0 and "rollout_begin_world" in msg, (rc, msg)
    for t in buffers:
        assert t is None or bool((t == SENTINEL).all())


def test_the_valid_raw_call_runs():
    rc, _, (x, y, mean, wc) = _raw()
    assert rc == 0 and bool((x[:, 9:] == SENTINEL).all()) and bool((mean == 0).all())
    assert bool((x[:, 8] == torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 0, 0], device=DEV)).all())
    assert bool((x[:, :8] == 0).all()) and bool((y == 0).all()) and bool((wc == 0).all())
    # from step 1 on the two ranges carry the state, whatever the frames hold
    rc, _, (x, y, mean, wc) = _raw(cursor=_i32([1]), frame=_i32([0, 0]))
    assert rc == 0 and bool((x[:, :6] == 1).all()) and bool((x[:, 6:8] == 0).all()) and bool((wc == 0).all())
    # no previous data, no clean positions, no nodes
    rc, _, (x, _, _, _) = _raw(prev_start=0, prev_end=0, last_prev=None, wc=None)
    assert rc == 0 and bool((x[:, :8] == 0).all())
    rc, _, buffers = _raw(N=0)
    assert rc == 0 and all(bool((t == SENTINEL).all()) for t in buffers)


# ----------------------------------------------------------------------------- Rollout.rollout_resident
@pytest.mark.parametrize("graph", [False, True])
def test_reference_fixture_through_the_kernels(graph):
    """tests/golden/world_rollout_golden.npz, "frame" mode: per step the x the reference's model saw and
    edge_attr[:, :7] bit for bit, the norm column at 5·2^-24 relative, predictions within 1e-4·(1 + |ref|); val
    losses and the all-rollout RMSE within 1e-6 + 1e-4·ref (test_rollout_gpu.py's bounds against the reference)."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    gold = P.load_golden()
    k, S = gold["k"], gold["steps"]
    sim = Simulator(17, 8, 3, 0, 8, 0, 3, 6, EncodeProcessDecode(2, 17, 8, 3, 16, compute_dtype=torch.float32), DEV)
    missing, unexpected = sim.load_state_dict(gold["weights"], strict=True)
    assert not missing and not unexpected
    sim.eval()
    traj, ei = gold["traj"].to(DEV), gold["edge_index"].to(DEV)
    N, E = traj.shape[1], ei.shape[1]
    feed = ResidentTrajectories(traj, [0, N], (0, 3), k, world_pos=P.world_pos(k, ei))
    ea = torch.full((E, 8), SENTINEL, device=DEV)
    ea[:, :4] = gold["edge_attr_in"].to(DEV)
    batch = Data(x=torch.full((N, 8), SENTINEL, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei,
                 edge_attr=ea)
    ro = Rollout(sim, k + 3, graph=graph, feed=feed, world_edges="frame")
    for s in range(S):  # a run of s + 1 steps leaves step s's batch in the static buffers
        pred = ro.rollout_resident(batch, 0, s + 1).cpu()
        x, sea = ro._res.x.cpu(), ro._res.edge_attr.cpu()
        assert torch.equal(x, gold[f"x{s}"]), s
        assert torch.equal(sea[:, :7], gold[f"edge_attr{s}"][:, :7]), s
        torch.testing.assert_close(sea[:, 7], gold[f"edge_attr{s}"][:, 7], rtol=NORM_RTOL, atol=0)
        ref = gold[f"pred{s}"]
        assert bool(((pred[s] - ref).abs() <= 1e-4 * (1 + ref.abs())).all()), (s, float((pred[s] - ref).abs().max()))
    assert ro.resident_records == (1 if graph else 0)
    ro.clear()
    ro.rollout_resident(batch, 0, S)
    for a, b in zip([float(l) for l in ro.losses], gold["val_loss"].tolist()):
        assert abs(a - b) <= 1e-6 + 1e-4 * b, (a, b)
    ref_rmse = float(gold["val_all_rollout_rmse"][0])
    assert abs(ro.all_rollout_rmse() - ref_rmse) <= 1e-6 + 1e-4 * ref_rmse


def test_small_plate_captured_equals_eager_and_the_host_loop():
    """plate_sample(nx=6, ny=4, nz=2) twice, frames rounded to 2^-12, T = 4, fp32 MP 2 h 32: in both edge modes the
    captured rollout equals the eager one and the per-frame host loop (batches by the torch rules on the CPU, then
    Rollout.step) bit for bit, over two trajectories with different starts on one recorded graph; a repeated run
    reproduces itself; changing the mode re-records."""
    from graphphysics.dataset.resident import ResidentTrajectories, fill_world_torch, world_edge_features_torch
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    traj, gp, ei, clean_ea = P.small_plate(DEV, T)
    keep_traj, keep_ea = traj.clone(), clean_ea.clone()
    traj_c, ei_c, ea_c = traj.cpu(), ei.cpu(), clean_ea.cpu()
    N = traj.shape[1]
    torch.manual_seed(0)
    sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, EncodeProcessDecode(2, 15, 8, 3, 32, compute_dtype=torch.float32), DEV)
    with torch.no_grad():  # the normalisers' statistics, from two training-mode forwards
        for fr in ([0, 1], [2, 0]):
            x, y, _ = fill_world_torch(traj_c, gp, torch.tensor(fr, dtype=torch.int32), (0, 3), 3, [], None, None)
            e = world_edge_features_torch(x, ei_c, ea_c.clone(), EA_START)
            sim(Data(x=x.to(DEV), y=y.to(DEV), edge_index=ei, edge_attr=e.to(DEV)))
    sim.eval()

    def make(graph, mode):
        feed = ResidentTrajectories(traj, gp, (0, 3), 3, world_pos=P.world_pos(3, ei))
        return Rollout(sim, 6, graph=graph, feed=feed, world_edges=mode)

    batch = Data(x=torch.zeros(N, 7, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=clean_ea)
    runs = (([0, 1], 2), ([1, 0], 2))  # (start frame per graph, steps)
    cap, got = None, {}
    for mode in ("frame", "prediction"):
        eager, cap = make(False, mode), make(True, mode)
        for starts, steps in runs:
            want, old, xs, eas = P.host_loop(sim, traj_c, gp, ei_c, ea_c, starts, steps, mode, 3, DEV)
            a, b = eager.rollout_resident(batch, starts, steps), cap.rollout_resident(batch, starts, steps)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b) and torch.equal(b, want), (mode, starts)
            assert torch.equal(torch.stack(cap.losses[-steps:]), torch.stack(eager.losses[-steps:]))
            assert torch.equal(torch.stack(cap.losses[-steps:]), torch.stack(old.losses))
            for ro in (eager, cap):  # the last step's batch as the model saw it
                assert torch.equal(ro._res.x.cpu(), xs[-1]) and torch.equal(ro._res.edge_attr.cpu(), eas[-1])
            got[mode, tuple(starts)] = b
        assert cap.resident_records == 1 and eager.resident_records == 0
        assert abs(cap.all_rollout_rmse() - eager.all_rollout_rmse()) <= 1e-6 * eager.all_rollout_rmse()
        assert torch.equal(cap.rollout_resident(batch, *runs[0]), got[mode, (0, 1)])  # the same bits again
        assert cap.resident_records == 1
    # step 0 is the same in both modes; later steps are not
    assert torch.equal(got["frame", (0, 1)][0], got["prediction", (0, 1)][0])
    assert not torch.equal(got["frame", (0, 1)][1], got["prediction", (0, 1)][1])
    cap.world_edges = "frame"  # the mode is part of what was recorded
    assert torch.equal(cap.rollout_resident(batch, *runs[0]), got["frame", (0, 1)]) and cap.resident_records == 2
    assert torch.equal(traj, keep_traj) and torch.equal(clean_ea, keep_ea)
