"""The resident rollout on aneurysm data on the GPU: libmgn's mgn_rollout_begin_aneurysm against the same rule
written as torch ops (dataset.resident.rollout_begin_aneurysm_torch, evaluated on the CPU) and against
mgn_feed_batch_aneurysm at the same frame, its argument checks, the reference's own validation loop
(tests/golden/aneurysm_rollout_golden.npz) through the kernels, and Rollout.rollout_resident(acceleration=...) —
captured and eager — against the per-frame host loop on a small tetrahedral grid.

The kernel copies fp32 values and subtracts once, so every comparison of it is bit equality (torch.equal). The
statistics table is mgn_feed_inflow_stats' (test_feed_aneurysm_gpu.py); the kernel-against-rule tests hand both
sides the same table."""
import numpy as np
import pytest
import torch

import _aneurysm as A
from _aneurysm import RUNS, SENTINEL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _buffers(N, ldx, dev):
    return dict(x=torch.full((N, ldx), SENTINEL, device=dev), y=torch.full((N, 3), SENTINEL, device=dev))


def _cpu_feed(traj, pos, gp):
    from graphphysics.dataset.resident import ResidentTrajectories

    return ResidentTrajectories(traj, gp, (0, 3), traj.shape[2] + 9, aneurysm={"pos": pos})


SIZES = {
    "one_node": [1],
    "uneven": [5, 64, 193],  # spans that cross a wave and a 256-thread block
    "empty_graph": [0, 65, 7],
    "long_graph": [1300, 3],  # more than one block of elements per graph; 325 inflow nodes
}


@pytest.mark.parametrize("F", [4, 5])  # rows of 14 and 15 floats
@pytest.mark.parametrize("name", list(SIZES))
def test_kernel_equals_the_torch_rule_bit_for_bit(name, F):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rollout_begin_aneurysm_torch

    sizes = SIZES[name]
    traj, pos, gp = A.case(sizes, F, T)
    feed = _cpu_feed(traj, pos, gp)
    node_type, stats = feed.node_type, feed.inflow_stats
    N, B, Fx = traj.shape[1], len(sizes), F + 10
    g = torch.Generator().manual_seed(3 + N)
    last, last_prev = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    dev = [t.to(DEV) for t in (traj, pos, node_type, stats)]
    keep = [t.clone() for t in dev]
    traj_d, pos_d, type_d, stats_d = dev
    gp_d = _i32(gp)
    for cursor in (0, 1, 2):
        # uneven frames, graph 0 at the last step that has a successor: frame + cursor == T - 2
        frames = [(T - 2 - cursor) - (b % (T - 2 - cursor)) for b in range(B)]
        assert frames[0] + cursor == T - 2 and min(frames) + cursor >= 1
        for prev, ldx in ((None, Fx), ((F, F + 3), Fx + 2), ((F + 3, F + 6), Fx), ((F, F + 3), Fx), (None, Fx + 2)):
            k, w = _buffers(N, ldx, DEV), _buffers(N, ldx, "cpu")
            cur = _i32([cursor])
            nat.rollout_begin_aneurysm(traj_d, gp_d, _i32(frames), cur, (0, 3), pos_d, type_d, stats_d, (0, 3), prev,
                                       last.to(DEV), last_prev.to(DEV) if prev else None, k["x"], k["y"])
            rollout_begin_aneurysm_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), cursor, (0, 3), pos,
                                         node_type, stats, (0, 3), prev, last, last_prev if prev else None, w["x"],
                                         w["y"])
            torch.cuda.synchronize()
            x, y = k["x"].cpu(), k["y"].cpu()
            assert torch.equal(x, w["x"]) and torch.equal(y, w["y"]), (cursor, prev, ldx)  # sentinel columns included
            assert int(cur) == cursor  # only read
            # the rule itself, independent of the torch form
            assert bool((x[:, Fx:] == SENTINEL).all())
            fed = set(range(0, 3)) | (set(range(*prev)) if prev else set()) if cursor else set()
            for b, f in enumerate(frames):
                rows, t = slice(gp[b], gp[b + 1]), f + cursor
                n = gp[b + 1] - gp[b]
                assert torch.equal(y[rows], traj[t + 1, rows, 0:3])
                assert torch.equal(x[rows, 3:F], traj[t, rows, 3:F])
                assert torch.equal(x[rows, 0:3], last[rows] if cursor else traj[t, rows, 0:3])
                if F not in fed:
                    assert torch.equal(x[rows, F:F + 3], traj[t, rows, 0:3] - traj[t - 1, rows, 0:3])
                if F + 3 not in fed:
                    assert torch.equal(x[rows, F + 3:F + 6], pos[rows])
                assert torch.equal(x[rows, F + 6:F + 9], stats[t, b].expand(n, 3))
                assert torch.equal(x[rows, F + 9], node_type[rows])
                if prev and cursor:
                    assert torch.equal(x[rows, prev[0]:prev[1]], last_prev[rows])
    for a, b in zip(dev, keep):
        assert torch.equal(a, b)


def test_the_same_bits_as_the_feed_at_that_frame():
    """Random normal frames (the differences round): x and y at cursor s are mgn_feed_batch_aneurysm's with frame + s
    and no noise, bit for bit, but for the fed-back columns; a second launch gives the same bits."""
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    sizes, F = [700, 1301, 40], 6
    gp = A.offsets(sizes)
    _, pos, _ = A.case(sizes, F, T)
    g = torch.Generator().manual_seed(5)
    traj = torch.randn(T, gp[-1], F, generator=g)
    traj[:, :, 3] = (torch.rand(gp[-1], generator=g) < 0.25).float()
    N, Fx = gp[-1], F + 10
    feed = ResidentTrajectories(traj.contiguous().to(DEV), gp, (0, 3), F + 9, aneurysm={"pos": pos.to(DEV)})
    last = torch.randn(N, 3, generator=g).to(DEV)
    last_prev = torch.randn(N, 3, generator=g).to(DEV)
    frames = [1, 2, 1]
    for cursor in (0, 1):
        k, w = _buffers(N, Fx, DEV), _buffers(N, Fx, DEV)

        def begin(buf):
            nat.rollout_begin_aneurysm(feed.traj, feed.graph_ptr, _i32(frames), _i32([cursor]), (0, 3), feed.pos,
                                       feed.node_type, feed.inflow_stats, (0, 3), (F, F + 3), last, last_prev,
                                       buf["x"], buf["y"])

        begin(k)
        nat.feed_batch_aneurysm(feed.traj, feed.graph_ptr, _i32([f + cursor for f in frames]), (0, 3), feed.pos,
                                feed.node_type, feed.inflow_stats, [], None, None, w["x"], w["y"])
        torch.cuda.synchronize()
        assert torch.equal(k["y"], w["y"])
        assert torch.equal(k["x"][:, 3:F], w["x"][:, 3:F]) and torch.equal(k["x"][:, F + 3:], w["x"][:, F + 3:])
        assert torch.equal(k["x"][:, 0:3], last if cursor else w["x"][:, 0:3])
        assert torch.equal(k["x"][:, F:F + 3], last_prev if cursor else w["x"][:, F:F + 3])
        again = _buffers(N, Fx, DEV)
        begin(again)
        assert torch.equal(again["x"], k["x"]) and torch.equal(again["y"], k["y"])


def test_a_step_outside_the_trajectory_writes_nothing_of_that_graph():
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rollout_begin_aneurysm_torch

    sizes, F = [6, 70, 9], 5
    traj, pos, gp = A.case(sizes, F, T)
    feed = _cpu_feed(traj, pos, gp)
    N, Fx = traj.shape[1], F + 10
    frames, cursor = [T - 2, 1, -1], 1  # graph 0: frame + cursor == T - 1 has no successor; graph 2: no predecessor
    last = torch.ones(N, 3)
    k, w = _buffers(N, Fx, DEV), _buffers(N, Fx, "cpu")
    nat.rollout_begin_aneurysm(traj.to(DEV), _i32(gp), _i32(frames), _i32([cursor]), (0, 3), pos.to(DEV),
                               feed.node_type.to(DEV), feed.inflow_stats.to(DEV), (0, 3), None, last.to(DEV), None,
                               k["x"], k["y"])
    rollout_begin_aneurysm_torch(traj, gp, torch.tensor(frames, dtype=torch.int32), cursor, (0, 3), pos, feed.node_type,
                                 feed.inflow_stats, (0, 3), None, last, None, w["x"], w["y"])
    torch.cuda.synchronize()
    for key in ("x", "y"):
        assert bool((k[key][:6] == SENTINEL).all()) and bool((k[key][76:] == SENTINEL).all()), key
        assert not bool((k[key][6:76] == SENTINEL).any()), key
        assert torch.equal(k[key].cpu(), w[key])
    assert torch.equal(k["y"][6:76].cpu(), traj[3, 6:76, 0:3])


def _raw(**over):
    """mgn_rollout_begin_aneurysm called directly with valid arguments for a [4, 10, 5] trajectory, except `over`.
    Returns (status, message, the buffers x / y pre-filled with a sentinel)."""
    from graphphysics import _native as nat

    Tr, N, F = 4, 10, 5
    a = {"traj": torch.zeros(Tr, N, F, device=DEV), "T": Tr, "N": N, "F": F, "graph_ptr": _i32([0, 4, 10]), "B": 2,
         "frame": _i32([1, 2]), "cursor": _i32([0]), "y_start": 0, "y_end": 3, "pos": torch.ones(N, 3, device=DEV),
         "node_type": torch.full((N,), 4.0, device=DEV), "stats": torch.full((Tr - 1, 2, 3), 2.0, device=DEV),
         "out_start": 0, "out_end": 3, "prev_start": 5, "prev_end": 8, "last": torch.full((N, 3), 7.0, device=DEV),
         "ld_last": 3, "last_prev": torch.full((N, 3), 9.0, device=DEV), "ld_prev": 3,
         "x": torch.full((N, 17), SENTINEL, device=DEV), "ldx": 17, "y": torch.full((N, 3), SENTINEL, device=DEV),
         "ldy": 3}
    a.update(over)
    p = nat.ptr
    rc = nat.lib().mgn_rollout_begin_aneurysm(p(a["traj"]), a["T"], a["N"], a["F"], p(a["graph_ptr"]), a["B"],
                                              p(a["frame"]), p(a["cursor"]), a["y_start"], a["y_end"], p(a["pos"]),
                                              p(a["node_type"]), p(a["stats"]), a["out_start"], a["out_end"],
                                              a["prev_start"], a["prev_end"], p(a["last"]), a["ld_last"],
                                              p(a["last_prev"]), a["ld_prev"], p(a["x"]), a["ldx"], p(a["y"]), a["ldy"],
                                              nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, nat.lib().mgn_last_error().decode(), [a[k] for k in ("x", "y")]


BAD = {
    # what mgn_rollout_begin refuses, ranges and ldx against F + 10 = 15
    "N<0": dict(N=-1), "B<0": dict(B=-1), "y_end>F": dict(y_end=6), "y_reversed": dict(y_start=4, y_end=3),
    "y_start<0": dict(y_start=-1), "out_empty": dict(out_start=1, out_end=1), "out_start<0": dict(out_start=-1),
    "out_end>F+10": dict(out_end=16), "prev_end>F+10": dict(prev_start=13, prev_end=16),
    "prev_reversed": dict(prev_start=6, prev_end=5), "prev_start<0": dict(prev_start=-1),
    "ranges_overlap": dict(prev_start=2, prev_end=5), "ldx<F+10": dict(ldx=14), "ldy<width": dict(ldy=2),
    "ld_last<width": dict(ld_last=2), "ld_prev<width": dict(ld_prev=2), "traj_null": dict(traj=None),
    "graph_ptr_null": dict(graph_ptr=None), "frame_null": dict(frame=None), "cursor_null": dict(cursor=None),
    "x_null": dict(x=None), "y_null": dict(y=None),
    # its own
    "T<3": dict(T=2), "F<4": dict(F=3), "out_holds_type": dict(out_start=12, out_end=15, prev_start=0, prev_end=0),
    "prev_holds_type": dict(prev_start=12, prev_end=15), "prev_is_type": dict(prev_start=14, prev_end=15, ld_prev=1),
    "pos_null": dict(pos=None), "node_type_null": dict(node_type=None), "stats_null": dict(stats=None),
    "last_null": dict(last=None), "last_prev_null": dict(last_prev=None),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(name):
    rc, msg, buffers = _raw(**BAD[name])
    assert rc != 0 and "rollout_begin_aneurysm" in msg, (rc, msg)
    for t in buffers:
        assert t is None or bool((t == SENTINEL).all())


def test_the_valid_raw_call_runs():
    rc, _, (x, y) = _raw()
    want = torch.tensor([0.0] * 8 + [1.0] * 3 + [2.0] * 3 + [4.0], device=DEV)
    assert rc == 0 and torch.equal(x[:, :15], want.expand(10, 15)) and bool((x[:, 15:] == SENTINEL).all())
    assert bool((y == 0).all())
    # from step 1 on the two ranges carry the state, whatever the frames hold
    rc, _, (x, y) = _raw(cursor=_i32([1]), frame=_i32([1, 1]))
    want = torch.tensor([7.0] * 3 + [0.0] * 2 + [9.0] * 3 + [1.0] * 3 + [2.0] * 3 + [4.0], device=DEV)
    assert rc == 0 and torch.equal(x[:, :15], want.expand(10, 15)) and bool((x[:, 15:] == SENTINEL).all())
    # no previous data; no nodes, no graphs
    rc, _, (x, _) = _raw(cursor=_i32([1]), frame=_i32([1, 1]), prev_start=0, prev_end=0, last_prev=None)
    assert rc == 0 and bool((x[:, 5:8] == 0).all()) and bool((x[:, 0:3] == 7).all())
    for over in (dict(N=0), dict(B=0), dict(N=0, traj=None, x=None)):
        rc, msg, buffers = _raw(**over)
        assert rc == 0, msg
        assert all(t is None or bool((t == SENTINEL).all()) for t in buffers)


# ----------------------------------------------------------------------------- Rollout.rollout_resident
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("run", list(RUNS))
def test_reference_fixture_through_the_kernels(run, graph):
    """tests/golden/aneurysm_rollout_golden.npz with test_rollout_aneurysm_cpu.py's bounds
    (_aneurysm.check_fixture): x bit for bit but the mean (the derived bound) and, from step 1 on, the fed-back columns of unmasked nodes; predictions within
    1e-4·(1 + |ref|); losses and the RMSE within 1e-6 + 1e-4·ref."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    gold = A.load_golden()
    sim = Simulator(22, 4, 3, 0, 13, 0, 3, 13, EncodeProcessDecode(2, 22, 4, 3, 16, compute_dtype=torch.float32), DEV)
    missing, unexpected = sim.load_state_dict(gold["weights"], strict=True)
    assert not missing and not unexpected
    sim.eval()
    traj, pos, ei = gold["traj"].to(DEV), gold["pos"].to(DEV), gold["edge_index"].to(DEV)
    N, F = traj.shape[1], traj.shape[2]
    batch = Data(x=torch.full((N, F + 10), SENTINEL, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei,
                 edge_attr=gold["edge_attr"].to(DEV))

    def make():
        feed = ResidentTrajectories(traj, [0, N], (0, 3), F + 9, aneurysm={"pos": pos})
        return Rollout(sim, F + 9, graph=graph, feed=feed, acceleration=RUNS[run])

    ro = make()

    def seen(s):  # a run of s + 1 steps from frame 1 leaves step s's batch in the static buffers
        pred = ro.rollout_resident(batch, 1, s + 1).cpu()
        return ro._res.x.cpu(), pred

    whole = make()
    whole.rollout_resident(batch, 1)
    A.check_fixture(gold, run, seen, [float(l) for l in whole.losses], whole.all_rollout_rmse())
    assert ro.resident_records == (1 if graph else 0)


T_GRID = 5


@pytest.fixture(scope="module")
def grid():
    """Two copies of meshes.tet_grid(11, 6, 5) (330 nodes each), as test_feed_aneurysm_gpu.py's grid: the plane
    y = 0 is the inflow (x < 0) and outflow (x >= 0) face, the plane z = 0 carries the wall flag. T = 5 frames
    [velocity, wall flag] of multiples of 2^-10; the second graph's velocities are 1.5 times the first's. Returns
    (traj [5, 660, 4] on the device, node offsets, pos [660, 3], edge_index [2, E])."""
    from graphphysics.utils import meshes

    p, cells = meshes.tet_grid(11, 6, 5, 0.25, origin=(-1.25, 0.0, 0.0))
    n = p.shape[0]
    ei1 = torch.as_tensor(np.asarray(meshes.tetra_to_edge_index(cells, n)), dtype=torch.int64)
    g = torch.Generator().manual_seed(3)
    v = torch.round(0.1 * torch.randn(T_GRID, n, 3, generator=g) * 1024.0) / 1024.0
    wall = torch.from_numpy((p[:, 2] == 0).astype(np.float32))[None, :, None].expand(T_GRID, n, 1)
    traj = torch.cat([torch.cat([v, wall], dim=2), torch.cat([1.5 * v, wall], dim=2)], dim=1).contiguous().to(DEV)
    pos = torch.from_numpy(np.concatenate([p, p], 0)).contiguous().to(DEV)
    ei = torch.cat([ei1, ei1 + n], dim=1).contiguous().to(DEV)
    assert n == 330 and int((pos[:, 1] == 0).sum()) == 2 * 55
    return traj, [0, n, 2 * n], pos, ei


def _grid_sim(grid, K=0):
    """An fp32 transformer model without edge_attr (MP 2, h 32, 4 heads; K > 0: a mixture head), its normalisers
    accumulated over two training-mode forwards on build_features rows."""
    from graphphysics.external.aneurysm import build_features
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.utils.data import Data

    traj, gp, pos, ei = grid
    torch.manual_seed(0)
    kw = dict(num_mixture_components=K, temperature=0.5) if K else {}
    m = EncodeTransformDecode(2, 13 + 9, 3, hidden_size=32, num_heads=4, compute_dtype=torch.float32, **kw)
    sim = Simulator(13 + 9, 0, 3, 0, 13, 0, 3, 13, m, DEV)
    with torch.no_grad():
        for t in (1, 3):
            items = [build_features(Data(x=traj[t, gp[b]:gp[b + 1]].clone(), y=traj[t + 1, gp[b]:gp[b + 1], 0:3].clone(),
                                         pos=pos[gp[b]:gp[b + 1]], previous_data=traj[t - 1, gp[b]:gp[b + 1], 0:3].clone()))
                     for b in range(2)]
            sim(Data(x=torch.cat([d.x for d in items]), y=torch.cat([d.y for d in items]), edge_index=ei,
                     edge_attr=None))
    sim.eval()
    return sim


def test_small_grid_captured_equals_eager_and_the_host_loop(grid):
    """In both modes the captured rollout equals the eager one and the per-frame host loop
    (external.aneurysm.build_features per graph, then Rollout.step) bit for bit, over two trajectories with different
    starts on one recorded graph; a repeated run reproduces itself; changing the mode re-records."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    traj, gp, pos, ei = grid
    keep_traj, keep_pos = traj.clone(), pos.clone()
    N = traj.shape[1]
    sim = _grid_sim(grid)

    def make(graph, mode):
        feed = ResidentTrajectories(traj, gp, (0, 3), 13, aneurysm={"pos": pos})
        return Rollout(sim, 13, graph=graph, feed=feed, acceleration=mode)

    batch = Data(x=torch.zeros(N, 14, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=None)
    runs = (([1, 2], 2), ([2, 1], 2))  # (start frame per graph, steps)
    cap, got = None, {}
    for mode in ("frame", "prediction"):
        eager, cap = make(False, mode), make(True, mode)
        for starts, steps in runs:
            want, old, xs = A.host_loop(sim, traj, pos, gp, ei, None, starts, steps, mode)
            a, b = eager.rollout_resident(batch, starts, steps), cap.rollout_resident(batch, starts, steps)
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b) and torch.equal(b, want), (mode, starts)
            assert torch.equal(torch.stack(cap.losses[-steps:]), torch.stack(eager.losses[-steps:]))
            assert torch.equal(torch.stack(cap.losses[-steps:]), torch.stack(old.losses))
            for ro in (eager, cap):  # the last step's batch as the model saw it
                assert torch.equal(ro._res.x, xs[-1])
            got[mode, tuple(starts)] = b
        assert cap.resident_records == 1 and eager.resident_records == 0
        assert abs(cap.all_rollout_rmse() - eager.all_rollout_rmse()) <= 1e-6 * eager.all_rollout_rmse()
        assert torch.equal(cap.rollout_resident(batch, *runs[0]), got[mode, (1, 2)])  # the same bits again
        assert cap.resident_records == 1
    # step 0 is the same in both modes; later steps are not
    assert torch.equal(got["frame", (1, 2)][0], got["prediction", (1, 2)][0])
    assert not torch.equal(got["frame", (1, 2)][1], got["prediction", (1, 2)][1])
    cap.acceleration = "frame"  # the mode is part of what was recorded
    assert torch.equal(cap.rollout_resident(batch, *runs[0]), got["frame", (1, 2)]) and cap.resident_records == 2
    assert torch.equal(traj, keep_traj) and torch.equal(pos, keep_pos)


def test_mixture_head_rolls_out_inside_the_captured_graph(grid):
    """K = 3, temperature 0.5, captured: finite predictions, nodes outside NORMAL / OUTFLOW carry the target exactly,
    one record."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    traj, gp, pos, ei = grid
    N = traj.shape[1]
    sim = _grid_sim(grid, K=3)
    feed = ResidentTrajectories(traj, gp, (0, 3), 13, aneurysm={"pos": pos})
    ro = Rollout(sim, 13, graph=True, feed=feed, acceleration="prediction")
    batch = Data(x=torch.zeros(N, 14, device=DEV), y=torch.zeros(N, 3, device=DEV), edge_index=ei, edge_attr=None)
    preds = ro.rollout_resident(batch, 1)
    torch.cuda.synchronize()
    assert preds.shape == (3, N, 3) and bool(torch.isfinite(preds).all())
    keep = ~((feed.node_type == 0) | (feed.node_type == 5))
    assert 0 < int(keep.sum()) < N
    for s in range(3):
        assert torch.equal(preds[s][keep], traj[2 + s, :, 0:3][keep])
        assert not torch.equal(preds[s][~keep], traj[2 + s, :, 0:3][~keep])
    assert ro.resident_records == 1 and all(bool(torch.isfinite(l)) for l in ro.losses)
