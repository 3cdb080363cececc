"""Resident rollout on the GPU: libmgn's mgn_rollout_begin / mgn_rollout_end against the same rules written as
torch ops (dataset.resident.rollout_begin_torch / rollout_end_torch), and Rollout.rollout_resident — captured and
eager — against the existing Rollout.rollout and the reference's own validation loop
(tests/golden/rollout_golden.npz).

The kernels copy and select fp32 values, subtract once, and sum the loss in mgn_masked_mse's order over its row
term, so x, y, the state, the kept predictions and the loss are compared for bit equality; only sq (a sum
masked_mse does not form) has a tolerance: 1e-6 relative to the fp64 sum."""
import functools
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


# ----------------------------------------------------------------------------- the kernels
# F = 7: out columns (1, 3), previous data (4, 6), node type in column 6; x two columns wider than F
F, LDX, T, CAP = 7, 9, 6, 4
SIZES = {"one_node": [1], "block_and_wave_edges": [257, 0, 70], "strided_rows": [16000, 411]}


@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("name", list(SIZES))
def test_kernels_equal_the_torch_rules_bit_for_bit(name, prev):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rollout_begin_torch, rollout_end_torch
    from graphphysics.utils.loss import masked_mse

    sizes = SIZES[name]
    N, B = sum(sizes), len(sizes)
    assert name != "strided_rows" or N > 64 * 256  # a thread of the partial sums owns more than one row
    g = torch.Generator().manual_seed(7 + N)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, 6] = torch.tensor([0.0, 0.0, 4.0, 5.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    traj = traj.to(DEV)
    keep_traj = traj.clone()
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    frames = [1, 0, 2][:B]
    gp_d = torch.tensor(gp, dtype=torch.int32, device=DEV)
    fr_d = torch.tensor(frames, dtype=torch.int32, device=DEV)
    pcols = (4, 6) if prev else None

    def state():
        return dict(x=torch.full((N, LDX), SENTINEL, device=DEV), y=torch.full((N, 2), SENTINEL, device=DEV),
                    last=torch.full((N, 2), 11.0, device=DEV),
                    last_prev=torch.full((N, 2), 13.0, device=DEV) if prev else None,
                    preds=torch.full((CAP, N, 2), SENTINEL, device=DEV), loss=torch.full((CAP,), SENTINEL, device=DEV),
                    sq=torch.full((CAP,), SENTINEL, device=DEV), cursor=torch.zeros(1, dtype=torch.int32, device=DEV))

    k, w = state(), state()  # the kernels' state, the torch rules' state
    ws = nat.rollout_end_workspace(N, DEV)
    for s in range(3):
        out = torch.randn(N, 2, generator=g).to(DEV)
        nat.rollout_begin(traj, gp_d, fr_d, k["cursor"], (1, 3), (1, 3), pcols, k["last"], k["last_prev"], k["x"], k["y"])
        rollout_begin_torch(traj, gp, fr_d, w["cursor"], (1, 3), (1, 3), pcols, w["last"], w["last_prev"], w["x"], w["y"])
        assert torch.equal(k["x"], w["x"]) and torch.equal(k["y"], w["y"]), s
        assert bool((k["x"][:, F:] == SENTINEL).all())
        if s > 0:  # the rule itself: the previous prediction sits in the output columns
            assert torch.equal(k["x"][:, 1:3], k["last"])
        assert int(k["cursor"]) == s  # begin does not advance it
        nat.rollout_end(out, k["y"], k["x"], 6, [0, 5], 1, k["last"], k["last_prev"], k["preds"], k["cursor"], k["loss"],
                        k["sq"], ws)
        pred = rollout_end_torch(out, w["y"], w["x"], 6, [0, 5], 1, w["last"], w["last_prev"], w["preds"], w["cursor"],
                                 w["loss"], w["sq"])
        torch.cuda.synchronize()
        assert torch.equal(k["last"], w["last"]) and torch.equal(k["last"], pred)
        if prev:
            assert torch.equal(k["last_prev"], w["last_prev"])
        assert torch.equal(k["preds"][s], pred)
        assert bool((k["preds"][s + 1:] == SENTINEL).all()) and bool((k["loss"][s + 1:] == SENTINEL).all())
        assert bool((k["sq"][s + 1:] == SENTINEL).all())
        assert torch.equal(k["preds"][:s], w["preds"][:s]) and torch.equal(k["loss"][:s], w["loss"][:s])
        want = masked_mse(k["y"], pred, k["x"][:, 6], [0, 5])
        assert torch.equal(k["loss"][s], want) and torch.equal(w["loss"][s], want), (float(k["loss"][s]), float(want))
        sq64 = float(((pred.double() - k["y"].double()) ** 2).sum())
        assert abs(float(k["sq"][s]) - sq64) <= 1e-6 * sq64, (float(k["sq"][s]), sq64)
        assert int(k["cursor"]) == s + 1 and int(w["cursor"]) == s + 1
    assert torch.equal(traj, keep_traj)


def test_end_without_kept_predictions_and_no_nodes():
    from graphphysics import _native as nat

    N = 70
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, LDX, generator=g)
    x[:, 6] = torch.tensor([0.0, 4.0, 5.0, 6.0, 0.0])[torch.randint(0, 5, (N,), generator=g)]
    x, y, out = x.to(DEV), torch.randn(N, 2, generator=g).to(DEV), torch.randn(N, 2, generator=g).to(DEV)
    last, cursor = torch.zeros(N, 2, device=DEV), torch.full((1,), 2, dtype=torch.int32, device=DEV)
    loss, sq = torch.full((CAP,), SENTINEL, device=DEV), torch.full((CAP,), SENTINEL, device=DEV)
    nat.rollout_end(out, y, x, 6, [0, 5], 1, last, None, None, cursor, loss, sq)
    torch.cuda.synchronize()
    normal = (x[:, 6] == 0) | (x[:, 6] == 5)
    assert torch.equal(last, torch.where(normal[:, None], out, y)) and int(cursor) == 3
    assert loss.tolist()[:2] == [SENTINEL, SENTINEL] and float(loss[2]) > 0 and float(loss[3]) == SENTINEL
    e = torch.zeros(0, 2, device=DEV)
    nat.rollout_end(e, e, torch.zeros(0, LDX, device=DEV), 6, [0, 5], 1, e, None, None, cursor, loss, sq)
    nat.rollout_begin(torch.zeros(3, 0, F, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                      torch.zeros(1, dtype=torch.int32, device=DEV), cursor, (1, 3), (1, 3), None, e,
                      None, torch.zeros(0, LDX, device=DEV), e)
    torch.cuda.synchronize()
    assert int(cursor) == 3


# ----------------------------------------------------------------------------- models
def _mesh_traj(layout):
    """The cylinder mesh's 6 stored frames as traj [6, 1923, F] on the device, the static graph tensors, and the
    5 per-frame batches the existing path consumes. layout "v": [vx, vy, type]; "dv": [vx, vy, dvx, dvy, type]."""
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    m = meshes.load_cylinder_mesh()
    b = meshes.cylinder_batch(1, t=0, mesh=m)
    vel, nt = m["velocity"].astype(np.float32), m["node_type"].astype(np.float32)
    ntc = np.broadcast_to(nt[None, :, None], (vel.shape[0], nt.shape[0], 1))
    if layout == "v":
        one = np.concatenate([vel, ntc], axis=2)
    else:
        dv = np.concatenate([np.zeros_like(vel[:1]), vel[1:] - vel[:-1]], axis=0)
        one = np.concatenate([vel, dv, ntc], axis=2)
    traj = torch.from_numpy(np.ascontiguousarray(one)).to(DEV)
    ei, ea = torch.from_numpy(b["edge_index"]).to(DEV), torch.from_numpy(b["edge_attr"]).to(DEV)
    frames = [Data(x=traj[t].clone(), y=traj[t + 1, :, 0:2].clone(), edge_index=ei, edge_attr=ea) for t in range(5)]
    return traj, ei, ea, frames


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(sim in eval mode, Rollout keyword arguments, node type index, traj, static batch, and the existing eager
    path's predictions, losses and RMSE on the 5 frames), computed once per model."""
    from graphphysics.models.processors import EncodeProcessDecode, EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    traj, ei, ea, frames = _mesh_traj("dv" if kind == "prev" else "v")
    torch.manual_seed(0)
    kw, nti = {}, 2
    if kind == "fp32":
        sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(5, 11, 3, 2, 32, compute_dtype=torch.float32), DEV)
    elif kind == "bf16":
        sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(15, 11, 3, 2, 128, compute_dtype=torch.bfloat16),
                        DEV)
    elif kind == "transformer":
        ea = None
        frames = [Data(x=f.x, y=f.y, edge_index=ei, edge_attr=None) for f in frames]
        m = EncodeTransformDecode(2, 11, 2, hidden_size=64, num_heads=4, compute_dtype=torch.float32)
        sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, DEV)
    else:  # previous data: [vx, vy, dvx, dvy, type]
        nti, kw = 4, dict(use_previous_data=True, previous_data_start=2, previous_data_end=4)
        sim = Simulator(13, 3, 2, 0, 4, 0, 2, 4, EncodeProcessDecode(3, 13, 3, 2, 32, compute_dtype=torch.float32), DEV)
    for f in frames[:2]:  # normaliser statistics from two training-mode forwards
        with torch.no_grad():
            sim(f)
    sim.eval()
    old = Rollout(sim, nti, graph=False, **kw)
    want = old.rollout(frames)
    batch = Data(x=frames[0].x.clone(), y=frames[0].y.clone(), edge_index=ei, edge_attr=ea)
    torch.cuda.synchronize()
    return sim, kw, nti, traj, batch, want, torch.stack(old.losses), old.all_rollout_rmse()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "transformer", "prev"])
def test_resident_rollout_equals_the_existing_rollout(kind, graph):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    sim, kw, nti, traj, batch, want, want_losses, want_rmse = _case(kind)
    keep = traj.clone()
    feed = ResidentTrajectories(traj, [0, traj.shape[1]], (0, 2), nti)
    ro = Rollout(sim, nti, graph=graph, feed=feed, **kw)
    got = ro.rollout_resident(batch, 0, 5)
    assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())
    assert len(ro.losses) == 5 and all(l.dim() == 0 and l.is_cuda for l in ro.losses)
    assert torch.equal(torch.stack(ro.losses), want_losses)
    assert abs(ro.all_rollout_rmse() - want_rmse) <= 1e-6 * want_rmse
    assert ro.resident_records == (1 if graph else 0)
    assert torch.equal(traj, keep)
    if kind == "prev":  # the feedback really ran: the last step's input carries pred3 and pred3 − pred2
        assert torch.equal(ro._res.x[:, 0:2], got[3]) and torch.equal(ro._res.x[:, 2:4], got[3] - got[2])


def test_the_same_trajectory_twice_is_bit_identical():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    sim, kw, nti, traj, batch, want, _, _ = _case("fp32")
    ro = Rollout(sim, nti, graph=True, feed=ResidentTrajectories(traj, [0, traj.shape[1]], (0, 2), nti))
    a = ro.rollout_resident(batch, 0, 5)
    b = ro.rollout_resident(batch, 0, 5)
    assert torch.equal(a, b) and torch.equal(a, want)
    assert torch.equal(torch.stack(ro.losses[:5]), torch.stack(ro.losses[5:]))
    assert ro.resident_records == 1


def test_keep_predictions_false_gives_the_same_losses_and_rmse():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    sim, kw, nti, traj, batch, _, want_losses, want_rmse = _case("fp32")
    ro = Rollout(sim, nti, graph=True, feed=ResidentTrajectories(traj, [0, traj.shape[1]], (0, 2), nti))
    assert ro.rollout_resident(batch, 0, 5, keep_predictions=False) is None
    assert ro._res.preds is None
    assert torch.equal(torch.stack(ro.losses), want_losses)
    assert abs(ro.all_rollout_rmse() - want_rmse) <= 1e-6 * want_rmse


def test_resident_rollout_matches_the_reference_fixture():
    """tests/golden/rollout_golden.npz: the reference's own validation loop over two trajectories (frames 0-4,
    then 1-3) with the cfgA model; the bounds of test_rollout_gpu.py::test_rollout_matches_reference_fixture.
    Both trajectories run on one recorded graph."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    g = np.load(os.path.join(G, "rollout_golden.npz"))
    assert g["plan"].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4], [1, 1], [1, 2], [1, 3]]
    m = EncodeProcessDecode(5, 11, 3, 2, 32, compute_dtype=torch.float32)
    sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, m, DEV)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}
    missing, unexpected = sim.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    sim.eval()
    traj, ei, ea, frames = _mesh_traj("v")
    batch = Data(x=frames[0].x.clone(), y=frames[0].y.clone(), edge_index=ei, edge_attr=ea)
    ro = Rollout(sim, 2, graph=True, feed=ResidentTrajectories(traj, [0, traj.shape[1]], (0, 2), 2))
    got = torch.cat([ro.rollout_resident(batch, 0, 5), ro.rollout_resident(batch, 1, 3)]).cpu()
    assert ro.resident_records == 1
    for i in range(8):
        ref = torch.from_numpy(g[f"pred{i}"])
        assert bool(((got[i] - ref).abs() <= 1e-4 * (1 + ref.abs())).all()), (i, float((got[i] - ref).abs().max()))
    assert len(ro.losses) == 8
    for a, b in zip([l.item() for l in ro.losses], g["val_loss"].tolist()):
        assert abs(a - b) <= 1e-6 + 1e-4 * b
    ref_rmse = float(g["val_all_rollout_rmse"][0])
    assert abs(ro.all_rollout_rmse() - ref_rmse) <= 1e-6 + 1e-4 * ref_rmse
