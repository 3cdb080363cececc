"""Rotation augmentation on the GPU: libmgn's mgn_feed_batch_rot / mgn_feed_rotate_rows against the same rule
written as torch ops (dataset.resident.fill_torch / rotate_rows_torch), mgn_feed_rotation_matrices against
Random3DRotate._build_rotation_matrix, and TrainStep(feed=ResidentTrajectories(..., rotate=...)): captured,
against eager, re-recorded on a mode switch, and the transformer.

The kernels write (a0*R0j + a1*R1j) + a2*R2j with every product and sum rounded on its own, the expression the torch
rule spells out with elementwise ops, so every comparison of x, y and edge_attr is bit equality (torch.equal). The
matrices themselves come from fp32 sine and cosine on the device and from Python floats on the host: those are
compared at atol 1e-5 (a bookkeeping bound: a swapped sign or a transposed entry is an error of order 0.1 at the
angles used, fp32 sine / cosine rounding of order 1e-7)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -777.0


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _traj(T, sizes, F, nti, seed=0):
    """Random [T, N, F] frames on the device; column nti: node types 0, 4, 5, 6 mixed (constant in time)."""
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, nti] = torch.tensor([0.0, 0.0, 4.0, 5.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    return traj.to(DEV), gp


def _matrices(angles):
    from graphphysics.dataset.preprocessing import Random3DRotate

    return torch.stack([Random3DRotate()._build_rotation_matrix(*a).reshape(9) for a in angles])


class _Batch:
    def __init__(self, x, y, edge_attr=None):
        self.x, self.y, self.edge_attr = x, y, edge_attr


SIZES, F11, NTI = [5, 0, 7, 300], 11, 10
TRIPLES, RANGES = [(0, 3), (4, 7), (7, 10)], [(0, 3), (4, 6)]


@pytest.mark.parametrize("noise", [True, False])
def test_feed_batch_rot_equals_fill_torch_bit_for_bit(noise):
    """An empty graph, graph boundaries inside a wave, more than one block; a noisy range that covers a triple and
    one that cuts one; x wider than F."""
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch

    traj, gp = _traj(3, SIZES, F11, NTI, seed=11)
    keep = traj.clone()
    N = traj.shape[1]
    par = {"noise_index_start": [0, 4], "noise_index_end": [3, 6], "noise_scale": [0.5, 0.02], "node_type_index": NTI}
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI, noise=par if noise else None, frames=[1, 0, 0, 1],
                                rotate={"feature_indices": TRIPLES})
    b = _Batch(torch.full((N, 13), SENTINEL, device=DEV), torch.full((N, 3), SENTINEL, device=DEV))
    torch.manual_seed(3)
    feed.fill(b)
    torch.cuda.synchronize()
    R, z = feed.R.clone(), (feed.z.clone() if noise else None)
    wx, wy = fill_torch(traj, gp, feed.frame, (0, 3), NTI, feed.ranges, feed.scales, z, TRIPLES, R)
    assert torch.equal(b.x[:, :F11], wx) and torch.equal(b.y, wy)
    assert bool((b.x[:, F11:] == SENTINEL).all())
    assert torch.equal(traj, keep)
    # the same rule on the host, from what the fill used
    cx, cy = fill_torch(traj.cpu(), gp, feed.frame.cpu(), (0, 3), NTI, feed.ranges,
                        feed.scales.cpu() if noise else None, z.cpu() if noise else None, TRIPLES, R.cpu())
    assert torch.equal(b.x[:, :F11].cpu(), cx) and torch.equal(b.y.cpu(), cy)
    # and it is a rotation of the clean frame: unrotated columns equal, rotated ones not
    clean, _ = fill_torch(traj, gp, feed.frame, (0, 3), NTI, [], None, None)
    assert torch.equal(b.x[:, 3], clean[:, 3]) and torch.equal(b.x[:, NTI], clean[:, NTI])
    assert not torch.equal(b.x[:, 7:10], clean[:, 7:10])
    torch.testing.assert_close(b.x[:, 7:10].norm(dim=1), clean[:, 7:10].norm(dim=1), rtol=1e-5, atol=1e-6)
    if noise:
        quiet, _ = fill_torch(traj, gp, feed.frame, (0, 3), NTI, [], None, None, TRIPLES, R)
        normal = clean[:, NTI] == 0
        assert torch.equal(b.x[:, :F11][~normal], quiet[~normal])
        assert not torch.equal(b.x[:, 0:3][normal], quiet[:, 0:3][normal])


def test_no_triples_is_mgn_feed_batch_bit_for_bit():
    from graphphysics import _native as nat

    traj, gp = _traj(3, SIZES, F11, NTI, seed=12)
    N = traj.shape[1]
    gp_d = torch.tensor(gp, dtype=torch.int32, device=DEV)
    fr = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=DEV)
    z = torch.randn(N, 5, generator=torch.Generator().manual_seed(5)).to(DEV)
    scales = torch.tensor([0.5, 0.02], device=DEV)
    out = []
    for triples in (None, []):
        x, y = torch.full((N, 13), SENTINEL, device=DEV), torch.full((N, 2), SENTINEL, device=DEV)
        nat.feed_batch(traj, gp_d, fr, (1, 3), NTI, RANGES, scales, z, x, y, triples, None)  # y 2 wide: allowed
        out.append((x, y))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not bool((out[1][0][:, :F11] == SENTINEL).any()) and bool((out[1][0][:, F11:] == SENTINEL).all())


ANGLES = [[0.7, -2.1, 2.9], [0.0, math.pi / 2, 0.0], [math.pi, -math.pi, 0.3], [-1.3, 0.4, 3.0], [0.0, 0.0, 0.0],
          [2.2, 1.1, -0.6]]


def test_rotation_matrices_against_the_host_formula():
    from graphphysics import _native as nat

    angles = torch.tensor(ANGLES, dtype=torch.float32, device=DEV)
    R = torch.full((6, 9), SENTINEL, device=DEV)
    nat.feed_rotation_matrices(angles, R)
    torch.cuda.synchronize()
    want = _matrices(ANGLES)
    err = (R.cpu() - want).abs().max()
    print("max |R - host|", float(err))
    assert float(err) <= 1e-5
    M = R.cpu().view(6, 3, 3)
    orth = (M @ M.transpose(1, 2) - torch.eye(3)).abs().max()
    print("max |R R^T - I|", float(orth))
    assert float(orth) <= 1e-5
    assert torch.equal(M[4], torch.eye(3))
    nat.feed_rotation_matrices(angles[:0], R[:0])  # no graphs: success without a launch


@pytest.mark.parametrize("E,A,triples", [(0, 4, [(0, 3)]), (1, 4, [(0, 3)]), (700, 4, [(0, 3)]),
                                          (700, 8, [(0, 3), (4, 7)]), (700, 8, [(1, 4)])])
def test_rotate_rows_equals_rotate_rows_torch_bit_for_bit(E, A, triples):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import rotate_rows_torch

    g = torch.Generator().manual_seed(E + A)
    src = torch.randn(E, A, generator=g).to(DEV)
    keep = src.clone()
    B = 6
    row_graph = torch.randint(0, B, (E,), generator=g).to(torch.int32)  # not sorted
    if E > 3:
        row_graph[3], row_graph[E - 1] = B, -1  # out of range: copied unrotated, R is not read
    row_graph = row_graph.to(DEV)
    R = _matrices(ANGLES).to(DEV)
    dst = torch.full((E, A + 2), SENTINEL, device=DEV)
    nat.feed_rotate_rows(src, row_graph, triples, R, dst)
    torch.cuda.synchronize()
    want = rotate_rows_torch(src, row_graph, triples, R)
    assert torch.equal(dst[:, :A], want)
    assert torch.equal(dst[:, :A].cpu(), rotate_rows_torch(src.cpu(), row_graph.cpu(), triples, R.cpu()))
    assert bool((dst[:, A:] == SENTINEL).all()) and torch.equal(src, keep)
    other = [c for c in range(A) if not any(s <= c < e for s, e in triples)]
    assert torch.equal(dst[:, other], src[:, other])
    if E > 3:
        assert torch.equal(dst[3, :A], src[3]) and torch.equal(dst[E - 1, :A], src[E - 1])
        s = triples[0][0]
        assert not torch.equal(dst[:3, s:s + 3], src[:3, s:s + 3])


def test_rotate_rows_refuses_overlapping_buffers():
    from graphphysics import _native as nat

    src = torch.zeros(10, 4, device=DEV)
    with pytest.raises((RuntimeError, ValueError), match="overlap"):
        nat.feed_rotate_rows(src, torch.zeros(10, dtype=torch.int32, device=DEV), [(0, 3)],
                             torch.zeros(1, 9, device=DEV), src)
    torch.cuda.synchronize()
    assert bool((src == 0).all())


# ----------------------------------------------------------------------------- TrainStep(feed=..., rotate=...)
F8, NTI8, TR8 = 8, 7, [(0, 3), (4, 7)]  # [velocity(3), pressure, position(3), node type]


def _toy(batch=2, T=4, seed=0):
    """(Data of `batch` copies of a 3 x 3 x 4 tetrahedral grid: x [N, 8], y [N, 3], edge_attr [dx, dy, dz, |d|];
    traj [T, N, 8]; node offsets)."""
    from graphphysics.utils import graph_build as GB
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    pos, cells = meshes.tet_grid(3, 3, 4, 0.5)
    n = pos.shape[0]
    g = torch.Generator().manual_seed(seed)
    pos_all = torch.cat([torch.from_numpy(pos) + 0.05 * torch.randn(n, 3, generator=g) for _ in range(batch)]).to(DEV)
    face = torch.cat([torch.from_numpy(cells).t() + i * n for i in range(batch)], dim=1).to(DEV)
    ei = GB.face_to_edge(face, batch * n)
    ea = GB.edge_features(pos_all, ei)
    N = batch * n
    traj = torch.randn(T, N, F8, generator=g)
    traj[:, :, 4:7] = pos_all.cpu()
    nt = torch.tensor([0.0, 0.0, 0.0, 4.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    traj[:, :, NTI8] = nt
    traj = traj.to(DEV)
    data = Data(x=traj[0].clone(), y=traj[1, :, 0:3].clone(), edge_index=ei, edge_attr=ea.clone())
    return data, traj, [i * n for i in range(batch + 1)], ea


def _epd(mp=2):
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    torch.manual_seed(0)
    sim = Simulator(16, 4, 3, 0, 7, 0, 3, NTI8, EncodeProcessDecode(mp, 16, 4, 3, 32, compute_dtype=torch.float32), DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    return sim, opt, CosineWarmupScheduler(opt, warmup=5, max_iters=100)


NOISE8 = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.02, "node_type_index": NTI8}


def test_captured_step_rotates_x_y_and_edge_attr_anew_on_every_replay():
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch, rotate_rows_torch
    from graphphysics.training.step import TrainStep

    data, traj, gp, ea = _toy()
    keep, keep_ea = traj.clone(), ea.clone()
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI8, noise=NOISE8,
                                rotate={"feature_indices": TR8, "edge_attr": ea, "edge_index": data.edge_index})
    sim, opt, sch = _epd()
    step = TrainStep(sim, opt, sch, data, graph=True, feed=feed)
    angles, eas, losses = [], [], []
    for _ in range(3):
        losses.append(float(step().item()))
        assert step.graph is not None
        wx, wy = fill_torch(traj, gp, feed.frame, (0, 3), NTI8, feed.ranges, feed.scales, feed.z, TR8, feed.R)
        assert torch.equal(step.batch.x, wx) and torch.equal(step.batch.y, wy)
        assert torch.equal(step.batch.edge_attr, rotate_rows_torch(ea, feed.row_graph, [(0, 3)], feed.R))
        torch.testing.assert_close(feed.R.cpu(), _matrices(feed.angles.tolist()), rtol=0, atol=1e-5)
        angles.append(feed.angles.clone())
        eas.append(step.batch.edge_attr.clone())
    assert all(np.isfinite(losses))
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    for a, b, ea_a, ea_b in ((angles[0], angles[1], eas[0], eas[1]), (angles[1], angles[2], eas[1], eas[2])):
        assert not torch.equal(a, b)  # the generator advanced inside the graph
        assert bool((a.cpu() >= -pi32).all()) and bool((a.cpu() < pi32).all())
        assert not torch.equal(ea_a[:, 0:3], ea_b[:, 0:3])
        assert torch.equal(ea_a[:, 3], ea_b[:, 3]) and torch.equal(ea_a[:, 3], keep_ea[:, 3])  # |d| is not rotated
    assert torch.equal(traj, keep) and torch.equal(ea, keep_ea)
    assert step.batch.edge_attr is not data.edge_attr and step.batch.edge_attr.data_ptr() != ea.data_ptr()


FRAMES = ([0, 2], [1, 0], [2, 1])
ROTS = ([[0.7, -2.1, 2.9], [0.0, math.pi / 2, 0.0]], [[-1.3, 0.4, 3.0], [2.2, 1.1, -0.6]],
        [[0.1, 0.2, 0.3], [3.0, -3.0, 1.5]])


def _run_fed(graph):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.step import TrainStep

    data, traj, gp, ea = _toy()
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI8,
                                rotate={"feature_indices": TR8, "edge_attr": ea, "edge_index": data.edge_index})
    sim, opt, sch = _epd()
    step = TrainStep(sim, opt, sch, data, graph=graph, feed=feed)
    losses = []
    for fr, rot in zip(FRAMES, ROTS):
        feed.set_frames(fr)
        feed.set_rotations(rot)
        losses.append(float(step().item()))
    torch.cuda.synchronize()
    return (losses, [p.detach().clone() for p in sim.parameters()], [b.detach().clone() for b in sim.buffers()],
            [t.detach().clone() for t in opt.param_groups[0]["flat_state"]], opt.param_groups[0]["step_count"],
            sch.last_epoch, opt.param_groups[0]["lr"])


def test_captured_rotated_step_equals_eager():
    """Explicit frames and angles, changed before each of 3 steps, noise off: captured == eager at the tolerances
    of test_feed_gpu.py::test_captured_fed_step_equals_eager_and_the_host_loop."""
    res = [_run_fed(False), _run_fed(True)]
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-6)
    for a, b in zip(res[0][1], res[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(res[0][2], res[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    for a, b in zip(res[0][3], res[1][3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    assert res[0][4:] == res[1][4:] and res[1][4] == 3
    assert len(set(res[1][0])) == 3  # three different batches


def test_switching_set_rotations_re_records_the_step():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.step import TrainStep

    data, traj, gp, ea = _toy()
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI8, frames=[0, 1],
                                rotate={"feature_indices": TR8, "edge_attr": ea, "edge_index": data.edge_index})
    sim, opt, sch = _epd()
    step = TrainStep(sim, opt, sch, data, graph=True, feed=feed)
    step()
    g0 = step.graph
    step()
    assert step.graph is g0 and step._feed_random == (False, True)
    explicit = torch.tensor(ROTS[0])
    feed.set_rotations(explicit)
    step()
    g1 = step.graph
    assert g1 is not g0 and step._feed_random == (False, False)
    assert torch.equal(feed.angles.cpu(), explicit)  # the recorded fill draws no angles
    feed.set_rotations(ROTS[1])
    step()
    assert step.graph is g1 and torch.equal(feed.angles.cpu(), torch.tensor(ROTS[1]))  # rewritten, not re-recorded
    torch.testing.assert_close(feed.R.cpu(), _matrices(ROTS[1]), rtol=0, atol=1e-5)
    feed.set_rotations("random")
    step()
    assert step.graph is not g1 and not torch.equal(feed.angles.cpu(), torch.tensor(ROTS[1]))


def test_transformer_trains_from_a_rotated_feed():
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    data, traj, gp, _ = _toy(1)
    data = Data(x=data.x, y=data.y, edge_index=data.edge_index, edge_attr=None)
    torch.manual_seed(0)
    m = EncodeTransformDecode(2, 16, 3, hidden_size=64, num_heads=4, compute_dtype=torch.float32)
    sim = Simulator(16, 0, 3, 0, 7, 0, 3, NTI8, m, DEV)
    opt = FusedAdamW(sim.parameters(), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
    sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100)
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI8, noise=NOISE8, rotate={"feature_indices": TR8})
    step = TrainStep(sim, opt, sch, data, graph=True, feed=feed)
    losses = [float(step().item()) for _ in range(3)]
    assert step.graph is not None and all(np.isfinite(losses)), losses
    assert step.batch.edge_attr is None
    wx, wy = fill_torch(traj, gp, feed.frame, (0, 3), NTI8, feed.ranges, feed.scales, feed.z, TR8, feed.R)
    assert torch.equal(step.batch.x, wx) and torch.equal(step.batch.y, wy)
    assert not torch.equal(feed.angles, torch.zeros_like(feed.angles))
