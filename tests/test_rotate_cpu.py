"""Rotation augmentation on the CPU (no kernels): dataset.preprocessing.Random3DRotate against the reference's own
Random3DRotate.forward (tests/golden/rotate_golden.npz, written by tests/golden/make_rotate_golden.py), the
rotation rule of fill_torch / rotate_rows_torch, the host-side validation of ResidentTrajectories(rotate=...) and
set_rotations, and the argument checks of the three new libmgn entry points (no device needed).

Tolerance of a rotated value against the reference: 8 * 2^-24 * (|a| @ |R|), elementwise. The classical bound of
a three-term fp32 dot product evaluated in any order is 3u * sum|a_i R_ij| + O(u^2) with u = 2^-24 (at most
(1+u)^3 - 1 per term; a fused multiply-add only lowers it); 4u covers the O(u^2) term, and the bound is stated for
BOTH sides (the reference's BLAS `@` and this package's), hence 8u."""
import math
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -24
FI = [(0, 3), (4, 7)]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(G, "rotate_golden.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k]) for k in z.files}


class _Batch:
    def __init__(self, x, y, edge_attr=None):
        self.x, self.y, self.edge_attr = x, y, edge_attr


def _fixed(angles):
    """Random3DRotate(FI) whose random angles are `angles`."""
    from graphphysics.dataset.preprocessing import Random3DRotate

    t = Random3DRotate(feature_indices=list(FI))
    t._get_random_angles = lambda: list(angles)
    return t


@pytest.mark.parametrize("case", ["a", "b"])
def test_build_rotation_matrix_is_the_references(gold, case):
    from graphphysics.dataset.preprocessing import Random3DRotate

    m = Random3DRotate()._build_rotation_matrix(*[float(v) for v in gold["angles_" + case]])
    assert m.dtype == torch.float32 and torch.equal(m, gold["matrix_" + case])


@pytest.mark.parametrize("case", ["a", "b"])
def test_forward_reproduces_the_reference(gold, case):
    from graphphysics.utils.data import Data

    t = _fixed([float(v) for v in gold["angles_" + case]])
    x_in, y_in, pos_in = gold["x_in"], gold["y_in"], gold["pos_in"]
    R = gold["matrix_" + case]
    d = t.forward(Data(x=x_in.clone(), y=y_in.clone(), pos=pos_in.clone()))
    untouched = [c for c in range(x_in.shape[1]) if not any(s <= c < e for s, e in FI)]
    assert torch.equal(d.x[:, untouched], gold["x_out_" + case][:, untouched])
    assert torch.equal(d.x[:, untouched], x_in[:, untouched])
    for got, want, a in [(d.x[:, 0:3], gold["x_out_" + case][:, 0:3], x_in[:, 0:3]),
                         (d.x[:, 4:7], gold["x_out_" + case][:, 4:7], x_in[:, 4:7]),
                         (d.y, gold["y_out_" + case], y_in), (d.pos, gold["pos_out_" + case], pos_in)]:
        bound = 8 * U * (a.abs().double() @ R.abs().double())
        err = (got.double() - want.double()).abs()
        print(case, "max err / (2^-24 |a|@|R|):", float((err / (bound / 8)).max()))
        assert bool((err <= bound).all())
    assert not torch.equal(d.x[:, 0:3], x_in[:, 0:3])


def test_explicit_sum_is_within_the_bound_of_the_reference(gold):
    """The three-term sum the kernels and fill_torch use, against the reference's stored `@` results."""
    from graphphysics.dataset.resident import _rot3

    for case in ("a", "b"):
        R = gold["matrix_" + case]
        for a, want in ((gold["y_in"], gold["y_out_" + case]), (gold["pos_in"], gold["pos_out_" + case]),
                        (gold["x_in"][:, 4:7], gold["x_out_" + case][:, 4:7])):
            got = _rot3(a, R.reshape(1, 3, 3).expand(a.shape[0], 3, 3))
            bound = 8 * U * (a.abs().double() @ R.abs().double())
            assert bool(((got.double() - want.double()).abs() <= bound).all())


def test_call_mutates_x_in_place_and_rebinds_pos_and_y(gold):
    from graphphysics.utils.data import Data

    x, y, pos = gold["x_in"].clone(), gold["y_in"].clone(), gold["pos_in"].clone()
    d = Data(x=x, y=y, pos=pos)
    out = _fixed([0.7, -2.1, 2.9])(d)
    assert out is not d
    assert out.x is x and d.x is x and not torch.equal(x, gold["x_in"])  # written in place: the caller sees it
    assert d.y is y and torch.equal(y, gold["y_in"]) and out.y is not y  # rebound on the copy only
    assert d.pos is pos and torch.equal(pos, gold["pos_in"]) and out.pos is not pos
    bound = 8 * U * (gold["x_in"][:, 0:3].abs().double() @ gold["matrix_a"].abs().double())
    assert bool(((out.x[:, 0:3].double() - gold["x_out_a"][:, 0:3].double()).abs() <= bound).all())


def test_a_wider_y_comes_back_three_wide_and_ranges_must_be_three_wide(gold):
    from graphphysics.dataset.preprocessing import Random3DRotate
    from graphphysics.utils.data import Data

    y5 = torch.cat([gold["y_in"], gold["y_in"][:, :2]], dim=1)
    d = _fixed([0.7, -2.1, 2.9]).forward(Data(x=gold["x_in"].clone(), y=y5, pos=None))
    assert tuple(d.y.shape) == (40, 3)
    bound = 8 * U * (gold["y_in"].abs().double() @ gold["matrix_a"].abs().double())
    assert bool(((d.y.double() - gold["y_out_a"].double()).abs() <= bound).all())
    with pytest.raises(AssertionError):
        Random3DRotate(feature_indices=[(0, 2)])
    with pytest.raises(AssertionError):
        Random3DRotate(feature_indices=[(0, 3), (4, 8)])
    with pytest.raises(AssertionError, match="3-dimensional"):
        Random3DRotate().forward(Data(x=gold["x_in"].clone(), y=gold["y_in"].clone(), pos=torch.zeros(40, 2)))
    assert Random3DRotate().feature_indices == []


def test_random_angles_are_three_uniform_draws_in_radians():
    import random

    from graphphysics.dataset.preprocessing import Random3DRotate

    random.seed(7)
    want = [math.radians(random.uniform(-180, 180)) for _ in range(3)]
    random.seed(7)
    assert Random3DRotate()._get_random_angles() == want
    assert all(-math.pi <= a <= math.pi for a in want)


def test_random3drotate_inside_build_preprocessing(gold):
    from graphphysics.dataset.preprocessing import Random3DRotate, build_preprocessing
    from graphphysics.utils.data import Data

    t = _fixed([0.7, -2.1, 2.9])
    assert isinstance(t, Random3DRotate)
    pre = build_preprocessing(extra_node_features=[t], add_edges_features=False)
    assert pre.transforms[0] is t
    d = pre(Data(x=gold["x_in"].clone(), y=gold["y_in"].clone(), pos=gold["pos_in"].clone(), face=None))
    bound = 8 * U * (gold["pos_in"].abs().double() @ gold["matrix_a"].abs().double())
    assert bool(((d.pos.double() - gold["pos_out_a"].double()).abs() <= bound).all())
    assert tuple(d.y.shape) == (40, 3) and not torch.equal(d.x, gold["x_in"])


# ----------------------------------------------------------------------------- fill_torch / rotate_rows_torch
def _traj(T, sizes, F, nti, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, nti] = torch.tensor([0.0, 0.0, 4.0, 5.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    return traj, gp


def _matrices(angles):
    from graphphysics.dataset.preprocessing import Random3DRotate

    return torch.stack([Random3DRotate()._build_rotation_matrix(*a).reshape(9) for a in angles])


TRIPLES, RANGES, NTI, F11 = [(0, 3), (4, 7), (7, 10)], [(0, 3), (4, 6)], 10, 11
ANGLES = [[0.7, -2.1, 2.9], [0.0, math.pi / 2, 0.0], [-1.3, 0.4, 3.0]]


def test_fill_torch_rotates_first_then_adds_noise_on_normal_rows():
    from graphphysics.dataset.resident import fill_torch

    traj, gp = _traj(4, [6, 0, 9], F11, NTI, seed=3)
    keep = traj.clone()
    frames = [2, 0, 1]
    frame = torch.tensor(frames, dtype=torch.int32)
    R = _matrices(ANGLES)
    z = torch.randn(15, 5, generator=torch.Generator().manual_seed(1))
    scales = torch.tensor([0.5, 0.25])
    x, y = fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, z, TRIPLES, R)
    x0, y0 = fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, None, TRIPLES, R)  # rotated, no noise
    for g, f in enumerate(frames):
        rows = slice(gp[g], gp[g + 1])
        Rg = R[g].view(3, 3)
        clean, nxt = keep[f, rows], keep[f + 1, rows]
        for s, e in TRIPLES:
            a = clean[:, s:e]
            want = (a[:, 0:1] * Rg[0] + a[:, 1:2] * Rg[1]) + a[:, 2:3] * Rg[2]
            assert torch.equal(x0[rows, s:e], want)
            assert bool(((want.double() - a.double() @ Rg.double()).abs()
                         <= 4 * U * (a.abs().double() @ Rg.abs().double())).all())
        wy = (nxt[:, 0:1] * Rg[0] + nxt[:, 1:2] * Rg[1]) + nxt[:, 2:3] * Rg[2]
        assert torch.equal(y[rows], wy) and torch.equal(y0[rows], wy)  # the rotated next CLEAN frame
        # columns outside triples and noisy ranges: the frame bit for bit
        assert torch.equal(x[rows, 3], clean[:, 3]) and torch.equal(x[rows, 10], clean[:, 10])
        normal = clean[:, NTI] == 0
        # noise second, on NORMAL rows only, on top of the rotated value
        zc = 0
        for i, (s, e) in enumerate(RANGES):
            want = torch.where(normal[:, None], x0[rows, s:e] + z[rows, zc:zc + e - s] * scales[i], x0[rows, s:e])
            assert torch.equal(x[rows, s:e], want)
            zc += e - s
        assert torch.equal(x[rows][~normal], x0[rows][~normal])  # rotated but not noised
        assert torch.equal(x[rows, 6:10], x0[rows, 6:10])  # rotated columns outside the noisy ranges
        if int(normal.sum()):
            assert not torch.equal(x[rows, 0:3][normal], x0[rows, 0:3][normal])
    assert not torch.equal(x0[:, 0:3], fill_torch(traj, gp, frame, (0, 3), NTI, [], None, None)[0][:, 0:3])
    assert torch.equal(traj, keep)


def test_identity_rotation_equals_the_unrotated_fill_bit_for_bit():
    from graphphysics.dataset.resident import fill_torch

    traj, gp = _traj(3, [5, 8], F11, NTI, seed=4)
    frame = torch.tensor([1, 0], dtype=torch.int32)
    z = torch.randn(13, 5, generator=torch.Generator().manual_seed(2))
    scales = torch.tensor([0.5, 0.25])
    eye = torch.eye(3).reshape(1, 9).repeat(2, 1)
    x, y = fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, z, TRIPLES, eye)
    wx, wy = fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, z)
    assert torch.equal(x, wx) and torch.equal(y, wy)
    wx2, wy2 = fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, z, None, None)
    assert torch.equal(wx, wx2) and torch.equal(wy, wy2)
    with pytest.raises(ValueError):
        fill_torch(traj, gp, frame, (0, 2), NTI, RANGES, scales, z, TRIPLES, eye)  # y must be 3 wide
    with pytest.raises(ValueError):
        fill_torch(traj, gp, frame, (0, 3), NTI, RANGES, scales, z, TRIPLES, None)


def test_rotate_rows_torch_rule():
    from graphphysics.dataset.resident import rotate_rows_torch

    g = torch.Generator().manual_seed(5)
    src = torch.randn(9, 8, generator=g)
    keep = src.clone()
    row_graph = torch.tensor([2, 0, 1, 1, 7, 0, 2, -1, 1], dtype=torch.int32)  # unsorted; 7 and -1 out of range
    R = _matrices(ANGLES)
    out = rotate_rows_torch(src, row_graph, [(0, 3), (4, 7)], R)
    assert out is not src and torch.equal(src, keep)
    assert torch.equal(out[:, 3], src[:, 3]) and torch.equal(out[:, 7], src[:, 7])
    for r, gid in enumerate(row_graph.tolist()):
        if not 0 <= gid < 3:
            assert torch.equal(out[r], src[r])
            continue
        Rg = R[gid].view(3, 3)
        for s in (0, 4):
            a = src[r, s:s + 3]
            assert torch.equal(out[r, s:s + 3], (a[0] * Rg[0] + a[1] * Rg[1]) + a[2] * Rg[2])
    assert tuple(rotate_rows_torch(src[:0], row_graph[:0], [(0, 3)], R).shape) == (0, 8)
    # lengths are kept by a rotation: |d| of [dx, dy, dz, |d|] stays what it was, the vector keeps its norm
    assert torch.allclose(out[:4, 0:3].norm(dim=1), src[:4, 0:3].norm(dim=1), rtol=1e-5)


# ----------------------------------------------------------------------------- ResidentTrajectories(rotate=...)
def _edges(gp):
    """A ring inside every graph: [2, E] node pairs that never cross graphs."""
    src, dst = [], []
    for a, b in zip(gp, gp[1:]):
        for i in range(a, b):
            src.append(i)
            dst.append(a + (i + 1 - a) % (b - a))
    return torch.tensor([src, dst])


def test_feed_leaves_traj_and_clean_edge_attr_unchanged_after_three_fills():
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch, rotate_rows_torch

    traj, gp = _traj(4, [6, 9], F11, NTI, seed=6)
    ei = _edges(gp)
    ea = torch.randn(ei.shape[1], 4, generator=torch.Generator().manual_seed(8))
    keep, keep_ea = traj.clone(), ea.clone()
    noise = {"noise_index_start": [0, 4], "noise_index_end": [3, 6], "noise_scale": [0.5, 0.25], "node_type_index": NTI}
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI, noise=noise,
                                rotate={"feature_indices": TRIPLES, "edge_attr": ea, "edge_index": ei})
    assert feed.random_rotations is True and feed.edge_triples == [(0, 3)]
    assert feed.row_graph.dtype == torch.int32 and feed.row_graph.tolist() == [0] * 6 + [1] * 9
    assert tuple(feed.angles.shape) == (2, 3) and tuple(feed.R.shape) == (2, 9)
    b = _Batch(torch.full((15, 13), -7.0), torch.zeros(15, 3), torch.full((15, 6), -7.0))
    ptrs = (feed.angles.data_ptr(), feed.R.data_ptr())
    seen = []
    torch.manual_seed(0)
    for _ in range(3):
        feed.fill(b)
        seen.append(feed.angles.clone())
        assert torch.equal(feed.R, _matrices(feed.angles.tolist()))
        wx, wy = fill_torch(traj, gp, feed.frame, (0, 3), NTI, feed.ranges, feed.scales, feed.z, TRIPLES, feed.R)
        assert torch.equal(b.x[:, :11], wx) and torch.equal(b.y, wy)
        assert torch.equal(b.edge_attr[:, :4], rotate_rows_torch(ea, feed.row_graph, [(0, 3)], feed.R))
        assert torch.equal(b.edge_attr[:, 3], keep_ea[:, 3])
        assert bool((b.x[:, 11:] == -7.0).all()) and bool((b.edge_attr[:, 4:] == -7.0).all())
    assert (feed.angles.data_ptr(), feed.R.data_ptr()) == ptrs
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert torch.equal(traj, keep) and torch.equal(ea, keep_ea)
    with pytest.raises(ValueError, match="clean edge_attr"):
        feed.fill(_Batch(b.x, b.y, ea))
    for bad in (None, torch.zeros(15, 3), torch.zeros(14, 4), torch.zeros(15, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="edge_attr"):
            feed.fill(_Batch(b.x, b.y, bad))


def test_rotate_none_changes_nothing():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(4, [6, 9], F11, NTI, seed=6)
    feed = ResidentTrajectories(traj, gp, (0, 2), NTI, frames=[1, 2], rotate=None)
    assert feed.angles is None and feed.R is None and feed.row_graph is None and feed.random_rotations is None
    b = _Batch(torch.zeros(15, 11), torch.zeros(15, 2))
    feed.fill(b)
    assert torch.equal(b.x[:6], traj[1, :6]) and torch.equal(b.y[6:], traj[3, 6:, 0:2])
    with pytest.raises(ValueError):
        feed.set_rotations("random")


def test_rotate_arguments_are_validated():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(3, [5, 4], F11, NTI)
    ei = _edges(gp)
    ea = torch.randn(9, 4)

    def make(y_columns=(0, 3), **kw):
        r = {"feature_indices": [(0, 3), (4, 7)], "edge_attr": ea, "edge_index": ei}
        r.update(kw)
        return ResidentTrajectories(traj, gp, y_columns, NTI, rotate={k: v for k, v in r.items() if v is not ...})

    assert make().triples == [(0, 3), (4, 7)]
    cross = ei.clone()
    cross[1, 2] = 7  # node 2 (graph 0) -> node 7 (graph 1)
    with pytest.raises(ValueError, match="different graphs"):
        make(edge_index=cross)
    with pytest.raises(ValueError, match="exactly 3"):
        make(feature_indices=[(0, 2)])
    with pytest.raises(ValueError, match="exactly 3"):
        make(edge_feature_indices=[(0, 4)])
    with pytest.raises(ValueError, match="overlap"):
        make(feature_indices=[(0, 3), (2, 5)])
    with pytest.raises(ValueError, match="node_type_index"):
        make(feature_indices=[(8, 11)])
    with pytest.raises(ValueError, match="at most 4"):
        ResidentTrajectories(torch.zeros(2, 9, 16), gp, (0, 3), 15,
                             rotate={"feature_indices": [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15)]})
    with pytest.raises(ValueError, match="outside"):
        make(feature_indices=[(9, 12)])
    with pytest.raises(ValueError, match="outside"):
        make(edge_feature_indices=[(2, 5)])
    with pytest.raises(ValueError, match="3 wide"):
        make(y_columns=(0, 2))
    with pytest.raises(ValueError, match="3 wide"):
        make(y_columns=(0, 4))
    for bad in (ea.double(), ea[0], ea[:8], torch.randn(9, 8)[:, ::2]):
        with pytest.raises(ValueError, match="edge_"):
            make(edge_attr=bad)
    with pytest.raises(ValueError, match="edge_index"):
        make(edge_index=...)
    with pytest.raises(ValueError, match="edge_index"):
        make(edge_index=ei[:, :8])
    with pytest.raises(ValueError, match="edge_index"):
        make(edge_index=torch.full((2, 9), 9))
    with pytest.raises(ValueError, match="without edge_attr"):
        make(edge_attr=..., edge_index=ei)
    with pytest.raises(ValueError, match="keys"):
        make(angles=[0, 0, 0])
    with pytest.raises(ValueError, match="keys"):
        ResidentTrajectories(traj, gp, (0, 3), NTI, rotate=[(0, 3)])
    with pytest.raises(ValueError, match="at least one"):
        make(feature_indices=[])
    # the transformer's case: no edge_attr at all
    f = ResidentTrajectories(traj, gp, (0, 3), NTI, rotate={"feature_indices": [(0, 3)]})
    assert f.edge_attr is None and f.row_graph is None
    f.fill(_Batch(torch.zeros(9, 11), torch.zeros(9, 3)))


def test_set_rotations():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(3, [2] * 8, F11, NTI)
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI, rotate={"feature_indices": [(0, 3)]})
    b = _Batch(torch.zeros(16, 11), torch.zeros(16, 3))
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    torch.manual_seed(0)
    seen = []
    for _ in range(40):
        feed.fill(b)
        seen.append(feed.angles.clone())
    seen = torch.stack(seen)
    assert bool((seen >= -pi32).all()) and bool((seen < pi32).all())
    assert float(seen.min()) < -2.5 and float(seen.max()) > 2.5 and len(set(seen.flatten().tolist())) > 900
    explicit = [[0.1 * g, -0.2 * g, 0.3] for g in range(8)]
    feed.set_rotations(explicit)
    assert feed.random_rotations is False
    for _ in range(2):
        feed.fill(b)
        assert torch.equal(feed.angles, torch.tensor(explicit))
    assert torch.equal(feed.R, _matrices(torch.tensor(explicit).tolist()))
    feed.set_rotations(torch.tensor(explicit) * 2)
    assert torch.equal(feed.angles, torch.tensor(explicit) * 2)
    for bad in ([[0.0, 0.0, 0.0]] * 7, [[0.0, 0.0]] * 8, [0.0] * 8, torch.zeros(8, 3, 1), "fixed",
                [[float("nan"), 0.0, 0.0]] * 8):
        with pytest.raises(ValueError):
            feed.set_rotations(bad)
    assert feed.random_rotations is False and torch.equal(feed.angles, torch.tensor(explicit) * 2)
    feed.set_rotations("random")
    assert feed.random_rotations is True
    feed.fill(b)
    assert not torch.equal(feed.angles, torch.tensor(explicit) * 2)


def test_train_step_tracks_the_feeds_rotation_mode():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.step import TrainStep

    traj, gp = _traj(3, [5, 4], F11, NTI)
    feed = ResidentTrajectories(traj, gp, (0, 3), NTI, rotate={"feature_indices": [(0, 3)]})
    sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(2, 11, 3, 2, 8), torch.device("cpu"))
    opt = torch.optim.AdamW(sim.parameters(), lr=1e-3)
    step = TrainStep(sim, opt, torch.optim.lr_scheduler.StepLR(opt, 10), _Batch(torch.zeros(9, 11), torch.zeros(9, 3)),
                     graph=False, feed=feed)
    assert step._feed_mode() == (True, True)
    feed.set_rotations([[0.0, 0.0, 0.0]] * 2)
    feed.set_frames([0, 1])
    assert step._feed_mode() == (False, False)
    plain = ResidentTrajectories(traj, gp, (0, 3), NTI)
    assert TrainStep(sim, opt, step.sched, step.batch, graph=False, feed=plain)._feed_mode() == (True, None)


# ----------------------------------------------------------------------------- libmgn argument checks, no device
def test_library_refuses_bad_rotation_arguments_without_a_device():
    """The three entry points check their arguments on the host before any device work: a nonzero status and a
    message, here with null pointers (nothing is launched); no nodes / graphs / rows is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    lib = nat.lib()
    R = 0x1000  # a non-null address that is never dereferenced: every call here returns before a launch

    def batch(T=3, N=10, F=11, B=2, ys=0, ye=3, ti=10, ranges=((0, 3), (4, 6)), n=None, ldz=8, ldx=13, ldy=3,
              triples=((0, 3), (4, 7)), tn=None, R=R):
        rg, tr = nat.feed_ranges(ranges), nat.feed_ranges(triples)
        if n is not None:
            rg.n = n
        if tn is not None:
            tr.n = tn
        rc = lib.mgn_feed_batch_rot(None, T, N, F, None, B, None, ys, ye, ti, rg, None, None, ldz, None, ldx, None,
                                    ldy, tr, R, None)
        return rc, lib.mgn_last_error().decode()

    assert batch(N=0)[0] == 0 and batch(B=0)[0] == 0
    assert batch(N=0, triples=(), R=None)[0] == 0 and batch(N=0, ys=0, ye=0)[0] == 0
    bad = {"width 2": dict(triples=((0, 2),)), "width 4": dict(triples=((0, 4),)), "start<0": dict(triples=((-1, 2),)),
           "end>F": dict(triples=((9, 12),)), "overlap": dict(triples=((0, 3), (2, 5))),
           "type inside": dict(triples=((8, 11),)), "type inside 2": dict(ti=5), "y 2 wide": dict(ye=2),
           "y 4 wide": dict(ye=4, ldy=4), "R null": dict(R=None), "tn>4": dict(tn=5), "tn<0": dict(tn=-1),
           # everything mgn_feed_batch refuses
           "T<2": dict(T=1), "F<1": dict(F=0), "range end>F": dict(ranges=((0, 3), (4, 12))),
           "range start<0": dict(ranges=((-1, 2),)), "range reversed": dict(ranges=((2, 1),)),
           "ranges overlap": dict(ranges=((0, 3), (2, 6))), "y end>F": dict(ys=9, ye=12), "ys<0": dict(ys=-1, ye=2),
           "y reversed": dict(ys=3, ye=2), "ti=F": dict(ti=11), "ti<0": dict(ti=-1), "n>4": dict(n=5),
           "n<0": dict(n=-1), "ldx<F": dict(ldx=10), "ldy<3": dict(ldy=2), "null pointers": dict()}
    for name, kw in bad.items():
        rc, msg = batch(N=0, **kw) if name != "null pointers" else batch(**kw)  # N = 0: refused before the early return
        assert rc != 0 and "feed_batch_rot" in msg, (name, rc, msg)
    assert "R" in batch(N=0, R=None)[1] and "3" in batch(N=0, triples=((0, 2),))[1]

    def rows(rows=10, cols=4, ld_src=4, B=2, triples=((0, 3),), tn=None, R=R, ld_dst=6):
        tr = nat.feed_ranges(triples)
        if tn is not None:
            tr.n = tn
        rc = lib.mgn_feed_rotate_rows(None, rows, cols, ld_src, None, B, tr, R, None, ld_dst, None)
        return rc, lib.mgn_last_error().decode()

    assert rows(rows=0)[0] == 0 and rows(rows=0, triples=(), R=None)[0] == 0
    for name, kw in {"width 2": dict(triples=((0, 2),)), "end>cols": dict(triples=((2, 5),)),
                     "start<0": dict(triples=((-1, 2),)), "overlap": dict(cols=8, ld_src=8, ld_dst=8,
                                                                          triples=((0, 3), (1, 4))),
                     "R null": dict(R=None), "ld_src<cols": dict(ld_src=3), "ld_dst<cols": dict(ld_dst=3),
                     "cols<1": dict(cols=0, triples=()), "rows<0": dict(rows=-1), "tn>4": dict(tn=5)}.items():
        rc, msg = rows(rows=0, **kw) if name != "rows<0" else rows(**kw)
        assert rc != 0 and "feed_rotate_rows" in msg, (name, rc, msg)
    rc, msg = rows()  # valid but null pointers
    assert rc != 0 and "feed_rotate_rows" in msg

    assert lib.mgn_feed_rotation_matrices(None, 0, None, None) == 0
    assert lib.mgn_feed_rotation_matrices(None, -1, None, None) != 0
    assert lib.mgn_feed_rotation_matrices(None, 2, None, None) != 0
    assert "feed_rotation_matrices" in lib.mgn_last_error().decode()
    for name in ("mgn_feed_rotation_matrices", "mgn_feed_batch_rot", "mgn_feed_rotate_rows"):
        assert name in nat.EXPORTS
