"""Resident trajectories on the CPU (no kernels): fill_torch against the reference's own add_noise
(tests/golden/feed_golden.npz, written by tests/golden/make_feed_golden.py), the frame / next-frame rule, the
stored trajectories staying clean, and the host-side validation of ResidentTrajectories and TrainStep(feed=)."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(G, "feed_golden.npz"))
    d = {k: z[k] for k in z.files}
    d["ranges"] = [tuple(int(v) for v in r) for r in d["ranges"]]
    return d


def _traj(T, sizes, F, nti, seed=0):
    """[T, N, F] random frames whose node-type column is constant over time and mixes 0, 4, 5, 6."""
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, nti] = torch.tensor([0.0, 0.0, 4.0, 5.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    return traj, gp


class _Batch:
    def __init__(self, x, y):
        self.x, self.y = x, y


@pytest.mark.parametrize("key,t", [("x_out", None), ("x_out_t", 0.25)])
def test_fill_torch_reproduces_the_reference_add_noise_bit_for_bit(gold, key, t):
    """One graph, T = 2, frame 0, traj[0] = the fixture's x_in: x is the reference's add_noise output bit for
    bit, for the plain scales and for the curriculum scales set_noise_t(t) computes."""
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch

    x_in, z = torch.from_numpy(gold["x_in"]), torch.from_numpy(gold["z"])
    N, F = x_in.shape
    nti = int(gold["node_type_index"])
    traj = torch.stack([x_in, x_in + 1.0])
    noise = {"noise_index_start": [s for s, _ in gold["ranges"]], "noise_index_end": [e for _, e in gold["ranges"]],
             "noise_scale": [float(s) for s in gold["scales"]], "node_type_index": nti}
    feed = ResidentTrajectories(traj, [0, N], (0, 2), nti, noise=noise, frames=[0])
    feed.set_noise_t(t)
    want_scales = gold["scales"] if t is None else gold["scales_t"]
    assert torch.equal(feed.scales, torch.tensor(want_scales, dtype=torch.float32))
    x, y = fill_torch(traj, [0, N], feed.frame, (0, 2), nti, feed.ranges, feed.scales, z)
    x_out = torch.from_numpy(gold[key])
    assert torch.equal(x, x_out)
    # rows of another type, and every column outside the ranges, are x_in exactly
    normal = x_in[:, nti] == 0
    assert 0 < int(normal.sum()) < N
    assert torch.equal(x[~normal], x_in[~normal])
    outside = [c for c in range(F) if not any(s <= c < e for s, e in gold["ranges"])]
    assert outside and torch.equal(x[:, outside], x_in[:, outside])
    assert not torch.equal(x[normal][:, [0, 1, 3, 4]], x_in[normal][:, [0, 1, 3, 4]])
    assert torch.equal(y, traj[1][:, 0:2])
    feed.set_noise_t(None)
    assert torch.equal(feed.scales, torch.tensor(gold["scales"], dtype=torch.float32))


def test_y_is_the_next_clean_frame_and_x_the_chosen_frame_per_graph():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(5, [3, 0, 7, 4], 6, 5)
    keep = traj.clone()
    noise = {"noise_index_start": [0, 3], "noise_index_end": [2, 4], "noise_scale": [0.1, 0.2], "node_type_index": 5}
    feed = ResidentTrajectories(traj, gp, (1, 4), 5, noise=noise, frames=[3, 0, 0, 2])
    b = _Batch(torch.full((14, 8), -7.0), torch.zeros(14, 3))
    feed.fill(b)
    normal = traj[0, :, 5] == 0
    for g, f in enumerate([3, 0, 0, 2]):
        rows = slice(gp[g], gp[g + 1])
        assert torch.equal(b.y[rows], keep[f + 1, rows, 1:4])
        assert torch.equal(b.x[rows, 2], keep[f, rows, 2]) and torch.equal(b.x[rows, 4:6], keep[f, rows, 4:6])
        other = ~normal[rows]
        assert torch.equal(b.x[rows, :6][other], keep[f, rows][other])
        want = keep[f, rows, 0:2] + feed.z[rows, 0:2] * feed.scales[0]
        assert torch.equal(b.x[rows, 0:2][~other], want[~other])
    assert torch.equal(b.x[:, 6:], torch.full((14, 2), -7.0))  # columns beyond F are left alone
    assert torch.equal(traj, keep)


def test_traj_is_bitwise_unchanged_after_three_noisy_fills():
    """The accumulation trap of the in-place add_noise on device-resident frames: the feed never writes traj, and
    every fill is noise on the CLEAN frame (|x - clean| stays at the scale of one draw)."""
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(4, [20, 13], 3, 2, seed=1)
    keep = traj.clone()
    noise = {"noise_index_start": 0, "noise_index_end": 2, "noise_scale": 0.5, "node_type_index": 2}
    feed = ResidentTrajectories(traj, gp, (0, 2), 2, noise=noise, frames=[1, 2])
    b = _Batch(torch.zeros(33, 3), torch.zeros(33, 2))
    seen = []
    for _ in range(3):
        feed.fill(b)
        seen.append(b.x.clone())
        clean = torch.cat([keep[1, :20], keep[2, 20:]])
        assert torch.equal(b.x[:, :2] - clean[:, :2] != 0, (clean[:, 2] == 0)[:, None].expand(-1, 2))
        want = clean[:, :2] + feed.z * feed.scales[0]
        assert torch.equal(b.x[:, :2][clean[:, 2] == 0], want[clean[:, 2] == 0])
    assert torch.equal(traj, keep)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_random_frames_stay_in_range_and_explicit_frames_stick():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(6, [2] * 8, 3, 2)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    assert feed.z is None and feed.scales is None and feed.frame.dtype == torch.int32
    b = _Batch(torch.zeros(16, 3), torch.zeros(16, 2))
    torch.manual_seed(0)
    seen = set()
    for _ in range(50):
        feed.fill(b)
        seen.update(feed.frame.tolist())
    assert seen == {0, 1, 2, 3, 4}
    feed.set_frames(torch.tensor([4, 0, 1, 2, 3, 4, 0, 1]))
    for _ in range(2):
        feed.fill(b)
        assert feed.frame.tolist() == [4, 0, 1, 2, 3, 4, 0, 1]
    assert torch.equal(b.x[:2], traj[4, :2]) and torch.equal(b.y[2:4], traj[1, 2:4, :2])
    feed.set_frames("random")
    assert feed.random_frames


def test_set_frames_rejects_frames_without_a_successor_and_wrong_lengths():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(6, [2, 3], 3, 2)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2, frames=[4, 0])
    for bad in ([5, 0], [0, -1], [0], [0, 1, 2], torch.tensor([0, 5])):
        with pytest.raises(ValueError):
            feed.set_frames(bad)
    assert feed.frame.tolist() == [4, 0] and not feed.random_frames
    with pytest.raises(ValueError):
        feed.set_frames("sequential")
    with pytest.raises(ValueError):
        ResidentTrajectories(traj, gp, (0, 2), 2, frames=[5, 0])


def test_noise_parameters_follow_the_reference_checks():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(3, [5], 6, 5)

    def make(**kw):
        n = {"noise_index_start": [0, 3], "noise_index_end": [2, 5], "noise_scale": [0.1, 0.2], "node_type_index": 5}
        n.update(kw)
        return ResidentTrajectories(traj, gp, (0, 2), 5, noise=n)

    with pytest.raises(ValueError, match="noise_index_start and noise_index_end must have the same length."):
        make(noise_index_end=[2])
    with pytest.raises(ValueError,
                       match="noise_scale must have the same length as noise_index_start and noise_index_end."):
        make(noise_scale=[0.1])
    with pytest.raises(ValueError, match="node_type_index"):
        make(node_type_index=2)
    with pytest.raises(ValueError, match="overlap"):
        make(noise_index_start=[0, 1])
    with pytest.raises(ValueError, match="outside"):
        make(noise_index_end=[2, 7])
    with pytest.raises(ValueError, match="at most 4"):
        make(noise_index_start=[0, 1, 2, 3, 4], noise_index_end=[1, 2, 3, 4, 5], noise_scale=0.1)
    f = make(noise_index_start=0, noise_index_end=2, noise_scale=0.3)  # an int, an int, a float
    assert f.ranges == [(0, 2)] and tuple(f.z.shape) == (5, 2)
    assert torch.equal(f.scales, torch.tensor([0.3], dtype=torch.float32))
    f = make(noise_scale=0.3)  # one float for every range
    assert torch.equal(f.scales, torch.tensor([0.3, 0.3], dtype=torch.float32)) and tuple(f.z.shape) == (5, 4)


def test_graph_ptr_and_shapes_are_validated():
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, gp = _traj(3, [5, 4], 3, 2)
    for bad in ([1, 5, 9], [0, 5, 8], [0, 6, 5, 9], [0], [0, 5, 10]):
        with pytest.raises(ValueError, match="graph_ptr"):
            ResidentTrajectories(traj, bad, (0, 2), 2)
    assert ResidentTrajectories(traj, torch.tensor([0, 5, 5, 9]), (0, 2), 2).B == 3
    with pytest.raises(ValueError):
        ResidentTrajectories(traj[:1], gp, (0, 2), 2)  # one frame has no successor
    with pytest.raises(ValueError):
        ResidentTrajectories(traj.double(), gp, (0, 2), 2)
    with pytest.raises(ValueError):
        ResidentTrajectories(traj, gp, (2, 4), 2)
    with pytest.raises(ValueError):
        ResidentTrajectories(traj, gp, (0, 2), 3)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    for x, y in ((torch.zeros(9, 2), torch.zeros(9, 2)), (torch.zeros(8, 3), torch.zeros(8, 2)),
                 (torch.zeros(9, 3), torch.zeros(9, 3)), (torch.zeros(9, 3, dtype=torch.float64), torch.zeros(9, 2))):
        with pytest.raises(ValueError):
            feed.fill(_Batch(x, y))


def test_train_step_accepts_and_stores_a_feed():
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.step import TrainStep

    traj, gp = _traj(3, [5, 4], 3, 2)
    feed = ResidentTrajectories(traj, gp, (0, 2), 2)
    sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(2, 11, 3, 2, 8), torch.device("cpu"))
    opt = torch.optim.AdamW(sim.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, 10)
    batch = _Batch(torch.zeros(9, 3), torch.zeros(9, 2))
    assert TrainStep(sim, opt, sched, batch, graph=False, feed=feed).feed is feed
    assert TrainStep(sim, opt, sched, batch, graph=False).feed is None


def test_library_refuses_bad_arguments_without_a_device():
    """mgn_feed_batch checks its arguments on the host before any device work: a nonzero status and a message,
    here with null pointers (nothing is launched); no nodes is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    def call(T=3, N=10, F=6, B=2, ys=0, ye=2, ti=5, ranges=((0, 2), (3, 5)), n=None, ldz=8, ldx=8, ldy=2):
        rg = nat.feed_ranges(ranges)
        if n is not None:
            rg.n = n
        rc = nat.lib().mgn_feed_batch(None, T, N, F, None, B, None, ys, ye, ti, rg, None, None, ldz, None, ldx, None,
                                      ldy, None)
        return rc, nat.lib().mgn_last_error().decode()

    assert call(N=0)[0] == 0 and call(B=0)[0] == 0
    for kw in (dict(T=1), dict(F=0), dict(ranges=((0, 2), (3, 7))), dict(ranges=((-1, 2),)), dict(ranges=((2, 1),)),
               dict(ranges=((0, 2), (1, 5))), dict(ye=7), dict(ys=-1), dict(ys=3, ye=2), dict(ti=6), dict(ti=-1),
               dict(n=5), dict(n=-1), dict(ldx=5), dict(ldy=1), dict()):  # the last: valid but null pointers
        rc, msg = call(**kw)
        assert rc != 0 and "feed_batch" in msg, (kw, rc, msg)
    with pytest.raises(ValueError):
        nat.feed_ranges([(0, 1)] * 5)
