"""Aneurysm features in the resident feed on the CPU (no kernels): graphphysics.external.aneurysm and
ResidentTrajectories(aneurysm=...) through its torch path (dataset.resident.inflow_stats_torch /
fill_aneurysm_torch) against the reference's own build_features -> add_noise
(tests/golden/aneurysm_feed_golden.npz, written by tests/golden/make_aneurysm_feed_golden.py), the mean's two
bounds, hand-made value sets, the host-side refusals, the frame draw and the 8-entry noise struct.

Every column of the row but the mean is compared bit for bit. The mean is the fp64 sum of the distinct values in
ascending order divided by their count; the reference's is an fp32 torch.mean of unspecified order, whose
worst-case error is n·u·Σ|v| / n (u = 2^-24) plus the final rounding: the bound of the comparison with it."""
import math
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
U24, U53 = 2.0 ** -24, 2.0 ** -53
CONFIG_NOISE = {"noise_index_start": [0, 1, 2, 4, 5, 6], "noise_index_end": [1, 2, 3, 5, 6, 7],
                "noise_scale": [10.0, 10.0, 1.0, 10.0, 10.0, 1.0]}  # coarse-aneurysm.json


class _Batch:
    def __init__(self, x, y, **kw):
        self.x, self.y = x, y
        for k, v in kw.items():
            setattr(self, k, v)


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(G, "aneurysm_feed_golden.npz"))
    d = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k] for k in z.files}
    d["ranges"] = [tuple(int(v) for v in r) for r in z["ranges"]]
    d["scales"] = [float(s) for s in z["scales"]]
    return d


def gold_feed(gold, dev="cpu"):
    """The fixture as a feed: T = 3, one graph, frame 1."""
    from graphphysics.dataset.resident import ResidentTrajectories

    traj = torch.stack([gold["prev_frame"], gold["frame"], gold["next_frame"]]).contiguous().to(dev)
    F = traj.shape[2]
    noise = {"noise_index_start": [s for s, _ in gold["ranges"]], "noise_index_end": [e for _, e in gold["ranges"]],
             "noise_scale": gold["scales"], "node_type_index": F + 9}
    feed = ResidentTrajectories(traj, [0, traj.shape[1]], (0, 3), F + 9, noise=noise, frames=[1],
                                aneurysm={"pos": gold["pos"].to(dev).contiguous()})
    return feed, traj


def mean_bound_ref(distinct, m_ref):
    """|mean − m_ref| allowed against the reference's fp32 torch.mean: 2^-24·|m_ref| + 2^-24·Σ|v|."""
    return U24 * abs(m_ref) + U24 * math.fsum(abs(v) for v in distinct)


def check_row(x, gold, which="x_out"):
    """x [48, 14] against the fixture: every column but the mean bit for bit, the mean within the derived bound."""
    want, F = gold[which], gold["frame"].shape[1]
    cols = [c for c in range(F + 10) if c != F + 6]
    assert torch.equal(x[:, cols], want[:, cols])
    m, m_ref = x[:, F + 6], float(want[0, F + 6])
    assert bool((m == m[0]).all())
    assert abs(float(m[0]) - m_ref) <= mean_bound_ref(gold["distinct"].tolist(), m_ref)


def test_fixture_through_the_torch_rules(gold):
    from graphphysics.dataset.resident import fill_aneurysm_torch
    from graphphysics.external.aneurysm import aneurysm_node_type, build_features
    from graphphysics.utils.data import Data

    F = gold["frame"].shape[1]
    g = Data(x=gold["frame"].clone(), y=gold["next_frame"][:, 0:3].clone(), pos=gold["pos"].clone(),
             previous_data={"Vitesse": gold["prev_frame"][:, 0:3].numpy().copy()})
    assert torch.equal(aneurysm_node_type(g), gold["node_type"])
    assert aneurysm_node_type(g).dtype == torch.float32
    g = build_features(g)
    assert tuple(g.x.shape) == (48, F + 10)
    check_row(g.x, gold, "x_clean")
    # previous_data as a tensor [N, >= 3]: the same row
    g2 = build_features(Data(x=gold["frame"].clone(), y=gold["next_frame"].clone(), pos=gold["pos"].clone(),
                             previous_data=gold["prev_frame"].clone()))
    assert torch.equal(g2.x, g.x)

    feed, traj = gold_feed(gold)
    keep = traj.clone()
    assert torch.equal(feed.node_type, gold["node_type"])
    x, y = fill_aneurysm_torch(traj, [0, 48], feed.frame, feed.pos, feed.node_type, feed.inflow_stats, (0, 3),
                               feed.ranges, feed.scales, gold["z"])
    check_row(x, gold, "x_out")
    assert torch.equal(y, gold["next_frame"][:, 0:3])
    xc, _ = fill_aneurysm_torch(traj, [0, 48], feed.frame, feed.pos, feed.node_type, feed.inflow_stats, (0, 3),
                                [], None, None)
    assert torch.equal(xc, g.x)  # the fill's clean row is build_features' row, the mean included
    assert torch.equal(traj, keep)


def test_fill_on_cpu_tensors_writes_the_row_and_leaves_the_stored_data_clean(gold):
    feed, traj = gold_feed(gold)
    keep, keep_pos = traj.clone(), feed.pos.clone()
    F = traj.shape[2]
    b = _Batch(torch.full((48, F + 12), SENTINEL), torch.zeros(48, 3))
    seen = []
    for _ in range(3):
        feed.fill(b)
        seen.append(b.x.clone())
        assert bool((b.x[:, F + 10:] == SENTINEL).all())
        assert torch.equal(b.y, gold["next_frame"][:, 0:3])
        other = gold["node_type"] != 0
        clean_cols = [c for c in range(F + 10) if c != F + 6]
        assert torch.equal(b.x[other][:, clean_cols], gold["x_clean"][other][:, clean_cols])
    noisy = [0, 1, 2, 4, 5, 6]
    normal = gold["node_type"] == 0
    for a, c in zip(seen, seen[1:]):
        assert not torch.equal(a[normal][:, noisy], c[normal][:, noisy])
        assert torch.equal(a[:, 7:F + 10], c[:, 7:F + 10]) and torch.equal(a[:, 3], c[:, 3])
    assert torch.equal(traj, keep) and torch.equal(feed.pos, keep_pos)


def test_mean_is_within_the_derived_bound_of_the_reference(gold):
    from graphphysics.dataset.resident import inflow_stats_torch

    F = gold["frame"].shape[1]
    s = inflow_stats_torch(gold["frame"], gold["next_frame"], gold["node_type"] == 4)
    assert s.dtype == torch.float32 and tuple(s.shape) == (3,)
    ref = gold["x_clean"][0, F + 6:F + 9]
    assert torch.equal(s[1:], ref[1:])  # min and max: exact
    distinct = gold["distinct"].tolist()
    bound = mean_bound_ref(distinct, float(ref[0]))
    print(f"mean {float(s[0])!r}, reference {float(ref[0])!r}, bound {bound:.3e}")
    assert abs(float(s[0]) - float(ref[0])) <= bound


def _fsum_check(cur, nxt, mask):
    """inflow_stats_torch against math.fsum over the distinct set: |got − m| <= 2^-24·|m| + n·2^-53·Σ|v|."""
    from graphphysics.dataset.resident import inflow_stats_torch

    got = inflow_stats_torch(cur, nxt, mask)
    d = (nxt[:, 0:3] - cur[:, 0:3])[mask].reshape(-1).tolist()
    if not bool(mask.all()):
        d.append(0.0)
    distinct = sorted(set(float(v) + 0.0 for v in d))  # -0.0 == 0.0: one member
    n = len(distinct)
    m = math.fsum(distinct) / n
    assert abs(float(got[0]) - m) <= U24 * abs(m) + n * U53 * math.fsum(abs(v) for v in distinct)
    assert float(got[1]) == distinct[0] and float(got[2]) == distinct[-1]
    return got, distinct


def test_exact_mean_against_fsum(gold):
    _fsum_check(gold["frame"], gold["next_frame"], gold["node_type"] == 4)
    g = torch.Generator().manual_seed(3)
    for n, m in ((1, 1), (70, 70), (600, 200), (2000, 1365)):
        cur, nxt = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g) * 100.0
        mask = torch.zeros(n, dtype=torch.bool)
        mask[torch.randperm(n, generator=g)[:m]] = True
        nxt[: n // 3, 0:3] = cur[: n // 3, 0:3] + 0.5  # many equal differences
        _, distinct = _fsum_check(cur, nxt, mask)
        assert len(distinct) <= 3 * m + 1


def _stats(values_per_row, inflow):
    """inflow_stats_torch on rows whose next − current is `values_per_row` (current is zero)."""
    from graphphysics.dataset.resident import inflow_stats_torch

    nxt = torch.zeros(len(values_per_row), 4)
    nxt[:, 0:3] = torch.tensor(values_per_row, dtype=torch.float32)
    return inflow_stats_torch(torch.zeros_like(nxt), nxt, torch.tensor(inflow))


def test_hand_made_value_sets():
    # {1, 1, 2} on one inflow row plus the masked zero of the other row: the distinct set is {0, 1, 2}
    s = _stats([[1.0, 1.0, 2.0], [9.0, 9.0, 9.0]], [True, False])
    assert s.tolist() == [(0.0 + 1.0 + 2.0) / 3, 0.0, 2.0] and s.tolist()[0] == 1.0
    # the same values with every node inflow: no zero in the set, {1, 2}
    s = _stats([[1.0, 1.0, 2.0]], [True])
    assert s.tolist() == [1.5, 1.0, 2.0]
    # a plain mean of the four gathered values would be 1.0 too, by accident of counts: {1, 1, 4} + zero differs
    s = _stats([[1.0, 1.0, 4.0], [9.0, 9.0, 9.0]], [True, False])
    assert s.tolist() == [np.float32(5.0 / 3.0), 0.0, 4.0]
    # no inflow node
    assert _stats([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [False, False]).tolist() == [0.0, 0.0, 0.0]
    # all nodes inflow: no zero
    s = _stats([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [True, True])
    assert s.tolist() == [3.5, 1.0, 6.0]
    # -0.0 and 0.0 merge, and with the masked zero: {-1, 0, 2}
    s = _stats([[-0.0, 0.0, 2.0], [-1.0, -0.0, 0.0], [7.0, 7.0, 7.0]], [True, True, False])
    assert s.tolist() == [np.float32(1.0 / 3.0), -1.0, 2.0]
    s = _stats([[-0.0, 0.0, -0.0]], [True])
    assert s.tolist() == [0.0, 0.0, 0.0] and not bool(torch.signbit(s).any())


# ------------------------------------------------------------------------------------------------ refusals
def _args(T=4, n=6, F=4):
    g = torch.Generator().manual_seed(0)
    traj = torch.randn(T, n, F, generator=g)
    traj[:, :, 3:4] = 0.0
    pos = torch.randn(n, 3, generator=g)
    pos[0, 1], pos[0, 0] = 0.0, -1.0
    return traj, pos.contiguous()


def _feed(traj, pos, noise=None, **kw):
    from graphphysics.dataset.resident import ResidentTrajectories

    F = traj.shape[2]
    kw.setdefault("aneurysm", {"pos": pos})
    return ResidentTrajectories(traj, [0, traj.shape[1]], (0, 3), kw.pop("node_type_index", F + 9), noise=noise, **kw)


def test_refuses_rotate_together_with_aneurysm():
    traj, pos = _args()
    with pytest.raises(ValueError, match="aneurysm= together with rotate= or world_pos="):
        _feed(traj, pos, rotate={"feature_indices": [(0, 3)]})


def test_refuses_world_pos_together_with_aneurysm():
    traj, pos = _args()
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6}
    with pytest.raises(ValueError, match="aneurysm= together with rotate= or world_pos="):
        _feed(traj, pos, world_pos=wp)


def test_refuses_unknown_keys():
    traj, pos = _args()
    with pytest.raises(ValueError, match="aneurysm must be a dict with keys among"):
        _feed(traj, pos, aneurysm={"pos": pos, "velocity": 3})
    with pytest.raises(ValueError, match="aneurysm must be a dict with keys among"):
        _feed(traj, pos, aneurysm={})


@pytest.mark.parametrize("bad", ["shape", "dtype", "device", "not_a_tensor"])
def test_refuses_a_pos_of_another_shape_dtype_or_device(bad):
    traj, pos = _args()
    wrong = {"shape": pos[:, :2].contiguous(), "dtype": pos.double(), "device": pos.to("meta"),
             "not_a_tensor": pos.tolist()}[bad]
    with pytest.raises(ValueError, match=r"aneurysm pos must be a contiguous fp32 \[6, 3\] tensor on cpu"):
        _feed(traj, pos, aneurysm={"pos": wrong})


def test_refuses_narrow_frames():
    traj, pos = _args(F=3)
    with pytest.raises(ValueError, match="F = 3 >= 4"):
        _feed(traj, pos)


def test_refuses_two_frames():
    traj, pos = _args(T=2)
    with pytest.raises(ValueError, match="at least 3 frames"):
        _feed(traj, pos)


def test_refuses_a_node_type_index_that_is_not_the_last_batch_column():
    traj, pos = _args()
    with pytest.raises(ValueError, match=r"must be the batch column F \+ 9 = 13"):
        _feed(traj, pos, node_type_index=3)
    with pytest.raises(ValueError, match="noise node_type_index 3 differs from node_type_index 13"):
        _feed(traj, pos, noise=dict(CONFIG_NOISE, node_type_index=3))


def test_refuses_a_noisy_range_that_contains_the_type_column():
    traj, pos = _args()
    noise = {"noise_index_start": [0, 12], "noise_index_end": [3, 14], "noise_scale": [1.0, 1.0], "node_type_index": 13}
    with pytest.raises(ValueError, match=r"a noisy column range contains the node type \(batch column 13\)"):
        _feed(traj, pos, noise=noise)


def test_refuses_a_graph_whose_value_set_exceeds_the_capacity():
    from graphphysics import _native as nat

    cap = nat.MGN_FEED_INFLOW_CAPACITY
    assert cap >= 4096
    m = cap // 3 + 1  # 3·m > cap
    n = m + 2
    traj = torch.zeros(3, n, 4)
    pos = torch.ones(n, 3)
    pos[:m, 1], pos[:m, 0] = 0.0, -1.0
    with pytest.raises(ValueError, match=f"exceeds the capacity of {cap} values"):
        _feed(traj, pos)
    # one inflow node fewer fits: 3·(m − 1) + 1 <= cap
    pos[m - 1, 1] = 1.0
    assert 3 * (m - 1) + 1 <= cap
    feed = _feed(traj, pos)
    assert tuple(feed.inflow_stats.shape) == (2, 1, 3) and int(feed.inflow_ptr[1]) == m - 1


def test_rollout_refuses_an_aneurysm_feed():
    from graphphysics.training.rollout import Rollout

    class _Sim:
        output_index_start, output_index_end, device = 0, 3, "cpu"

    traj, pos = _args()
    with pytest.raises(ValueError, match="resident rollout of a feed built with aneurysm= is not supported yet.*later "
                                         "pull request"):
        Rollout(_Sim(), 13, feed=_feed(traj, pos))


def test_set_frames_refuses_frame_zero_and_the_last_frame():
    traj, pos = _args(T=5)
    feed = _feed(traj, pos)
    for bad in ([0], [4]):
        with pytest.raises(ValueError, match=r"frames must lie in \[1, 3\]"):
            feed.set_frames(bad)
    with pytest.raises(ValueError, match=r"frames must lie in \[1, 3\]"):
        _feed(traj, pos, frames=[0])
    feed.set_frames([3])
    assert feed.frame.tolist() == [3]


def test_drawn_frames_stay_inside_1_and_T_minus_2():
    from graphphysics.dataset.resident import ResidentTrajectories

    T, F = 5, 4
    g = torch.Generator().manual_seed(1)
    traj = torch.randn(T, 9, F, generator=g)
    pos = torch.randn(9, 3, generator=g)
    feed = ResidentTrajectories(traj, [0, 4, 9], (0, 3), F + 9, aneurysm={"pos": pos})
    b = _Batch(torch.zeros(9, F + 10), torch.zeros(9, 3))
    torch.manual_seed(0)
    seen = set()
    for _ in range(200):
        feed.fill(b)
        fr = feed.frame.tolist()
        assert all(1 <= f <= T - 2 for f in fr)
        seen.update(fr)
        for gi, rows in enumerate((slice(0, 4), slice(4, 9))):
            assert torch.equal(b.x[rows, :F], traj[fr[gi], rows])
            assert torch.equal(b.x[rows, F:F + 3], traj[fr[gi], rows, 0:3] - traj[fr[gi] - 1, rows, 0:3])
            assert torch.equal(b.y[rows], traj[fr[gi] + 1, rows, 0:3])
    assert seen == {1, 2, 3}


def test_six_noise_ranges_are_accepted_here_and_refused_by_a_plain_feed():
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories

    traj, pos = _args()
    feed = _feed(traj, pos, noise=dict(CONFIG_NOISE, node_type_index=13))
    assert len(feed.ranges) == 6 and tuple(feed.z.shape) == (6, 6) and isinstance(feed._ranges_c, nat.FeedRanges8)
    assert feed._ranges_c.n == 6 and nat.MGN_FEED_ANEURYSM_MAX_RANGES == 8 and nat.MGN_FEED_MAX_RANGES == 4
    wide = torch.zeros(4, 6, 14)
    with pytest.raises(ValueError, match="at most 4 noisy column ranges are supported, got 6"):
        ResidentTrajectories(wide, [0, 6], (0, 3), 13, noise=dict(CONFIG_NOISE, node_type_index=13))
    nine = {"noise_index_start": list(range(9)), "noise_index_end": list(range(1, 10)), "noise_scale": [1.0] * 9,
            "node_type_index": 13}
    with pytest.raises(ValueError, match="at most 8 noisy column ranges are supported, got 9"):
        _feed(traj, pos, noise=nine)


def test_refresh_stats_recomputes_the_table():
    traj, pos = _args(T=4)
    feed = _feed(traj, pos)
    before = feed.inflow_stats.clone()
    assert tuple(before.shape) == (3, 1, 3)
    addr = feed.inflow_stats.data_ptr()
    traj[2, 0, 0:3] += 1.0  # node 0 is the inflow node
    feed.refresh_stats()
    assert feed.inflow_stats.data_ptr() == addr
    assert not torch.equal(feed.inflow_stats[1], before[1]) and not torch.equal(feed.inflow_stats[2], before[2])
    assert torch.equal(feed.inflow_stats[0], before[0])
