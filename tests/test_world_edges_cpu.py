"""Per-frame world edges on the CPU (no kernels): dataset.resident.world_topology_torch against the reference's
own add_world_edges (tests/golden/world_edges_golden.npz, written by tests/golden/make_world_edges_golden.py) and
against a plain stable-sort restatement of mgn_topology_build; every refused dynamic_edges= configuration; the
capacity error; and the CPU paths of ResidentTrajectories.fill and Rollout.rollout_resident against the per-frame
host loop (add_world_edges per graph, then the step) on a torch transformer."""
import pytest
import torch

import _world_edges as WE
from _world_edges import K, N1


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def gold():
    return WE.load_golden()


@pytest.fixture(scope="module")
def plate(gold):
    return WE.plate(gold)


def test_torch_rule_gives_the_reference_edge_index_per_frame(gold):
    from graphphysics.dataset.resident import world_topology_torch

    types, mesh = gold["plate_type"], gold["plate_mesh"]
    for g in range(2):
        for f in range(4):
            ei, _ = world_topology_torch(gold["plate_pos"][g, f], types, [0, N1], mesh, gold["plate_radius"], 10)
            assert torch.equal(ei, gold[f"plate_ei_{g}_{f}"]), (g, f)
            assert ei.shape[1] - mesh.shape[1] == int(gold["plate_world_counts"][g, f])


def test_torch_rule_on_the_hand_made_graph(gold):
    """A pair at exactly the radius is linked, one an ulp beyond is not, a pair that is a mesh edge appears once,
    HANDLE and OBSTACLE–OBSTACLE pairs are never linked, the lonely node stays lonely: the reference's verdicts."""
    from graphphysics.dataset.resident import world_topology_torch

    ei, arrays = world_topology_torch(gold["hand_pos"], gold["hand_type"], [0, 12], gold["hand_mesh"],
                                      gold["hand_radius"], 2)
    assert torch.equal(ei, gold["hand_ei"])
    pairs = set(map(tuple, ei.t().tolist()))
    assert (0, 1) in pairs and (1, 0) in pairs and (0, 2) not in pairs and (0, 4) not in pairs
    assert int(((ei[0] == 0) & (ei[1] == 3)).sum()) == 1 and not bool((ei == 6).any())
    want = WE.stable_arrays(ei, 12)
    for k in WE.ARRAYS:
        assert torch.equal(arrays[k], want[k]), k


@pytest.mark.parametrize("frames", [(0, 0), (3, 2), (1, 3), (3, 3)])
def test_torch_rule_batched_never_links_two_graphs_and_its_arrays_are_the_stable_sort(gold, plate, frames):
    from graphphysics.dataset.resident import world_topology_torch

    traj, gp, mesh = plate
    pos = torch.cat([traj[frames[0], :N1, 0:3], traj[frames[1], N1:, 0:3]])
    ei, arrays = world_topology_torch(pos, traj[0, :, K], gp, mesh, gold["plate_radius"], 10)
    assert torch.equal(ei, WE.ref_edge_index(gold, frames))
    # the two plates overlap in space: a search across the whole batch would link them
    whole, _ = world_topology_torch(pos, traj[0, :, K], [0, 2 * N1], mesh, gold["plate_radius"])
    assert whole.shape[1] > ei.shape[1]
    want = WE.stable_arrays(ei, 2 * N1)
    for k in WE.ARRAYS:
        assert arrays[k].dtype == torch.int32 and torch.equal(arrays[k], want[k]), k
    assert torch.equal(arrays["row_ptr"], arrays["col_ptr"])


def test_capacity(gold, plate):
    """max_neighbors = 10 (the fixture's largest world in-degree) builds every frame; 9 raises on frame 3 (and builds
    the frames whose largest in-degree is below 10: 5, 5, 10, 10 in the first graph, 5, 5, 7, 10 in the second)."""
    from graphphysics.dataset.resident import world_topology_torch

    types, mesh = gold["plate_type"], gold["plate_mesh"]
    for f in range(4):
        world_topology_torch(gold["plate_pos"][0, f], types, [0, N1], mesh, 0.03, 10)
    for g, f in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2)):
        world_topology_torch(gold["plate_pos"][g, f], types, [0, N1], mesh, 0.03, 9)
    for g in range(2):
        with pytest.raises(ValueError, match="max_neighbors"):
            world_topology_torch(gold["plate_pos"][g, 3], types, [0, N1], mesh, 0.03, 9)
    # through the feed's CPU fill
    traj, gp, mesh2 = WE.plate(gold)
    feed = WE.dyn_feed(traj, gp, mesh2, W=9, frames=[1, 2])
    batch = _Batch(x=torch.zeros(2 * N1, 7), y=torch.zeros(2 * N1, 3), edge_index=feed.edge_index, edge_attr=None)
    feed.fill(batch)
    feed.set_frames([3, 0])
    with pytest.raises(ValueError, match="max_neighbors"):
        feed.fill(batch)


def _swap(mesh, i, j):
    m = mesh.clone()
    m[:, [i, j]] = m[:, [j, i]]
    return m


def test_every_refused_configuration_raises(plate):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    traj, gp, mesh = plate
    ok = {"edge_index": mesh, "radius": 0.03, "max_neighbors": 10}

    def make(de=ok, wp=None, **kw):
        return ResidentTrajectories(traj, gp, (0, 3), K, world_pos=WE.world_pos() if wp is None else wp,
                                    dynamic_edges=de, **kw)

    make()
    cross = torch.cat([mesh, torch.tensor([[N1 - 1, N1], [N1, N1 - 1]])], dim=1)  # sorted, symmetric, across graphs
    cross = cross[:, torch.argsort(cross[0] * 2 * N1 + cross[1])]
    with pytest.raises(ValueError, match="different graphs"):
        make(dict(ok, edge_index=cross))
    bad_meshes = {
        "asymmetric": mesh[:, 1:],
        "unsorted": _swap(mesh, 0, 1),
        "duplicate": torch.cat([mesh[:, :1], mesh], dim=1),
        "self-loop": torch.cat([torch.zeros(2, 1, dtype=torch.int64), mesh], dim=1),
        "across graphs": cross,
        "out of range": torch.cat([mesh, torch.tensor([[2 * N1], [2 * N1 + 1]])], dim=1),
        "float": mesh.float(),
    }
    for name, m in bad_meshes.items():
        with pytest.raises(ValueError):
            make(dict(ok, edge_index=m))
            pytest.fail(name)
    for bad in (dict(ok, radius=0.0), dict(ok, radius=-1.0), dict(ok, radius=float("nan")),
                dict(ok, radius=float("inf")), dict(ok, max_neighbors=0), dict(ok, max_neighbors=2.5),
                dict(ok, extra=1), {"edge_index": mesh, "radius": 0.03}, "yes"):
        with pytest.raises(ValueError):
            make(bad)
    with pytest.raises(ValueError, match="rotate"):
        ResidentTrajectories(traj, gp, (0, 3), K, dynamic_edges=ok, rotate={"feature_indices": [(0, 3)]})
    with pytest.raises(ValueError, match="aneurysm"):
        ResidentTrajectories(traj, gp, (0, 3), K, dynamic_edges=ok, aneurysm={"pos": torch.zeros(2 * N1, 3)})
    with pytest.raises(ValueError, match="world_pos"):
        ResidentTrajectories(traj, gp, (0, 3), K, dynamic_edges=ok)
    with pytest.raises(ValueError, match="edge_attr"):
        make(wp=dict(WE.world_pos(), edge_index=mesh, edge_attr_start=4))
    # the rollout: "off" and None have no adjacency to fall back to
    sim = WE.plate_transformer(torch.device("cpu")).eval()
    for mode in ("off", None):
        with pytest.raises(ValueError):
            Rollout(sim, K + 3, graph=False, feed=make(), world_edges=mode)
    feed = make()
    ro = Rollout(sim, K + 3, graph=False, feed=feed, world_edges="frame")
    other = _Batch(x=torch.zeros(2 * N1, 7), y=torch.zeros(2 * N1, 3), edge_index=mesh, edge_attr=None, pos=None)
    with pytest.raises(ValueError, match="feed.edge_index"):
        ro.rollout_resident(other, 0, 1)
    # a feed without dynamic_edges= behaves as before
    plain = ResidentTrajectories(traj, gp, (0, 3), K, world_pos=WE.world_pos())
    assert plain.dynamic is False and plain.edge_index is None and plain.topology is None
    with pytest.raises(ValueError):
        plain.build_edges(traj[0], traj[0, :, K])


NOISE = {"noise_index_start": [0], "noise_index_end": [3], "noise_scale": [0.002], "node_type_index": K + 3}


def test_cpu_fill_matches_the_host_loop(gold, plate):
    """fill on CPU tensors: x and y by fill_world_torch, then the world edges of the NOISY x; the live columns of
    feed.edge_index are what the oracle's cKDTree restatement of add_world_edges gives per graph on that x, and a
    torch transformer on them gives the host loop's output bit for bit."""
    traj, gp, mesh = plate
    sim = WE.plate_transformer(torch.device("cpu")).eval()
    feed = WE.dyn_feed(traj, gp, mesh, W=16, noise=NOISE, frames=[0, 0])
    batch = _Batch(x=torch.zeros(2 * N1, 7), y=torch.zeros(2 * N1, 3), edge_index=feed.edge_index, edge_attr=None,
                   pos=None)
    keep = traj.clone()
    counts = []
    for seed, frames in ((1, (0, 0)), (2, (3, 2)), (3, (1, 3))):
        feed.set_frames(list(frames))
        torch.manual_seed(seed)
        feed.fill(batch)
        assert not torch.equal(batch.x[:N1, 0:3], traj[frames[0], :N1, 0:3])  # the noise is in
        want = WE.host_edges(batch.x, gp, mesh)
        got = feed.current_edge_index()
        assert int(feed.num_edges_dev) == want.shape[1] and torch.equal(got, want)
        arrays = WE.stable_arrays(want, 2 * N1)
        for k in WE.ARRAYS:
            assert torch.equal(feed.topology_arrays[k], arrays[k]), k
        with torch.no_grad():
            a = sim(_Batch(x=batch.x, y=batch.y, edge_index=got, edge_attr=None, pos=None))[2]
            b = sim(_Batch(x=batch.x, y=batch.y, edge_index=want.clone(), edge_attr=None, pos=None))[2]
        assert torch.equal(a, b)
        counts.append(want.shape[1])
    assert len(set(counts)) > 1 and torch.equal(traj, keep)
    # a zero noise scale: the fixture's counts
    feed.set_noise_t(1.0)
    feed.set_frames([3, 2])
    feed.fill(batch)
    assert int(feed.num_edges_dev) == WE.ref_counts(gold, (3, 2))
    assert torch.equal(feed.current_edge_index(), WE.ref_edge_index(gold, (3, 2)))


@pytest.mark.parametrize("mode", ["frame", "prediction"])
def test_cpu_resident_rollout_equals_the_host_loop(gold, plate, mode):
    from graphphysics.training.rollout import Rollout

    traj, gp, mesh = plate
    sim = WE.plate_transformer(torch.device("cpu")).eval()
    want, old, counts, _ = WE.rollout_host_loop(sim, traj, gp, mesh, [0, 0], 3, mode)
    feed = WE.dyn_feed(traj, gp, mesh, W=16)
    ro = Rollout(sim, K + 3, graph=False, feed=feed, world_edges=mode)
    batch = _Batch(x=torch.zeros(2 * N1, 7), y=torch.zeros(2 * N1, 3), edge_index=feed.edge_index, edge_attr=None,
                   pos=None)
    got = ro.rollout_resident(batch, 0, 3)
    assert torch.equal(got, want)
    assert torch.equal(torch.stack(ro.losses), torch.stack(old.losses))
    assert ro.resident_num_edges.tolist() == counts
    if mode == "frame":
        assert counts == [WE.ref_counts(gold, (s, s)) for s in range(3)]
    # other start frames, per graph
    want2, _, counts2, _ = WE.rollout_host_loop(sim, traj, gp, mesh, [1, 0], 2, mode)
    assert torch.equal(ro.rollout_resident(batch, [1, 0], 2), want2)
    assert ro.resident_num_edges.tolist() == counts2


def test_bad_raw_arguments_are_refused_before_any_launch():
    """mgn_world_topology_build's host-side refusals, through ctypes with fake non-NULL addresses that are never
    dereferenced: nothing is launched, so this needs no device. N == 0 is success."""
    import ctypes

    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    L = nat.load()
    p = ctypes.c_void_p(4096)  # non-NULL, never read: every case below returns before the first launch

    def call(N=10, B=1, E_m=4, radius=0.03, W=4, ld_pos=7, ld_type=7, pos=p, err=p, ws_bytes=None, num_edges=p):
        if ws_bytes is None:
            ws_bytes = L.mgn_world_topology_workspace_bytes(N, W)
        return L.mgn_world_topology_build(pos, ld_pos, p, ld_type, p, B, N, p, p, E_m, radius, W, p, p, p, p, p, p, p,
                                          num_edges, err, p, ws_bytes, None)

    assert call(N=0, B=0, E_m=0) == 0  # no nodes: success without a launch
    for kw, text in ((dict(W=0), b"max_neighbors"), (dict(W=-3), b"max_neighbors"), (dict(radius=0.0), b"radius"),
                     (dict(radius=-0.03), b"radius"), (dict(radius=float("nan")), b"radius"),
                     (dict(radius=float("inf")), b"radius"), (dict(ld_pos=2), b"ld_pos"), (dict(ld_type=0), b"ld_type"),
                     (dict(N=-1), b">= 0"), (dict(E_m=-1), b">= 0"), (dict(B=0), b"B == 0"),
                     (dict(N=2 ** 30 + 1, ws_bytes=2 ** 40), b"2^30"), (dict(N=2 ** 28, W=16, ws_bytes=2 ** 40), b"int32"),
                     (dict(pos=None), b"null pointer"), (dict(err=None), b"error word"),
                     (dict(num_edges=None), b"null pointer"), (dict(ws_bytes=16), b"workspace")):
        assert call(**kw) != 0, kw
        assert text.lower() in L.mgn_last_error().lower(), (kw, L.mgn_last_error())
    assert L.mgn_world_topology_workspace_bytes(1000, 16) >= 1000 * 4 + 1000 * 16 * 4
    with pytest.raises(ValueError, match="max_neighbors"):
        nat._raise_for(nat.ERR_WORLD_CAPACITY | (2 << nat.ERR_SKIP_SHIFT))
    assert nat.ERR_WORLD_CAPACITY & nat.ERR_ANY
