"""World edges and random long-range edges in one topology, on the CPU: dataset.resident.world_random_topology_torch
against a brute-force union (the world pairs by a plain loop in fp64, the random lists by test_random_edges_cpu's literal
walk over the mesh ∪ world adjacency); a feed built with dynamic_edges= and random_edges= on CPU tensors; what it
refuses; the new symbols and the C-side refusals, which need no device.

Everything here is integer work (plus one fp64 comparison per pair): every comparison is exact."""
import ctypes

import pytest
import torch

import _world_edges as WE
import test_random_edges_cpu as RC

SIZES = [1, 2, 37, 300, 5]


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------------------------------------- helpers (GPU tests too)
def brute_world(pos, types, gp, radius):
    """The directed world edges [2, E_w] of every graph, by a plain loop: i, j of one graph, one NORMAL (0) and one
    OBSTACLE (1), (v0·v0 + v1·v1) + v2·v2 <= radius² on Python floats (fp64) from the fp32 positions."""
    p, t, r2 = pos[:, 0:3].double().tolist(), types.tolist(), float(radius) * float(radius)
    out = []
    for a, b in zip(gp, gp[1:]):
        for i in range(a, b):
            if t[i] not in (0.0, 1.0):
                continue
            for j in range(a, b):
                if t[j] not in (0.0, 1.0) or t[j] == t[i]:
                    continue
                v0, v1, v2 = p[i][0] - p[j][0], p[i][1] - p[j][1], p[i][2] - p[j][2]
                if (v0 * v0 + v1 * v1) + v2 * v2 <= r2:
                    out.append((i, j))
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2).t().contiguous()


def world_union(pos, types, gp, mesh, radius):
    """(mesh ∪ world edge_index sorted by (row, col), the largest number of world neighbours — pairs that are no mesh
    edges — of one node)."""
    N = gp[-1]
    w = brute_world(pos, types, gp, radius)
    mkey = mesh[0] * N + mesh[1]
    wkey = w[0] * N + w[1]
    wkey = wkey[~torch.isin(wkey, mkey)]
    deg = int(torch.bincount(torch.div(wkey, N, rounding_mode="floor"), minlength=N).max()) if wkey.numel() else 0
    key = torch.sort(torch.cat([mkey, wkey])).values
    return torch.stack([torch.div(key, N, rounding_mode="floor"), key % N]), deg


def draw(C, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2 ** 31 - 1, (C, 2), generator=g, dtype=torch.int64).to(torch.int32).to(dev)


def case(seed, ratio=1.0, sizes=SIZES, obstacles=False, **kw):
    """WE.random_case plus the candidate offsets at `ratio` (counted from the mesh) and the brute-force mesh ∪ world
    adjacency with its largest world degree. obstacles: the first node of every graph is made an OBSTACLE, which a
    world_pos= feed asks of every graph."""
    from graphphysics.dataset.resident import random_candidate_ptr

    pos, types, gp, mesh, radius = WE.random_case(sizes, seed, **kw)
    if obstacles:
        types[[a for a, b in zip(gp, gp[1:]) if b > a]] = 1.0
    ei_w, deg = world_union(pos, types, gp, mesh, radius)
    return dict(pos=pos, types=types, gp=gp, mesh=mesh, radius=radius, cp=random_candidate_ptr(gp, mesh, ratio),
                ei_w=ei_w, deg=deg)


def brute_union(c, pairs, max_new, enabled=True):
    """mesh ∪ world ∪ random by brute force: the literal walk of the random rule over the mesh ∪ world adjacency.
    Returns (edge_index, the random lists)."""
    lists, _ = RC.literal_rule(pairs.tolist(), c["gp"], c["cp"], c["ei_w"], max_new, enabled)
    return RC.edge_index_of(lists, c["ei_w"], c["gp"][-1]), lists


def combined_feed(traj, gp, mesh, W=16, ratio=0.5, max_new=8, radius=0.03, **kw):
    from graphphysics.dataset.resident import ResidentTrajectories

    return ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=WE.world_pos(),
                                dynamic_edges={"edge_index": mesh, "radius": radius, "max_neighbors": W},
                                random_edges={"edge_index": mesh, "ratio": ratio, "max_new": max_new},
                                one_topology=True, **kw)


def batch_of(feed, dev="cpu"):
    return _Batch(x=torch.zeros(feed.N, feed.Fx, device=dev), y=torch.zeros(feed.N, 3, device=dev),
                  edge_index=feed.edge_index, edge_attr=None, pos=None)


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("max_new", [1, 2, 16, 64])
def test_torch_rule_equals_the_brute_force_union(max_new):
    from graphphysics.dataset.resident import world_random_topology_torch

    for seed in (1, 2):
        c = case(seed)
        N, C = c["gp"][-1], c["cp"][-1]
        assert c["deg"] >= 2 and C > 300
        pairs = draw(C, 10 + seed)
        # half of the big graph's candidates are world edges of this build and mesh edges: both must be discarded
        mkey = c["mesh"][0] * N + c["mesh"][1]
        world = c["ei_w"][:, ~torch.isin(c["ei_w"][0] * N + c["ei_w"][1], mkey)]
        lo = c["gp"][3]
        world = world[:, world[0] >= lo] - lo
        assert world.shape[1] >= 20
        at = c["cp"][3]
        pairs[at:at + 20] = world[:, :20].t().int()
        ei, arrays = world_random_topology_torch(c["pos"], c["types"], pairs, c["gp"], c["mesh"], c["radius"],
                                                 max(c["deg"], 1), max_new, cand_ptr=c["cp"])
        want, lists = brute_union(c, pairs, max_new)
        assert torch.equal(ei, want)
        key = ei[0] * N + ei[1]
        assert bool((key[1:] > key[:-1]).all())  # sorted by (row, col), every edge once
        assert torch.equal(torch.sort(ei[1] * N + ei[0]).values, key)  # symmetric
        assert not bool((ei[0] == ei[1]).any())
        # no random edge is a mesh or world edge, and no node gains more than max_new
        wkey = c["ei_w"][0] * N + c["ei_w"][1]
        new = key[~torch.isin(key, wkey)]
        assert new.numel() == sum(len(L) for L in lists) > 0
        assert key.numel() == wkey.numel() + new.numel()
        assert int(torch.bincount(torch.div(new, N, rounding_mode="floor"), minlength=N).max()) <= max_new
        stable = WE.stable_arrays(ei, N)
        for k in WE.ARRAYS:
            assert arrays[k].dtype == torch.int32 and torch.equal(arrays[k], stable[k]), k
        # switched off: step 1's result
        off, _ = world_random_topology_torch(c["pos"], c["types"], pairs, c["gp"], c["mesh"], c["radius"],
                                             max(c["deg"], 1), max_new, False, cand_ptr=c["cp"])
        assert torch.equal(off, c["ei_w"])


def test_capacity_is_the_world_rule_s_and_max_new_raises_nothing():
    from graphphysics.dataset.resident import world_random_topology_torch

    c = case(3)
    pairs = draw(c["cp"][-1], 5)
    with pytest.raises(ValueError, match="max_neighbors"):
        world_random_topology_torch(c["pos"], c["types"], pairs, c["gp"], c["mesh"], c["radius"], c["deg"] - 1, 16,
                                    cand_ptr=c["cp"])
    lo, n = c["gp"][3], 300
    pairs[c["cp"][3]:c["cp"][4], 0] = 17  # every candidate of the big graph on one node: far over max_new
    ei, _ = world_random_topology_torch(c["pos"], c["types"], pairs, c["gp"], c["mesh"], c["radius"], c["deg"], 2,
                                        cand_ptr=c["cp"])
    assert torch.equal(ei, brute_union(c, pairs, 2)[0])
    assert int((ei[0] == lo + 17).sum()) == int((c["ei_w"][0] == lo + 17).sum()) + 2


# ---------------------------------------------------------------------------------------------- the feed
def test_cpu_feed_fills_the_combined_rule():
    """Constructing the feed with both on CPU tensors works, and fill writes the rule's edge_index: explicit pairs,
    drawn pairs, switched off, and build_edges on positions of the caller's."""
    from graphphysics.dataset.resident import world_random_topology_torch, world_topology_torch

    gold = WE.load_golden()
    traj, gp, mesh = WE.plate(gold)
    feed = combined_feed(traj, gp, mesh, frames=[3, 2])
    assert feed.dynamic and feed.random and feed.topology is None and feed.random_pairs is True
    N, E_m = feed.N, mesh.shape[1]
    assert tuple(feed.edge_index.shape) == (2, E_m + N * (16 + 8))
    C = feed.pairs.shape[0]
    assert C == feed._cand_list[-1] == 2 * (round(0.5 * (E_m // 2)) // 2)  # counted from the mesh edges alone
    batch = batch_of(feed)

    def rule(enabled=True):
        return world_random_topology_torch(batch.x, batch.x[:, WE.K + 3], feed.pairs, gp, mesh, 0.03, 16, 8, enabled,
                                           cand_ptr=feed._cand_list)

    pairs = draw(C, 1)
    feed.set_pairs(pairs)
    assert feed.fill(batch) is batch and torch.equal(feed.pairs, pairs)
    ei, arrays = rule()
    world = WE.ref_edge_index(gold, (3, 2))
    assert torch.equal(feed.current_edge_index(), ei) and ei.shape[1] > world.shape[1] + C
    for k in WE.ARRAYS:
        assert torch.equal(feed.topology_arrays[k], arrays[k]), k
    key, wkey = ei[0] * N + ei[1], world[0] * N + world[1]
    assert bool(torch.isin(wkey, key).all())  # the reference's world edges of these frames are all there
    # drawn pairs: new ones on every fill
    feed.set_pairs("random")
    torch.manual_seed(3)
    feed.fill(batch)
    first = feed.pairs.clone()
    assert not torch.equal(first, pairs) and torch.equal(feed.current_edge_index(), rule()[0])
    feed.fill(batch)
    assert not torch.equal(feed.pairs, first) and torch.equal(feed.current_edge_index(), rule()[0])
    # switched off: the reference's add_world_edges of these frames, a dynamic_edges= feed's result
    feed.set_random_edges(False)
    feed.fill(batch)
    assert torch.equal(feed.current_edge_index(), world)
    assert torch.equal(feed.current_edge_index(), world_topology_torch(batch.x, batch.x[:, WE.K + 3], gp, mesh, 0.03)[0])
    # build_edges: the combined build on other positions with the current pairs, nothing drawn
    feed.set_random_edges(True)
    held = feed.pairs.clone()
    pos = traj[0, :, 0:3].contiguous()
    feed.build_edges(pos, traj[0, :, WE.K])
    want, _ = world_random_topology_torch(pos, traj[0, :, WE.K], held, gp, mesh, 0.03, 16, 8, cand_ptr=feed._cand_list)
    assert torch.equal(feed.pairs, held) and torch.equal(feed.current_edge_index(), want)
    # a node over max_neighbors raises at once on CPU tensors, as for dynamic_edges=
    small = combined_feed(traj, gp, mesh, W=9, frames=[3, 3])
    with pytest.raises(ValueError, match="max_neighbors"):
        small.fill(batch_of(small))


def test_noise_comes_before_the_build():
    """The build reads the noisy x, as the reference's add_world_edges does: with a noise of the radius' size the world
    edges differ from the clean frame's, and they are the rule's on batch.x."""
    from graphphysics.dataset.resident import world_random_topology_torch

    gold = WE.load_golden()
    traj, gp, mesh = WE.plate(gold)
    noise = {"noise_index_start": [0], "noise_index_end": [3], "noise_scale": [0.01], "node_type_index": WE.K + 3}
    feed = combined_feed(traj, gp, mesh, W=64, noise=noise, frames=[3, 3])
    feed.set_random_edges(False)
    batch = batch_of(feed)
    torch.manual_seed(0)
    feed.fill(batch)
    got = feed.current_edge_index().clone()
    want, _ = world_random_topology_torch(batch.x, batch.x[:, WE.K + 3], feed.pairs, gp, mesh, 0.03, 64, 8, False,
                                          cand_ptr=feed._cand_list)
    clean = WE.ref_edge_index(gold, (3, 3))
    assert torch.equal(got, want) and (got.shape != clean.shape or not torch.equal(got, clean))


def test_refusals():
    from graphphysics.dataset.resident import ResidentTrajectories

    gold = WE.load_golden()
    traj, gp, mesh = WE.plate(gold)
    dyn = {"edge_index": mesh, "radius": 0.03, "max_neighbors": 16}
    ran = {"edge_index": mesh, "ratio": 0.5, "max_new": 8}

    def make(de=dyn, re=ran, wp=WE.world_pos(), **kw):
        kw.setdefault("one_topology", True)
        return ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=wp, dynamic_edges=de, random_edges=re, **kw)

    make(re=dict(ran, edge_index=mesh.clone()))  # equal, not identical
    # without the request the two together stay refused, as before; the request needs both
    with pytest.raises(ValueError, match="one_topology=True"):
        make(one_topology=False)
    for kw in (dict(de=None), dict(re=None)):
        with pytest.raises(ValueError, match="needs both"):
            make(**kw)
    other = mesh[:, (mesh[0] >= 2) & (mesh[1] >= 2)]  # still sorted, symmetric and unique
    for de, re in ((dict(dyn, edge_index=other), ran), (dyn, dict(ran, edge_index=other)),
                   (dyn, dict(ran, edge_index=mesh[:, :0]))):
        with pytest.raises(ValueError, match="same edge_index"):
            make(de, re)
    with pytest.raises(ValueError, match="rotate"):
        make(rotate={"feature_indices": [(0, 3)]})
    with pytest.raises(ValueError, match="aneurysm"):
        make(wp=None, aneurysm={"pos": torch.zeros(traj.shape[1], 3)})
    with pytest.raises(ValueError, match="world_pos"):
        make(wp=None)
    with pytest.raises(ValueError, match="edge_attr"):
        make(wp=dict(WE.world_pos(), edge_index=mesh, edge_attr_start=4))
    with pytest.raises(ValueError, match="max_new"):
        make(re=dict(ran, max_new=65))
    with pytest.raises(ValueError, match="max_neighbors"):
        make(de=dict(dyn, max_neighbors=0))
    feed = make()
    with pytest.raises(ValueError, match="build_edges"):
        feed.build_random_edges()
    # the rollout: "off" stays refused, the modes need the feed's own tensor
    from graphphysics.training.rollout import Rollout

    sim = WE.plate_transformer(torch.device("cpu")).eval()
    with pytest.raises(ValueError, match="dynamic_edges"):
        Rollout(sim, WE.K + 3, graph=False, feed=feed, world_edges="off").rollout_resident(batch_of(feed), 0, 2)


# ---------------------------------------------------------------------------------------------- the C side
def test_symbols_and_host_side_refusals():
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    lib = nat.load()
    size = lib.mgn_world_random_topology_workspace_bytes

    def al(n):
        return (n + 255) & ~255

    N, W, R, C = 1000, 16, 8, 3000
    assert size(N, W, R, C) == al(4 * N) + al(4 * N * W) + al(4 * N) + 2 * al(4 * N * R) + al(4 * C) + al(8 * C)
    assert size(0, 0, 0, 0) == size(1, 1, 1, 1) > 0
    one = ctypes.c_uint32()
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)

    def build(N=4, B=1, E_m=0, C=2, radius=0.1, W=4, R=4, ld_pos=3, ld_type=1, err=p, enabled=p, ws_bytes=1 << 20):
        return lib.mgn_world_random_topology_build(p, ld_pos, p, ld_type, p, p, C, p, B, N, p, p, E_m, radius, W, R,
                                                   enabled, p, p, p, p, p, p, p, p, err, p, ws_bytes, None)

    for kw, word in ((dict(W=0), b"max_neighbors"), (dict(R=0), b"max_new"), (dict(R=65), b"max_new"),
                     (dict(radius=0.0), b"radius"), (dict(radius=float("inf")), b"radius"), (dict(ld_pos=2), b"ld_pos"),
                     (dict(ld_type=0), b"ld_type"), (dict(C=-1), b">= 0"), (dict(N=-1), b">= 0"),
                     (dict(N=1 << 28, W=4, R=4, ws_bytes=1 << 40), b"int32"), (dict(err=None), b"error word"),
                     (dict(enabled=None), b"enabled"), (dict(ws_bytes=16), b"workspace"), (dict(B=0), b"B == 0"),
                     (dict(C=(1 << 30) + 1, ws_bytes=1 << 40), b"num_candidates")):
        assert build(**kw) != 0, kw
        assert word in lib.mgn_last_error(), (kw, lib.mgn_last_error())
    assert build(N=0, B=0, C=0) == 0  # no nodes: success without a launch
