"""Random long-range edges on the CPU (no kernels): dataset.resident.random_topology_torch against hand-written
expectations and against a literal, node-by-node walk of the rule (literal_rule below); the drop rule at max_new = 1 and
2; the switch; every refused configuration; the distribution of the drawn edges through the CPU fill of a
random_edges= feed; the new symbols and the C-side refusals, which need no device.

Everything here is integer work: every comparison is exact."""
import ctypes
import os

import pytest
import torch

import _world_edges as WE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------------------------------------- helpers (GPU tests too)
def sym_mesh(und, N):
    """The sorted, symmetric, unique edge_index [2, E] of a list of unordered pairs."""
    if not und:
        return torch.zeros(2, 0, dtype=torch.int64)
    u = torch.tensor(und, dtype=torch.int64)
    key = torch.unique(torch.cat([u[:, 0] * N + u[:, 1], u[:, 1] * N + u[:, 0]]))
    return torch.stack([torch.div(key, N, rounding_mode="floor"), key % N])


def grid_mesh(nx, ny):
    """A triangulated nx × ny grid: every cell split along one diagonal."""
    und = []
    for i in range(nx):
        for j in range(ny):
            a = i * ny + j
            if j + 1 < ny:
                und.append((a, a + 1))
            if i + 1 < nx:
                und.append((a, a + ny))
            if i + 1 < nx and j + 1 < ny:
                und.append((a, a + ny + 1))
    return sym_mesh(und, nx * ny)


def literal_rule(pairs, gp, cp, mesh, W, enabled=True):
    """The rule walked as it is stated: per node, its graph's candidates in order, pass 1 with the flags, then pass 2.
    Returns (the new-neighbour list of every node, ascending; the flags)."""
    N, C = gp[-1], len(pairs)
    nbr = [set() for _ in range(N)]
    for r, c in mesh.t().tolist():
        nbr[r].add(c)
    flag = [0] * C
    lists = [[] for _ in range(N)]
    if not enabled:
        return lists, flag
    for g in range(len(gp) - 1):
        lo, n = gp[g], gp[g + 1] - gp[g]
        for i in range(lo, lo + n):
            L = []
            for c in range(cp[g], cp[g + 1]):
                a, b = lo + int(pairs[c][0]) % n, lo + int(pairs[c][1]) % n
                if i not in (a, b) or a == b:
                    continue
                j = b if a == i else a
                if j in nbr[i]:
                    continue
                if any(j == e for e, _ in L):
                    continue
                if len(L) == W:
                    flag[c] = 1
                else:
                    L.append((j, c))
            lists[i] = L
    return [sorted(j for j, c in L if not flag[c]) for L in lists], flag


def edge_index_of(lists, mesh, N):
    """The union of the mesh and the lists, sorted by (row, col)."""
    new = [(i, j) for i, L in enumerate(lists) for j in L]
    key = mesh[0] * N + mesh[1]
    if new:
        t = torch.tensor(new, dtype=torch.int64)
        key = torch.cat([key, t[:, 0] * N + t[:, 1]])
    key = torch.sort(key).values
    return torch.stack([torch.div(key, max(N, 1), rounding_mode="floor"), key % max(N, 1)])


def check_against_literal(pairs, gp, cp, mesh, W, enabled=True):
    """random_topology_torch equals the literal walk, and its arrays are mgn_topology_build's; returns its result."""
    from graphphysics.dataset.resident import random_topology_torch

    pairs = torch.as_tensor(pairs, dtype=torch.int32).reshape(-1, 2)
    N = gp[-1]
    ei, arrays = random_topology_torch(pairs, gp, mesh, W, enabled, cand_ptr=cp)
    lists, _ = literal_rule(pairs.tolist(), gp, cp, mesh, W, enabled)
    assert all(len(L) <= W for L in lists)
    for i, L in enumerate(lists):  # symmetric
        assert all(i in lists[j] for j in L)
    assert torch.equal(ei, edge_index_of(lists, mesh, N))
    want = WE.stable_arrays(ei, N)
    for k in WE.ARRAYS:
        assert arrays[k].dtype == torch.int32 and torch.equal(arrays[k], want[k]), k
    return ei, arrays, lists


def uneven_case(seed=5):
    """Graphs of 1, 0, 300 and 5 nodes with a random symmetric mesh inside each: a graph boundary inside a workgroup of
    256 nodes and a node range across the boundary between two workgroups. Returns (node offsets, mesh)."""
    _, _, gp, mesh, _ = WE.random_case(sizes=[1, 0, 300, 5], seed=seed)
    return gp, mesh


def plain_feed(gp, mesh, ratio, W, dev="cpu", T=3, **kw):
    """A plain resident feed (frame rows [velocity (3), node type]) with random_edges=."""
    from graphphysics.dataset.resident import ResidentTrajectories

    g = torch.Generator().manual_seed(gp[-1])
    traj = torch.cat([torch.randn(T, gp[-1], 3, generator=g), torch.zeros(T, gp[-1], 1)], dim=2).contiguous().to(dev)
    return ResidentTrajectories(traj, gp, (0, 3), 3, random_edges={"edge_index": mesh, "ratio": ratio, "max_new": W},
                                **kw)


def batch_of(feed, dev="cpu"):
    return _Batch(x=torch.zeros(feed.N, feed.Fx, device=dev), y=torch.zeros(feed.N, 3, device=dev),
                  edge_index=feed.edge_index, edge_attr=None, pos=None)


PATHS = sym_mesh([(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8)], 9)  # a path of 5 nodes and one of 4


# ---------------------------------------------------------------------------------------------- the rule
def test_hand_checked_case():
    """Graphs of 5 and 4 nodes (paths). Graph 0: a self-pair, a mesh edge, a new pair, its repeat, its reversed repeat,
    a pair whose modulo wraps (7 % 5 = 2, 14 % 5 = 4). Graph 1: a new pair, its repeat through a wrap (5 % 4 = 1), a
    second new pair. Node 2 ends with exactly max_new = 2 new neighbours: nothing is dropped."""
    pairs = [(0, 0), (0, 1), (0, 2), (0, 2), (2, 0), (7, 14), (1, 3), (5, 3), (0, 2)]
    gp, cp = [0, 5, 9], [0, 6, 9]
    ei, arrays, lists = check_against_literal(pairs, gp, cp, PATHS, 2)
    assert lists == [[2], [], [0, 4], [], [2], [7], [8], [5], [6]]
    new = {(0, 2), (2, 0), (2, 4), (4, 2), (6, 8), (8, 6), (5, 7), (7, 5)}
    assert set(map(tuple, ei.t().tolist())) == set(map(tuple, PATHS.t().tolist())) | new
    assert ei.shape[1] == PATHS.shape[1] + 8
    key = ei[0] * 9 + ei[1]
    assert bool((key[1:] > key[:-1]).all())  # sorted by (row, col), every edge once
    # mgn_topology_build's definition on that edge_index
    E = ei.shape[1]
    eid, perm = arrays["csc_eid"].long(), arrays["row_perm"].long()
    assert torch.equal(eid[perm], torch.arange(E)) and torch.equal(perm[eid], torch.arange(E))
    assert torch.equal(arrays["col_ptr"][1:] - arrays["col_ptr"][:-1], torch.bincount(ei[0], minlength=9).int())
    assert torch.equal(arrays["csc_src"].long(), ei[0][eid]) and torch.equal(arrays["csc_dst"].long(), ei[1][eid])
    assert torch.equal(arrays["row_ptr"], arrays["col_ptr"])


def test_drop_rule_at_max_new_1():
    """No mesh, one graph of 4 nodes, candidates (0,1), (1,2), (2,3) at max_new = 1: node 1 is full when (1,2) comes and
    flags it, which removes the entry node 2 had room for; node 2 is full (with that entry) when (2,3) comes and flags
    it, which removes node 3's. Only 0–1 survives."""
    none = torch.zeros(2, 0, dtype=torch.int64)
    ei, _, lists = check_against_literal([(0, 1), (1, 2), (2, 3)], [0, 4], [0, 3], none, 1)
    assert lists == [[1], [0], [], []] and ei.tolist() == [[0, 1], [1, 0]]
    # a repeat of a dropped pair is dropped again and changes nothing: (0,2) twice after (0,1)
    ei, _, lists = check_against_literal([(0, 1), (0, 2), (0, 2), (2, 3)], [0, 4], [0, 4], none, 1)
    assert lists == [[1], [0], [], []]
    _, flag = literal_rule([(0, 1), (0, 2), (0, 2), (2, 3)], [0, 4], [0, 4], none, 1)
    assert flag == [0, 1, 1, 1]


def test_drop_rule_at_max_new_2():
    """One graph of 5 nodes, no mesh, max_new = 2: node 0 takes 1 and 2 and flags (0,3); node 3 had appended 0 for it,
    takes 4, and is full when (3,1) comes: flagged, which removes the 3 node 1 had room for."""
    none = torch.zeros(2, 0, dtype=torch.int64)
    pairs = [(0, 1), (0, 2), (0, 3), (3, 4), (3, 1)]
    ei, _, lists = check_against_literal(pairs, [0, 5], [0, 5], none, 2)
    assert lists == [[1, 2], [0], [0], [4], [3]]
    assert literal_rule(pairs, [0, 5], [0, 5], none, 2)[1] == [0, 0, 1, 0, 1]
    # with room for everything nothing is dropped
    _, _, lists = check_against_literal(pairs, [0, 5], [0, 5], none, 3)
    assert lists == [[1, 2, 3], [0, 3], [0], [0, 1, 4], [3]]


@pytest.mark.parametrize("W", [1, 2, 3, 16])
def test_torch_rule_equals_the_literal_walk_on_random_cases(W):
    """Small graphs and many candidates, so that repeats, mesh hits, self-pairs and overflows all occur."""
    for seed in range(12):
        sizes = [[7, 0, 9], [1, 12], [30], [2, 3, 4]][seed % 4]
        _, _, gp, mesh, _ = WE.random_case(sizes=sizes, seed=seed)
        g = torch.Generator().manual_seed(100 + seed)
        cp = [0]
        for n in sizes:
            cp.append(cp[-1] + (0 if n < 2 else 3 * n))  # six endpoints a node: lists of 1 or 2 overflow
        pairs = torch.randint(0, 2 ** 31 - 1, (cp[-1], 2), generator=g, dtype=torch.int64).to(torch.int32)
        ei, _, lists = check_against_literal(pairs, gp, cp, mesh, W)
        if W <= 2 and seed % 4 == 2:
            assert sum(literal_rule(pairs.tolist(), gp, cp, mesh, W)[1]) > 0, "the case drops nothing"


def test_disabled_gives_the_mesh_exactly_and_tiny_graphs_get_no_candidates():
    from graphphysics.dataset.resident import random_candidate_ptr, random_topology_torch

    pairs = torch.tensor([(0, 2), (1, 3), (0, 2)], dtype=torch.int32)
    ei, arrays = random_topology_torch(pairs, [0, 5, 9], PATHS, 4, enabled=False, cand_ptr=[0, 2, 3])
    assert torch.equal(ei, PATHS)
    want = WE.stable_arrays(PATHS, 9)
    for k in WE.ARRAYS:
        assert torch.equal(arrays[k], want[k]), k
    on, _ = random_topology_torch(pairs, [0, 5, 9], PATHS, 4, cand_ptr=[0, 2, 3])
    assert on.shape[1] == PATHS.shape[1] + 6
    # C_g = round(ratio · E_g) // 2, and 0 for graphs of 0 or 1 nodes
    gp = [0, 1, 1, 6, 10]
    mesh = PATHS + 1  # the two paths behind a lonely node and an empty graph
    assert random_candidate_ptr(gp, mesh, 1.0) == [0, 0, 0, 4, 7]
    assert random_candidate_ptr(gp, mesh, 0.5) == [0, 0, 0, 2, 3]  # round(4) // 2, round(3) // 2
    assert random_candidate_ptr(gp, mesh, 0.3) == [0, 0, 0, 1, 2]  # round(2.4) // 2, round(1.8) // 2
    feed = plain_feed(gp, mesh, 1.0, 4)
    assert feed.cand_ptr.tolist() == [0, 0, 0, 4, 7] and tuple(feed.pairs.shape) == (7, 2)
    assert feed.pairs.dtype == torch.int32 and feed.random_enabled.tolist() == [1]
    assert tuple(feed.edge_index.shape) == (2, mesh.shape[1] + 10 * 4) and feed.edge_index.dtype == torch.int64


# ---------------------------------------------------------------------------------------------- the feed on CPU tensors
def test_cpu_fill_switch_and_explicit_pairs():
    from graphphysics.dataset.resident import random_topology_torch

    gp = [0, 5, 9]
    feed = plain_feed(gp, PATHS, 1.0, 2)
    assert feed.random is True and feed.dynamic is False and feed.random_pairs is True and feed.topology is None
    batch = batch_of(feed)
    torch.manual_seed(0)
    feed.fill(batch)
    first = feed.pairs.clone()
    assert int(first.min()) >= 0 and len(set(first.reshape(-1).tolist())) > 1
    want, arrays = random_topology_torch(first, gp, PATHS, 2, cand_ptr=feed.cand_ptr)
    assert torch.equal(feed.current_edge_index(), want) and int(feed.num_edges_dev) == want.shape[1]
    for k in WE.ARRAYS:
        assert torch.equal(feed.topology_arrays[k], arrays[k]), k
    feed.fill(batch)
    assert not torch.equal(feed.pairs, first)  # consecutive fills draw anew
    # explicit pairs stay until "random" comes back
    C = feed.pairs.shape[0]
    mine = torch.arange(2 * C).reshape(C, 2)
    feed.set_pairs(mine)
    assert feed.random_pairs is False
    feed.fill(batch)
    feed.fill(batch)
    assert torch.equal(feed.pairs, mine.int())
    assert torch.equal(feed.current_edge_index(), random_topology_torch(mine, gp, PATHS, 2, cand_ptr=feed.cand_ptr)[0])
    # off: the mesh; the documented recipe for validation needs no fill
    feed.set_random_edges(False)
    feed.build_random_edges()
    assert torch.equal(feed.current_edge_index(), PATHS)
    feed.fill(batch)
    assert torch.equal(feed.current_edge_index(), PATHS)
    feed.set_random_edges(True)
    feed.set_pairs("random")
    feed.fill(batch)
    assert feed.random_pairs is True and not torch.equal(feed.pairs, mine.int())


def test_distribution_on_a_small_graph():
    """A ring of 12 nodes beside a ring of 7, ratio 1.0, 400 fills from one seed: no self-loop, no pair across the two
    graphs and no mesh pair twice is ever there; every one of the 54 non-mesh pairs of the first ring is added at
    least once (about 3,600 valid draws over 54 pairs: a miss has probability below 1e-25)."""
    ring = [(i, (i + 1) % 12) for i in range(12)] + [(12 + i, 12 + (i + 1) % 7) for i in range(7)]
    mesh = sym_mesh(ring, 19)
    feed = plain_feed([0, 12, 19], mesh, 1.0, 16)
    assert feed.cand_ptr.tolist() == [0, 12, 19]
    batch = batch_of(feed)
    mesh_keys = set((mesh[0] * 19 + mesh[1]).tolist())
    torch.manual_seed(1234)
    seen, counts = set(), set()
    for _ in range(400):
        feed.fill(batch)
        ei = feed.current_edge_index()
        key = ei[0] * 19 + ei[1]
        assert bool((key[1:] > key[:-1]).all())  # sorted and unique: no mesh pair added twice
        assert not bool((ei[0] == ei[1]).any())
        assert not bool(((ei[0] < 12) != (ei[1] < 12)).any())
        assert mesh_keys <= set(key.tolist())
        assert torch.equal(torch.sort(ei[1] * 19 + ei[0]).values, key)  # symmetric
        seen |= set(key.tolist()) - mesh_keys
        counts.add(ei.shape[1])
    first = {(i, j) for i in range(12) for j in range(12) if i != j and i * 19 + j not in mesh_keys}
    assert len(first) == 2 * 54 and {i * 19 + j for i, j in first} <= seen
    assert len(counts) > 1


def test_distribution_on_a_grid():
    """A triangulated 27 × 26 grid (702 nodes) at ratio 0.5, max_new 16, 20 fills from one seed: every live edge count
    lies in [E_m + 0.9 · 2C, E_m + 2C]. A candidate is lost to a self-pair (1 / n), a mesh edge (about 6 / n) or a
    repeat (about C / (n² / 2)): under 2 % together, and a node over 16 new neighbours at a mean of 3 is rarer still."""
    mesh = grid_mesh(27, 26)
    feed = plain_feed([0, 702], mesh, 0.5, 16)
    E_m, C = mesh.shape[1], feed.pairs.shape[0]
    assert C == round(0.5 * E_m) // 2 and C > 900
    batch = batch_of(feed)
    torch.manual_seed(7)
    counts, last = [], None
    for _ in range(20):
        feed.fill(batch)
        counts.append(int(feed.num_edges_dev))
        ei = feed.current_edge_index().clone()
        assert last is None or ei.shape != last.shape or not torch.equal(ei, last)  # consecutive fills differ
        last = ei
    print("live edge counts", counts, "bounds", E_m + 0.9 * 2 * C, E_m + 2 * C)
    assert all(E_m + 0.9 * 2 * C <= n <= E_m + 2 * C for n in counts)


def test_aneurysm_and_world_feeds_take_random_edges():
    """The allowed combinations build and fill on CPU tensors: aneurysm=, and world_pos= without its edge side."""
    import _aneurysm as AN
    from graphphysics.dataset.resident import ResidentTrajectories, random_topology_torch

    traj, pos, gp = AN.case([6, 5], 4, 4)
    mesh = sym_mesh([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 9), (9, 10)], 11)
    re = {"edge_index": mesh, "ratio": 1.0, "max_new": 3}
    feed = ResidentTrajectories(traj, gp, (0, 3), 13, aneurysm={"pos": pos}, random_edges=re)
    batch = batch_of(feed)
    feed.fill(batch)
    want, _ = random_topology_torch(feed.pairs, gp, mesh, 3, cand_ptr=feed.cand_ptr)
    assert torch.equal(feed.current_edge_index(), want) and want.shape[1] > mesh.shape[1]
    gold = WE.load_golden()
    ptraj, pgp, pmesh = WE.plate(gold)
    feed = ResidentTrajectories(ptraj, pgp, (0, 3), WE.K, world_pos=WE.world_pos(),
                                random_edges={"edge_index": pmesh, "ratio": 0.5, "max_new": 8})
    batch = batch_of(feed)
    feed.fill(batch)
    want, _ = random_topology_torch(feed.pairs, pgp, pmesh, 8, cand_ptr=feed.cand_ptr)
    assert torch.equal(feed.current_edge_index(), want) and want.shape[1] > pmesh.shape[1]


# ---------------------------------------------------------------------------------------------- refusals
def test_every_refused_configuration_raises():
    from graphphysics.dataset.resident import ResidentTrajectories, random_topology_torch
    from graphphysics.training.step import TrainStep

    gp = [0, 5, 9]
    ok = {"edge_index": PATHS, "ratio": 0.5, "max_new": 4}
    traj = torch.zeros(3, 9, 4)

    def make(re=ok, **kw):
        return ResidentTrajectories(traj, gp, (0, 3), 3, random_edges=re, **kw)

    make()
    for bad in (0.0, -0.5, 1.5, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="ratio"):
            make(dict(ok, ratio=bad))
    for bad in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="max_new"):
            make(dict(ok, max_new=bad))
    make(dict(ok, ratio=1, max_new=64))
    with pytest.raises(ValueError, match="sorted"):
        make(dict(ok, edge_index=PATHS[:, [1, 0] + list(range(2, PATHS.shape[1]))]))
    with pytest.raises(ValueError, match="symmetric"):
        make(dict(ok, edge_index=PATHS[:, 1:]))
    with pytest.raises(ValueError, match="different graphs"):
        make(dict(ok, edge_index=sym_mesh([(0, 1), (4, 5)], 9)))
    for bad in ({"edge_index": PATHS, "ratio": 0.5}, dict(ok, radius=0.1), "yes", {}):
        with pytest.raises(ValueError, match="keys"):
            make(bad)
    # combinations
    world = dict(WE.world_pos())
    gold = WE.load_golden()
    ptraj, pgp, pmesh = WE.plate(gold)
    pre = dict(ok, edge_index=pmesh)
    with pytest.raises(ValueError, match="dynamic_edges"):
        ResidentTrajectories(ptraj, pgp, (0, 3), WE.K, world_pos=world, random_edges=pre,
                             dynamic_edges={"edge_index": pmesh, "radius": 0.03, "max_neighbors": 4})
    with pytest.raises(ValueError, match="edge_attr"):
        ResidentTrajectories(ptraj, pgp, (0, 3), WE.K, random_edges=pre,
                             world_pos=dict(world, edge_index=pmesh, edge_attr_start=4))
    with pytest.raises(ValueError, match="edge_attr"):
        make(rotate={"feature_indices": [(0, 3)], "edge_attr": torch.zeros(PATHS.shape[1], 4), "edge_index": PATHS})
    make(rotate={"feature_indices": [(0, 3)]})  # a rotation of x and y alone goes with random edges
    # the switches of a feed without random_edges=
    plain = ResidentTrajectories(traj, gp, (0, 3), 3)
    assert plain.random is False and plain.random_pairs is None and plain.pairs is None and plain.edge_index is None
    for call in (plain.build_random_edges, lambda: plain.set_random_edges(False), lambda: plain.set_pairs("random")):
        with pytest.raises(ValueError, match="random_edges"):
            call()
    with pytest.raises(ValueError):
        plain.current_edge_index()
    # set_pairs
    feed = make(dict(ok, ratio=1.0))
    C = feed.pairs.shape[0]
    assert C == 7
    for bad in ("drawn", torch.zeros(C, 3, dtype=torch.int64), torch.zeros(C + 1, 2, dtype=torch.int64),
                torch.zeros(C, 2), torch.full((C, 2), -1), torch.full((C, 2), 2 ** 31)):
        with pytest.raises(ValueError):
            feed.set_pairs(bad)
    # the rule itself
    pairs = torch.zeros(3, 2, dtype=torch.int32)
    for cp in ([0, 3], [0, 2, 2], [1, 2, 3], [0, 4, 3]):
        with pytest.raises(ValueError, match="cand_ptr"):
            random_topology_torch(pairs, gp, PATHS, 2, cand_ptr=cp)
    with pytest.raises(ValueError, match="max_new"):
        random_topology_torch(pairs, gp, PATHS, 0, cand_ptr=[0, 2, 3])
    with pytest.raises(ValueError, match="non-negative"):
        random_topology_torch(pairs - 1, gp, PATHS, 2, cand_ptr=[0, 2, 3])
    # TrainStep: a model that reads edge_attr, and a batch whose edge_index is not the feed's

    class _EdgeSim:
        edge_input_size, model = 4, None

        def parameters(self):
            return []

    class _NodeSim(_EdgeSim):
        edge_input_size = None

    feed = make()
    with pytest.raises(ValueError, match="edge_attr"):
        TrainStep(_EdgeSim(), None, None, batch_of(feed), graph=False, feed=feed)
    b = batch_of(feed)
    b.edge_attr = torch.zeros(PATHS.shape[1], 4)
    with pytest.raises(ValueError, match="edge_attr"):
        TrainStep(_NodeSim(), None, None, b, graph=False, feed=feed)
    b = batch_of(feed)
    b.edge_index = PATHS
    with pytest.raises(ValueError, match="feed.edge_index"):
        TrainStep(_NodeSim(), None, None, b, graph=False, feed=feed)
    TrainStep(_NodeSim(), None, None, batch_of(feed), graph=False, feed=feed)


def test_resident_rollout_on_cpu_runs_on_the_last_build():
    """rollout_resident does not rebuild: switched off and built once, the feed's rollout equals that of a plain feed
    on the mesh edge_index; switched on, it runs on the pairs of the last build."""
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.training.rollout import Rollout

    gold = WE.load_golden()
    traj, gp, mesh = WE.plate(gold)
    sim = WE.plate_transformer(torch.device("cpu")).eval()
    feed = ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=WE.world_pos(),
                                random_edges={"edge_index": mesh, "ratio": 0.5, "max_new": 8})
    plain = ResidentTrajectories(traj, gp, (0, 3), WE.K, world_pos=WE.world_pos())
    N = traj.shape[1]

    def run(f, ei):
        ro = Rollout(sim, WE.K + 3, graph=False, feed=f, world_edges="off")
        b = _Batch(x=torch.zeros(N, 7), y=torch.zeros(N, 3), edge_index=ei, edge_attr=None, pos=None)
        return ro.rollout_resident(b, 0, 2)

    want = run(plain, mesh)
    feed.set_random_edges(False)
    feed.build_random_edges()
    assert torch.equal(run(feed, feed.current_edge_index()), want)
    feed.set_random_edges(True)
    torch.manual_seed(3)
    feed.pairs.random_(0, 2 ** 31 - 1)
    feed.build_random_edges()
    ei = feed.current_edge_index().clone()
    got = run(feed, feed.current_edge_index())
    assert torch.equal(feed.current_edge_index(), ei) and ei.shape[1] > mesh.shape[1]  # no rebuild in the rollout
    assert not torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_abi_and_c_side_refusals_need_no_device():
    """mgn_random_topology_build's host-side refusals, through ctypes with fake non-NULL addresses that are never
    dereferenced: nothing is launched. N == 0 is success."""
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat

    L = nat.load()
    assert L.mgn_abi_version() == 17 and nat.ABI_VERSION == 17
    for name in ("mgn_random_topology_workspace_bytes", "mgn_random_topology_build"):
        assert name in nat.EXPORTS and hasattr(L, name)
    with open(os.path.join(ROOT, "include", "mgn.h")) as f:
        header = f.read()
    assert "#define MGN_HAS_RANDOM_EDGES 1" in header and "#define MGN_ABI_VERSION 17" in header
    assert "dataset/dataset.py:104-137" in header
    p = ctypes.c_void_p(4096)  # non-NULL, never read: every case below returns before the first launch

    def call(N=10, B=1, E_m=4, W=4, C=6, pairs=p, cand=p, enabled=p, num_edges=p, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mgn_random_topology_workspace_bytes(N, W, C)
        return L.mgn_random_topology_build(pairs, cand, C, p, B, N, p, p, E_m, W, enabled, p, p, p, p, p, p, p,
                                           num_edges, p, ws_bytes, None)

    assert call(N=0, B=0, E_m=0, C=0) == 0  # no nodes: success without a launch
    for kw, text in ((dict(W=0), b"max_new"), (dict(W=65), b"max_new"), (dict(W=-3), b"max_new"),
                     (dict(N=-1), b">= 0"), (dict(E_m=-1), b">= 0"), (dict(C=-1), b">= 0"), (dict(B=0), b"B == 0"),
                     (dict(N=2 ** 30 + 1, ws_bytes=2 ** 40), b"2^30"),
                     (dict(N=2 ** 28, W=16, ws_bytes=2 ** 40), b"int32"),
                     (dict(C=2 ** 30 + 1, ws_bytes=2 ** 40), b"num_candidates"),
                     (dict(pairs=None), b"null pointer"), (dict(cand=None), b"null pointer"),
                     (dict(enabled=None), b"enabled"), (dict(num_edges=None), b"null pointer"),
                     (dict(ws_bytes=16), b"workspace")):
        assert call(**kw) != 0, kw
        assert text.lower() in L.mgn_last_error().lower(), (kw, L.mgn_last_error())
    assert L.mgn_random_topology_workspace_bytes(1000, 16, 500) >= 1000 * 4 + 2 * 1000 * 16 * 4 + 500 * 4
    # a cand_ptr that is not monotone is refused where it is built, on the host
    with pytest.raises(ValueError, match="cand_ptr"):
        from graphphysics.models._engine import RandomTopology

        RandomTopology(PATHS, [0, 5, 9], 9, [0, 4, 3], 2, "cpu")
