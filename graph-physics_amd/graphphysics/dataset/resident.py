"""Training batches from trajectories that stay resident, and clean, on the device.

What the reference does per item in Dataset.__getitem__ — x is frame t of a trajectory, y the dynamic
columns of frame t + 1 (reference dataset/h5_dataset.py:81-92, dataset/hierarchical.py:96-116), then
add_noise on the noisy columns of NORMAL nodes (dataset/preprocessing.py:177-238) — as ONE libmgn launch
(mgn_feed_batch) that writes a batch's x and y in place from per-graph frame indices. The frame indices
(torch.randint) and the Gaussian draws (torch.randn) are device work too, so ResidentTrajectories.fill can be
recorded at the head of a captured training step (TrainStep(..., feed=...)) and draws anew on every replay.

The stored frames are only ever read: the in-place write of preprocessing.add_noise, applied to frames kept
on the device, would pile noise on noise epoch after epoch (the reference re-reads every item from disk and
never sees this); here the noise goes into the batch, never into `traj`.

Rotation augmentation (rotate=; the reference's Random3DRotate, dataset/preprocessing.py:277-366) lives where
the noise lives: three angles per graph drawn on the device, a matrix per graph (mgn_feed_rotation_matrices),
the column triples of x and the 3 columns of y rotated by the fill's own launch ahead of the noise
(mgn_feed_batch_rot), and the triples of a clean edge_attr rotated into the batch's by one more launch
(mgn_feed_rotate_rows). The rule is row vector times matrix written term by term, (a0·R0j + a1·R1j) + a2·R2j,
so the torch ops of fill_torch / rotate_rows_torch give the kernels' bits.

World positions (world_pos=; Lagrangian data such as DeformingPlate, the reference's world_pos_parameters
stages add_obstacles_next_pos and add_world_pos_features, dataset/preprocessing.py:49-89 and 143-174, in
build_preprocessing's order): the batch row is [world(3), obstacle displacement(3), the other frame columns] —
the displacement of a row's own next clean position for OBSTACLE rows, the per-graph mean of those (a fixed-order
fp32 sum divided by the count) for the others — written by mgn_feed_batch_world (a reduction per graph, then the
fill) with the noise on top, in batch-layout columns; then, when the feed was given an edge_index,
mgn_feed_world_edge_features writes the relative world positions of the noisy x and their norm into four
columns of batch.edge_attr. fill_world_torch / world_edge_features_torch state both rules term by term.

Aneurysm features (aneurysm=; the reference's external/aneurysm.py build_features, which its train.py hard-wires
as extra_node_features and coarse-aneurysm.json / c-a-gmm.json are written for): the batch row is [frame row (F) ‖
a − p (3) ‖ pos (3) ‖ mean, min, max ‖ node type], a the drawn frame and p the one before it, so this mode does
read the previous frame; the three statistics, over the distinct next-frame accelerations of the graph's inflow
nodes, are computed once for every (frame, graph) by mgn_feed_inflow_stats (a sort in LDS per pair, an fp64 sum in
ascending order) and picked by the fill, mgn_feed_batch_aneurysm, one launch with the noise on top in batch-layout
columns (up to 8 ranges here: the configs have six). inflow_stats_torch / fill_aneurysm_torch state both rules;
graphphysics.external.aneurysm.build_features is the per-item transform on the same rules.

World edges that change from frame to frame (dynamic_edges=, with world_pos=; the reference's add_world_edges,
dataset/preprocessing.py:92-140, which build_preprocessing runs per item after the noise, and which is the only path
from the obstacle to the plate in a transformer config such as plate.json, whose attention is masked by the
adjacency): after the fill and the noise, mgn_world_topology_build finds every graph's OBSTACLE–NORMAL pairs within
the radius from the noisy x, merges them into the static mesh adjacency and rewrites, in place and without the host,
the six arrays of the feed's topology, its edge_index and its edge count. batch.edge_index is the feed's own tensor,
bound to that topology (models._engine.bind_topology), so a recorded step keeps reading the same addresses and every
replay attends over the contacts of its own batch. world_topology_torch states the rule.

Random long-range edges (random_edges=; the reference's BaseDataset._add_random_edges, dataset/dataset.py:104-137,
the dataset.new_edges_ratio of every transformer config: per item PyG's add_random_edge(p, force_undirected=True) adds
"random jumps", a new set of long-range attention partners on every sample): after the fill, the feed draws its
candidate pairs (pairs.random_(0, 2**31 − 1): torch's generator, recorded, new on every replay) and
mgn_random_topology_build rewrites the feed's topology, edge_index and edge count in place, as dynamic_edges= does.
random_topology_torch states the rule:
  * graph g with n_g nodes and E_g directed mesh edges has the fixed number C_g = round(ratio · E_g) // 2 of candidate
    pairs (add_random_edge asks for round(p · E) directed edges and samples half as many unordered pairs), none when
    n_g < 2; candidate c of graph g is (u, v) = pairs[c], with the endpoints a = lo_g + u % n_g, b = lo_g + v % n_g;
  * for node i, over its graph's candidates in order, a candidate is live when i is an endpoint, a != b, and the
    other endpoint j is no mesh neighbour of i. Pass 1 keeps a list L_i: a live candidate whose j is in L_i is skipped
    (a repeat); else, when L_i holds max_new entries, the candidate is dropped (flagged); else j is appended, c beside
    it. Pass 2: i's new neighbours are the entries of L_i whose candidate is unflagged, ascending;
  * an unordered pair survives exactly when its first candidate is unflagged, at both endpoints alike, so the lists
    are symmetric; the result is the union of the mesh edges and the lists, sorted by (row, col), every edge once.
Dropping is the capacity policy here, where dynamic_edges= raises: there an edge over capacity is physics lost; here the
number of new neighbours of a node is about Poisson with mean ratio · degree, some node of a large batch overflows
once in a few thousand steps, and a training run must not stop for that. Relation to PyG — recalled, not checked: PyG
is not installed here and the reference holds none of its code — add_random_edge routes through negative_sampling,
which samples non-edges without replacement; this rule samples with replacement and discards self-pairs, mesh edges and
repeats without redrawing, so it adds slightly fewer edges, by a fraction of about (1 + degree) / n_g + C_g / (n_g² / 2).
The distribution follows PyG's; the draws for a seed do not.

Both together (dynamic_edges= and random_edges= on one feed, given the same mesh edge_index, with one_topology=True —
without it the two stay refused, as before: the capacity and the candidate rule below are the caller's choice, not a
silent merge; plate.json with dataset.new_edges_ratio on): the reference builds a sample's adjacency in a fixed order — _apply_preprocessing runs
add_world_edges on the sample's frame, _add_random_edges then adds its random jumps on top of the edge_index that
left (dataset/h5_dataset.py:102-105) — and so does the fill: the world fill and the noise, the draw of pairs, then ONE
mgn_world_random_topology_build from the noisy x, which rewrites one topology of the capacity E_m + N · (max_neighbors
+ max_new). world_random_topology_torch states the rule, the two rules above composed: a candidate that is a world
edge of this build is discarded like a mesh edge, max_new caps the random neighbours only, max_neighbors the world
neighbours (over it: MGN_ERR_WORLD_CAPACITY, as for dynamic_edges=). A stated deviation: the number of candidates stays
round(ratio · E_g) // 2 over the MESH edges of graph g, where the reference counts the mesh plus the world edges of the
sample; the count sizes tensors and launches of a recorded step and must be fixed at construction (on the plate batch
the README measures, the world edges are 590–800 of about 120,000 edges, under 0.7 %).

Not supported: `previous_data` outside aneurysm= (there it is the frame before the drawn one), dynamic_edges= and
random_edges= for models with edge_attr (the MGN path: its launch shapes depend on the edge count; the edge_index given
inside world_pos= stays static for the life of the feed), rotate= together with world_pos=, aneurysm=
together with either, a wall flag that changes over time (aneurysm= takes the node types from frame 0), and trajectories
of unequal length in one batch. batch.edge_index is written only by a dynamic_edges= or random_edges= feed (through its
own tensor), batch.edge_attr only by a rotating feed that was given a clean edge_attr and by a world_pos= feed that was
given an edge_index.

The validation rollout reads the same resident frames (training.rollout.Rollout.rollout_resident):
rollout_begin_torch / rollout_end_torch state, as torch ops on any device, the two rules libmgn's
mgn_rollout_begin / mgn_rollout_end run around the Simulator's evaluation forward; there previous data is
supported, noise is not applied. On a world_pos= feed (Rollout(..., world_edges=...)) the begin stage is
mgn_rollout_begin_world, stated by rollout_begin_world_torch on fill_world_torch's own expressions: the
noise-free batch row of frame start + s, then the feedback in batch-layout columns; the four edge_attr columns
come from world_edge_features_torch / mgn_feed_world_edge_features, on the clean world positions of the frame or
on the x the model is about to see, as the caller chooses. On an aneurysm= feed (Rollout(..., acceleration=...))
the begin stage is mgn_rollout_begin_aneurysm, stated by rollout_begin_aneurysm_torch on fill_aneurysm_torch's own
expressions: the noise-free row of frame start + s (frames start + s − 1 and start + s + 1 are read too), then the
feedback; the acceleration columns either follow the clean frames or are the previous-data columns, as the caller
chooses, and the inflow statistics are always those of the clean-frame table.
"""
import math

import torch

from graphphysics import _native as nat
from graphphysics.utils.nodetype import NodeType


def _noise_lists(noise):
    """(starts, ends, scales) of the reference's noise_parameters, with add_noise's checks and messages."""
    start, end, scale = noise["noise_index_start"], noise["noise_index_end"], noise["noise_scale"]
    if isinstance(start, int):
        start = [start]
    if isinstance(end, int):
        end = [end]
    if isinstance(scale, (int, float)):
        scale = [float(scale)] * len(start)
    if len(start) != len(end):
        raise ValueError("noise_index_start and noise_index_end must have the same length.")
    if len(scale) != len(start):
        raise ValueError("noise_scale must have the same length as noise_index_start and noise_index_end.")
    return [int(s) for s in start], [int(e) for e in end], [float(s) for s in scale]


def _check_ranges(ranges, F, limit=nat.MGN_FEED_MAX_RANGES):
    if len(ranges) > limit:
        raise ValueError(f"at most {limit} noisy column ranges are supported, got {len(ranges)}")
    for i, (s, e) in enumerate(ranges):
        if not 0 <= s <= e <= F:
            raise ValueError(f"noisy column range ({s}, {e}) is outside [0, {F}]")
        for s2, e2 in ranges[:i]:
            if s < e and s2 < e2 and s < e2 and s2 < e:
                raise ValueError(f"noisy column ranges ({s2}, {e2}) and ({s}, {e}) overlap")


def _check_triples(triples, width, name, what):
    """[(s, s + 3), ...] as ints, after the checks of a rotation's column triples (ValueError)."""
    try:
        triples = [(int(s), int(e)) for s, e in triples]
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a list of (start, end) column pairs, got {triples!r}") from None
    if len(triples) > nat.MGN_FEED_MAX_RANGES:
        raise ValueError(f"at most {nat.MGN_FEED_MAX_RANGES} column triples are supported, got {len(triples)}")
    for i, (s, e) in enumerate(triples):
        if e - s != 3:
            raise ValueError(f"each range of {name} must span exactly 3 columns (xyz), got ({s}, {e})")
        if not 0 <= s < e <= width:
            raise ValueError(f"column triple ({s}, {e}) is outside the {width} columns of {what}")
        for s2, e2 in triples[:i]:
            if s < e2 and s2 < e:
                raise ValueError(f"column triples ({s2}, {e2}) and ({s}, {e}) overlap")
    return triples


def _node_graph(graph_ptr, N, device):
    """Graph id of every node from node offsets [B+1] (a host list or a tensor)."""
    gp = torch.as_tensor(graph_ptr, dtype=torch.int64).to(device)
    return torch.repeat_interleave(torch.arange(gp.numel() - 1, device=device), gp[1:] - gp[:-1], output_size=N)


def _rot3(a, Rm):
    """Row vectors a [n, 3] times the per-row matrices Rm [n, 3, 3] as the kernels write it, term by term:
    (a0·R[0][j] + a1·R[1][j]) + a2·R[2][j]. Elementwise ops round every product and every sum on their own,
    which a matmul (BLAS may fuse multiply-adds, and orders the sum as it likes) does not promise."""
    return (a[:, 0:1] * Rm[:, 0] + a[:, 1:2] * Rm[:, 1]) + a[:, 2:3] * Rm[:, 2]


def rotate_rows_torch(src, row_graph, triples, R):
    """mgn_feed_rotate_rows' rule as torch ops on any device: a new tensor, src [rows, cols] with the columns of
    every triple (s, s + 3) of row r rotated by R[row_graph[r]] (R [B, 9], row-major 3x3 per graph); other
    columns, and the rows whose graph id is outside [0, B), are src bit for bit."""
    out = src.clone()
    B = R.shape[0]
    if src.shape[0] == 0 or B == 0:
        return out
    g = row_graph.to(src.device, torch.int64)
    valid = ((g >= 0) & (g < B))[:, None]
    Rm = R.to(src.device)[g.clamp(0, B - 1)].view(-1, 3, 3)
    for s, e in triples:
        a = src[:, s:e]
        out[:, s:e] = torch.where(valid, _rot3(a, Rm), a)
    return out


def fill_torch(traj, graph_ptr, frame, y_columns, node_type_index, ranges, scales, z, triples=None, R=None):
    """mgn_feed_batch's rule as torch ops on any device: returns (x [N, F], y [N, y_end - y_start]) as new
    tensors. x = frame[g] of traj for the nodes of graph g, plus z[:, zc] * scales[i] on the columns of
    noisy range i of the rows whose (clean) node type is NORMAL — zc runs over the ranges in order; y = the
    y_columns of the next clean frame. z None: no noise. triples [(s, s + 3), ...] and R [B, 9]
    (mgn_feed_batch_rot's rule): the columns of every triple of x, and y (3 wide then), are rotated by the
    matrix of the row's graph, before the noise. What ResidentTrajectories.fill runs on CPU tensors, and what
    the kernels are tested and timed against."""
    T, N, F = traj.shape
    rows = torch.arange(N, device=traj.device)
    node_graph = _node_graph(graph_ptr, N, traj.device)
    t = frame.to(traj.device, torch.int64)[node_graph]
    x = traj[t, rows]
    y = traj[t + 1, rows, y_columns[0]:y_columns[1]].contiguous()
    if triples:
        if R is None:
            raise ValueError("column triples without R")
        if y_columns[1] - y_columns[0] != 3:
            raise ValueError(f"with column triples y_columns {tuple(y_columns)} must be 3 wide")
        Rm = R.to(traj.device)[node_graph].view(-1, 3, 3)
        for s, e in triples:  # triples do not overlap: each reads its own three clean columns
            x[:, s:e] = _rot3(x[:, s:e], Rm)
        y = _rot3(y, Rm)
    if z is not None:
        normal = (x[:, node_type_index] == NodeType.NORMAL)[:, None]
        zc = 0
        for i, (s, e) in enumerate(ranges):
            feature = x[:, s:e]
            noise = z[:, zc:zc + e - s] * scales[i]
            x[:, s:e] = torch.where(normal, feature + noise, feature)
            zc += e - s
    return x, y


def fill_world_torch(traj, graph_ptr, frame, y_columns, node_type_index, ranges, scales, z):
    """mgn_feed_batch_world's rule as torch ops on any device: returns (x [N, F + 3], y [N, y_end - y_start],
    obstacle_mean [B, 3]) as new tensors. With a = frame[g] of traj and n the next frame: disp = n[:, 0:3] −
    a[:, 0:3] from clean values; obstacle_mean[g] = the sum of disp over the OBSTACLE rows of g divided by their
    count M (0 for M = 0), written sum(0) / M — a division, as torch.mean on the CPU, by a tensor: a GPU division
    by a host scalar multiplies by the reciprocal —; x = [a[:, 0:3], disp on OBSTACLE rows and obstacle_mean[g]
    on the others, a[:, 3:]]; then fill_torch's noise with `ranges` in the columns of this batch layout and the
    node type read from the clean frame column node_type_index; y = the y_columns of n. What
    ResidentTrajectories(world_pos=...).fill runs on CPU tensors, and what the kernels are tested against."""
    T, N, F = traj.shape
    dev = traj.device
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    rows = torch.arange(N, device=dev)
    node_graph = _node_graph(gp, N, dev)
    t = frame.to(dev, torch.int64)[node_graph]
    a, n = traj[t, rows], traj[t + 1, rows]
    y = n[:, y_columns[0]:y_columns[1]].contiguous()
    disp = n[:, 0:3] - a[:, 0:3]
    obstacle = a[:, node_type_index] == NodeType.OBSTACLE
    mean = torch.zeros(len(gp) - 1, 3, dtype=torch.float32, device=dev)
    for g in range(len(gp) - 1):
        d = disp[gp[g]:gp[g + 1]][obstacle[gp[g]:gp[g + 1]]]
        if d.shape[0] > 0:
            mean[g] = d.sum(0) / torch.full((), d.shape[0], dtype=torch.float32, device=dev)
    x = torch.cat([a[:, 0:3], torch.where(obstacle[:, None], disp, mean[node_graph]), a[:, 3:]], dim=1)
    if z is not None:
        normal = (a[:, node_type_index] == NodeType.NORMAL)[:, None]
        zc = 0
        for i, (s, e) in enumerate(ranges):
            feature = x[:, s:e]
            noise = z[:, zc:zc + e - s] * scales[i]
            x[:, s:e] = torch.where(normal, feature + noise, feature)
            zc += e - s
    return x, y, mean


def inflow_stats_torch(cur, nxt, inflow_mask):
    """mgn_feed_inflow_stats' rule for one (frame, graph) pair, on any device: fp32 [3] = (mean, min, max) of the
    value set S of the reference's build_features (external/aneurysm.py: next_acceleration[~inflow] = 0; .unique()).
    d = nxt[:, 0:3] − cur[:, 0:3], one rounded fp32 subtraction; S = the 3·M components of d on the M inflow rows,
    plus 0.0 when at least one row is not inflow; equal values (==, so -0.0 and 0.0 are one value, kept as +0.0)
    count once. min and max are exact. mean = the fp64 sum of the distinct values in ascending order, one addition
    after the other, divided in fp64 by their count and rounded once to fp32: the kernel's bits. The reference
    takes torch.mean of the fp32 set, in fp32 and with whatever order its reduction has, so this mean may differ
    from the reference's by the error of that fp32 sum, |mean − m_ref| <= 2^-24·|m_ref| + 2^-24·Σ|v| over the
    distinct values v, and is the more accurate of the two. S is never empty for N >= 1 (no rows: zeros). With
    non-finite values the result is unspecified. The sum runs on the host (a sequential fp64 sum is what the
    kernel's one thread does; a device reduction orders it otherwise)."""
    dev = cur.device
    if cur.shape[0] == 0:
        return torch.zeros(3, dtype=torch.float32, device=dev)
    mask = inflow_mask.to(dev, torch.bool)
    d = nxt[:, 0:3] - cur[:, 0:3]
    vals = d[mask].reshape(-1)
    if not bool(mask.all()):
        vals = torch.cat([vals, torch.zeros(1, dtype=torch.float32, device=dev)])
    distinct = torch.unique(vals + 0.0).tolist()  # ascending; -0.0 + 0.0 = +0.0
    total = 0.0
    for v in distinct:  # Python floats are fp64: the kernel's sum, term by term
        total += v
    return torch.tensor([total / len(distinct), distinct[0], distinct[-1]], dtype=torch.float32, device=dev)


def fill_aneurysm_torch(traj, graph_ptr, frame, pos, node_type, stats, y_columns, ranges, scales, z):
    """mgn_feed_batch_aneurysm's rule as torch ops on any device: returns (x [N, F + 10], y [N, y_end - y_start]) as
    new tensors. With t = frame[g], a = traj[t], p = traj[t − 1] and n = traj[t + 1]: x = [a (F) ‖ a[:, 0:3] −
    p[:, 0:3] ‖ pos (3) ‖ stats[t, g] = mean, min, max ‖ node_type], the row of the reference's build_features
    (graphphysics.external.aneurysm); then fill_torch's noise — a rounded product, then a rounded sum, on the rows
    whose node_type is NORMAL — with `ranges` in the columns of this batch layout; every column draws its own
    normal, so the noise on the velocity and on the acceleration is independent, as in the reference, whose
    add_noise runs after build_features. y = the y_columns of n. stats: fp32 [T − 1, B, 3], inflow_stats_torch of
    every (frame, graph). z None: no noise. What ResidentTrajectories(aneurysm=...).fill runs on CPU tensors, and
    what the kernel is tested against."""
    T, N, F = traj.shape
    dev = traj.device
    rows = torch.arange(N, device=dev)
    node_graph = _node_graph(graph_ptr, N, dev)
    t = frame.to(dev, torch.int64)[node_graph]
    a, p, n = traj[t, rows], traj[t - 1, rows], traj[t + 1, rows]
    y = n[:, y_columns[0]:y_columns[1]].contiguous()
    x = torch.cat([a, a[:, 0:3] - p[:, 0:3], pos.to(dev), stats.to(dev)[t, node_graph], node_type.to(dev)[:, None]],
                  dim=1)
    if z is not None:
        normal = (node_type.to(dev) == NodeType.NORMAL)[:, None]
        zc = 0
        for i, (s, e) in enumerate(ranges):
            feature = x[:, s:e]
            noise = z[:, zc:zc + e - s] * scales[i]
            x[:, s:e] = torch.where(normal, feature + noise, feature)
            zc += e - s
    return x, y


def world_edge_features_torch(x, edge_index, edge_attr, start):
    """mgn_feed_world_edge_features' rule as torch ops on any device, in place on edge_attr [E, >= start + 4]:
    v = x[senders, 0:3] − x[receivers, 0:3] (senders = edge_index[0]) into columns [start, start + 3) and
    sqrt((v0·v0 + v1·v1) + v2·v2), term by term, into column start + 3; other columns are not touched. The
    kernel's square root is correctly rounded; torch.sqrt in fp32 does not promise that (on the CPU, a contiguous
    tensor goes through a vector library that is accurate to 1 ulp only), so the root of the fp32 sum is taken in
    fp64 and rounded to fp32: 53 bits are more than the 2·24 + 2 that make this double rounding exact."""
    ei = edge_index.to(x.device, torch.int64)
    v = x[ei[0], 0:3] - x[ei[1], 0:3]
    edge_attr[:, start:start + 3] = v
    sumsq = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    edge_attr[:, start + 3] = torch.sqrt(sumsq.double()).float()
    return edge_attr


def check_mesh_edges(edge_index, graph_ptr, N):
    """The host-side preconditions of a dynamic_edges mesh (ValueError): an integer [2, E_m] tensor with node ids in
    [0, N), sorted by (row, col), without duplicates or self-loops, symmetric, every edge inside one graph — what
    FaceToEdge + to_undirected emit for a batch. Returns it as int64 on the CPU."""
    ei = edge_index
    if not torch.is_tensor(ei) or ei.dim() != 2 or ei.shape[0] != 2 or ei.is_floating_point() or ei.dtype == torch.bool:
        raise ValueError("dynamic_edges edge_index must be an integer [2, E] tensor")
    ei = ei.to("cpu", torch.int64).contiguous()
    if ei.shape[1] == 0:
        return ei
    if int(ei.min()) < 0 or int(ei.max()) >= N:
        raise ValueError(f"dynamic_edges edge_index holds node ids outside [0, {N})")
    if bool((ei[0] == ei[1]).any()):
        raise ValueError(f"dynamic_edges edge_index holds a self-loop (edge {int(torch.nonzero(ei[0] == ei[1])[0])})")
    key = ei[0] * N + ei[1]
    if bool((key[1:] <= key[:-1]).any()):
        bad = int(torch.nonzero(key[1:] <= key[:-1])[0]) + 1
        what = "a duplicate" if int(key[bad]) == int(key[bad - 1]) else "not sorted by (row, col)"
        raise ValueError(f"dynamic_edges edge_index must be sorted by (row, col) and unique: edge {bad} is {what}")
    back = ei[1] * N + ei[0]
    if not torch.equal(torch.sort(back).values, key):
        raise ValueError("dynamic_edges edge_index must be symmetric: an edge has no reverse edge")
    node_graph = _node_graph(graph_ptr, N, "cpu")
    cross = node_graph[ei[0]] != node_graph[ei[1]]
    if bool(cross.any()):
        raise ValueError(f"dynamic_edges edge {int(torch.nonzero(cross)[0])} joins nodes of different graphs")
    return ei


def world_topology_torch(pos, node_type, graph_ptr, mesh_edge_index, radius, max_neighbors=None):
    """mgn_world_topology_build's rule as torch ops on any device — the reference's add_world_edges
    (dataset/preprocessing.py:92-140) applied to every graph of the batch on its own, then batched. Nodes i, j of one
    graph are linked when one is NORMAL, the other OBSTACLE, and the squared distance of their fp32 positions
    pos[:, 0:3], taken in fp64 as (v0·v0 + v1·v1) + v2·v2 with v the fp64 difference, is <= radius·radius (cKDTree's
    verdict); the result is the union of the mesh edges (check_mesh_edges' preconditions) and both directions of
    every pair, sorted by (row, col), every edge once. Returns (edge_index int64 [2, E], arrays): arrays is a dict of
    the six int32 tensors csc_src, csc_dst, csc_eid, row_perm [E] and col_ptr, row_ptr [N + 1] that
    mgn_topology_build gives for that edge_index, derived as the kernel derives them — the adjacency is symmetric, so
    the target-sorted list is the (row, col)-sorted one with its rows swapped, and an edge's place in the other order
    is the rank of its reverse. max_neighbors: a node with more world neighbours (pairs that are not mesh edges)
    raises the ValueError of MGN_ERR_WORLD_CAPACITY. What a dynamic_edges= feed runs on CPU tensors, and what the
    kernels are tested against."""
    dev, N = pos.device, pos.shape[0]
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    mesh = mesh_edge_index.to(dev, torch.int64)
    p, t, r2 = pos[:, 0:3].double(), node_type.to(dev), float(radius) * float(radius)
    wi, wj = [], []
    for a, b in zip(gp, gp[1:]):
        if b <= a:
            continue
        v = p[a:b, None, :] - p[None, a:b, :]
        d2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        normal, obstacle = t[a:b] == NodeType.NORMAL, t[a:b] == NodeType.OBSTACLE
        pair = (normal[:, None] & obstacle[None, :]) | (obstacle[:, None] & normal[None, :])
        i, j = torch.nonzero(pair & (d2 <= r2), as_tuple=True)
        wi.append(i + a)
        wj.append(j + a)
    mesh_key = mesh[0] * N + mesh[1]
    if wi:
        world_key = torch.cat(wi) * N + torch.cat(wj)
        world_key = world_key[~torch.isin(world_key, mesh_key)]  # already a mesh edge: to_undirected keeps one
    else:
        world_key = mesh_key[:0]
    if max_neighbors is not None and world_key.numel() and \
            int(torch.bincount(torch.div(world_key, max(N, 1), rounding_mode="floor")).max()) > int(max_neighbors):
        raise nat.world_capacity_error()
    return _topology_of_keys(torch.sort(torch.cat([mesh_key, world_key])).values, N)


def _topology_of_keys(key, N):
    """(edge_index, arrays) of a symmetric adjacency given as its ascending, unique keys row · N + col: what
    world_topology_torch and random_topology_torch return."""
    dev = key.device
    row, col = torch.div(key, max(N, 1), rounding_mode="floor"), key % max(N, 1)
    ptr = torch.searchsorted(row.contiguous(), torch.arange(N + 1, device=dev)).to(torch.int32)
    # target-sorted position k holds edge (src = col[k] → dst = row[k]); its id in (row, col) order is the rank of
    # the reversed pair, and row_perm is that permutation's inverse
    eid = torch.searchsorted(key, col * N + row)
    perm = torch.empty_like(eid)
    perm[eid] = torch.arange(eid.numel(), device=dev)
    arrays = {"csc_src": col.to(torch.int32), "csc_dst": row.to(torch.int32), "csc_eid": eid.to(torch.int32),
              "row_perm": perm.to(torch.int32), "col_ptr": ptr, "row_ptr": ptr.clone()}
    return torch.stack([row, col]), arrays


def random_candidate_ptr(graph_ptr, mesh_edge_index, ratio):
    """The candidate offsets [B + 1] (a host list) of a random_edges= feed: graph g with n_g nodes and E_g directed
    mesh edges gets C_g = round(ratio · E_g) // 2 candidate pairs — PyG's add_random_edge(p, force_undirected=True)
    asks for round(p · E) directed edges and samples half as many unordered pairs — and none when n_g < 2."""
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    row = mesh_edge_index[0].to("cpu", torch.int64).contiguous()
    bounds = torch.searchsorted(row, torch.tensor(gp, dtype=torch.int64)).tolist()  # the mesh is sorted by row
    ptr = [0]
    for g in range(len(gp) - 1):
        E_g = bounds[g + 1] - bounds[g]
        ptr.append(ptr[-1] + (round(float(ratio) * E_g) // 2 if gp[g + 1] - gp[g] >= 2 else 0))
    return ptr


def random_topology_torch(pairs, graph_ptr, mesh_edge_index, max_new, enabled=True, *, cand_ptr):
    """mgn_random_topology_build's rule as torch ops on any device (module docstring, "Random long-range edges").
    pairs: integer [C, 2], non-negative; cand_ptr: [B + 1] candidate offsets of every graph, from 0 to C
    (random_candidate_ptr); mesh_edge_index: check_mesh_edges' preconditions. Candidate c of graph g = [lo_g, lo_g +
    n_g) has the endpoints a = lo_g + pairs[c, 0] % n_g and b = lo_g + pairs[c, 1] % n_g. For node i, over its graph's
    candidates in order, a candidate is live when i is an endpoint, a != b and the other endpoint j is no mesh
    neighbour of i; pass 1 keeps a list L_i: a live candidate whose j is in L_i is skipped, else with |L_i| == max_new
    it is dropped (flagged), else j is appended with c beside it; pass 2: i's new neighbours are the entries of L_i
    whose candidate is unflagged, ascending. The result is the union of the mesh edges and those lists (they are
    symmetric), sorted by (row, col), every edge once: returns (edge_index int64 [2, E], arrays) as
    world_topology_torch does. enabled False: the mesh alone. No error for a node over max_new: dropping is the
    capacity policy.

    Vectorised, not walked: a candidate gives two events (i, j, c) = (a, b, c), (b, a, c). Of the live events with the
    same (i, j) only the first in candidate order can append — a later one finds j in L_i, or, when the first was
    dropped, finds the list still full (lists only grow in pass 1) and is dropped as well, being in no list; the k-th
    such first event of node i, in candidate order, is appended when k < max_new and flags its candidate otherwise.
    What a random_edges= feed runs on CPU tensors, and what the kernels are tested against."""
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    cp = [int(v) for v in (cand_ptr.tolist() if torch.is_tensor(cand_ptr) else cand_ptr)]
    N, W, dev = gp[-1], int(max_new), pairs.device
    C = pairs.shape[0]
    if len(cp) != len(gp) or cp[0] != 0 or cp[-1] != C or any(b < a for a, b in zip(cp, cp[1:])):
        raise ValueError(f"cand_ptr must hold B + 1 = {len(gp)} non-decreasing candidate offsets from 0 to C = {C}, "
                         f"got {cp}")
    if W < 1:
        raise ValueError(f"max_new {max_new} must be >= 1")
    mesh = mesh_edge_index.to(dev, torch.int64)
    mesh_key = mesh[0] * N + mesh[1]
    if not enabled or C == 0:
        return _topology_of_keys(mesh_key, N)
    counts = torch.tensor([b - a for a, b in zip(cp, cp[1:])], dtype=torch.int64, device=dev)
    graph = torch.repeat_interleave(torch.arange(len(cp) - 1, device=dev), counts, output_size=C)
    lo = torch.tensor(gp[:-1], dtype=torch.int64, device=dev)[graph]
    n = torch.tensor([b - a for a, b in zip(gp, gp[1:])], dtype=torch.int64, device=dev)[graph]
    if bool((n < 1).any()):
        raise ValueError("cand_ptr gives candidates to a graph without nodes")
    p = pairs.to(torch.int64)
    if bool((p < 0).any()):
        raise ValueError("pairs must be non-negative")
    a, b = lo + p[:, 0] % n, lo + p[:, 1] % n
    # events in candidate order: 2c is (a, b, c), 2c + 1 is (b, a, c)
    ev_i, ev_j = torch.stack([a, b], dim=1).reshape(-1), torch.stack([b, a], dim=1).reshape(-1)
    ev_c = torch.arange(C, device=dev).repeat_interleave(2)
    key = ev_i * N + ev_j
    live = (ev_i != ev_j) & ~torch.isin(key, mesh_key)
    key, ev_c = key[live], ev_c[live]
    # the first event of every (i, j): a stable sort by key keeps candidate order inside a run
    order = torch.sort(key, stable=True).indices
    key, ev_c = key[order], ev_c[order]
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    key, ev_c = key[first], ev_c[first]
    # its place among node i's first events, in candidate order
    order = torch.sort(ev_c, stable=True).indices
    key, ev_c = key[order], ev_c[order]
    ev_i = torch.div(key, max(N, 1), rounding_mode="floor")
    order = torch.sort(ev_i, stable=True).indices
    key, ev_c, ev_i = key[order], ev_c[order], ev_i[order]
    start = torch.searchsorted(ev_i.contiguous(), ev_i.contiguous())  # the first event of the node's run
    appended = torch.arange(key.numel(), device=dev) - start < W
    flag = torch.zeros(C, dtype=torch.bool, device=dev)
    flag[ev_c[~appended]] = True
    new_key = key[appended & ~flag[ev_c]]
    return _topology_of_keys(torch.sort(torch.cat([mesh_key, new_key])).values, N)


def world_random_topology_torch(pos, node_type, pairs, graph_ptr, mesh_edge_index, radius, max_neighbors, max_new,
                                enabled=True, *, cand_ptr):
    """mgn_world_random_topology_build's rule as torch ops on any device: the two rules above composed in the
    reference's order (_apply_preprocessing runs add_world_edges on the sample's frame, _add_random_edges then adds
    its random jumps on top of the edge_index that left; dataset/h5_dataset.py:102-105, dataset/dataset.py:104-137):
      1. ei_w = world_topology_torch(pos, node_type, graph_ptr, mesh_edge_index, radius, max_neighbors)'s edge_index —
         sorted, symmetric, unique, every edge inside one graph: check_mesh_edges' preconditions;
      2. random_topology_torch(pairs, graph_ptr, ei_w, max_new, enabled, cand_ptr=cand_ptr).
    So a candidate that is a self-pair, a mesh edge, a world edge of this build or a repeat is discarded; max_new caps
    the new random neighbours only; a candidate dropped at one endpoint is removed at the other. enabled False: step
    1's result. A node over max_neighbors raises the ValueError of MGN_ERR_WORLD_CAPACITY, a node over max_new nothing.
    Returns (edge_index int64 [2, E], arrays) as both rules do.

    A stated deviation from the reference: cand_ptr stays random_candidate_ptr(graph_ptr, MESH edges, ratio), where the
    reference's add_random_edge counts round(p · E) over the mesh plus the world edges of the sample. The number of
    candidates sizes launches and tensors of a recorded step, so it must be fixed at construction; on a plate batch
    the world edges are under 1 % of the edges. What a feed with dynamic_edges= and random_edges= runs on CPU tensors,
    and what the kernels are tested against."""
    ei_w, _ = world_topology_torch(pos, node_type, graph_ptr, mesh_edge_index, radius, max_neighbors)
    return random_topology_torch(pairs.to(pos.device), graph_ptr, ei_w, max_new, enabled, cand_ptr=cand_ptr)


def check_rollout_columns(F, y_columns, out_columns, prev_columns, node_type_index):
    """The host-side preconditions of a resident rollout (ValueError): the model's output columns, the target
    columns and, when used, the previous-data columns have one width d; the output and previous-data ranges
    lie inside [0, F), do not overlap, and do not contain the node-type column (the rollout writes them,
    and reads the node type of the written row). For a world_pos= feed F is the batch width (the frame's + 3)
    and the output, previous-data and node-type columns are batch-layout columns; y_columns stay frame columns
    (only their width is compared); for an aneurysm= feed F is the batch width too (the frame's + 10). Returns d."""
    (ys, ye), (os_, oe) = (int(v) for v in y_columns), (int(v) for v in out_columns)
    d = oe - os_
    if d < 1 or not 0 <= os_ < oe <= F:
        raise ValueError(f"output columns ({os_}, {oe}) must be a non-empty range inside [0, {F})")
    if ye - ys != d:
        raise ValueError(f"the feed's y_columns ({ys}, {ye}) and the output columns ({os_}, {oe}) differ in width")
    k = int(node_type_index)
    if os_ <= k < oe:
        raise ValueError(f"node_type_index {k} lies inside the output columns ({os_}, {oe})")
    if prev_columns is not None:
        ps, pe = (int(v) for v in prev_columns)
        if not 0 <= ps < pe <= F:
            raise ValueError(f"previous-data columns ({ps}, {pe}) must be a non-empty range inside [0, {F})")
        if pe - ps != d:
            raise ValueError(f"previous-data columns ({ps}, {pe}) and the output columns ({os_}, {oe}) differ in width")
        if ps < oe and os_ < pe:
            raise ValueError(f"previous-data columns ({ps}, {pe}) overlap the output columns ({os_}, {oe})")
        if ps <= k < pe:
            raise ValueError(f"node_type_index {k} lies inside the previous-data columns ({ps}, {pe})")
    return d


def rollout_begin_torch(traj, graph_ptr, frame, cursor, y_columns, out_columns, prev_columns, last, last_prev, x, y):
    """mgn_rollout_begin's rule as torch ops on any device, in place on x [N, >= F] and y [N, d]: with
    s = cursor (a one-element int tensor or an int) x[:, :F] = frame[g] + s of traj for the nodes of graph g,
    then, when s > 0, x[:, out_columns] = last and x[:, prev_columns] = last_prev (prev_columns None: no
    previous data); y = y_columns of the following frame. traj is only read. The CPU path of
    Rollout.rollout_resident, and what the kernel is tested and timed against."""
    T, N, F = traj.shape
    s = int(cursor)
    rows = torch.arange(N, device=traj.device)
    t = frame.to(traj.device, torch.int64)[_node_graph(graph_ptr, N, traj.device)] + s
    x[:, :F] = traj[t, rows]
    if s > 0:
        x[:, out_columns[0]:out_columns[1]] = last
        if prev_columns is not None and prev_columns[1] > prev_columns[0]:
            x[:, prev_columns[0]:prev_columns[1]] = last_prev
    y.copy_(traj[t + 1, rows, y_columns[0]:y_columns[1]])


def rollout_begin_world_torch(traj, graph_ptr, frame, cursor, y_columns, type_index, out_columns, prev_columns, last,
                              last_prev, x, y, obstacle_mean, world_clean=None):
    """mgn_rollout_begin_world's rule as torch ops on any device, in place on x [N, >= F + 3], y [N, d],
    obstacle_mean [B, 3] and world_clean [N, 3] (None: not kept): with s = cursor (a one-element int tensor or an
    int) and t = frame[g] + s, fill_world_torch's noise-free batch of frame t — x[:, :F + 3] = [world(3), obstacle
    displacement(3), the other frame columns], y = y_columns of frame t + 1, obstacle_mean — then, when s > 0,
    x[:, out_columns] = last and x[:, prev_columns] = last_prev in BATCH-layout columns (prev_columns None: no
    previous data): the displacement and the mean always come from the clean frames, as in the reference, whose
    dataset item is built before _make_prediction writes the prediction back. world_clean = the clean world
    positions of frame t. type_index is the node-type column of a frame row. A graph whose t is outside [0, T - 2]
    is left alone: its rows of x, y and world_clean and its row of obstacle_mean. traj is only read. The CPU path
    of Rollout.rollout_resident on a world_pos= feed, and what the kernel is tested and timed against."""
    T, N, F = traj.shape
    s = int(cursor)
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    t = frame.to(traj.device, torch.int64) + s
    valid = (t >= 0) & (t <= T - 2)
    fx, fy, mean = fill_world_torch(traj, gp, t.clamp(0, T - 2), y_columns, type_index, [], None, None)
    if s > 0:
        fx[:, out_columns[0]:out_columns[1]] = last
        if prev_columns is not None and prev_columns[1] > prev_columns[0]:
            fx[:, prev_columns[0]:prev_columns[1]] = last_prev
    clean = traj[t.clamp(0, T - 2)[_node_graph(gp, N, traj.device)], torch.arange(N, device=traj.device), 0:3]
    if bool(valid.all()):
        x[:, :F + 3] = fx
        y.copy_(fy)
        obstacle_mean.copy_(mean)
        if world_clean is not None:
            world_clean.copy_(clean)
        return
    rows = valid[_node_graph(gp, N, traj.device)]
    x[:, :F + 3] = torch.where(rows[:, None], fx, x[:, :F + 3])
    y.copy_(torch.where(rows[:, None], fy, y))
    obstacle_mean.copy_(torch.where(valid[:, None], mean, obstacle_mean))
    if world_clean is not None:
        world_clean.copy_(torch.where(rows[:, None], clean, world_clean))


def rollout_begin_aneurysm_torch(traj, graph_ptr, frame, cursor, y_columns, pos, node_type, stats, out_columns,
                                 prev_columns, last, last_prev, x, y):
    """mgn_rollout_begin_aneurysm's rule as torch ops on any device, in place on x [N, >= F + 10] and y [N, d]: with
    s = cursor (a one-element int tensor or an int) and t = frame[g] + s, fill_aneurysm_torch's noise-free batch of
    frame t — x[:, :F + 10] = [frame row ‖ a − p ‖ pos ‖ stats[t, g] ‖ node_type], y = y_columns of frame t + 1 —
    then, when s > 0, x[:, out_columns] = last and x[:, prev_columns] = last_prev in BATCH-layout columns
    (prev_columns None: no previous data). With prev_columns (F, F + 3) the acceleration columns carry the previous
    step's predicted − current, the reference's use_previous_data; without them they follow the clean frames. The
    statistics always come from the clean-frame table, as in the reference, whose dataset item is built before
    _make_prediction writes the prediction back. A graph whose t is outside [1, T − 2] (frame t − 1 is read too) is
    left alone: none of its rows of x or y is written. traj, pos, node_type and stats are only read. The CPU path
    of Rollout.rollout_resident on an aneurysm= feed, and what the kernel is tested and timed against."""
    T, N, F = traj.shape
    s = int(cursor)
    gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
    t = frame.to(traj.device, torch.int64) + s
    valid = (t >= 1) & (t <= T - 2)
    fx, fy = fill_aneurysm_torch(traj, gp, t.clamp(1, T - 2), pos, node_type, stats, y_columns, [], None, None)
    if s > 0:
        fx[:, out_columns[0]:out_columns[1]] = last
        if prev_columns is not None and prev_columns[1] > prev_columns[0]:
            fx[:, prev_columns[0]:prev_columns[1]] = last_prev
    if bool(valid.all()):
        x[:, :F + 10] = fx
        y.copy_(fy)
        return
    rows = valid[_node_graph(gp, N, traj.device)]
    x[:, :F + 10] = torch.where(rows[:, None], fx, x[:, :F + 10])
    y.copy_(torch.where(rows[:, None], fy, y))


def rollout_end_torch(out, y, x, node_type_index, masks, out_start, last, last_prev, preds, cursor, loss, sq):
    """mgn_rollout_end's rule as torch ops on any device, in place on its state: with s = cursor,
    pred = y where the node type x[:, node_type_index] is neither NORMAL nor OUTFLOW (training.rollout.build_mask)
    and out elsewhere; last_prev = pred - x[:, out columns] (None: not kept), last = pred, preds[s] = pred (None:
    not kept), loss[s] = masked_mse(y, pred, node type, masks) — masked_mse itself —, sq[s] = Σ (pred - y)²,
    cursor += 1 (cursor: a one-element int tensor). Returns pred."""
    from graphphysics.utils.loss import masked_mse

    s = int(cursor)
    d = out.shape[1]
    node_type = x[:, node_type_index]
    keep = torch.logical_not(torch.logical_or(node_type == NodeType.NORMAL, node_type == NodeType.OUTFLOW))
    pred = torch.where(keep[:, None], y, out)
    if last_prev is not None:
        last_prev.copy_(pred - x[:, out_start:out_start + d])
    last.copy_(pred)
    if preds is not None:
        preds[s] = pred
    loss[s] = masked_mse(y, pred, node_type, list(masks))
    sq[s] = ((pred - y) ** 2).sum()
    cursor += 1
    return pred


class ResidentTrajectories:
    """traj: fp32 [T, N, F] on the device, N the nodes of the batch's graphs concatenated (as
    meshes.cylinder_batch lays them out), every graph with the same T frames. graph_ptr: [B+1] node offsets
    (host list or tensor; validated). y_columns = (start, end): the columns of the next frame that are the
    target. noise: the reference's noise_parameters dict (noise_index_start / noise_index_end / noise_scale
    as an int, a float or lists; its node_type_index must equal node_type_index) or None. frames: "random"
    (every fill draws one frame per graph, uniform over the frames that have a successor) or explicit
    per-graph frames (see set_frames).

    frame [B] int32, z [N, W] fp32 (None without noise) and scales [n] fp32 (None without noise) are
    allocated once and only rewritten: a captured graph keeps reading the same addresses, tests and users
    read there what the last fill used. Not supported: previous_data (except with aneurysm=, below), trajectories
    of unequal length (module docstring).

    rotate: None, or the rotation augmentation of the reference's Random3DRotate, one rotation per graph and
    fill, as a dict
      {"feature_indices": [(0, 3), (4, 7)],   # column triples of x (its argument); list position columns too
       "edge_attr": clean_edge_attr,          # optional: fp32 [E, A] kept clean on the device
       "edge_index": edge_index,              # required with edge_attr: [2, E]
       "edge_feature_indices": [(0, 3)]}      # column triples of edge_attr; default [(0, 3)]
    y_columns must be 3 wide then: y is rotated too. angles [B, 3] (radians: alpha about z, beta about y,
    gamma about x) and R [B, 9] (row-major 3x3 per graph) are persistent like frame and z; row_graph [E] int32
    is the graph of every edge, built once. fill writes the rotated edge_attr into batch.edge_attr[:, :A]; the
    clean edge_attr, like traj, is only read. batch.pos is not touched (no model here reads it in the step).
    See set_rotations.

    world_pos: None, or the reference's world_pos_parameters (Lagrangian data such as DeformingPlate: world
    position in frame columns [0, 3)) plus the edge side, as a dict
      {"world_pos_index_start": 0, "world_pos_index_end": 3,   # the reference hard-codes the width 3
       "node_type_index": node_type_index + 3,                 # batch layout, as the config writes it
       "edge_index": edge_index,                               # optional: [2, E], static for the life of the feed
       "edge_attr_start": 4}                                   # required with edge_index: first written column
    The batch row is then F + 3 wide, [world(3), obstacle displacement(3), the other frame columns], so the
    node type of frame column node_type_index sits in batch column node_type_index + 3; noise's indices and its
    node_type_index are in that batch layout too. y_columns must begin with the world position (start 0, end
    >= 3). Every graph needs an OBSTACLE node: checked on frame 0, node types are assumed constant over the
    frames. obstacle_mean [B, 3] is persistent like frame and z; senders / receivers [E] int32 are built once.
    With an edge side fill writes batch.edge_attr[:, edge_attr_start : edge_attr_start + 4] from the noisy x and
    touches no other column (the mesh's Cartesian ‖ Distance columns stay). Not together with rotate=.

    dynamic_edges: None, or per-fill world edges for a model without edge_attr, with world_pos= (without its
    edge_index / edge_attr_start), as a dict
      {"edge_index": mesh_ei,    # [2, E_m]: the whole batch's block-diagonal mesh edges as FaceToEdge + to_undirected
                                 # emit them: sorted by (row, col), unique, symmetric, no self-loops, no edge across
                                 # two graphs — checked once here (check_mesh_edges)
       "radius": 0.03,           # the reference's add_world_edges radius
       "max_neighbors": 16}      # capacity: the most world neighbours one node may have
    The feed then owns topology (models._engine.DynamicTopology; None on CPU tensors), edge_index (int64 [2, E_cap],
    E_cap = E_m + N · max_neighbors: the tensor the caller puts into batch.edge_index; its first num_edges columns are
    the reference's edge_index of the last fill, the rest is unspecified) and num_edges_dev (int32 [1]). fill rebuilds
    them after the noise from batch.x[:, 0:3] and the batch's node-type column, as the reference's add_world_edges
    reads them. A node with more than max_neighbors world neighbours is an error: on the device the step's optimizer
    update is skipped and the next poll raises ValueError (MGN_ERR_WORLD_CAPACITY), on CPU tensors fill raises at
    once. Node types are those of frame 0, as world_pos= assumes. Not together with rotate= or aneurysm=. Its
    validation rollout: Rollout(..., feed=, world_edges="frame" | "prediction").

    aneurysm: None, or {"pos": pos} — pos fp32 [N, 3] on the feed's device, static and only read — for the row of
    the reference's external/aneurysm.py build_features. Frame rows are [velocity (3), wall flag (column 3), ...],
    F >= 4, T >= 3. The batch row is F + 10 wide, [frame row ‖ a − p ‖ pos ‖ mean, min, max ‖ node type], so
    node_type_index and the noise's node_type_index are the batch column F + 9, and the noise's indices are in
    that layout too (up to 8 ranges in this mode). Built once, persistent and only rewritten like frame and z:
    node_type [N] from frame 0 (the wall flag is assumed constant over the frames, as world_pos= assumes of node
    types), inflow_ptr [B + 1] / inflow_rows (the inflow nodes of every graph) and inflow_stats [T − 1, B, 3],
    the statistics of every frame that has a successor; refresh_stats() recomputes that table. Frames are drawn
    over [1, T − 2] (frame t − 1 is read) and set_frames refuses 0. A graph whose inflow nodes make more than
    MGN_FEED_INFLOW_CAPACITY values is refused. Not together with rotate= or world_pos=. Its validation rollout:
    Rollout(..., feed=, acceleration="frame" | "prediction").

    random_edges: None, or new random long-range edges on every fill for a model without edge_attr (module docstring),
    as a dict
      {"edge_index": mesh_ei,    # [2, E_m]: the batch's mesh edges, check_mesh_edges' preconditions as for dynamic_edges
       "ratio": 0.5,             # the reference's dataset.new_edges_ratio, in (0, 1]
       "max_new": 16}            # capacity: the most new neighbours one node may get, in [1, 64]; more are dropped
    The feed then owns topology (models._engine.RandomTopology; None on CPU tensors), edge_index (int64 [2, E_cap],
    E_cap = E_m + N · max_new: the tensor the caller puts into batch.edge_index), num_edges_dev (int32 [1]), pairs
    (int32 [C, 2], the candidates of the last fill), cand_ptr (int32 [B + 1]) and random_enabled (int32 [1]). fill
    draws pairs and calls build_random_edges(). set_random_edges(False) makes every build write the mesh adjacency
    (validation) without a new recording; set_pairs gives explicit pairs (tests). With the plain fill, with aneurysm=
    and with a world_pos= that has no edge side; not with a rotate= that carries an edge_attr or a world_pos= with an
    edge_index. Rollout.rollout_resident on such a feed does not rebuild: it runs on the topology of the last
    build_random_edges(); for validation, feed.set_random_edges(False); feed.build_random_edges().

    one_topology: True with both dynamic_edges= and random_edges= (the two edge_index tensors must be equal; without
    one_topology=True the two together raise ValueError, as they did before this mode existed): ONE topology
    (models._engine.WorldRandomTopology) of the capacity E_cap = E_m + N · (max_neighbors + max_new) holds mesh ∪ world
    ∪ random edges. fill does the world fill and the noise, draws pairs, then runs one build_edges on the noisy x
    (world_random_topology_torch's rule). build_edges(pos, node_type) is the combined build, with the feed's current
    pairs and random_enabled; build_random_edges() raises ValueError (it has no positions). set_random_edges, set_pairs
    and current_edge_index work as above; a node over max_neighbors is an error, a node over max_new drops. Its
    validation rollout: set_random_edges(False), then Rollout(..., feed=, world_edges="frame" | "prediction"), which
    rebuilds every step and draws nothing."""

    ROTATE_KEYS = ("feature_indices", "edge_attr", "edge_index", "edge_feature_indices")
    WORLD_KEYS = ("world_pos_index_start", "world_pos_index_end", "node_type_index", "edge_index", "edge_attr_start")
    ANEURYSM_KEYS = ("pos",)
    DYNAMIC_KEYS = ("edge_index", "radius", "max_neighbors")
    RANDOM_KEYS = ("edge_index", "ratio", "max_new")

    def __init__(self, traj, graph_ptr, y_columns, node_type_index, noise=None, frames="random", rotate=None,
                 world_pos=None, aneurysm=None, dynamic_edges=None, random_edges=None, one_topology=False):
        if not torch.is_tensor(traj) or traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
            raise ValueError("traj must be a contiguous fp32 [T, N, F] tensor")
        T, N, F = traj.shape
        if T < 2:
            raise ValueError("traj needs at least 2 frames: x is frame t, y comes from frame t + 1")
        gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
        if len(gp) < 2 or gp[0] != 0 or gp[-1] != N or any(b < a for a, b in zip(gp, gp[1:])):
            raise ValueError(f"graph_ptr must hold B + 1 non-decreasing node offsets from 0 to N = {N}, got {gp}")
        ys, ye = int(y_columns[0]), int(y_columns[1])
        if not 0 <= ys < ye <= F:
            raise ValueError(f"y_columns ({ys}, {ye}) must be a non-empty range inside [0, {F}]")
        # aneurysm=: the batch row is [frame row ‖ a − p ‖ pos ‖ mean, min, max ‖ node type], 10 wider than a frame
        # row, and the node type is its last column, F + 9: no column of a frame row
        self.aneurysm = aneurysm is not None
        if self.aneurysm:
            if rotate is not None or world_pos is not None:
                raise ValueError("aneurysm= together with rotate= or world_pos= is not supported")
            if int(node_type_index) != F + 9:
                raise ValueError(f"with aneurysm=, node_type_index {node_type_index} must be the batch column F + 9 = "
                                 f"{F + 9} (the last column of the row build_features makes)")
        elif not 0 <= int(node_type_index) < F:
            raise ValueError(f"node_type_index {node_type_index} is outside [0, {F})")
        if dynamic_edges is not None:
            if rotate is not None or aneurysm is not None:
                raise ValueError("dynamic_edges= together with rotate= or aneurysm= is not supported")
            if world_pos is None:
                raise ValueError("dynamic_edges= needs world_pos=: the world edges follow the world positions")
        if one_topology and (dynamic_edges is None or random_edges is None):
            raise ValueError("one_topology=True needs both dynamic_edges= and random_edges=")
        if random_edges is not None:
            if dynamic_edges is not None and not one_topology:
                # as before this mode existed: the two are not silently merged, the caller asks for it
                raise ValueError("random_edges= together with dynamic_edges= is not supported: one topology per feed "
                                 "(one_topology=True builds both into one, E_cap = E_m + N * (max_neighbors + "
                                 "max_new))")
            if isinstance(rotate, dict) and rotate.get("edge_attr") is not None:
                raise ValueError("random_edges= together with a rotate= that carries an edge_attr is not supported: "
                                 "models with edge_attr are not supported (their launch shapes depend on the edge "
                                 "count)")
            if isinstance(world_pos, dict) and world_pos.get("edge_index") is not None:
                raise ValueError("random_edges= needs a world_pos= without edge_index / edge_attr_start: models with "
                                 "edge_attr are not supported (their launch shapes depend on the edge count)")
        self.traj, self.T, self.N, self.F, self.B = traj, T, N, F, len(gp) - 1
        self.y_columns, self.node_type_index = (ys, ye), int(node_type_index)
        dev = traj.device
        self.graph_ptr = torch.tensor(gp, dtype=torch.int32, device=dev)
        self.ranges, self._base_scales, self.scales, self.z = [], [], None, None
        # world_pos=: the batch row is [world(3), displacement(3), the other columns], 3 wider than a frame row
        self.world = world_pos is not None
        self.obstacle_mean, self.senders, self.receivers, self.edge_attr_start = None, None, None, None
        if self.world:
            if rotate is not None:
                raise ValueError("rotate= together with world_pos= is not supported")
            self._init_world(world_pos, gp)
        # dynamic_edges=: the world edges of every fill, as a topology rebuilt in place (see build_edges)
        self.dynamic = dynamic_edges is not None
        # random_edges=: new long-range edges on every fill, as a topology rebuilt in place (see build_random_edges).
        # With dynamic_edges= as well: ONE topology of mesh ∪ world ∪ random edges, rebuilt by build_edges
        self.random = random_edges is not None
        self.topology, self.edge_index, self.num_edges_dev, self.topology_arrays = None, None, None, None
        if self.dynamic:
            self._init_dynamic(dynamic_edges, gp)
        self.pairs, self.cand_ptr, self.random_enabled = None, None, None
        self.random_pairs = None  # None: no random edges; True: drawn on every fill; False: explicit pairs
        if self.random:
            self._init_random(random_edges, gp)
        if self.dynamic and self.random:
            self._init_world_random(gp)
        self.pos, self.node_type, self.inflow_stats, self.inflow_ptr, self.inflow_rows = None, None, None, None, None
        if self.aneurysm:
            self._init_aneurysm(aneurysm, gp)
        self.Fx = F + 10 if self.aneurysm else F + 3 if self.world else F  # the width of a batch row
        type_column = self.node_type_index + 3 if self.world else self.node_type_index
        if noise is not None:
            if int(noise["node_type_index"]) != type_column:
                raise ValueError(f"noise node_type_index {noise['node_type_index']} differs from node_type_index "
                                 f"{type_column}" + (" (batch layout: the frame's node_type_index + 3)"
                                                     if self.world else ""))
            start, end, self._base_scales = _noise_lists(noise)
            self.ranges = list(zip(start, end))
            if self.aneurysm:
                _check_ranges(self.ranges, self.Fx, nat.MGN_FEED_ANEURYSM_MAX_RANGES)
            else:
                _check_ranges(self.ranges, self.Fx)
            if (self.world or self.aneurysm) and any(s <= type_column < e for s, e in self.ranges):
                raise ValueError(f"a noisy column range contains the node type (batch column {type_column})")
            width = sum(e - s for s, e in self.ranges)
            if width > 0:
                self.scales = torch.tensor(self._base_scales, dtype=torch.float32, device=dev)
                self.z = torch.zeros(N, width, dtype=torch.float32, device=dev)
        self._ranges_c = nat.feed_ranges8(self.ranges) if self.aneurysm else nat.feed_ranges(self.ranges)
        self.frame = torch.full((self.B,), 1 if self.aneurysm else 0, dtype=torch.int32, device=dev)
        self.random_frames = True
        self.set_frames(frames)
        self.triples, self.angles, self.R = [], None, None
        self.edge_attr, self.edge_triples, self.row_graph = None, [], None
        self.random_rotations = None  # None: no rotation; True: drawn on every fill; False: explicit angles
        if rotate is not None:
            self._init_rotate(rotate, gp)

    def _init_world(self, wp, gp):
        if not isinstance(wp, dict) or any(k not in self.WORLD_KEYS for k in wp):
            raise ValueError(f"world_pos must be a dict with keys among {self.WORLD_KEYS}, got {wp!r}")
        dev, k, F, N = self.traj.device, self.node_type_index, self.F, self.N
        try:
            ws, we, nti = (int(wp[key]) for key in self.WORLD_KEYS[:3])
        except KeyError as ex:
            raise ValueError(f"world_pos needs {ex.args[0]}") from None
        if ws != 0 or we - ws != 3:
            raise ValueError(f"world_pos columns ({ws}, {we}) must be (0, 3): the reference's displacement is 3 wide "
                             "and the columns ahead of the world position are dropped")
        if F < 4 or k < 3:
            raise ValueError(f"world_pos needs frame rows [world(3), ..., node type, ...]: F = {F} >= 4 and "
                             f"node_type_index = {k} >= 3")
        if nti != k + 3:
            raise ValueError(f"world_pos node_type_index {nti} differs from node_type_index + 3 = {k + 3} (the batch "
                             "layout, after the 3 displacement columns are inserted)")
        ys, ye = self.y_columns
        if ys != 0 or ye < 3:
            raise ValueError(f"with world_pos, y_columns ({ys}, {ye}) must begin with the world position: start 0, "
                             "end >= 3")
        obstacle = self.traj[0, :, k] == NodeType.OBSTACLE
        for g in range(self.B):
            if not bool(obstacle[gp[g]:gp[g + 1]].any()):
                raise ValueError(f"graph {g} has no OBSTACLE node in frame 0: its mean obstacle displacement is "
                                 "undefined (NaN in the reference)")
        ei, start = wp.get("edge_index"), wp.get("edge_attr_start")
        if (ei is None) != (start is None):
            raise ValueError("world_pos: edge_index and edge_attr_start go together")
        if ei is not None:
            if not torch.is_tensor(ei) or ei.dim() != 2 or ei.shape[0] != 2 or ei.is_floating_point() or \
                    ei.dtype == torch.bool:
                raise ValueError("world_pos edge_index must be an integer [2, E] tensor")
            if int(start) < 0:
                raise ValueError(f"world_pos edge_attr_start {start} must be >= 0")
            ei = ei.to(dev, torch.int64)
            if ei.shape[1] > 0 and (int(ei.min()) < 0 or int(ei.max()) >= N):
                raise ValueError(f"world_pos edge_index holds node ids outside [0, {N})")
            self.senders, self.receivers = ei[0].to(torch.int32).contiguous(), ei[1].to(torch.int32).contiguous()
            self.edge_attr_start, self._world_edge_index = int(start), ei
        self.obstacle_mean = torch.zeros(self.B, 3, dtype=torch.float32, device=dev)

    def _init_dynamic(self, de, gp):
        if not isinstance(de, dict) or any(k not in self.DYNAMIC_KEYS for k in de) or \
                any(k not in de for k in self.DYNAMIC_KEYS):
            raise ValueError(f"dynamic_edges must be a dict with the keys {self.DYNAMIC_KEYS}, got {de!r}")
        if self.senders is not None:
            raise ValueError("dynamic_edges= needs a world_pos= without edge_index / edge_attr_start: models with "
                             "edge_attr are not supported (their launch shapes depend on the edge count)")
        radius, W = de["radius"], de["max_neighbors"]
        if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0.0 < float(radius) < math.inf:
            raise ValueError(f"dynamic_edges radius {radius!r} must be a positive finite number")
        if isinstance(W, bool) or not isinstance(W, int) or W < 1:
            raise ValueError(f"dynamic_edges max_neighbors {W!r} must be an int >= 1")
        dev, N = self.traj.device, self.N
        mesh = check_mesh_edges(de["edge_index"], gp, N)
        E_cap = mesh.shape[1] + N * W
        if E_cap > 2 ** 31 - 1:
            raise ValueError(f"dynamic_edges: E_m + N * max_neighbors = {E_cap} does not fit int32")
        self.radius, self.max_neighbors, self._gp_list = float(radius), W, gp
        self.mesh_edge_index = mesh.to(dev)
        if self.random:
            return  # with random_edges= as well: the one topology of both is made by _init_world_random
        if dev.type == "cuda":
            from graphphysics.models import _engine

            self.topology = _engine.DynamicTopology(mesh, gp, N, self.radius, W, dev)
            self.edge_index, self.num_edges_dev = self.topology.edge_index, self.topology.num_edges_dev
            _engine.bind_topology(self.edge_index, self.topology)
        else:
            self.edge_index = torch.zeros(2, max(E_cap, 1), dtype=torch.int64)
            self.num_edges_dev = torch.zeros(1, dtype=torch.int32)

    def _init_world_random(self, gp):
        """dynamic_edges= and random_edges= together, after both were checked: one topology of the capacity E_cap =
        E_m + N · (max_neighbors + max_new), rebuilt by build_edges."""
        dev, N, mesh = self.traj.device, self.N, self.mesh_edge_index.cpu()
        E_cap = mesh.shape[1] + N * (self.max_neighbors + self.max_new)
        if E_cap > 2 ** 31 - 1:
            raise ValueError(f"dynamic_edges + random_edges: E_m + N * (max_neighbors + max_new) = {E_cap} does not "
                             "fit int32")
        if dev.type == "cuda":
            from graphphysics.models import _engine

            self.topology = _engine.WorldRandomTopology(mesh, gp, N, self.radius, self.max_neighbors, self._cand_list,
                                                        self.max_new, dev)
            self.edge_index, self.num_edges_dev = self.topology.edge_index, self.topology.num_edges_dev
            _engine.bind_topology(self.edge_index, self.topology)
        else:
            self.edge_index = torch.zeros(2, max(E_cap, 1), dtype=torch.int64)
            self.num_edges_dev = torch.zeros(1, dtype=torch.int32)

    def build_edges(self, pos, node_type):
        """Rebuild the world edges from pos fp32 [N, >= 3] and node_type fp32 [N] (views of the batch's x): HIP
        tensors, mgn_world_topology_build into self.topology (device work only, capturable); CPU tensors,
        world_topology_torch into edge_index[:, :E], num_edges_dev and topology_arrays (a node over max_neighbors
        raises at once there; on the device it flags the error word). On a feed that has random_edges= as well: the
        combined build, mgn_world_random_topology_build / world_random_topology_torch, with the feed's current pairs
        and its random_enabled word (nothing is drawn here)."""
        if not self.dynamic:
            raise ValueError("build_edges: this feed was built without dynamic_edges=")
        if pos.is_cuda:
            if self.random:
                self.topology.build(pos, node_type, self.pairs, self.random_enabled)
            else:
                self.topology.build(pos, node_type)
            return
        if self.random:
            ei, arrays = world_random_topology_torch(pos, node_type, self.pairs, self._gp_list, self.mesh_edge_index,
                                                     self.radius, self.max_neighbors, self.max_new,
                                                     bool(int(self.random_enabled)), cand_ptr=self._cand_list)
        else:
            ei, arrays = world_topology_torch(pos, node_type, self._gp_list, self.mesh_edge_index, self.radius,
                                              self.max_neighbors)
        self.edge_index[:, :ei.shape[1]] = ei
        self.num_edges_dev.fill_(ei.shape[1])
        self.topology_arrays = arrays

    def current_edge_index(self):
        """edge_index[:, :num_edges] of the last build, a view (reads the count back: for CPU models and tests)."""
        if not self.dynamic and not self.random:
            raise ValueError("current_edge_index: this feed was built without dynamic_edges=")
        return self.edge_index[:, :int(self.num_edges_dev)]

    def _init_random(self, re, gp):
        if not isinstance(re, dict) or any(k not in self.RANDOM_KEYS for k in re) or \
                any(k not in re for k in self.RANDOM_KEYS):
            raise ValueError(f"random_edges must be a dict with the keys {self.RANDOM_KEYS}, got {re!r}")
        ratio, W = re["ratio"], re["max_new"]
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"random_edges ratio {ratio!r} must lie in (0, 1] (the reference's new_edges_ratio)")
        if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= nat.RANDOM_MAX_NEW:
            raise ValueError(f"random_edges max_new {W!r} must be an int in [1, {nat.RANDOM_MAX_NEW}]")
        dev, N = self.traj.device, self.N
        mesh = check_mesh_edges(re["edge_index"], gp, N)
        if self.dynamic and not torch.equal(mesh, self.mesh_edge_index.cpu()):
            raise ValueError("dynamic_edges= and random_edges= must be given the same edge_index: one mesh, one "
                             "topology per feed")
        E_cap = mesh.shape[1] + N * W
        if E_cap > 2 ** 31 - 1:
            raise ValueError(f"random_edges: E_m + N * max_new = {E_cap} does not fit int32")
        self.ratio, self.max_new, self._gp_list = float(ratio), W, gp
        self._cand_list = random_candidate_ptr(gp, mesh, self.ratio)
        self.mesh_edge_index = mesh.to(dev)
        self.cand_ptr = torch.tensor(self._cand_list, dtype=torch.int32, device=dev)
        self.pairs = torch.zeros(self._cand_list[-1], 2, dtype=torch.int32, device=dev)
        self.random_enabled = torch.ones(1, dtype=torch.int32, device=dev)
        self.random_pairs = True
        if self.dynamic:
            return  # with dynamic_edges= as well: the one topology of both is made by _init_world_random
        if dev.type == "cuda":
            from graphphysics.models import _engine

            self.topology = _engine.RandomTopology(mesh, gp, N, self._cand_list, W, dev)
            self.edge_index, self.num_edges_dev = self.topology.edge_index, self.topology.num_edges_dev
            _engine.bind_topology(self.edge_index, self.topology)
        else:
            self.edge_index = torch.zeros(2, max(E_cap, 1), dtype=torch.int64)
            self.num_edges_dev = torch.zeros(1, dtype=torch.int32)

    def build_random_edges(self):
        """Rebuild the topology from the feed's pairs and its random_enabled word: HIP tensors,
        mgn_random_topology_build into self.topology (device work only, capturable); CPU tensors,
        random_topology_torch into edge_index[:, :E], num_edges_dev and topology_arrays. fill calls it after its draw;
        for validation, feed.set_random_edges(False); feed.build_random_edges() leaves the mesh adjacency."""
        if not self.random:
            raise ValueError("build_random_edges: this feed was built without random_edges=")
        if self.dynamic:
            raise ValueError("build_random_edges: this feed has dynamic_edges= as well, its one topology needs the "
                             "positions: use build_edges(pos, node_type)")
        if self.pairs.is_cuda:
            self.topology.build(self.pairs, self.random_enabled)
            return
        ei, arrays = random_topology_torch(self.pairs, self._gp_list, self.mesh_edge_index, self.max_new,
                                           bool(int(self.random_enabled)), cand_ptr=self._cand_list)
        self.edge_index[:, :ei.shape[1]] = ei
        self.num_edges_dev.fill_(ei.shape[1])
        self.topology_arrays = arrays

    def set_random_edges(self, enabled):
        """Switch the random edges off (every build then writes the mesh adjacency: validation) or on again. Rewrites
        the persistent random_enabled word, which a captured graph reads at replay: no re-capture."""
        if not self.random:
            raise ValueError("set_random_edges: this feed was built without random_edges=")
        self.random_enabled.fill_(1 if enabled else 0)

    def set_pairs(self, pairs):
        """"random" (the default of a feed with random_edges=): every fill draws pairs.random_(0, 2**31 - 1). An integer
        [C, 2] host list / CPU tensor of non-negative values below 2**31: the fills use these until the next
        set_pairs (for tests). ValueError without random_edges=, or for another shape."""
        if not self.random:
            raise ValueError("set_pairs: this feed was built without random_edges=")
        C = self.pairs.shape[0]
        if isinstance(pairs, str):
            if pairs != "random":
                raise ValueError(f'pairs must be "random" or an integer [{C}, 2] tensor, got {pairs!r}')
            self.random_pairs = True
            return
        p = torch.as_tensor(pairs).cpu()
        if p.is_floating_point() or p.dtype == torch.bool or tuple(p.shape) != (C, 2):
            raise ValueError(f"expected integer pairs [{C}, 2], got {tuple(p.shape)} {p.dtype}")
        if C and (int(p.min()) < 0 or int(p.max()) > 2 ** 31 - 1):
            raise ValueError("pairs must lie in [0, 2**31 - 1]")
        self.random_pairs = False
        self.pairs.copy_(p.to(torch.int32))

    def _fill_random(self):
        if self.random_pairs:
            self.pairs.random_(0, 2 ** 31 - 1)  # torch's generator: recorded, and new on every replay
        self.build_random_edges()

    def _init_aneurysm(self, an, gp):
        if not isinstance(an, dict) or any(k not in self.ANEURYSM_KEYS for k in an) or "pos" not in an:
            raise ValueError(f"aneurysm must be a dict with keys among {self.ANEURYSM_KEYS} ('pos' is required), "
                             f"got {an!r}")
        dev, F, N, T = self.traj.device, self.F, self.N, self.T
        if F < 4:
            raise ValueError(f"aneurysm needs frame rows [velocity (3), wall flag, ...]: F = {F} >= 4")
        if T < 3:
            raise ValueError(f"aneurysm needs at least 3 frames (x reads frames t - 1 and t, y frame t + 1), got T = {T}")
        pos = an["pos"]
        if not torch.is_tensor(pos) or pos.dtype != torch.float32 or tuple(pos.shape) != (N, 3) or \
                pos.device != dev or not pos.is_contiguous():
            raise ValueError(f"aneurysm pos must be a contiguous fp32 [{N}, 3] tensor on {dev}")
        from graphphysics.external.aneurysm import node_type_of

        self.pos = pos
        self.node_type = node_type_of(self.traj[0], pos).contiguous()  # the wall flag of frame 0: assumed constant
        inflow = self.node_type == NodeType.INFLOW
        self._inflow_mask = inflow
        counts = torch.stack([inflow[gp[g]:gp[g + 1]].sum() for g in range(self.B)]).tolist()
        # the size of a graph's value set: three components per inflow node, and the zero of the other nodes
        sizes = [3 * m + (1 if m < gp[g + 1] - gp[g] else 0) for g, m in enumerate(counts)]
        cap = nat.MGN_FEED_INFLOW_CAPACITY
        for g, values in enumerate(sizes):
            if values > cap:
                raise ValueError(f"graph {g} has {counts[g]} inflow nodes: its value set of {values} accelerations "
                                 f"exceeds the capacity of {cap} values of mgn_feed_inflow_stats")
        self._max_values = max(sizes)
        ptr = [0]
        for m in counts:
            ptr.append(ptr[-1] + m)
        self.inflow_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
        self.inflow_rows = torch.nonzero(inflow).reshape(-1).to(torch.int32).contiguous()  # ascending: grouped by graph
        self.inflow_stats = torch.zeros(T - 1, self.B, 3, dtype=torch.float32, device=dev)
        self._gp = gp
        self.refresh_stats()

    def refresh_stats(self):
        """Recompute inflow_stats [T − 1, B, 3] from traj, in place (after the caller rewrote frames of traj; the
        node types and the inflow node lists stay those of construction). HIP tensors: one mgn_feed_inflow_stats
        launch; CPU tensors: inflow_stats_torch per (frame, graph)."""
        if not self.aneurysm:
            raise ValueError("refresh_stats: this feed was built without aneurysm=")
        with torch.no_grad():
            if self.traj.is_cuda:
                nat.feed_inflow_stats(self.traj, self.graph_ptr, self.inflow_ptr, self.inflow_rows, self._max_values,
                                      self.inflow_stats)
                return
            gp = self._gp
            for t in range(self.T - 1):
                for g in range(self.B):
                    rows = slice(gp[g], gp[g + 1])
                    self.inflow_stats[t, g] = inflow_stats_torch(self.traj[t, rows], self.traj[t + 1, rows],
                                                                 self._inflow_mask[rows])

    def _init_rotate(self, rotate, gp):
        if not isinstance(rotate, dict) or any(k not in self.ROTATE_KEYS for k in rotate):
            raise ValueError(f"rotate must be a dict with keys among {self.ROTATE_KEYS}, got {rotate!r}")
        dev, k = self.traj.device, self.node_type_index
        self.triples = _check_triples(rotate.get("feature_indices") or [], self.F, "feature_indices", "x")
        if not self.triples:
            raise ValueError("rotate needs at least one column triple of x in feature_indices")
        for s, e in self.triples:
            if s <= k < e:
                raise ValueError(f"node_type_index {k} lies inside the rotated columns ({s}, {e})")
        ys, ye = self.y_columns
        if ye - ys != 3:
            raise ValueError(f"with rotate, y_columns ({ys}, {ye}) must be 3 wide: y is rotated as one 3D vector")
        ea, ei = rotate.get("edge_attr"), rotate.get("edge_index")
        if ea is None:
            if ei is not None or rotate.get("edge_feature_indices") is not None:
                raise ValueError("rotate: edge_index / edge_feature_indices are given without edge_attr")
        else:
            if not torch.is_tensor(ea) or ea.dtype != torch.float32 or ea.dim() != 2 or ea.device != dev or \
                    not ea.is_contiguous():
                raise ValueError(f"rotate edge_attr must be a contiguous fp32 [E, A] tensor on {dev}")
            E, A = ea.shape
            if not torch.is_tensor(ei) or ei.dim() != 2 or tuple(ei.shape) != (2, E) or ei.is_floating_point():
                raise ValueError(f"rotate edge_index must be an integer [2, {E}] tensor (required with edge_attr)")
            et = rotate.get("edge_feature_indices")
            self.edge_triples = _check_triples([(0, 3)] if et is None else et, A, "edge_feature_indices", "edge_attr")
            ei = ei.to(dev, torch.int64)
            if E > 0 and (int(ei.min()) < 0 or int(ei.max()) >= self.N):
                raise ValueError(f"rotate edge_index holds node ids outside [0, {self.N})")
            node_graph = _node_graph(gp, self.N, dev)
            g_src, g_dst = node_graph[ei[0]], node_graph[ei[1]]
            if E > 0 and not torch.equal(g_src, g_dst):
                bad = int(torch.nonzero(g_src != g_dst)[0])
                raise ValueError(f"edge {bad} joins nodes of different graphs: one rotation per graph cannot rotate it")
            self.edge_attr, self.row_graph = ea, g_src.to(torch.int32).contiguous()
        self._triples_c, self._edge_triples_c = nat.feed_ranges(self.triples), nat.feed_ranges(self.edge_triples)
        self.angles = torch.zeros(self.B, 3, dtype=torch.float32, device=dev)
        self.R = torch.zeros(self.B, 9, dtype=torch.float32, device=dev)
        self.random_rotations = True

    def set_rotations(self, angles):
        """"random" (the default of a feed with rotate=): every fill draws angles.uniform_(-π, π), one rotation
        per graph. A host list / CPU tensor [B, 3] of radians {alpha (z), beta (y), gamma (x)}: the fills use
        these until the next set_rotations. ValueError without rotate=, or for another shape."""
        if self.angles is None:
            raise ValueError("set_rotations: this feed was built without rotate=")
        if isinstance(angles, str):
            if angles != "random":
                raise ValueError(f'angles must be "random" or [{self.B}, 3] radians, got {angles!r}')
            self.random_rotations = True
            return
        a = torch.as_tensor(angles, dtype=torch.float32).cpu()
        if tuple(a.shape) != (self.B, 3):
            raise ValueError(f"expected three angles per graph, [{self.B}, 3], got {tuple(a.shape)}")
        if not bool(torch.isfinite(a).all()):
            raise ValueError("angles must be finite")
        self.random_rotations = False
        self.angles.copy_(a)

    def set_frames(self, frames):
        """"random": every fill draws its frames. A host list / CPU tensor of B frames, each in [0, T-2]
        ([1, T-2] with aneurysm=; ValueError otherwise): the fills use these until the next set_frames."""
        if isinstance(frames, str):
            if frames != "random":
                raise ValueError(f'frames must be "random" or B = {self.B} frame indices, got {frames!r}')
            self.random_frames = True
            return
        fr = [int(f) for f in (frames.tolist() if torch.is_tensor(frames) else frames)]
        if len(fr) != self.B:
            raise ValueError(f"expected one frame per graph ({self.B}), got {len(fr)}")
        if self.aneurysm and any(f < 1 or f > self.T - 2 for f in fr):
            raise ValueError(f"with aneurysm=, frames must lie in [1, {self.T - 2}] (frame t needs its predecessor "
                             f"t - 1 and its successor t + 1), got {fr}")
        if any(f < 0 or f > self.T - 2 for f in fr):
            raise ValueError(f"frames must lie in [0, {self.T - 2}] (frame t needs its successor t + 1), got {fr}")
        self.random_frames = False
        self.frame.copy_(torch.tensor(fr, dtype=torch.int32))

    def set_noise_t(self, t):
        """The reference's noise curriculum: scale_i = 10 · scale_i · (1 + cos(t π)); None: the plain scales.
        Rewrites the persistent scales tensor (a captured graph reads it at replay: no re-capture)."""
        if self.scales is None:
            return
        s = self._base_scales if t is None else [10 * b * (1 + math.cos(t * math.pi)) for b in self._base_scales]
        self.scales.copy_(torch.tensor(s, dtype=torch.float32))

    def fill(self, batch):
        """Write batch.x[:, :F] and batch.y in place: device work only, capturable. HIP tensors: the frame /
        noise draws and one mgn_feed_batch launch (no fallback); CPU tensors: fill_torch. With rotate=: the
        angle draw, mgn_feed_rotation_matrices, one mgn_feed_batch_rot in mgn_feed_batch's place and, when a
        clean edge_attr was given, one mgn_feed_rotate_rows into batch.edge_attr[:, :A]; CPU tensors: the
        reference's matrix per graph, fill_torch and rotate_rows_torch. With world_pos=: batch.x[:, :F + 3], one
        mgn_feed_batch_world (two launches) in mgn_feed_batch's place and, with an edge side, one
        mgn_feed_world_edge_features into batch.edge_attr[:, start:start + 4]; CPU tensors: fill_world_torch and
        world_edge_features_torch. With aneurysm=: batch.x[:, :F + 10], one mgn_feed_batch_aneurysm in
        mgn_feed_batch's place (the statistics table was built at construction); CPU tensors: fill_aneurysm_torch.
        With dynamic_edges=: after the world fill, build_edges on the noisy x (mgn_world_topology_build, three
        launches; CPU tensors: world_topology_torch), and batch.edge_index must be the feed's edge_index. With
        random_edges=: after any of these fills, the draw of pairs and build_random_edges (mgn_random_topology_build,
        a memset and five launches; CPU tensors: random_topology_torch), and batch.edge_index must be the feed's
        edge_index. With both: after the world fill, the draw of pairs and ONE build_edges on the noisy x
        (mgn_world_random_topology_build, a memset and six launches; CPU tensors: world_random_topology_torch)."""
        x, y = batch.x, batch.y
        if x.device != self.traj.device or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != self.N or \
                x.shape[1] < self.Fx:
            raise ValueError(f"batch.x must be fp32 [{self.N}, >= {self.Fx}] on {self.traj.device}, got "
                             f"{tuple(x.shape)} {x.dtype} on {x.device}")
        wy = self.y_columns[1] - self.y_columns[0]
        if y is None or y.device != x.device or y.dtype != torch.float32 or tuple(y.shape) != (self.N, wy):
            raise ValueError(f"batch.y must be fp32 [{self.N}, {wy}] on {self.traj.device}")
        rot = self.angles is not None
        ea = None
        if rot and self.edge_attr is not None:
            ea, (E, A) = getattr(batch, "edge_attr", None), self.edge_attr.shape
            if ea is None or ea.device != x.device or ea.dtype != torch.float32 or ea.dim() != 2 or \
                    ea.shape[0] != E or ea.shape[1] < A or (ea.shape[1] > 1 and ea.stride(1) != 1):
                raise ValueError(f"batch.edge_attr must be fp32 [{E}, >= {A}] on {self.traj.device}")
            if E > 0 and ea.data_ptr() == self.edge_attr.data_ptr():
                raise ValueError("batch.edge_attr is the feed's clean edge_attr: the fill would rotate it in place; "
                                 "give the batch a copy")
        wea = None
        if self.senders is not None:
            wea, E, A = getattr(batch, "edge_attr", None), self.senders.numel(), self.edge_attr_start + 4
            if wea is None or wea.device != x.device or wea.dtype != torch.float32 or wea.dim() != 2 or \
                    wea.shape[0] != E or wea.shape[1] < A or wea.stride(1) != 1:
                raise ValueError(f"batch.edge_attr must be fp32 [{E}, >= {A}] on {self.traj.device} with unit column "
                                 "stride")
        if self.dynamic and x.is_cuda and getattr(batch, "edge_index", None) is not self.edge_index:
            raise ValueError("with dynamic_edges=, batch.edge_index must be the feed's own edge_index tensor "
                             "(feed.edge_index): it is the handle of the topology the fill rebuilds")
        if self.random and x.is_cuda and getattr(batch, "edge_index", None) is not self.edge_index:
            raise ValueError("with random_edges=, batch.edge_index must be the feed's own edge_index tensor "
                             "(feed.edge_index): it is the handle of the topology the fill rebuilds")
        with torch.no_grad():
            if self.random_frames:
                # torch.randint(0, T-1, (B,)) into the persistent tensor; aneurysm=: frame t - 1 is read too
                self.frame.random_(1 if self.aneurysm else 0, self.T - 1)
            if self.z is not None:
                self.z.normal_()
            if self.aneurysm:
                if self.traj.is_cuda:
                    nat.feed_batch_aneurysm(self.traj, self.graph_ptr, self.frame, self.y_columns, self.pos,
                                            self.node_type, self.inflow_stats, self._ranges_c, self.scales, self.z,
                                            x, y)
                else:
                    fx, fy = fill_aneurysm_torch(self.traj, self.graph_ptr, self.frame, self.pos, self.node_type,
                                                 self.inflow_stats, self.y_columns, self.ranges, self.scales, self.z)
                    x[:, :self.Fx] = fx
                    y.copy_(fy)
                if self.random:
                    self._fill_random()
                return batch
            if self.world:
                if self.traj.is_cuda:
                    nat.feed_batch_world(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                                         self._ranges_c, self.scales, self.z, x, y, self.obstacle_mean)
                    if wea is not None:
                        nat.feed_world_edge_features(self.senders, self.receivers, x, wea, self.edge_attr_start)
                else:
                    fx, fy, mean = fill_world_torch(self.traj, self.graph_ptr, self.frame, self.y_columns,
                                                    self.node_type_index, self.ranges, self.scales, self.z)
                    x[:, :self.Fx] = fx
                    y.copy_(fy)
                    self.obstacle_mean.copy_(mean)
                    if wea is not None:
                        world_edge_features_torch(x, self._world_edge_index, wea, self.edge_attr_start)
                if self.dynamic:  # add_world_edges reads the (noisy) world positions and the batch's node types
                    if self.random and self.random_pairs:  # both: the draw, then ONE build of mesh ∪ world ∪ random
                        self.pairs.random_(0, 2 ** 31 - 1)
                    self.build_edges(x, x[:, self.node_type_index + 3])
                elif self.random:
                    self._fill_random()
                return batch
            if rot and self.random_rotations:
                self.angles.uniform_(-math.pi, math.pi)  # one rotation per graph, as the reference's per item
            if self.traj.is_cuda:
                if rot:
                    nat.feed_rotation_matrices(self.angles, self.R)
                    nat.feed_batch(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                                   self._ranges_c, self.scales, self.z, x, y, self._triples_c, self.R)
                    if ea is not None:
                        nat.feed_rotate_rows(self.edge_attr, self.row_graph, self._edge_triples_c, self.R, ea)
                else:
                    nat.feed_batch(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                                   self._ranges_c, self.scales, self.z, x, y)
            else:
                if rot:
                    from graphphysics.dataset.preprocessing import Random3DRotate

                    build = Random3DRotate()._build_rotation_matrix
                    if self.B:
                        self.R.copy_(torch.stack([build(*a).reshape(9) for a in self.angles.tolist()]))
                fx, fy = fill_torch(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                                    self.ranges, self.scales, self.z, self.triples, self.R)
                x[:, :self.F] = fx
                y.copy_(fy)
                if ea is not None:
                    ea[:, :self.edge_attr.shape[1]] = rotate_rows_torch(self.edge_attr, self.row_graph,
                                                                        self.edge_triples, self.R)
            if self.random:
                self._fill_random()
        return batch
