"""Shared by test_world_edges_cpu.py / test_world_edges_gpu.py: the reference fixture of per-frame world edges
(tests/golden/world_edges_golden.npz, written by tests/golden/make_world_edges_golden.py), the two-plate resident
trajectories built from it, a plain stable-sort restatement of mgn_topology_build, seeded random cases, the plate
transformer and the per-frame host loops (add_world_edges per graph, a fresh topology, then the step) that a
dynamic_edges= feed replaces."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
K = 3  # node-type column of a frame row [world(3), type]; batch column K + 3
N1 = 98  # nodes of one plate


def load_golden():
    z = np.load(os.path.join(G, "world_edges_golden.npz"))
    return {k: torch.from_numpy(z[k]) if z[k].ndim else float(z[k]) for k in z.files}


def plate(gold, dev=torch.device("cpu")):
    """(traj [5, 196, 4] on dev: the fixture's two graphs side by side, frame rows [world(3), node type], the
    fixture's four frames and the last one once more, so that frame 3 has a successor and can be drawn; node offsets;
    the batch's block-diagonal mesh edge_index [2, 1504] on the CPU)."""
    pos, types = gold["plate_pos"], gold["plate_type"]
    pos = torch.cat([pos, pos[:, -1:]], dim=1)
    T = pos.shape[1]
    traj = torch.cat([torch.cat([pos[g], types[None, :, None].expand(T, -1, 1)], dim=2) for g in range(2)], dim=1)
    mesh = torch.cat([gold["plate_mesh"], gold["plate_mesh"] + N1], dim=1)
    return traj.contiguous().to(dev), [0, N1, 2 * N1], mesh


def ref_edge_index(gold, frames):
    """The reference's edge_index of the batch whose graph g shows frame frames[g]: add_world_edges per graph, then
    batched."""
    return torch.cat([gold[f"plate_ei_{g}_{f}"] + g * N1 for g, f in enumerate(frames)], dim=1)


def ref_counts(gold, frames):
    return sum(int(gold[f"plate_ei_{g}_{f}"].shape[1]) for g, f in enumerate(frames))


def stable_arrays(ei, N):
    """mgn_topology_build restated with plain stable sorts: target-sorted order = stable sort of the edge ids by col;
    row_perm = stable sort of the target-sorted positions by their source."""
    ei = ei.cpu()
    eid = torch.sort(ei[1], stable=True).indices
    src, dst = ei[0][eid], ei[1][eid]
    perm = torch.sort(src, stable=True).indices
    ar = torch.arange(N + 1)
    i32 = torch.int32
    return {"csc_src": src.to(i32), "csc_dst": dst.to(i32), "csc_eid": eid.to(i32), "row_perm": perm.to(i32),
            "col_ptr": torch.searchsorted(dst.contiguous(), ar).to(i32),
            "row_ptr": torch.searchsorted(src[perm].contiguous(), ar).to(i32)}


ARRAYS = ("csc_src", "csc_dst", "csc_eid", "row_perm", "col_ptr", "row_ptr")


def world_pos():
    return {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": K + 3}


def dyn_feed(traj, gp, mesh, W=10, radius=0.03, **kw):
    from graphphysics.dataset.resident import ResidentTrajectories

    return ResidentTrajectories(traj, gp, (0, 3), K, world_pos=world_pos(),
                                dynamic_edges={"edge_index": mesh, "radius": radius, "max_neighbors": W}, **kw)


def host_edges(x, gp, mesh, radius=0.03):
    """add_world_edges per graph on the batch rows x (CPU; world position in [0, 3), node type in column K + 3),
    then batched: the oracle's cKDTree restatement of the reference."""
    from oracle import graph_oracle as GO

    out = []
    for a, b in zip(gp, gp[1:]):
        m = mesh[:, (mesh[0] >= a) & (mesh[0] < b)] - a
        out.append(GO.world_edges(x[a:b, 0:3].contiguous(), x[a:b, K + 3], m, radius) + a)
    return torch.cat(out, dim=1)


def random_case(sizes, seed, W=None, all_obstacle=None, no_obstacle=None, radius=0.125):
    """Seeded random graphs on the CPU: positions uniform in a box that gives a handful of contacts per node, types
    mixed NORMAL / OBSTACLE / HANDLE, a random symmetric mesh inside each graph. Returns (pos [N, 3], types [N],
    node offsets, mesh [2, E_m], radius)."""
    g = torch.Generator().manual_seed(seed)
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    N = gp[-1]
    pos = torch.rand(N, 3, generator=g) * 0.5
    types = torch.tensor([0.0, 0.0, 1.0, 1.0, 3.0])[torch.randint(0, 5, (N,), generator=g)]
    for b, (a, e) in enumerate(zip(gp, gp[1:])):
        if b == all_obstacle:
            types[a:e] = 1.0
        if b == no_obstacle:
            types[a:e] = torch.where(types[a:e] == 1.0, torch.zeros(()), types[a:e])
    und = [torch.randint(a, e, (2, 2 * (e - a)), generator=g) for a, e in zip(gp, gp[1:]) if e - a > 1]
    if und:
        und = torch.cat(und, dim=1)
        und = und[:, und[0] != und[1]]
        key = torch.unique(torch.cat([und[0] * N + und[1], und[1] * N + und[0]]))
        mesh = torch.stack([torch.div(key, N, rounding_mode="floor"), key % N])
    else:
        mesh = torch.zeros(2, 0, dtype=torch.int64)
    return pos, types, gp, mesh, radius


def plate_transformer(dev, hidden=16, heads=4, dtype=torch.float32, seed=0):
    """plate.json's model shape at test size: a Simulator without edge features (node_in 6 + 9 one-hot, outputs the
    world position) on EncodeTransformDecode(2, ...)."""
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator

    torch.manual_seed(seed)
    return Simulator(15, 0, 3, 0, 6, 0, 3, K + 3,
                     EncodeTransformDecode(2, 15, 3, hidden_size=hidden, num_heads=heads, compute_dtype=dtype), dev)


def rollout_host_loop(sim, traj, gp, mesh, starts, steps, mode, dev=torch.device("cpu")):
    """The per-frame loop the resident rollout replaces (tests/_plate.py's, with add_world_edges in it): per step the
    clean batch of frames start + s by fill_world_torch on the CPU; the reference's add_world_edges per graph on the
    clean x ("frame") or on the x with the previous prediction in its columns ("prediction"); a NEW edge_index tensor
    (so a fresh topology) on `dev`; Rollout.step. traj, mesh: CPU tensors. Returns (predictions, Rollout, edge counts,
    the clean x of every step)."""
    from graphphysics.dataset.resident import fill_world_torch
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    ro = Rollout(sim, K + 3, graph=False)
    preds, counts, xs = [], [], []
    for s in range(steps):
        fr = torch.tensor([f + s for f in starts], dtype=torch.int32)
        x, y, _ = fill_world_torch(traj, gp, fr, (0, 3), K, [], None, None)
        seen = x.clone()
        if ro.last_prediction is not None:
            seen[:, 0:3] = ro.last_prediction.cpu()
        ei = host_edges(x if mode == "frame" else seen, gp, mesh)
        counts.append(int(ei.shape[1]))
        pred, _ = ro.step(Data(x=x.to(dev), y=y.to(dev), edge_index=ei.to(dev), edge_attr=None))
        preds.append(pred)
        xs.append(x)
    return torch.stack(preds), ro, counts, xs
