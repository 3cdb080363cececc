"""Shared by test_rollout_world_cpu.py / test_rollout_world_gpu.py: the reference fixture of the Lagrangian
rollout (tests/golden/world_rollout_golden.npz), a CPU simulator built on the oracle for the torch path, hand-made
dyadic trajectories, the small plate of test_feed_world_gpu.py restated, and the per-frame host loop that
Rollout.rollout_resident(world_edges=...) replaces."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
NORM_RTOL = 5 * 2.0 ** -24  # the reference's torch.norm against the term-by-term form (test_feed_world_cpu.py)
EA_START = 4  # first world column of edge_attr: the mesh's Cartesian ‖ Distance columns come first


def load_golden():
    z = np.load(os.path.join(G, "world_rollout_golden.npz"))
    g = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k] for k in z.files if not k.startswith("w::")}
    g["weights"] = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    g["k"] = int(z["node_type_index"])
    g["steps"] = g["traj"].shape[0] - 1
    return g


class OracleSim:
    """The fixture's Simulator (MP 2, h 16, features = batch columns [0, 8), outputs [0, 3), node type in batch
    column 6) on the CPU oracle, with what Rollout reads of a Simulator: the evaluation forward on an attribute
    bag, the output columns, the device, the mode."""

    output_index_start, output_index_end, device, training = 0, 3, torch.device("cpu"), False

    def __init__(self, weights):
        from oracle import mgn_oracle as O

        model = O.OracleEPD(2, 17, 8, 3, 16)
        model.load_state_dict({k[len("model."):]: v for k, v in weights.items() if k.startswith("model.")})
        self.sim = O.OracleSimulator(model, 17, 8, 3, feature_slice=(0, 8), output_slice=(0, 3), node_type_index=6)
        for name, norm in (("_output_normalizer", self.sim.out_norm), ("_node_normalizer", self.sim.node_norm),
                           ("_edge_normalizer", self.sim.edge_norm)):
            norm.acc_sum, norm.acc_sum_squared = weights[name + "._acc_sum"], weights[name + "._acc_sum_squared"]
            norm.acc_count, norm.num_acc = weights[name + "._acc_count"], weights[name + "._num_accumulations"]

    def __call__(self, fr):
        with torch.no_grad():
            return self.sim.forward(fr.x, fr.y, fr.edge_index, fr.edge_attr, training=False)


def offsets(sizes):
    gp = [0]
    for s in sizes:
        gp.append(gp[-1] + s)
    return gp


def case(sizes, F, T, k=None, all_obstacle=None, dyadic=True, seed=0):
    """CPU [T, N, F] frames (column k, default the last, the node type: NORMAL 0, OBSTACLE 1, HANDLE 3 mixed, the
    first node of every graph an OBSTACLE; graph `all_obstacle` entirely), node offsets. dyadic: multiples of 2^-8
    in [-1, 1], so every displacement and every sum of fewer than 2^13 of them is exact in fp32."""
    k = F - 1 if k is None else k
    g = torch.Generator().manual_seed(seed + 31 * F + T + 7 * len(sizes) + sum(sizes))
    N, gp = sum(sizes), offsets(sizes)
    if dyadic:
        traj = torch.randint(-256, 257, (T, N, F), generator=g).float() / 256.0
    else:
        traj = torch.randn(T, N, F, generator=g)
    types = torch.tensor([0.0, 0.0, 1.0, 3.0])[torch.randint(0, 4, (N,), generator=g)]
    for b, s in enumerate(sizes):
        if s:
            types[gp[b]] = 1.0
        if b == all_obstacle:
            types[gp[b]:gp[b + 1]] = 1.0
    traj[:, :, k] = types
    return traj.contiguous(), gp


def edges(N, gp=None, seed=0):
    """[2, E] int64 on the CPU: random pairs (inside each graph when node offsets are given), a self-loop, and the
    first edge repeated."""
    g = torch.Generator().manual_seed(seed + N)
    if gp is None:
        ei = torch.randint(0, N, (2, 3 * N + 5), generator=g)
    else:
        ei = torch.cat([torch.randint(a, b, (2, 3 * (b - a)), generator=g) for a, b in zip(gp, gp[1:]) if b > a], dim=1)
    loop = torch.tensor([[N - 1], [N - 1]])
    return torch.cat([ei, loop, ei[:, :1]], dim=1)


def world_pos(k, ei=None):
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": k + 3}
    if ei is not None:
        wp.update(edge_index=ei, edge_attr_start=EA_START)
    return wp


def small_plate(dev, T=4):
    """plate_sample(nx=6, ny=4, nz=2) twice, T frames interpolated between its x and y (the second graph moves 1.5
    times as far), rounded to multiples of 2^-12 (every obstacle sum is exact), the static edges and mesh edge
    features of plate_graph. Returns (traj [T, N, 4] on dev, node offsets, edge_index [2, E], edge_attr [E, 8])."""
    from graphphysics.utils import meshes

    kw = dict(nx=6, ny=4, nz=2)
    s = meshes.plate_sample(seed=0, **kw)
    g, _ = meshes.plate_graph(dev, seed=0, **kw)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
    graphs = []
    for amp in (1.0, 1.5):
        frames = []
        for f in range(T):
            w = x0[:, 0:3] + (amp * f / (T - 1)) * (y0 - x0[:, 0:3])
            frames.append(torch.cat([torch.round(w * 4096.0) / 4096.0, x0[:, 3:4]], dim=1))
        graphs.append(torch.stack(frames))
    traj = torch.cat(graphs, dim=1).contiguous().to(dev)
    ei = torch.cat([g.edge_index, g.edge_index + n], dim=1).contiguous()
    ea = torch.cat([g.edge_attr, g.edge_attr], dim=0).contiguous()
    assert traj.shape == (T, 2 * n, 4) and ea.shape[1] == 8
    return traj, [0, n, 2 * n], ei, ea


def host_loop(sim, traj, gp, ei, edge_attr, starts, steps, mode, k, dev=torch.device("cpu")):
    """The per-frame loop the resident rollout replaces: for every step the batch of the clean frames start + s by
    the torch rules on the CPU (fill_world_torch without noise; the world columns of a copy of edge_attr by
    world_edge_features_torch, from the clean x for "frame", from the x with the previous prediction in its columns
    for "prediction", not at all for "off"), moved to `dev`, then Rollout.step, which feeds the prediction back.
    traj, ei, edge_attr: CPU tensors. Returns (predictions [steps, N, 3], the Rollout, the x and edge_attr of every
    step as the model saw them)."""
    from graphphysics.dataset.resident import fill_world_torch, world_edge_features_torch
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    ro = Rollout(sim, k + 3, graph=False)
    ei_dev = ei.to(dev)
    preds, xs, eas = [], [], []
    for s in range(steps):
        fr = torch.tensor([f + s for f in starts], dtype=torch.int32)
        x, y, _ = fill_world_torch(traj, gp, fr, (0, 3), k, [], None, None)
        seen = x.clone()
        if ro.last_prediction is not None:
            seen[:, 0:3] = ro.last_prediction.cpu()
        ea = edge_attr.clone()
        if mode != "off":
            world_edge_features_torch(x if mode == "frame" else seen, ei, ea, EA_START)
        pred, _ = ro.step(Data(x=x.to(dev), y=y.to(dev), edge_index=ei_dev, edge_attr=ea.to(dev)))
        preds.append(pred)
        xs.append(seen)
        eas.append(ea)
    return torch.stack(preds), ro, xs, eas
