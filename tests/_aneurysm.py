"""Shared by test_rollout_aneurysm_cpu.py / test_rollout_aneurysm_gpu.py: the reference fixture of the aneurysm
rollout (tests/golden/aneurysm_rollout_golden.npz), a CPU simulator built on the oracle for the torch path,
hand-made dyadic trajectories in the aneurysm layout, and the per-frame host loop that
Rollout.rollout_resident(acceleration=...) replaces."""
import math
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -777.0
U24 = 2.0 ** -24
RUNS = {"prev": "prediction", "frame": "frame"}  # the fixture's run -> Rollout(acceleration=...)


def load_golden():
    z = np.load(os.path.join(G, "aneurysm_rollout_golden.npz"))
    g = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k] for k in z.files if not k.startswith("w::")}
    g["weights"] = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    g["steps"] = g["traj"].shape[0] - 2  # from start frame 1
    return g


class OracleSim:
    """The fixture's Simulator (MP 2, h 16, features = batch columns [0, 13), outputs [0, 3), node type in batch
    column 13, edge_attr [E, 4]) on the CPU oracle, with what Rollout reads of a Simulator: the evaluation forward
    on an attribute bag, the output columns, the device, the mode."""

    output_index_start, output_index_end, device, training = 0, 3, torch.device("cpu"), False

    def __init__(self, weights):
        from oracle import mgn_oracle as O

        model = O.OracleEPD(2, 22, 4, 3, 16)
        model.load_state_dict({k[len("model."):]: v for k, v in weights.items() if k.startswith("model.")})
        self.sim = O.OracleSimulator(model, 22, 4, 3, feature_slice=(0, 13), output_slice=(0, 3), node_type_index=13)
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


def case(sizes, F, T, seed=0):
    """CPU (traj [T, N, F], pos [N, 3], node offsets): frames of multiples of 2^-8 in [-1, 1] with the wall flag
    (0 or 1, constant over the frames) in column 3. Of every graph of n nodes the first ceil(n / 4) lie on the inflow
    face (pos y == 0, x < 0), the next n // 5 on the outflow face, the others off it; a graph of one node is all
    inflow (its value set has no masked zero). The inflow velocities are multiples of 2^-3, so their accelerations
    repeat across nodes, components and frames."""
    g = torch.Generator().manual_seed(seed + 31 * F + T + 7 * len(sizes) + sum(sizes))
    N, gp = sum(sizes), offsets(sizes)
    traj = torch.randint(-256, 257, (T, N, F), generator=g).float() / 256.0
    traj[:, :, 3] = (torch.rand(N, generator=g) < 0.25).float()
    pos = torch.randint(-256, 257, (N, 3), generator=g).float() / 256.0
    pos[:, 1] = pos[:, 1].abs() + 0.25
    for b, n in enumerate(sizes):
        m, o = -(-n // 4), n // 5
        r = gp[b]
        pos[r:r + m, 1], pos[r:r + m, 0] = 0.0, -pos[r:r + m, 0].abs() - 0.125
        pos[r + m:r + m + o, 1], pos[r + m:r + m + o, 0] = 0.0, pos[r + m:r + m + o, 0].abs()
        traj[:, r:r + m, 0:3] = torch.randint(-8, 9, (T, m, 3), generator=g).float() / 8.0
    return traj.contiguous(), pos.contiguous(), gp


def edges(N, gp, seed=0):
    """[2, E] int64 on the CPU: random pairs inside each graph, a self-loop, and the first edge repeated."""
    g = torch.Generator().manual_seed(seed + N)
    ei = torch.cat([torch.randint(a, b, (2, 3 * (b - a)), generator=g) for a, b in zip(gp, gp[1:]) if b > a], dim=1)
    return torch.cat([ei, torch.tensor([[N - 1], [N - 1]]), ei[:, :1]], dim=1)


def mean_bound(traj, node_type, t, m_ref):
    """|mean − m_ref| allowed against the reference's fp32 torch.mean at frame t of a one-graph trajectory:
    2^-24·|m_ref| + 2^-24·Σ|v| over the distinct next-frame inflow accelerations v (test_feed_aneurysm_cpu.py)."""
    inflow = node_type == 4
    d = (traj[t + 1, :, 0:3] - traj[t, :, 0:3])[inflow].reshape(-1).tolist()
    if not bool(inflow.all()):
        d.append(0.0)
    return U24 * abs(m_ref) + U24 * math.fsum(abs(v) for v in set(float(v) + 0.0 for v in d))


def check_fixture(gold, run, seen, losses, rmse):
    """seen(s) -> (x the model saw at step s, predictions [s + 1, N, 3]) of a run from frame 1; losses and rmse of
    a whole run. The bounds of this file's docstring."""
    traj = gold["traj"]
    F, S = traj.shape[2], gold["steps"]
    node_type = gold[f"{run}::x0"][:, F + 9]
    masked = ~((node_type == 0) | (node_type == 5))
    assert 0 < int(masked.sum()) < traj.shape[1]
    fed = list(range(0, 3)) + (list(range(F, F + 3)) if run == "prev" else [])
    for s in range(S):
        x, pred = seen(s)
        want = gold[f"{run}::x{s}"]
        assert tuple(x.shape) == tuple(want.shape)
        cols = [c for c in range(F + 10) if c != F + 6 and not (s > 0 and c in fed)]
        assert torch.equal(x[:, cols], want[:, cols]), (run, s)
        if s > 0:  # masked nodes carry the target: exact differences of dyadic values
            assert torch.equal(x[masked][:, fed], want[masked][:, fed]), (run, s)
            assert not torch.equal(x[:, 0:3], traj[1 + s, :, 0:3])
            clean_acc = torch.equal(x[:, F:F + 3], traj[1 + s, :, 0:3] - traj[s, :, 0:3])
            assert clean_acc == (run == "frame")
        m, m_ref = x[:, F + 6], float(want[0, F + 6])
        assert bool((m == m[0]).all())
        assert abs(float(m[0]) - m_ref) <= mean_bound(traj, node_type, 1 + s, m_ref), (run, s)
        ref = gold[f"{run}::pred{s}"]
        assert bool(((pred[s] - ref).abs() <= 1e-4 * (1 + ref.abs())).all()), (s, float((pred[s] - ref).abs().max()))
        assert torch.equal(pred[s][masked], traj[2 + s, :, 0:3][masked])
    assert len(losses) == S
    for a, b in zip(losses, gold[f"{run}::val_loss"].tolist()):
        assert abs(a - b) <= 1e-6 + 1e-4 * b, (a, b)
    ref_rmse = float(gold[f"{run}::val_all_rollout_rmse"][0])
    assert abs(rmse - ref_rmse) <= 1e-6 + 1e-4 * ref_rmse


def host_loop(sim, traj, pos, gp, ei, edge_attr, starts, steps, mode):
    """The per-frame loop the resident rollout replaces, on the tensors' own device: for every step and graph a
    Data of the clean frame start + s (y the next frame's velocity, previous_data the frame before) through
    external.aneurysm.build_features, the graphs concatenated, then Rollout.step, which feeds the prediction back:
    with use_previous_data on columns (F, F + 3) for "prediction", without it for "frame". Returns (predictions
    [steps, N, 3], the Rollout, the x of every step as the model saw it)."""
    from graphphysics.external.aneurysm import build_features
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils.data import Data

    F = traj.shape[2]
    kw = dict(use_previous_data=True, previous_data_start=F, previous_data_end=F + 3) if mode == "prediction" else {}
    ro = Rollout(sim, F + 9, graph=False, **kw)
    preds, xs = [], []
    for s in range(steps):
        items = []
        for b, f in enumerate(starts):
            rows, t = slice(gp[b], gp[b + 1]), f + s
            items.append(build_features(Data(x=traj[t, rows].clone(), y=traj[t + 1, rows, 0:3].clone(), pos=pos[rows],
                                             previous_data=traj[t - 1, rows, 0:3].clone())))
        x, y = torch.cat([d.x for d in items]), torch.cat([d.y for d in items])
        seen = x.clone()
        if ro.last_prediction is not None:
            seen[:, 0:3] = ro.last_prediction
            if mode == "prediction":
                seen[:, F:F + 3] = ro.last_previous
        pred, _ = ro.step(Data(x=x, y=y, edge_index=ei, edge_attr=edge_attr))
        preds.append(pred)
        xs.append(seen)
    return torch.stack(preds), ro, xs
