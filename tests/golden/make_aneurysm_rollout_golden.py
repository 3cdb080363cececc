"""Golden vectors of the reference's validation rollout on aneurysm data: runs the REFERENCE's own build_features
(graphphysics/external/aneurysm.py:27-64, no noise: a validation item) on every clean frame of a short trajectory
that has a predecessor and a successor, then its validation_step / _make_prediction
(graphphysics/training/lightning_module.py:168-249) over those items, in fp32 on the CPU over the stand-ins in
tests/golden/_stubs, and writes tests/golden/aneurysm_rollout_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_aneurysm_rollout_golden.py

One graph: N = 48 nodes in the node layout of make_aneurysm_feed_golden.py (12 inflow nodes, of which node 3 carries
the wall flag; node 12 at pos (0, 0, z), which is OUTFLOW, and 5 more outflow nodes; 6 wall nodes off the face; 24
NORMAL), frame rows of F = 4 columns [velocity (3), wall flag], T = 6 frames, so 4 steps from start frame 1.
Velocities are multiples of 2^-10 and the accelerations of the inflow nodes are drawn from a few multiples of 2^-10,
so they repeat across nodes, components and frames and every difference is exact. E = 150 static directed edges (the
last but one repeats the first, the last is a self-loop) with random edge_attr [E, 4]. The model is a small
reference Simulator + EncodeProcessDecode (MP 2, h 16, node_in 13 + 9, edge_in 4, out 3; features = batch columns
[0, 13), output columns [0, 3), node type in batch column 13), its normalisers accumulated over the four items in
training mode first.

Two runs of validation_step over the same items: "prev", use_previous_data = True with columns 4, 7 (train.py's
defaults: the acceleration columns of an F = 4 frame), and "frame", use_previous_data = False.

The order the fixture pins: the dataset item of step s is built from the CLEAN frames t − 1, t, t + 1 (t = 1 + s),
and only then does _make_prediction write the previous prediction into x[:, 0:3] and, with use_previous_data,
predicted − current_output into x[:, 4:7]; nothing else is recomputed. Before anything is stored the generator
asserts that this rule written term by term reproduces the x the reference's model saw: every column bit for bit
except the mean column F + 6, which lies within 2^-24·|m| + 2^-24·Σ|v| of the fp64 ascending mean of the distinct
values (the bound derived in make_aneurysm_feed_golden.py). Stored (data only):
  traj [6, 48, 4] f32, pos [48, 3] f32, edge_index [2, 150] i64, edge_attr [150, 4] f32, w::<key> the Simulator's
  state_dict (weights and normaliser buffers), and per run r in {prev, frame} and step s = 0..3: r::x{s} [48, 14] f32
  (what the model saw), r::pred{s} [48, 3] f32 (predicted_outputs after the mask); r::val_loss [4] f64,
  r::val_all_rollout_rmse [1] f64; seed.
"""
import math
import os
import sys
import types

import numpy as np
import torch

from graphphysics.external.aneurysm import build_features  # noqa: E402  (reference)
from graphphysics.models.processors import EncodeProcessDecode  # noqa: E402  (reference)
from graphphysics.models.simulator import Simulator  # noqa: E402  (reference)
from graphphysics.utils.loss import L2Loss  # noqa: E402  (reference)
from graphphysics.utils.nodetype import NodeType  # noqa: E402  (reference)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F, E, T = 20250713, 48, 4, 150, 6
NORMAL, INFLOW, OUTFLOW, WALL = 0.0, 4.0, 5.0, 6.0
TYPE_COLUMN = F + 9
Q = 1.0 / 1024.0


def reference_lightning_module():
    """The reference LightningModule importable without lightning and the dataset / meshio stack, as
    make_world_rollout_golden.py's: `lightning.LightningModule` -> nn.Module with no-op save_hyperparameters and a
    log that records, the two helper modules it imports replaced by empty ones."""

    class _LM(torch.nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, name, value, **k):
            self.logged.setdefault(name, []).append(float(value))

    light = types.ModuleType("lightning")
    light.LightningModule = _LM
    sys.modules.setdefault("lightning", light)
    for name in ("graphphysics.training.parse_parameters", "graphphysics.utils.meshio_mesh"):
        mod = types.ModuleType(name)
        mod.get_model = mod.get_simulator = mod.convert_to_meshio_vtu = None
        sys.modules.setdefault(name, mod)
    from graphphysics.training.lightning_module import LightningModule

    return LightningModule


class _Batch(Data):
    def clone(self):
        return _Batch(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})


def item(traj, pos, t, ei, ea):
    """The reference's dataset item of clean frame t: x = frame t, y = the velocity of frame t + 1, previous_data
    the velocity of frame t − 1, through build_features."""
    g = _Batch(x=traj[t].clone(), y=traj[t + 1][:, 0:3].clone(), pos=pos.clone(), edge_index=ei.clone(),
               edge_attr=ea.clone(), traj_index=0, previous_data={"Vitesse": traj[t - 1][:, 0:3].numpy().copy()})
    return build_features(g)


def lightning(LM, sim, use_prev):
    lm = LM.__new__(LM)
    torch.nn.Module.__init__(lm)
    lm.logged = {}
    lm.current_epoch, lm.timestep = 0, 1.0
    lm.param = {"index": {"node_type_index": TYPE_COLUMN}}
    lm.model, lm.K, lm.loss = sim, 0, L2Loss()
    lm.loss_masks = [NodeType.NORMAL, NodeType.OUTFLOW]
    lm.use_previous_data = use_prev
    lm.previous_data_start, lm.previous_data_end = (F, F + 3) if use_prev else (None, None)
    lm.val_step_outputs, lm.val_step_targets, lm.trajectory_to_save = [], [], []
    lm.current_val_trajectory, lm.last_val_prediction, lm.last_previous_data_prediction = 0, None, None
    lm._save_trajectory_to_xdmf = lambda *a, **k: None
    lm._get_traj_savename = lambda *a, **k: ""
    return lm


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    # positions: nodes 0..11 on the inflow face, 12 at (0, 0, z), 13..17 on the outflow face, the others off it
    pos = rng.standard_normal((N, 3)).astype(np.float32)
    pos[:, 1] = np.abs(pos[:, 1]) + 0.25
    pos[0:18, 1] = 0.0
    pos[0:12, 0] = -np.abs(pos[0:12, 0]) - 0.125
    pos[12, 0] = 0.0
    pos[13:18, 0] = np.abs(pos[13:18, 0]) + 0.125
    wall = np.zeros(N, dtype=np.float32)
    wall[[3, 18, 19, 20, 21, 22, 23]] = 1.0  # node 3: a wall node on the inflow face
    # velocities: multiples of 2^-10; the inflow accelerations come from a short list, so they repeat
    # (five of the list per frame, so the statistics differ from frame to frame)
    steps_q = np.asarray([-64, -23, -5, 0, 3, 7, 12, 40, 57], dtype=np.float64) * Q
    frames = [np.round(rng.standard_normal((N, 3)) * 256.0) / 1024.0]
    for t in range(1, T):
        nxt = frames[-1] + np.round(rng.standard_normal((N, 3)) * 32.0) / 1024.0
        some = steps_q[rng.choice(len(steps_q), size=5, replace=False)]
        nxt[0:12] = frames[-1][0:12] + some[rng.integers(0, len(some), (12, 3))]
        frames.append(nxt)
    traj = torch.from_numpy(np.stack([np.concatenate([v, wall[:, None]], axis=1) for v in frames]).astype(np.float32))
    assert torch.equal(traj[:, :, 0:3] * 1024.0, torch.round(traj[:, :, 0:3] * 1024.0))  # dyadic after the cast
    pos_t = torch.from_numpy(pos)
    ei = torch.from_numpy(rng.integers(0, N, (2, E - 2)))
    ei = torch.cat([ei, ei[:, :1], torch.tensor([[N - 1], [N - 1]])], dim=1)  # a duplicate and a self-loop
    ea = torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32))

    node_type = torch.zeros(N)
    node_type[traj[0, :, 3] == 1.0] = WALL
    node_type[(pos_t[:, 1] == 0.0) & (pos_t[:, 0] <= 0)] = INFLOW
    node_type[(pos_t[:, 1] == 0.0) & (pos_t[:, 0] >= 0)] = OUTFLOW
    inflow = node_type == INFLOW
    assert int(inflow.sum()) == 12 and node_type[3] == INFLOW and node_type[12] == OUTFLOW
    assert int((node_type == OUTFLOW).sum()) == 6 and int((node_type == WALL).sum()) == 6
    assert int((node_type == NORMAL).sum()) == 24

    torch.manual_seed(0)
    model = EncodeProcessDecode(message_passing_num=2, node_input_size=13 + NodeType.SIZE, edge_input_size=4,
                                output_size=3, hidden_size=16)
    sim = Simulator(node_input_size=13 + NodeType.SIZE, edge_input_size=4, output_size=3, feature_index_start=0,
                    feature_index_end=13, output_index_start=0, output_index_end=3, node_type_index=TYPE_COLUMN,
                    model=model, device="cpu")
    sim.train()
    with torch.no_grad():
        for t in range(1, T - 1):  # the normalisers' statistics
            sim(item(traj, pos_t, t, ei, ea))
    sim.eval()

    out = {"traj": traj.numpy().copy(), "pos": pos_t.numpy().copy(), "edge_index": ei.numpy().astype(np.int64),
           "edge_attr": ea.numpy().copy(), "seed": np.asarray(SEED, dtype=np.int64)}
    for k, v in sim.state_dict().items():
        out["w::" + k] = v.detach().cpu().numpy().copy()

    LM = reference_lightning_module()
    preds = {}
    for run, use_prev in (("prev", True), ("frame", False)):
        lm = lightning(LM, sim, use_prev)
        last, last_prev = None, None
        for s in range(T - 2):
            t = 1 + s
            lm.validation_step(item(traj, pos_t, t, ei, ea), s)
            seen = lm.trajectory_to_save[-1]  # the clone _make_prediction ran the model on
            pred = lm.val_step_outputs[-1]
            x_seen = seen.x
            assert tuple(x_seen.shape) == (N, F + 10) and x_seen.dtype == torch.float32
            assert torch.equal(seen.edge_attr, ea) and torch.equal(seen.edge_index, ei)

            # the rule, term by term: everything from the clean frames t - 1, t, t + 1, then the feedback
            p, a, n = traj[t - 1], traj[t], traj[t + 1]
            d = n[:, 0:3] - a[:, 0:3]
            vals = torch.cat([d[inflow].reshape(-1), torch.zeros(1)]) + 0.0
            distinct = torch.unique(vals)
            assert distinct.numel() < vals.numel() - 6  # repeats across nodes and components
            assert float(distinct.min()) < 0 < float(distinct.max())
            total = 0.0
            for v in distinct.tolist():
                total += v
            mean = float(np.float32(total / distinct.numel()))
            m_ref = float(x_seen[0, F + 6])
            bound = 2.0 ** -24 * abs(m_ref) + 2.0 ** -24 * math.fsum(abs(v) for v in distinct.tolist())
            print(f"{run} step {s}: mean reference {m_ref!r}, fp64 ascending {mean!r}, |difference| "
                  f"{abs(mean - m_ref):.3e}, bound {bound:.3e}, {distinct.numel()} distinct of {vals.numel()} values")
            assert abs(mean - m_ref) <= bound
            assert bool((x_seen[:, F + 6] == x_seen[0, F + 6]).all())
            want = torch.cat([a, a[:, 0:3] - p[:, 0:3], pos_t,
                              torch.tensor([m_ref, float(distinct[0]), float(distinct[-1])]).expand(N, 3),
                              node_type[:, None]], dim=1)
            if last is not None:
                want[:, 0:3] = last
                if use_prev:
                    want[:, F:F + 3] = last_prev
            assert torch.equal(want, x_seen), f"{run} step {s}: the term-by-term rule does not reproduce the x"
            if last is not None:
                assert not torch.equal(x_seen[:, 0:3], a[:, 0:3])  # the feedback is visible
                clean_acc = torch.equal(x_seen[:, F:F + 3], a[:, 0:3] - p[:, 0:3])
                assert clean_acc == (not use_prev)
            keep = ~((node_type == NORMAL) | (node_type == OUTFLOW))
            assert torch.equal(pred[keep], n[:, 0:3][keep]) and not torch.equal(pred[~keep], n[:, 0:3][~keep])
            out[f"{run}::x{s}"], out[f"{run}::pred{s}"] = x_seen.numpy().copy(), pred.numpy().copy()
            last_prev = pred - x_seen[:, 0:3]  # predicted_outputs - current_output
            last = pred.clone()
            preds[run, s] = pred.clone()
        out[f"{run}::val_loss"] = np.array(lm.logged["val_loss"])
        lm.on_validation_epoch_end()
        out[f"{run}::val_all_rollout_rmse"] = np.array(lm.logged["val_all_rollout_rmse"])
        assert len(out[f"{run}::val_loss"]) == T - 2
    assert len({float(out[f"prev::x{s}"][0, F + 6]) for s in range(T - 2)}) > 2  # the statistics follow the frame
    # step 0 sees the same x in both runs; from step 1 on the acceleration columns differ, and so do the predictions
    assert torch.equal(preds["prev", 0], preds["frame", 0]) and not torch.equal(preds["prev", 1], preds["frame", 1])
    path = os.path.join(HERE, "aneurysm_rollout_golden.npz")
    np.savez_compressed(path, **out)
    for run in ("prev", "frame"):
        print(run, "val_loss", out[f"{run}::val_loss"].tolist(), "rmse", out[f"{run}::val_all_rollout_rmse"].tolist())
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
