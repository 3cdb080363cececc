"""Golden vectors of the reference's validation rollout on Lagrangian data (DeformingPlate's plate.json layout):
runs the REFERENCE's own dataset stages add_obstacles_next_pos -> add_world_pos_features
(graphphysics/dataset/preprocessing.py:49-89, 143-174, in build_preprocessing's order :401-427, no noise: a
validation item) on every clean frame of a short trajectory, then its validation_step / _make_prediction
(graphphysics/training/lightning_module.py:168-249) over those items, in fp32 on the CPU over the stand-ins in
tests/golden/_stubs, and writes tests/golden/world_rollout_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_world_rollout_golden.py

One graph: N = 40 nodes, frame rows of F = 5 columns [world position (3), node type (k = 3), one extra column], a
mix of NORMAL 0, OBSTACLE 1 and HANDLE 3 nodes with 5 obstacle nodes whose displacements all differ in every
frame, T = 5 frames (4 steps), E = 120 static directed edges (the last but one repeats the first, the last is a
self-loop), edge_attr_in [E, 4] (the mesh's Cartesian ‖ Distance columns). The model is a small reference
Simulator + EncodeProcessDecode (MP 2, h 16, node_in 8 + 9, edge_in 8, out 3; features = batch columns [0, 8),
output columns [0, 3), node type in batch column 6 as plate.json), its normalisers accumulated over the four
items in training mode first.

The order the fixture pins: the dataset item of step s is built from the CLEAN frame s (displacement, obstacle
mean and the relative world positions of the edges), and only then does _make_prediction write the previous
prediction into x[:, 0:3] — neither the displacement nor the edge features are recomputed from it. Before anything
is stored the generator asserts that the rule written term by term reproduces the x the reference's model saw and
the three relative-position columns bit for bit; the norm column (torch.norm, another 3-term reduction than
(v0·v0 + v1·v1) + v2·v2) is held to 5·2^-24 relative and stored as the reference wrote it. Stored (data only):
  traj [5, 40, 5] f32, node_type_index (of a frame row: 3), edge_index [2, 120] i64, edge_attr_in [120, 4] f32,
  w::<key> the Simulator's state_dict (weights and normaliser buffers), and per step s = 0..3: x{s} [40, 8] f32
  (what the model saw), edge_attr{s} [120, 8] f32, pred{s} [40, 3] f32 (predicted_outputs after the mask);
  val_loss [4] f64, val_all_rollout_rmse [1] f64, seed.
"""
import os
import sys
import types

import numpy as np
import torch

from graphphysics.dataset.preprocessing import add_obstacles_next_pos, add_world_pos_features  # noqa: E402  (reference)
from graphphysics.models.processors import EncodeProcessDecode  # noqa: E402  (reference)
from graphphysics.models.simulator import Simulator  # noqa: E402  (reference)
from graphphysics.utils.loss import L2Loss  # noqa: E402  (reference)
from graphphysics.utils.nodetype import NodeType  # noqa: E402  (reference)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F, K, E, T = 20250712, 40, 5, 3, 120, 5
NORMAL, OBSTACLE, HANDLE = 0.0, 1.0, 3.0


def reference_lightning_module():
    """The reference LightningModule importable without lightning and the dataset / meshio stack, as
    make_golden.py's _reference_lightning_module: `lightning.LightningModule` -> nn.Module with no-op
    save_hyperparameters and a log that records, the two helper modules it imports replaced by empty ones."""

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


def item(traj, t, ei, ea_in):
    """The reference's dataset item of clean frame t: x = frame t, y = the world position of frame t + 1, through
    add_obstacles_next_pos and add_world_pos_features."""
    g = _Batch(x=traj[t].clone(), y=traj[t + 1][:, 0:3].clone(), pos=traj[0][:, 0:3].clone(), edge_index=ei.clone(),
               edge_attr=ea_in.clone(), traj_index=0)
    g = add_obstacles_next_pos(g, 0, 3, K + 3)
    return add_world_pos_features(g, 0, 3)


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    frame0 = rng.standard_normal((N, F)).astype(np.float32)
    types_ = rng.permutation(np.asarray([OBSTACLE] * 5 + [HANDLE] * 6 + [NORMAL] * (N - 11), dtype=np.float32))
    frames = [frame0]
    for t in range(1, T):
        nxt = frames[-1].copy()
        nxt[:, 0:3] += (0.01 * rng.standard_normal((N, 3))).astype(np.float32)
        nxt[:, 4] += 1.0
        frames.append(nxt)
    traj = torch.from_numpy(np.stack(frames))
    traj[:, :, K] = torch.from_numpy(types_)
    obstacle = traj[0, :, K] == OBSTACLE
    assert int(obstacle.sum()) == 5 and int((traj[0, :, K] == HANDLE).sum()) == 6
    ei = torch.from_numpy(rng.integers(0, N, (2, E - 2)))
    ei = torch.cat([ei, ei[:, :1], torch.tensor([[N - 1], [N - 1]])], dim=1)  # a duplicate and a self-loop
    ea_in = torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32))

    torch.manual_seed(0)
    model = EncodeProcessDecode(message_passing_num=2, node_input_size=8 + NodeType.SIZE, edge_input_size=8,
                                output_size=3, hidden_size=16)
    sim = Simulator(node_input_size=8 + NodeType.SIZE, edge_input_size=8, output_size=3, feature_index_start=0,
                    feature_index_end=8, output_index_start=0, output_index_end=3, node_type_index=K + 3,
                    model=model, device="cpu")
    sim.train()
    with torch.no_grad():
        for t in range(T - 1):  # the normalisers' statistics
            sim(item(traj, t, ei, ea_in))
    sim.eval()

    LM = reference_lightning_module()
    lm = LM.__new__(LM)
    torch.nn.Module.__init__(lm)
    lm.logged = {}
    lm.current_epoch, lm.timestep = 0, 1.0
    lm.param = {"index": {"node_type_index": K + 3}}
    lm.model, lm.K, lm.loss = sim, 0, L2Loss()
    lm.loss_masks = [NodeType.NORMAL, NodeType.OUTFLOW]
    lm.use_previous_data, lm.previous_data_start, lm.previous_data_end = False, None, None
    lm.val_step_outputs, lm.val_step_targets, lm.trajectory_to_save = [], [], []
    lm.current_val_trajectory, lm.last_val_prediction, lm.last_previous_data_prediction = 0, None, None
    lm._save_trajectory_to_xdmf = lambda *a, **k: None
    lm._get_traj_savename = lambda *a, **k: ""

    out = {"traj": traj.numpy().copy(), "node_type_index": np.asarray(K, dtype=np.int32),
           "edge_index": ei.numpy().astype(np.int64), "edge_attr_in": ea_in.numpy().copy(),
           "seed": np.asarray(SEED, dtype=np.int64)}
    for k, v in sim.state_dict().items():
        out["w::" + k] = v.detach().cpu().numpy().copy()
    worst, last = 0.0, None
    for s in range(T - 1):
        lm.validation_step(item(traj, s, ei, ea_in), s)
        seen = lm.trajectory_to_save[-1]  # the clone _make_prediction ran the model on
        pred = lm.val_step_outputs[-1]
        x_seen, ea_seen = seen.x, seen.edge_attr
        assert tuple(x_seen.shape) == (N, F + 3) and tuple(ea_seen.shape) == (E, 8)

        # the rule, term by term: everything from the clean frame s, then the feedback
        a, n = traj[s], traj[s + 1]
        disp = n[:, 0:3] - a[:, 0:3]
        d = disp[obstacle]
        assert len({tuple(r) for r in d.tolist()}) == 5
        mean = d.sum(0) / torch.full((), d.shape[0], dtype=torch.float32)
        want = torch.cat([a[:, 0:3], torch.where(obstacle[:, None], disp, mean), a[:, 3:]], dim=1)
        if last is not None:
            want[:, 0:3] = last
        assert torch.equal(want, x_seen), f"step {s}: the term-by-term rule does not reproduce the reference's x"
        if last is not None:
            assert not torch.equal(x_seen[:, 0:3], a[:, 0:3])  # the feedback is visible
        v = a[ei[0], 0:3] - a[ei[1], 0:3]  # the clean frame, not the fed-back positions
        assert torch.equal(v, ea_seen[:, 4:7]), f"step {s}: the relative world positions differ from the reference's"
        assert torch.equal(ea_seen[:, :4], ea_in)
        norm = torch.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).double()).float()
        nz = ea_seen[:, 7] > 0
        worst = max(worst, float(((norm - ea_seen[:, 7]).abs()[nz] / ea_seen[:, 7][nz]).max()))
        assert torch.equal(norm[~nz], ea_seen[:, 7][~nz])  # the self-loop: 0
        keep = ~((a[:, K] == NORMAL) | (a[:, K] == 5.0))
        assert torch.equal(pred[keep], n[:, 0:3][keep]) and not torch.equal(pred[~keep], n[:, 0:3][~keep])
        out[f"x{s}"], out[f"edge_attr{s}"] = x_seen.numpy().copy(), ea_seen.numpy().copy()
        out[f"pred{s}"] = pred.numpy().copy()
        last = pred.clone()
    print("norm column: max relative difference to the term-by-term form", worst, "(2^-24 =", 2.0 ** -24, ")")
    assert worst <= 5 * 2.0 ** -24
    out["val_loss"] = np.array(lm.logged["val_loss"])
    lm.on_validation_epoch_end()
    out["val_all_rollout_rmse"] = np.array(lm.logged["val_all_rollout_rmse"])
    assert len(out["val_loss"]) == T - 1
    path = os.path.join(HERE, "world_rollout_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays; val_loss", out["val_loss"].tolist(), "rmse",
          out["val_all_rollout_rmse"].tolist())


if __name__ == "__main__":
    main()
