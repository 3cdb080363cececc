"""Golden vectors of the reference's world-position stages (Lagrangian data, DeformingPlate's plate.json): runs
the REFERENCE's own add_obstacles_next_pos -> add_noise -> add_world_pos_features
(graphphysics/dataset/preprocessing.py:49-89, 177-238, 143-174, in build_preprocessing's order :401-442) in fp32
on the CPU over the stand-ins in tests/golden/_stubs and writes tests/golden/world_feed_golden.npz. Run where the
reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_world_feed_golden.py

One small graph: N = 40 nodes, frame rows of F = 5 columns [world position (3), node type (k = 3), one extra
column], a mix of NORMAL 0, OBSTACLE 1 and HANDLE 3 nodes with 5 obstacle nodes whose displacements all differ,
E = 120 directed edges (the last one repeats the first), edge_attr [E, 4] pre-filled (the mesh's Cartesian ‖
Distance columns), noise on the batch-layout columns [(0, 3), (7, 8)] with scales [0.003, 0.1] and
node_type_index 6. The standard normals add_noise drew are recovered by re-seeding and repeating its randn_like
calls. Before anything is stored the generator asserts that the rule written term by term — the displacement from
clean values, the obstacle mean as sum(0) / M, the noise as a rounded product then a rounded sum, the relative
positions from the noisy x — reproduces the reference's x and its three relative-position columns bit for bit;
the norm column (torch.norm, another 3-term reduction than (v0·v0 + v1·v1) + v2·v2) is stored as the reference
wrote it. Stored (data only):
  frame [40, 5] f32, next_frame [40, 5] f32, z [40, 4] f32 (the ranges' columns side by side), ranges [2, 2] i32
  (batch layout), scales [2] f64, node_type_index (of a frame row: 3), edge_index [2, 120] i64,
  edge_attr_in [120, 4] f32, x_out [40, 8] f32, edge_attr_out [120, 8] f32, obstacle_mean [3] f32, seed.
"""
import os

import numpy as np
import torch

from graphphysics.dataset.preprocessing import (  # noqa: E402  (reference code)
    add_noise,
    add_obstacles_next_pos,
    add_world_pos_features,
)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F, K, E = 20250611, 40, 5, 3, 120
RANGES, SCALES = [(0, 3), (7, 8)], [0.003, 0.1]
NORMAL, OBSTACLE, HANDLE = 0.0, 1.0, 3.0


def drawn(x):
    """The standard normals add_noise drew on x [N, F + 3]: its randn_like calls, repeated under the same seed."""
    torch.manual_seed(SEED)
    return torch.cat([torch.randn_like(x[:, s:e]) for s, e in RANGES], dim=1)


def main():
    rng = np.random.default_rng(SEED)
    frame = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32))
    types = np.asarray([OBSTACLE] * 5 + [HANDLE] * 6 + [NORMAL] * (N - 11), dtype=np.float32)
    frame[:, K] = torch.from_numpy(rng.permutation(types))
    nxt = frame.clone()
    nxt[:, 0:3] += torch.from_numpy((0.01 * rng.standard_normal((N, 3))).astype(np.float32))
    nxt[:, 4] += 1.0
    obstacle, normal = frame[:, K] == OBSTACLE, (frame[:, K] == NORMAL)[:, None]
    assert int(obstacle.sum()) == 5 and 0 < int(normal.sum()) < N
    ei = torch.from_numpy(rng.integers(0, N, (2, E - 1)))
    ei = torch.cat([ei, ei[:, :1]], dim=1)  # one duplicate edge
    ea_in = torch.from_numpy(rng.standard_normal((E, 4)).astype(np.float32))

    torch.manual_seed(SEED)
    g = Data(x=frame.clone(), y=nxt[:, 0:3].clone(), edge_index=ei.clone(), edge_attr=ea_in.clone())
    g = add_obstacles_next_pos(g, 0, 3, K + 3)
    z = drawn(g.x)
    torch.manual_seed(SEED)
    g = add_noise(g, [s for s, _ in RANGES], [e for _, e in RANGES], list(SCALES), K + 3)
    g = add_world_pos_features(g, 0, 3)
    x_out, ea_out = g.x, g.edge_attr
    assert tuple(x_out.shape) == (N, F + 3) and tuple(ea_out.shape) == (E, 8)

    # the rule, term by term
    disp = nxt[:, 0:3] - frame[:, 0:3]
    d = disp[obstacle]
    assert len({tuple(r) for r in d.tolist()}) == 5
    mean = d.sum(0) / d.shape[0]
    assert torch.equal(mean, d.mean(0))
    want = torch.cat([frame[:, 0:3], torch.where(obstacle[:, None], disp, mean), frame[:, 3:]], dim=1)
    zc = 0
    for (s, e), scale in zip(RANGES, SCALES):
        noise = z[:, zc:zc + e - s] * torch.tensor(scale, dtype=torch.float32)
        want[:, s:e] = torch.where(normal, want[:, s:e] + noise, want[:, s:e])
        zc += e - s
    assert torch.equal(want, x_out), "the term-by-term rule does not reproduce the reference's x"
    assert torch.equal(x_out[:, K + 3], frame[:, K]) and not torch.equal(x_out[:, 0:3], frame[:, 0:3])
    v = want[ei[0], 0:3] - want[ei[1], 0:3]
    assert torch.equal(v, ea_out[:, 4:7]), "the relative world positions differ from the reference's"
    assert torch.equal(ea_out[:, :4], ea_in)
    norm = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    rel = ((norm - ea_out[:, 7]).abs() / ea_out[:, 7].clamp_min(1e-30)).max()
    print("norm column: max relative difference to the term-by-term form", float(rel), "(2^-24 =", 2.0 ** -24, ")")
    assert float(rel) <= 5 * 2.0 ** -24

    out = {"frame": frame.numpy(), "next_frame": nxt.numpy(), "z": z.numpy(),
           "ranges": np.asarray(RANGES, dtype=np.int32), "scales": np.asarray(SCALES, dtype=np.float64),
           "node_type_index": np.asarray(K, dtype=np.int32), "edge_index": ei.numpy().astype(np.int64),
           "edge_attr_in": ea_in.numpy(), "x_out": x_out.numpy(), "edge_attr_out": ea_out.numpy(),
           "obstacle_mean": mean.numpy(), "seed": np.asarray(SEED, dtype=np.int64)}
    path = os.path.join(HERE, "world_feed_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
