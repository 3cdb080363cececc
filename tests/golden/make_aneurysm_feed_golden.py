"""Golden vectors of the reference's aneurysm features: runs the REFERENCE's own build_features
(graphphysics/external/aneurysm.py) and then its add_noise (graphphysics/dataset/preprocessing.py:177-238) with
coarse-aneurysm.json's six noisy column ranges and scales, in fp32 on the CPU over the stand-ins in
tests/golden/_stubs, and writes tests/golden/aneurysm_feed_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_aneurysm_feed_golden.py

One small graph: N = 48 nodes, frame rows of F = 4 columns [velocity (3), wall flag], three frames (previous,
current, next). 12 inflow nodes (pos y == 0, x < 0), of which one carries the wall flag; one node at pos (0, 0, z),
which is OUTFLOW; 5 more outflow nodes; 6 wall nodes off the face; the other 24 NORMAL. The next-frame acceleration
on the inflow nodes repeats values across nodes and across components (multiples of 2^-10 on dyadic velocities, so
the repeats are exact), one inflow node has zero acceleration (which merges with the masked zero), and six inflow
nodes carry random accelerations, so the fp32 sum of the distinct values is not exact. Noise: the batch-layout
columns [(0,1), (1,2), (2,3), (4,5), (5,6), (6,7)] with scales [10, 10, 1, 10, 10, 1] and node_type_index 13. The
standard normals add_noise drew are recovered by re-seeding and repeating its randn_like calls. Before anything is
stored the generator asserts that the rule written term by term — the node types in the reference's order, the
acceleration from clean values, min and max of the distinct set, the noise as a rounded product then a rounded
sum — reproduces every column of the reference's x except the mean bit for bit, and that the fp64 ascending mean of
the distinct values lies within 2^-24·|m_ref| + 2^-24·Σ|v| of the reference's fp32 torch.mean (the worst-case
error n·u·Σ|v| of an fp32 sum of n terms in any order, divided by n, plus the final rounding). Stored (data only):
  prev_frame, frame, next_frame [48, 4] f32, pos [48, 3] f32, z [48, 6] f32 (the ranges' columns side by side),
  ranges [6, 2] i32 (batch layout), scales [6] f64, node_type [48] f32, x_clean [48, 14] f32 (build_features'
  output), x_out [48, 14] f32 (after add_noise), distinct [n] f32 (the distinct value set, ascending; its ends are
  the reference's min and max columns), seed.
"""
import math
import os

import numpy as np
import torch

from graphphysics.dataset.preprocessing import add_noise  # noqa: E402  (reference code)
from graphphysics.external.aneurysm import build_features  # noqa: E402  (reference code)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F = 20250712, 48, 4
RANGES = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)]
SCALES = [10.0, 10.0, 1.0, 10.0, 10.0, 1.0]
NORMAL, INFLOW, OUTFLOW, WALL = 0.0, 4.0, 5.0, 6.0
TYPE_COLUMN = F + 9


def drawn(x):
    """The standard normals add_noise drew on x [N, F + 10]: its randn_like calls, repeated under the same seed."""
    torch.manual_seed(SEED)
    return torch.cat([torch.randn_like(x[:, s:e]) for s, e in RANGES], dim=1)


def main():
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
    # velocities: multiples of 2^-10, so the chosen accelerations below are exact differences
    vel = lambda: np.round(rng.standard_normal((N, 3)) * 1024.0) / 1024.0  # noqa: E731
    prev, cur = vel().astype(np.float32), vel().astype(np.float32)
    nxt = (cur + np.round(rng.standard_normal((N, 3)) * 64.0) / 1024.0).astype(np.float32)
    q = 1.0 / 1024.0
    chosen = {0: (3 * q, -5 * q, 3 * q),  # a repeat across components
              1: (3 * q, 7 * q, -5 * q),  # and across nodes
              2: (0.0, 0.0, 0.0),  # an inflow node at rest: merges with the masked zero
              3: (7 * q, 7 * q, 40 * q),
              4: (-5 * q, 40 * q, -64 * q),
              5: (12 * q, 12 * q, 12 * q)}
    for r, d in chosen.items():
        nxt[r] = cur[r] + np.asarray(d, dtype=np.float32)
    nxt[6:12] = cur[6:12] + (0.05 * rng.standard_normal((6, 3))).astype(np.float32)  # inexact sums
    frame = lambda v: torch.from_numpy(np.concatenate([v, wall[:, None]], axis=1).astype(np.float32))  # noqa: E731
    prev_f, cur_f, nxt_f, pos_t = frame(prev), frame(cur), frame(nxt), torch.from_numpy(pos)

    g = Data(x=cur_f.clone(), y=nxt_f[:, 0:3].clone(), pos=pos_t.clone(),
             previous_data={"Vitesse": prev_f[:, 0:3].numpy().copy()})
    g = build_features(g)
    x_clean = g.x.clone()
    assert tuple(x_clean.shape) == (N, F + 10) and x_clean.dtype == torch.float32
    z = drawn(g.x)
    torch.manual_seed(SEED)
    g = add_noise(g, [s for s, _ in RANGES], [e for _, e in RANGES], list(SCALES), TYPE_COLUMN)
    x_out = g.x

    # the rule, term by term
    node_type = torch.zeros(N)
    node_type[cur_f[:, 3] == 1.0] = WALL
    node_type[(pos_t[:, 1] == 0.0) & (pos_t[:, 0] <= 0)] = INFLOW
    node_type[(pos_t[:, 1] == 0.0) & (pos_t[:, 0] >= 0)] = OUTFLOW
    assert torch.equal(node_type, x_clean[:, TYPE_COLUMN])
    inflow = node_type == INFLOW
    assert int(inflow.sum()) == 12 and node_type[3] == INFLOW and node_type[12] == OUTFLOW
    assert int((node_type == NORMAL).sum()) == 24 and int((node_type == WALL).sum()) == 6
    d = nxt_f[:, 0:3] - cur_f[:, 0:3]
    vals = torch.cat([d[inflow].reshape(-1), torch.zeros(1)]) + 0.0
    distinct = torch.unique(vals)
    assert distinct.numel() < vals.numel() - 6  # repeats across nodes and components, and the merged zero
    assert bool((d[2] == 0).all()) and float(distinct.min()) < 0 < float(distinct.max())
    m_ref = float(x_clean[0, F + 6])
    total = 0.0
    for v in distinct.tolist():
        total += v
    mean = float(np.float32(total / distinct.numel()))
    sum_abs = math.fsum(abs(v) for v in distinct.tolist())
    bound = 2.0 ** -24 * abs(m_ref) + 2.0 ** -24 * sum_abs
    print(f"mean: reference {m_ref!r}, fp64 ascending {mean!r}, |difference| {abs(mean - m_ref):.3e}, bound {bound:.3e}, "
          f"{distinct.numel()} distinct of {vals.numel()} values")
    assert abs(mean - m_ref) <= bound
    want = torch.cat([cur_f, cur_f[:, 0:3] - prev_f[:, 0:3], pos_t,
                      torch.tensor([m_ref, float(distinct[0]), float(distinct[-1])]).expand(N, 3),
                      node_type[:, None]], dim=1)
    assert torch.equal(want, x_clean), "the term-by-term rule does not reproduce build_features"
    normal = (node_type == NORMAL)[:, None]
    zc = 0
    for (s, e), scale in zip(RANGES, SCALES):
        noise = z[:, zc:zc + e - s] * torch.tensor(scale, dtype=torch.float32)
        want[:, s:e] = torch.where(normal, want[:, s:e] + noise, want[:, s:e])
        zc += e - s
    assert torch.equal(want, x_out), "the term-by-term rule does not reproduce add_noise after build_features"
    assert not torch.equal(x_out[:, 0:3], x_clean[:, 0:3]) and torch.equal(x_out[:, 7:], x_clean[:, 7:])
    assert torch.equal(x_out[:, 3], x_clean[:, 3])

    out = {"prev_frame": prev_f.numpy(), "frame": cur_f.numpy(), "next_frame": nxt_f.numpy(), "pos": pos_t.numpy(),
           "z": z.numpy(), "ranges": np.asarray(RANGES, dtype=np.int32), "scales": np.asarray(SCALES, dtype=np.float64),
           "node_type": node_type.numpy(), "x_clean": x_clean.numpy(), "x_out": x_out.numpy(),
           "distinct": distinct.numpy(), "seed": np.asarray(SEED, dtype=np.int64)}
    path = os.path.join(HERE, "aneurysm_feed_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
