"""Golden vectors of the reference's training noise: runs the REFERENCE's own add_noise
(graphphysics/dataset/preprocessing.py:177-238) in fp32 on the CPU over the stand-ins in tests/golden/_stubs
and writes tests/golden/feed_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_feed_golden.py

One small x: N = 40 nodes, F = 6 columns, column 5 the node type (a mix of NORMAL 0, INFLOW 4, OUTFLOW 5 and
WALL_BOUNDARY 6), noisy column ranges [(0, 2), (3, 5)] with scales [0.02, 0.5]. add_noise runs twice under
torch.manual_seed(SEED): plainly, and with the curriculum argument t = 0.25. The standard normals it drew are
recovered by re-seeding and repeating its randn_like calls (one per range, on the same views); the generator
asserts that x_in + z * scale on the NORMAL rows reproduces add_noise's output bit for bit before it stores
anything. Stored (data only):
  x_in [40, 6] f32, z [40, 4] f32 (the ranges' columns side by side, in range order), x_out [40, 6] f32,
  x_out_t [40, 6] f32 (the t run: the same z), ranges [2, 2] i32, scales [2] f64, node_type_index, t,
  scales_t [2] f64 (the two scale_ values 10 * scale * (1 + cos(t * pi)) of the t run), seed.
"""
import math
import os

import numpy as np
import torch

from graphphysics.dataset.preprocessing import add_noise  # noqa: E402  (reference code)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F, NTI = 20250607, 40, 6, 5
RANGES, SCALES, T_CURRICULUM = [(0, 2), (3, 5)], [0.02, 0.5], 0.25


def drawn(x_in):
    """The standard normals add_noise drew: its randn_like calls, repeated under the same seed."""
    torch.manual_seed(SEED)
    return torch.cat([torch.randn_like(x_in[:, s:e]) for s, e in RANGES], dim=1)


def run(x_in, t):
    torch.manual_seed(SEED)
    g = add_noise(Data(x=x_in.clone()), [s for s, _ in RANGES], [e for _, e in RANGES], list(SCALES), NTI, t=t)
    return g.x


def main():
    rng = np.random.default_rng(SEED)
    x_in = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32))
    x_in[:, NTI] = torch.from_numpy(rng.choice([0, 0, 0, 4, 5, 6], N).astype(np.float32))
    assert set(x_in[:, NTI].tolist()) == {0.0, 4.0, 5.0, 6.0}
    z = drawn(x_in)
    scales_t = [10 * s * (1 + math.cos(T_CURRICULUM * math.pi)) for s in SCALES]
    out = {"x_in": x_in.numpy(), "z": z.numpy(), "ranges": np.asarray(RANGES, dtype=np.int32),
           "scales": np.asarray(SCALES, dtype=np.float64), "node_type_index": np.asarray(NTI, dtype=np.int32),
           "t": np.asarray(T_CURRICULUM, dtype=np.float64), "scales_t": np.asarray(scales_t, dtype=np.float64),
           "seed": np.asarray(SEED, dtype=np.int64)}
    normal = (x_in[:, NTI] == 0)[:, None]
    for key, t, sc in (("x_out", None, SCALES), ("x_out_t", T_CURRICULUM, scales_t)):
        x_out = run(x_in, t)
        want, zc = x_in.clone(), 0
        for (s, e), scale in zip(RANGES, sc):
            noise = z[:, zc:zc + e - s] * torch.tensor(scale, dtype=torch.float32)
            want[:, s:e] = torch.where(normal, x_in[:, s:e] + noise, x_in[:, s:e])
            zc += e - s
        assert torch.equal(want, x_out), f"{key}: the recovered z does not reproduce add_noise"
        assert not torch.equal(x_out, x_in) and torch.equal(x_out[~normal[:, 0]], x_in[~normal[:, 0]])
        out[key] = x_out.numpy()
        print(key, "max |x_out - x_in|", float((x_out - x_in).abs().max()))
    path = os.path.join(HERE, "feed_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
