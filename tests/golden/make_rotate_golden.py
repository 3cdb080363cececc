"""Golden vectors of the reference's rotation augmentation: runs the REFERENCE's own Random3DRotate.forward
(graphphysics/dataset/preprocessing.py:277-366) in fp32 on the CPU over the stand-ins in tests/golden/_stubs and
writes tests/golden/rotate_golden.npz. Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_rotate_golden.py

The stand-in BaseTransform has no __call__, so forward is called directly; the random angles are replaced by
fixed ones (the transform's _get_random_angles is overridden on the instance). One small graph: N = 40 nodes,
x [40, 11], y [40, 3], pos [40, 3], feature_indices [(0, 3), (4, 7)]. Two cases: the angles [0.7, -2.1, 2.9]
(suffix _a) and the reference test's [0, pi/2, 0] (suffix _b). Stored (data only):
  x_in [40, 11] f32, y_in [40, 3] f32, pos_in [40, 3] f32, feature_indices [2, 2] i32, seed, and per case
  angles_* [3] f64, matrix_* [3, 3] f32 (what _build_rotation_matrix returned), x_out_* [40, 11] f32,
  y_out_* [40, 3] f32, pos_out_* [40, 3] f32.
"""
import math
import os

import numpy as np
import torch

from graphphysics.dataset.preprocessing import Random3DRotate  # noqa: E402  (reference code)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F = 20251020, 40, 11
FEATURE_INDICES = [(0, 3), (4, 7)]
CASES = {"a": [0.7, -2.1, 2.9], "b": [0.0, math.pi / 2, 0.0]}


def main():
    rng = np.random.default_rng(SEED)
    x_in = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32))
    y_in = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32))
    pos_in = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32))
    out = {"x_in": x_in.numpy(), "y_in": y_in.numpy(), "pos_in": pos_in.numpy(),
           "feature_indices": np.asarray(FEATURE_INDICES, dtype=np.int32), "seed": np.asarray(SEED, dtype=np.int64)}
    untouched = [c for c in range(F) if not any(s <= c < e for s, e in FEATURE_INDICES)]
    for key, angles in CASES.items():
        t = Random3DRotate(feature_indices=list(FEATURE_INDICES))
        t._get_random_angles = lambda angles=angles: list(angles)
        matrix = t._build_rotation_matrix(*angles)
        assert matrix.dtype == torch.float32 and tuple(matrix.shape) == (3, 3)
        g = t.forward(Data(x=x_in.clone(), y=y_in.clone(), pos=pos_in.clone()))
        assert torch.equal(g.x[:, untouched], x_in[:, untouched]) and not torch.equal(g.x, x_in)
        assert torch.allclose(matrix @ matrix.T, torch.eye(3), atol=1e-6)
        out["angles_" + key] = np.asarray(angles, dtype=np.float64)
        out["matrix_" + key] = matrix.numpy()
        out["x_out_" + key], out["y_out_" + key], out["pos_out_" + key] = g.x.numpy(), g.y.numpy(), g.pos.numpy()
        print(key, "max |x_out - x_in|", float((g.x - x_in).abs().max()))
    path = os.path.join(HERE, "rotate_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
