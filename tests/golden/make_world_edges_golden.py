"""Golden vectors of the reference's per-sample world edges (DeformingPlate's plate.json, a transformer config whose
attention is masked by them): runs the REFERENCE's own add_world_edges (graphphysics/dataset/preprocessing.py:92-140:
scipy cKDTree.query_pairs on the fp32 world positions, the OBSTACLE–NORMAL mask, cat with the mesh edges,
to_undirected) on the CPU over the stand-ins in tests/golden/_stubs and writes tests/golden/world_edges_golden.npz.
Run where the reference is available only:

    PYTHONPATH=tests/golden/_stubs:<reference> python tests/golden/make_world_edges_golden.py

The stub's torch_geometric.utils.to_undirected only raises, so the name inside the reference module is patched with
PyG's documented result — both directions, sorted by (row, col), unique — and the stubs stay as they are. This
project's mesh helpers are loaded by file path (the reference's package has the same name).

Plate: utils.meshes.plate_sample(nx=6, ny=4, nz=2), 98 nodes (40 NORMAL, 50 OBSTACLE, 8 HANDLE), 752 directed mesh
edges (FaceToEdge on its tetrahedra + to_undirected). Two graphs of T = 4 frames each: frame f = x + amp·f/3·(y − x)
rounded to multiples of 2^-12, amp 8.0 for the first graph and 5.0 for the second, so the obstacle sinks into the
plate and the contact set grows; the two graphs overlap in space. Radius 0.03 (plate.json). The directed world-edge
counts per frame are asserted against the reference's output before anything is stored:
    amp 8.0: 56, 60, 126, 142        amp 5.0: 56, 56, 84, 128        largest world in-degree 10 in both.

Hand-made: 12 nodes at dyadic positions, radius 2^-5: an OBSTACLE–NORMAL pair at exactly 2^-5 along one axis (the
reference's verdict decides: linked), one 1 fp32 ulp beyond it (not linked), an OBSTACLE–NORMAL pair inside the radius
that is also a mesh edge (once), a HANDLE node and an OBSTACLE–OBSTACLE pair inside the radius (never linked), a node
with no neighbour at all.

Stored (data only): plate_pos [2, 4, 98, 3] f32, plate_type [98] f32, plate_mesh [2, 752] i64, plate_radius f64,
plate_ei_{g}_{f} [2, E] i64 for g in 0..1, f in 0..3, plate_world_counts [2, 4] i64; hand_pos [12, 3] f32, hand_type
[12] f32, hand_mesh [2, 18] i64, hand_radius f64, hand_ei [2, E] i64."""
import importlib.util
import os
import sys

import numpy as np
import torch

import graphphysics.dataset.preprocessing as ref_pre  # noqa: E402  (reference code)
from torch_geometric.data import Data  # noqa: E402  (stub)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
RADIUS, T, AMPS = 0.03, 4, (8.0, 5.0)
COUNTS = {8.0: [56, 60, 126, 142], 5.0: [56, 56, 84, 128]}
MAX_IN_DEGREE = 10
NORMAL, OBSTACLE, HANDLE = 0.0, 1.0, 3.0


def pyg_to_undirected(edge_index, num_nodes=None):
    """torch_geometric.utils.to_undirected on an index-only graph, as documented: cat both directions, coalesce
    (sorted by row·N + col, duplicates removed)."""
    n = int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)
    row = torch.cat([edge_index[0], edge_index[1]])
    col = torch.cat([edge_index[1], edge_index[0]])
    key = torch.unique(row.long() * n + col.long())
    return torch.stack([torch.div(key, n, rounding_mode="floor"), key % n])


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_edges(pos, types, mesh, radius):
    x = torch.cat([pos, types[:, None]], dim=1)
    g = Data(x=x, edge_index=mesh.clone())
    if getattr(g, "num_nodes", None) is None:
        g.num_nodes = x.shape[0]
    return ref_pre.add_world_edges(g, 0, 3, 3, radius=radius).edge_index


def world_part(ei, mesh, n):
    key, mkey = ei[0] * n + ei[1], mesh[0] * n + mesh[1]
    assert bool(torch.isin(mkey, key).all())
    return ei[:, ~torch.isin(key, mkey)]


def main():
    ref_pre.to_undirected = pyg_to_undirected
    meshes = load_by_path("_mgn_meshes", os.path.join(ROOT, "graph-physics_amd", "graphphysics", "utils", "meshes.py"))
    sys.path.insert(0, ROOT)
    from oracle import graph_oracle as GO

    s = meshes.plate_sample(seed=0, nx=6, ny=4, nz=2)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
    types = x0[:, 3].clone()
    assert n == 98 and [int((types == t).sum()) for t in (NORMAL, OBSTACLE, HANDLE)] == [40, 50, 8]
    mesh = GO.face_to_edge(torch.from_numpy(s["cells"]).t().contiguous(), n)
    assert tuple(mesh.shape) == (2, 752)
    out = {"plate_type": types.numpy(), "plate_mesh": mesh.numpy().astype(np.int64),
           "plate_radius": np.asarray(RADIUS, dtype=np.float64)}
    pos_all, counts = [], []
    for g, amp in enumerate(AMPS):
        frames, cnt = [], []
        for f in range(T):
            w = x0[:, 0:3] + (amp * f / (T - 1)) * (y0 - x0[:, 0:3])
            w = torch.round(w * 4096.0) / 4096.0
            ei = reference_edges(w, types, mesh, RADIUS)
            world = world_part(ei, mesh, n)
            t0, t1 = types[world[0]], types[world[1]]
            assert bool((((t0 == OBSTACLE) & (t1 == NORMAL)) | ((t0 == NORMAL) & (t1 == OBSTACLE))).all())
            assert int(torch.bincount(world[1], minlength=n).max()) <= MAX_IN_DEGREE
            cnt.append(int(world.shape[1]))
            frames.append(w)
            out[f"plate_ei_{g}_{f}"] = ei.numpy().astype(np.int64)
        assert cnt == COUNTS[amp], (amp, cnt)
        assert int(torch.bincount(world_part(ei, mesh, n)[1], minlength=n).max()) == MAX_IN_DEGREE
        pos_all.append(torch.stack(frames))
        counts.append(cnt)
    out["plate_pos"] = torch.stack(pos_all).numpy()
    out["plate_world_counts"] = np.asarray(counts, dtype=np.int64)

    # hand-made, radius 2^-5
    r = 2.0 ** -5
    beyond = float(np.nextafter(np.float32(r), np.float32(1.0)))
    O, N_, H = OBSTACLE, NORMAL, HANDLE
    nodes = [(O, (0.0, 0.0, 0.0)), (N_, (r, 0.0, 0.0)), (N_, (0.0, beyond, 0.0)), (N_, (0.0, 0.0, r / 2)),
             (H, (r / 2, r / 2, 0.0)), (O, (0.0, -r / 2, 0.0)), (N_, (1.0, 1.0, 1.0)), (N_, (0.5, 0.0, 0.0)),
             (N_, (0.5, 0.25, 0.0)), (N_, (0.5, 0.0, 0.25)), (O, (0.5 + r / 2, 0.0, 0.0)), (N_, (0.75, 0.0, 0.0))]
    hpos = torch.tensor([p for _, p in nodes], dtype=torch.float32)
    htype = torch.tensor([t for t, _ in nodes], dtype=torch.float32)
    und = torch.tensor([[0, 3], [0, 5], [1, 2], [1, 4], [7, 8], [8, 9], [7, 9], [10, 11], [2, 3]]).t()
    hmesh = pyg_to_undirected(und, 12)
    hei = reference_edges(hpos, htype, hmesh, r)
    pairs = {tuple(p) for p in world_part(hei, hmesh, 12).t().tolist()}
    want = {(0, 1), (1, 0), (3, 5), (5, 3), (7, 10), (10, 7)}
    assert pairs == want, pairs  # 0-1 at exactly the radius is linked, 0-2 one ulp beyond is not, 0-3 is a mesh edge
    assert int(((hei[0] == 0) & (hei[1] == 3)).sum()) == 1 and not bool((hei == 6).any())
    out.update(hand_pos=hpos.numpy(), hand_type=htype.numpy(), hand_mesh=hmesh.numpy().astype(np.int64),
               hand_radius=np.asarray(r, dtype=np.float64), hand_ei=hei.numpy().astype(np.int64))
    path = os.path.join(HERE, "world_edges_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
