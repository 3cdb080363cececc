"""mgn_node_grad alone: the generic node_grad_kernel (impl 1) against chain16_node_grad_kernel (impl 2), bf16,
h = 128, on the benchmark's meshes (B copies of the CylinderFlow mesh, the plate with world edges, the k-hop-2
aneurysm mesh) and on random graphs of N nodes and mean degree d; one stream, the whole chip or a CU cap, HIP
events around each launch, the two kernels alternating; median microseconds per launch. The sizes the automatic
choice (mgn_mlp.hip node_grad_any) rests on.

    python tools/bench_node_grad.py [--reps 40] [--cus 0,160] [--out profiles/node_grad_sizes.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

H = 128
RANDOM = [(2048, 6), (15384, 6), (15384, 11), (15384, 16), (32768, 6)]


def graphs(dev, gen):
    """(name, N, edge_index on the device)"""
    import numpy as np

    from graphphysics.utils import graph_build as G
    from graphphysics.utils import meshes

    for b in (1, 2, 4, 8, 16):
        c = meshes.cylinder_batch(b, jitter=0.01)
        yield "cylinder_x%d" % b, c["x"].shape[0], torch.from_numpy(c["edge_index"]).to(dev)
    pg, _ = meshes.plate_graph(dev)
    yield "plate", pg.x.shape[0], pg.edge_index
    z = np.load(os.path.join(ROOT, "tests", "golden", "aneurysm_mesh.npz"))
    tet = torch.from_numpy(z["tetra"].astype(np.int64)).t().contiguous().to(dev)
    n = z["pos"].shape[0]
    yield "aneurysm_khop2", n, G.k_hop_edge_index(G.face_to_edge(tet, n), 2, n)
    for n, d in RANDOM:
        yield "random_d%d" % d, n, torch.randint(0, n, (2, n * d), generator=gen).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--cus", default="0,160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.models._engine import GraphTopology

    dev = torch.device("cuda:0")
    L = nat.lib()
    g = torch.Generator().manual_seed(0)
    elems = int(L.mgn_linear_pack_elems(H, 3 * H, nat.MGN_BF16))
    w32 = (0.1 * torch.randn(H, 3 * H, generator=g)).to(dev)
    pack = torch.zeros(2 * elems, dtype=torch.bfloat16, device=dev)
    job = nat.PackJob(w32.data_ptr(), pack.data_ptr(), pack.data_ptr() + 2 * elems, H, 3 * H, nat.MGN_BF16, 0, 0, 0,
                      0, 0)
    jobs = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(dev)
    nat.check(L.mgn_pack_weights(nat.ptr(jobs), 1, H * 3 * H, nat.stream_ptr(dev)))
    mlp = nat.Mlp()
    mlp.n_layers, mlp.in_dim, mlp.hidden, mlp.out_dim, mlp.has_norm, mlp.dtype = 4, 3 * H, H, H, 1, nat.MGN_BF16
    mlp.wpack, mlp.wtpack = pack.data_ptr(), pack.data_ptr() + 2 * elems
    lines = ["# graph N E cus generic_us chained_us (median of %d launches each, alternating)" % a.reps]
    for name, n, ei in graphs(dev, g):
        e = int(ei.shape[1])
        topo = GraphTopology(ei, n)
        rp = (n + 63) // 64 * 64
        dz0 = torch.randn(e, H, device=dev).to(torch.bfloat16)
        dxp = torch.randn(n, H, device=dev).to(torch.bfloat16)
        dx = torch.empty(n, H, dtype=torch.bfloat16, device=dev)
        dp8 = torch.empty(2 * rp * H, dtype=torch.bfloat16, device=dev)
        for cus in [int(c) for c in a.cus.split(",")]:
            t = {1: [], 2: []}
            for rep in range(a.reps + 5):
                for impl in (1, 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    nat.node_grad(topo.struct, mlp, dz0, dxp, dp8, dx, dx_pair=True, impl=impl, data_cus=cus)
                    e1.record()
                    e1.synchronize()
                    if rep >= 5:
                        t[impl].append(e0.elapsed_time(e1) * 1e3)
            lines.append("%s %d %d %d %.1f %.1f" % (name, n, e, cus, statistics.median(t[1]), statistics.median(t[2])))
            print(lines[-1], flush=True)
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
