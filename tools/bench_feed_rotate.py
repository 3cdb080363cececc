#!/usr/bin/env python
"""Times the rotated resident-trajectory fill (dataset.resident.ResidentTrajectories(..., rotate=...): libmgn's
mgn_feed_rotation_matrices, mgn_feed_batch_rot and mgn_feed_rotate_rows) on one HIP device against the unrotated
fill and against the torch composition it replaces, at the node and edge counts of two benchmark workloads with
synthetic data in the aneurysm column layout (F = 11: velocity (0, 3), pressure, acceleration (4, 7), position
(7, 10), node type; edge_attr [dx, dy, dz, |d|]; noise on the velocity columns; T = 8 frames resident):

    cfg_e   one graph, N = 22,535 nodes, E = 1,395,256 edges   (Cfg E, aneurysm k-hop 2)
    cfg_b   8 graphs, N = 15,384 nodes, E = 88,560 edges       (Cfg B's counts; CylinderFlow itself is 2D)

    python tools/bench_feed_rotate.py [--out profiles/feed_rotate_bench.json] [--window 0.5]

Per configuration, all in this process, alternating, device events over windows of at least --window seconds after
a warm-up, the best window's mean per call:
    fill_plain    ResidentTrajectories.fill without rotate= (frame draw, normal draw, mgn_feed_batch)
    fill_rot      the same feed with rotate= and no edge_attr (+ angle draw, matrices, mgn_feed_batch_rot)
    fill_rot_ea   ... with the clean edge_attr (+ mgn_feed_rotate_rows into the batch's edge_attr)
    torch_rot_ea  fill_torch(..., triples, R) + rotate_rows_torch on the device, given frames, normals and R
    kernels_in_graph   {matrices, batch_rot, rotate_rows, feed_batch}: 50 launches of each recorded in one hipGraph
                  and replayed, so the host's launch cost is not in the figure
algorithmic_bytes: what each rule must move, computed from the shapes — a label for that count over the measured
time, not a measurement of memory traffic. Before timing, the rotated fill is compared with the torch composition
bit for bit. Fails without a HIP device (no fallback)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

F, NTI, Y_COLUMNS, T = 11, 10, (0, 3), 8
TRIPLES = [(0, 3), (4, 7), (7, 10)]
NOISE = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.02, "node_type_index": NTI}
CONFIGS = {"cfg_e": dict(B=1, n=22535, E=1395256), "cfg_b": dict(B=8, n=1923, E=88560)}


def time_calls(fn, seconds):
    """Mean milliseconds per call over one window of at least `seconds` (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, reps, total = 0, 4, 0.0
    while total < seconds * 1e3:
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        total += start.elapsed_time(end)
        n += reps
        reps *= 2
    return total / n


def best_of(fns, seconds, rounds):
    """{name: best window's ms per call}, the variants alternating."""
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            best[k] = min(best[k], time_calls(f, seconds))
    return best


class Batch:
    def __init__(self, x, y, edge_attr=None):
        self.x, self.y, self.edge_attr = x, y, edge_attr


def run(name, B, n, E, dev, window, rounds):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch, rotate_rows_torch

    N = B * n
    g = torch.Generator().manual_seed(0)
    traj = torch.randn(T, N, F, generator=g)
    traj[:, :, NTI] = torch.tensor([0.0, 0.0, 0.0, 4.0, 6.0])[torch.randint(0, 5, (N,), generator=g)]
    traj = traj.to(dev)
    gp = [i * n for i in range(B + 1)]
    per = [E // B + (1 if i < E % B else 0) for i in range(B)]  # every edge inside one graph
    ei = torch.cat([torch.randint(0, n, (2, e), generator=g) + i * n for i, e in enumerate(per)], dim=1).to(dev)
    ea = torch.randn(E, 4, generator=g).to(dev)
    ea[:, 3] = ea[:, 0:3].norm(dim=1)

    plain = ResidentTrajectories(traj, gp, Y_COLUMNS, NTI, noise=NOISE)
    rot = ResidentTrajectories(traj, gp, Y_COLUMNS, NTI, noise=NOISE, rotate={"feature_indices": TRIPLES})
    rot_ea = ResidentTrajectories(traj, gp, Y_COLUMNS, NTI, noise=NOISE,
                                  rotate={"feature_indices": TRIPLES, "edge_attr": ea, "edge_index": ei})
    b = Batch(torch.zeros(N, F, device=dev), torch.zeros(N, 3, device=dev), torch.zeros(E, 4, device=dev))

    rot_ea.fill(b)
    wx, wy = fill_torch(traj, gp, rot_ea.frame, Y_COLUMNS, NTI, rot_ea.ranges, rot_ea.scales, rot_ea.z, TRIPLES,
                        rot_ea.R)
    we = rotate_rows_torch(ea, rot_ea.row_graph, [(0, 3)], rot_ea.R)
    torch.cuda.synchronize()
    if not (torch.equal(b.x, wx) and torch.equal(b.y, wy) and torch.equal(b.edge_attr, we)):
        raise SystemExit(f"bench_feed_rotate: {name}: the rotated fill and the torch composition disagree")

    def torch_rot_ea():
        fill_torch(traj, gp, rot_ea.frame, Y_COLUMNS, NTI, rot_ea.ranges, rot_ea.scales, rot_ea.z, TRIPLES, rot_ea.R)
        rotate_rows_torch(ea, rot_ea.row_graph, [(0, 3)], rot_ea.R)

    fills = {"fill_plain": lambda: plain.fill(b), "fill_rot": lambda: rot.fill(b),
             "fill_rot_ea": lambda: rot_ea.fill(b), "torch_rot_ea": torch_rot_ea}
    for f in fills.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    best_of(fills, window, 1)  # a process's first measurements run slow: one pass dropped
    fill_ms = best_of(fills, window, rounds)

    fd = rot_ea
    kernels = {
        "matrices": lambda: nat.feed_rotation_matrices(fd.angles, fd.R),
        "batch_rot": lambda: nat.feed_batch(traj, fd.graph_ptr, fd.frame, Y_COLUMNS, NTI, fd.ranges, fd.scales, fd.z,
                                            b.x, b.y, TRIPLES, fd.R),
        "rotate_rows": lambda: nat.feed_rotate_rows(ea, fd.row_graph, [(0, 3)], fd.R, b.edge_attr),
        "feed_batch": lambda: nat.feed_batch(traj, fd.graph_ptr, fd.frame, Y_COLUMNS, NTI, fd.ranges, fd.scales, fd.z,
                                             b.x, b.y),
    }
    reps, graphs = 50, {}
    for k, f in kernels.items():
        kg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(kg):
            for _ in range(reps):
                f()
        kg.replay()
        graphs[k] = kg.replay
    torch.cuda.synchronize()
    kernel_ms = {k: v / reps for k, v in best_of(graphs, window, rounds).items()}
    W = fd.z.shape[1]
    alg = {"batch_rot": 4 * (N * F + N * 3 + N * W + N * F + N * 3 + 9 * B),
           "feed_batch": 4 * (2 * N * F + 2 * N * 3 + N * W), "rotate_rows": 4 * (2 * E * 4 + E + 9 * B)}
    return {"B": B, "N": N, "E": E, "F": F, "T": T, "fill_ms": {k: round(v, 5) for k, v in fill_ms.items()},
            "rot_ea_over_plain_ms": round(fill_ms["fill_rot_ea"] - fill_ms["fill_plain"], 5),
            "torch_over_fill_rot_ea": round(fill_ms["torch_rot_ea"] / fill_ms["fill_rot_ea"], 2),
            "kernel_ms_in_graph": {k: round(v, 6) for k, v in kernel_ms.items()}, "algorithmic_bytes": alg,
            "algorithmic_bytes_per_s": {k: round(alg[k] / (kernel_ms[k] * 1e-3)) for k in alg}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default="cfg_e,cfg_b")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_rotate: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds}
    for name in args.configs.split(","):
        out[name] = run(name, dev=dev, window=args.window, rounds=args.rounds, **CONFIGS[name])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
