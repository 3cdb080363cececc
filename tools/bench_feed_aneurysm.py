#!/usr/bin/env python
"""Times the aneurysm features of the resident-trajectory feed (ResidentTrajectories(aneurysm=...), libmgn's
mgn_feed_inflow_stats and mgn_feed_batch_aneurysm) on one HIP device: the mock aneurysm mesh
(tests/golden/aneurysm_mesh.npz, 22,535 nodes, its 1-hop edges; 193 of its nodes lie on the inflow face) with T
synthetic frames [velocity (3), wall flag] resident, and coarse-aneurysm.json's own model (transformer, 10
message-passing blocks, hidden size 64, 4 heads, bf16) and noise (six column ranges).

    python tools/bench_feed_aneurysm.py [--out profiles/feed_aneurysm_bench.json] [--window 0.5]

"step": the captured bf16 training step, three ways, each with its own model, optimizer and graph:
    fixed      — TrainStep on one fixed batch;
    feed       — TrainStep(feed=...): frame and noise drawn, and the batch written, inside the graph;
    host_loop  — the way it replaces: per step a Data of the drawn frame and its predecessor through
                 external.aneurysm.build_features and preprocessing.add_noise, `step.batch = b` (TrainStep copies it
                 into the recorded tensors), replay.
"fill": kernel = mgn_feed_batch_aneurysm alone on given frames and normals; fill = ResidentTrajectories.fill (the
    frame draw, the normal draw and the call); stats = the one mgn_feed_inflow_stats launch over all T − 1 frames
    (run once per feed, at construction). "kernel in graph": 50 fills recorded in one hipGraph and replayed, so that
    the host's launch cost is not in the figure.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; the figure is the best window's mean per call. Expectation, stated in the JSON and not a
gate: the fed step differs from the fixed-batch step by about the fill's own time in a graph (plus its two draws).
Before timing, the fill is compared bit for bit with dataset.resident.fill_aneurysm_torch evaluated on the CPU, the
statistics with inflow_stats_torch. Fails without a HIP device (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_feed import best_of  # noqa: E402  (tools/bench_feed.py: the timing loop)

F, Y_COLUMNS = 4, (0, 3)
TYPE_COLUMN = F + 9
NOISE = {"noise_index_start": [0, 1, 2, 4, 5, 6], "noise_index_end": [1, 2, 3, 5, 6, 7],
         "noise_scale": [10.0, 10.0, 1.0, 10.0, 10.0, 1.0], "node_type_index": TYPE_COLUMN}  # coarse-aneurysm.json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--mp", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_aneurysm: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.dataset.preprocessing import add_noise
    from graphphysics.dataset.resident import ResidentTrajectories, fill_aneurysm_torch, inflow_stats_torch
    from graphphysics.external.aneurysm import build_features
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import graph_build
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    dev = torch.device("cuda:0")
    T = args.frames
    z = np.load(os.path.join(ROOT, "tests", "golden", "aneurysm_mesh.npz"))
    pos = torch.from_numpy(z["pos"].astype(np.float32)).contiguous().to(dev)
    tet = torch.from_numpy(z["tetra"].astype(np.int64)).t().contiguous().to(dev)
    N = pos.shape[0]
    edge_index = graph_build.face_to_edge(tet, N)  # k-hop 1
    # synthetic frames: a smooth pulsating velocity of every node plus a little per-frame randomness, 8 % wall nodes
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(N, 3, generator=gen)
    phase = torch.sin(2 * np.pi * torch.arange(T, dtype=torch.float32) / 20.0)[:, None, None]
    vel = base[None] * (1.0 + 0.5 * phase) + 0.01 * torch.randn(T, N, 3, generator=gen)
    wall = (torch.rand(N, generator=gen) < 0.08).float()[None, :, None].expand(T, N, 1)
    traj = torch.cat([vel, wall], dim=2).contiguous().to(dev)
    gp = [0, N]

    def data():
        return Data(x=torch.zeros(N, F + 10, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=edge_index,
                    edge_attr=None)

    # ------------------------------------------------------------------ the fill against the torch rules
    feed = ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_COLUMN, noise=NOISE, aneurysm={"pos": pos})
    inflow = feed.node_type == 4
    n_inflow = int(inflow.sum())
    batch = data()
    feed.fill(batch)
    torch.cuda.synchronize()
    stats = feed.inflow_stats.cpu()
    for t in (0, T // 2, T - 2):
        want = inflow_stats_torch(traj[t].cpu(), traj[t + 1].cpu(), inflow.cpu())
        if not torch.equal(stats[t, 0], want):
            raise SystemExit(f"bench_feed_aneurysm: the statistics of frame {t} and the torch rule disagree")
    wx, wy = fill_aneurysm_torch(traj.cpu(), gp, feed.frame.cpu(), pos.cpu(), feed.node_type.cpu(), stats, Y_COLUMNS,
                                 feed.ranges, feed.scales.cpu(), feed.z.cpu())
    if not (torch.equal(batch.x.cpu(), wx) and torch.equal(batch.y.cpu(), wy)):
        raise SystemExit("bench_feed_aneurysm: fill and the torch rule disagree")

    def kernel():
        nat.feed_batch_aneurysm(traj, feed.graph_ptr, feed.frame, Y_COLUMNS, feed.pos, feed.node_type,
                                feed.inflow_stats, feed._ranges_c, feed.scales, feed.z, batch.x, batch.y)

    fills = {"kernel": kernel, "fill": lambda: feed.fill(batch), "stats": feed.refresh_stats}
    for f in fills.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    best_of(fills, args.window, 1)  # a process's first measurements run slow: one pass dropped
    fill_ms = best_of(fills, args.window, args.rounds)

    reps = 50
    kg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(kg):
        for _ in range(reps):
            kernel()
    kg.replay()
    torch.cuda.synchronize()
    kernel_ms = best_of({"k": kg.replay}, args.window, args.rounds)["k"] / reps

    # ------------------------------------------------------------------ the captured bf16 step, three ways
    def make_step(feed_=None):
        torch.manual_seed(0)
        model = EncodeTransformDecode(args.mp, TYPE_COLUMN + 9, 3, hidden_size=args.hidden, num_heads=4,
                                      compute_dtype=torch.bfloat16)
        sim = Simulator(TYPE_COLUMN + 9, 0, 3, 0, TYPE_COLUMN, 0, 3, TYPE_COLUMN, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        b = data()
        feed.fill(b)  # a real batch for the fixed variant and for the statistics of the first steps
        return TrainStep(sim, opt, sched, b, graph=True, feed=feed_)

    fixed = make_step()
    fed = make_step(ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_COLUMN, noise=NOISE, aneurysm={"pos": pos}))
    host = make_step()

    def host_loop():
        f = int(torch.randint(1, T - 1, (1,)))
        d = Data(x=traj[f].clone(), y=traj[f + 1, :, 0:3].clone(), pos=pos, previous_data=traj[f - 1, :, 0:3])
        d = build_features(d)
        d = add_noise(d, NOISE["noise_index_start"], NOISE["noise_index_end"], NOISE["noise_scale"],
                      NOISE["node_type_index"])
        host.batch = Data(x=d.x, y=d.y, edge_index=edge_index, edge_attr=None)
        return host()

    steps = {"fixed": fixed, "feed": fed, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed_aneurysm: a step's loss is not finite: {losses}")
    best_of(steps, args.window, 1)
    step_ms = best_of(steps, args.window, args.rounds)

    over = step_ms["feed"] - step_ms["fixed"]
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "B": 1, "N": N, "E": int(edge_index.shape[1]), "F": F, "batch_row": F + 10, "T": T,
           "inflow_nodes": n_inflow, "values_per_set": feed._max_values, "mp": args.mp, "hidden": args.hidden,
           "heads": 4, "dtype": "bf16", "fill_ms": {k: round(v, 5) for k, v in fill_ms.items()},
           "kernel_ms_in_graph": round(kernel_ms, 6),
           "step_ms": {k: round(v, 5) for k, v in step_ms.items()},
           "feed_over_fixed_ms": round(over, 5),
           "host_loop_over_fixed_ms": round(step_ms["host_loop"] - step_ms["fixed"], 5),
           "expectation": "feed_over_fixed_ms is about the fill's own time inside a graph (kernel_ms_in_graph plus "
                          "the frame and normal draws); a finding if it is not, not a gate",
           "feed_over_fixed_in_fills": round(over / kernel_ms, 2) if kernel_ms > 0 else None,
           "feed_not_slower_than_host_loop": bool(step_ms["feed"] <= step_ms["host_loop"]),
           "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
