#!/usr/bin/env python
"""Times the world-position stages of the resident-trajectory feed (ResidentTrajectories(world_pos=...), libmgn's
mgn_feed_batch_world and mgn_feed_world_edge_features) on one HIP device, at Cfg C's size (DeformingPlate:
meshes.plate_sample defaults, 8 graphs of 1,350 nodes, frame rows [world position, node type], the static edges
of meshes.plate_graph, 15 message-passing blocks, hidden size 128, bf16) with T synthetic frames resident.

    python tools/bench_feed_world.py [--out profiles/feed_world_bench.json] [--window 0.5]

(a) "fill": one batch's x, y and the four world columns of edge_attr.  kernel = the two libmgn calls alone on given
    frames and normals; fill = ResidentTrajectories.fill (the frame draw, the normal draw and the calls);
    fill_torch = the same rules as torch ops on the device (dataset.resident.fill_world_torch and
    world_edge_features_torch) on the same given frames and normals.
(b) "step": the captured bf16 training step, three ways, each with its own model, optimizer and graph:
    fixed      — TrainStep on one fixed batch;
    feed       — TrainStep(feed=...): frames and noise drawn, and the batch written, inside the graph;
    host_loop  — the way it replaces: per step and per graph a Data of the drawn frame through the package's
                 add_obstacles_next_pos, add_noise and add_world_pos_features, the graphs concatenated,
                 `step.batch = b` (TrainStep copies it into the recorded tensors), replay.
(c) "kernel": 50 fills (both calls) recorded in one hipGraph and replayed, so that the host's launch cost is not in
    the figure.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; the figure is the best window's mean per call. Before timing, fill is compared with the
torch rules evaluated on the CPU (x, y and the edge columns bit for bit; the obstacle mean, whose sum the kernel
orders differently, to the distance two fp32 sums of its terms can have). Fails without a HIP device (no
fallback)."""
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

NOISE = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.003, "node_type_index": 6}
Y_COLUMNS, TYPE_INDEX, EA_START = (0, 3), 3, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--mp", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_world: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.dataset.preprocessing import add_noise, add_obstacles_next_pos, add_world_pos_features
    from graphphysics.dataset.resident import ResidentTrajectories, fill_world_torch, world_edge_features_torch
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames
    s = meshes.plate_sample(seed=0)
    g, _ = meshes.plate_graph(dev, seed=0)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n, E1 = x0.shape[0], g.edge_index.shape[1]
    N = n * B
    # synthetic trajectories: the sample's displacement x -> y walked in T - 1 steps, each graph a little further
    gen = torch.Generator().manual_seed(0)
    amp = 1.0 + 0.2 * torch.rand(B, generator=gen)
    t = torch.arange(T, dtype=torch.float32)[:, None, None, None] / (T - 1)
    world = x0[None, None, :, 0:3] + t * amp[None, :, None, None] * (y0 - x0[:, 0:3])[None, None]
    nt = x0[None, None, :, 3:4].expand(T, B, n, 1)
    traj = torch.cat([world, nt], dim=3).reshape(T, N, 4).contiguous().to(dev)
    gp = [i * n for i in range(B + 1)]
    ei1 = g.edge_index
    edge_index = torch.cat([ei1 + i * n for i in range(B)], dim=1).contiguous()
    mesh_ea = g.edge_attr[:, :EA_START].contiguous()  # Cartesian ‖ Distance of the mesh: static
    base_ea = torch.cat([g.edge_attr] * B, dim=0).contiguous()
    F = traj.shape[2]
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": TYPE_INDEX + 3,
          "edge_index": edge_index, "edge_attr_start": EA_START}

    def data():
        return Data(x=torch.zeros(N, F + 3, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=edge_index,
                    edge_attr=base_ea.clone())

    # ------------------------------------------------------------------ (a) fill against the torch rules
    feed = ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp)
    batch = data()
    feed.fill(batch)
    torch.cuda.synchronize()
    wx, wy, wm = fill_world_torch(traj.cpu(), gp, feed.frame.cpu(), Y_COLUMNS, TYPE_INDEX, feed.ranges,
                                  feed.scales.cpu(), feed.z.cpu())
    mean = feed.obstacle_mean.cpu()
    n_obstacle = int((x0[:, TYPE_INDEX] == 1).sum())  # two fp32 sums of M terms differ by at most 2 M 2^-24, relative
    if float(((mean - wm).abs() / wm.abs().clamp_min(1e-30)).max()) > n_obstacle * 2.0 ** -23:
        raise SystemExit("bench_feed_world: the obstacle mean is off")
    wx[:, 3:6] = torch.where((wx[:, 6] == 1)[:, None], wx[:, 3:6], mean.repeat_interleave(n, dim=0))
    wea = world_edge_features_torch(wx, edge_index.cpu(), base_ea.cpu(), EA_START)
    if not (torch.equal(batch.x.cpu(), wx) and torch.equal(batch.y.cpu(), wy) and torch.equal(batch.edge_attr.cpu(), wea)):
        raise SystemExit("bench_feed_world: fill and the torch rules disagree")

    def kernel():
        nat.feed_batch_world(traj, feed.graph_ptr, feed.frame, Y_COLUMNS, TYPE_INDEX, feed.ranges, feed.scales, feed.z,
                             batch.x, batch.y, feed.obstacle_mean)
        nat.feed_world_edge_features(feed.senders, feed.receivers, batch.x, batch.edge_attr, EA_START)

    scratch_ea = base_ea.clone()

    def rules():
        x, _, _ = fill_world_torch(traj, gp, feed.frame, Y_COLUMNS, TYPE_INDEX, feed.ranges, feed.scales, feed.z)
        world_edge_features_torch(x, edge_index, scratch_ea, EA_START)

    fills = {"kernel": kernel, "fill": lambda: feed.fill(batch), "fill_torch": rules}
    for f in fills.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    best_of(fills, args.window, 1)  # a process's first measurements run slow: one pass dropped
    fill_ms = best_of(fills, args.window, args.rounds)

    # ------------------------------------------------------------------ (c) the kernels without the host
    reps = 50
    kg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(kg):
        for _ in range(reps):
            kernel()
    kg.replay()
    torch.cuda.synchronize()
    kernel_ms = best_of({"k": kg.replay}, args.window, args.rounds)["k"] / reps

    # ------------------------------------------------------------------ (b) the captured bf16 step, three ways
    def make_step(feed_=None):
        torch.manual_seed(0)
        model = EncodeProcessDecode(args.mp, 15, 8, 3, args.hidden, compute_dtype=torch.bfloat16)
        sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        b = data()
        feed.fill(b)  # a real batch for the fixed variant and for the statistics of the first steps
        return TrainStep(sim, opt, sched, b, graph=True, feed=feed_)

    fixed = make_step()
    fed = make_step(ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp))
    host = make_step()

    def host_loop():
        frames = torch.randint(0, T - 1, (B,)).tolist()
        xs, ys, eas = [], [], []
        for i, f in enumerate(frames):
            rows = slice(gp[i], gp[i + 1])
            d = Data(x=traj[f, rows].clone(), y=traj[f + 1, rows, 0:3].clone(), edge_index=ei1, edge_attr=mesh_ea)
            d = add_obstacles_next_pos(d, 0, 3, TYPE_INDEX + 3)
            d = add_noise(d, NOISE["noise_index_start"], NOISE["noise_index_end"], NOISE["noise_scale"],
                          NOISE["node_type_index"])
            d = add_world_pos_features(d, 0, 3)
            xs.append(d.x)
            ys.append(d.y)
            eas.append(d.edge_attr)
        host.batch = Data(x=torch.cat(xs), y=torch.cat(ys), edge_index=edge_index, edge_attr=torch.cat(eas))
        return host()

    steps = {"fixed": fixed, "feed": fed, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed_world: a step's loss is not finite: {losses}")
    best_of(steps, args.window, 1)
    step_ms = best_of(steps, args.window, args.rounds)

    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "B": B, "N": N, "E": int(edge_index.shape[1]), "F": F, "T": T, "mp": args.mp, "hidden": args.hidden,
           "dtype": "bf16", "fill_ms": {k: round(v, 5) for k, v in fill_ms.items()},
           "fill_torch_over_fill": round(fill_ms["fill_torch"] / fill_ms["fill"], 2),
           "kernels_ms_in_graph": round(kernel_ms, 6),
           "step_ms": {k: round(v, 5) for k, v in step_ms.items()},
           "feed_over_fixed_ms": round(step_ms["feed"] - step_ms["fixed"], 5),
           "host_loop_over_fixed_ms": round(step_ms["host_loop"] - step_ms["fixed"], 5),
           "feed_not_slower_than_host_loop": bool(step_ms["feed"] <= step_ms["host_loop"]),
           "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
