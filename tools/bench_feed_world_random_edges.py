#!/usr/bin/env python
"""Times world edges and random long-range edges in ONE topology inside the captured step
(ResidentTrajectories(world_pos=..., dynamic_edges=..., random_edges=..., one_topology=True), libmgn's
mgn_world_random_topology_build) on one HIP device: plate.json's own model (EncodeTransformDecode, 10 blocks, hidden size 64, 4 heads, bf16, no edge
features) on 8 plates of meshes.plate_sample()'s default size (1,350 nodes each), frame rows [world position, node
type], T synthetic frames resident, radius 0.03, max_neighbors 16, ratio 0.5, max_new 16.

    python tools/bench_feed_world_random_edges.py [--out profiles/feed_world_random_edges_bench.json] [--window 0.5]

"step": the training step, four ways, each with its own model and optimizer:
    combined   — (a) captured TrainStep(feed=combined feed): frames, noise and pairs drawn, the batch written and the
                 topology of mesh ∪ world ∪ random edges rebuilt from the noisy x, all inside the one recorded graph;
    off        — (b) the same kind of feed after set_random_edges(False): the same recording's launches, no random edge;
    dynamic    — (c) captured TrainStep(feed=dynamic_edges=-only feed) on the same batch: what a user had before, and
                 the floor;
    host_loop  — (d) what (a) replaces: per step and per graph a Data of the drawn frame through the package's
                 add_obstacles_next_pos, add_noise and add_world_edges (mgn_radius_pairs and mgn_coalesce, each with
                 a stream synchronisation), the graphs concatenated, the pairs drawn and random_topology_torch on that
                 edge_index on device tensors, a new edge_index and so a new GraphTopology, then an EAGER TrainStep (a
                 captured one would have to be recorded anew for every edge_index, which costs more than the eager
                 step).
"build": the launches of one build alone, 50 times in one hipGraph, per build — the combined build beside
mgn_world_topology_build alone and mgn_random_topology_build alone on the same inputs; the host's launch cost is not
in it.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; every round's window mean is kept, and the figures are the smallest and the largest of
them (the run-to-run spread) — at least --rounds (default 3, never fewer than 2) rounds. Before timing, the combined
topology of a few fills is compared entry for entry with the torch rule on the same x and pairs. Fails without a HIP
device (no fallback)."""
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

from bench_feed import time_calls  # noqa: E402  (tools/bench_feed.py: one timing window)
from bench_feed_world_edges import NOISE, RADIUS, TYPE_INDEX, Y_COLUMNS, rounds_of, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--mp", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--max-neighbors", type=int, default=16)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--max-new", type=int, default=16)
    args = ap.parse_args()
    args.rounds = max(args.rounds, 2)
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_world_random_edges: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.dataset.preprocessing import add_noise, add_obstacles_next_pos, add_world_edges
    from graphphysics.dataset.resident import ResidentTrajectories, random_topology_torch, world_random_topology_torch
    from graphphysics.models._engine import DynamicTopology, RandomTopology
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import graph_build, meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    dev = torch.device("cuda:0")
    B, T, W, R = args.batch, args.frames, args.max_neighbors, args.max_new
    s = meshes.plate_sample(seed=0)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
    N = n * B
    mesh1 = graph_build.face_to_edge(torch.from_numpy(s["cells"]).t().contiguous().to(dev), n)  # FaceToEdge + to_undirected
    mesh = torch.cat([mesh1 + i * n for i in range(B)], dim=1).contiguous()
    # bench_feed_world_edges' synthetic trajectories: the obstacle sinks into the plate, the contact set changes
    gen = torch.Generator().manual_seed(0)
    amp = 4.0 + 2.0 * torch.rand(B, generator=gen)
    t = torch.arange(T, dtype=torch.float32)[:, None, None, None] / (T - 1)
    world = x0[None, None, :, 0:3] + t * amp[None, :, None, None] * (y0 - x0[:, 0:3])[None, None]
    nt = x0[None, None, :, 3:4].expand(T, B, n, 1)
    traj = torch.cat([world, nt], dim=3).reshape(T, N, 4).contiguous().to(dev)
    gp = [i * n for i in range(B + 1)]
    F = traj.shape[2]
    wp = {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": TYPE_INDEX + 3}
    de = {"edge_index": mesh, "radius": RADIUS, "max_neighbors": W}
    re = {"edge_index": mesh, "ratio": args.ratio, "max_new": R}

    def combined_feed():
        return ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp, dynamic_edges=de,
                                    random_edges=re, one_topology=True)

    # ------------------------------------------------------------------ the build against the torch rule
    feed = combined_feed()
    cand = feed.cand_ptr.tolist()
    batch = Data(x=torch.zeros(N, F + 3, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=feed.edge_index,
                 edge_attr=None)
    world_counts, new_counts = [], []
    for frames in ([0] * B, [T - 2] * B, None):
        feed.set_frames("random" if frames is None else frames)
        feed.fill(batch)
        nat.check_errors(dev)
        want, arrays = world_random_topology_torch(batch.x, batch.x[:, TYPE_INDEX + 3], feed.pairs, gp, mesh, RADIUS, W,
                                                   R, cand_ptr=cand)
        E = int(feed.num_edges_dev.item())
        ok = E == want.shape[1] and torch.equal(feed.edge_index[:, :E], want)
        for k in ("csc_src", "csc_dst", "csc_eid", "row_perm"):
            ok = ok and torch.equal(getattr(feed.topology, k)[:E], arrays[k])
        for k in ("col_ptr", "row_ptr"):
            ok = ok and torch.equal(getattr(feed.topology, k), arrays[k])
        if not ok:
            raise SystemExit("bench_feed_world_random_edges: the combined topology and the torch rule disagree")
        feed.set_random_edges(False)
        feed.build_edges(batch.x, batch.x[:, TYPE_INDEX + 3])
        feed.set_random_edges(True)
        E_w = int(feed.num_edges_dev.item())
        world_counts.append(E_w - mesh.shape[1])
        new_counts.append(E - E_w)

    # ------------------------------------------------------------------ the builds' launches without the host
    reps = 50
    x_fixed = batch.x.clone()
    pairs_fixed = feed.pairs.clone()
    on = torch.ones(1, dtype=torch.int32, device=dev)
    dyn_topo = DynamicTopology(mesh, gp, N, RADIUS, W, dev)
    ran_topo = RandomTopology(mesh, gp, N, cand, R, dev)
    builds = {"combined": lambda: feed.topology.build(x_fixed, x_fixed[:, TYPE_INDEX + 3], pairs_fixed, on),
              "world_alone": lambda: dyn_topo.build(x_fixed, x_fixed[:, TYPE_INDEX + 3]),
              "random_alone": lambda: ran_topo.build(pairs_fixed, on)}
    graphs = {}
    for k, f in builds.items():
        f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                f()
        g.replay()
        torch.cuda.synchronize()
        graphs[k] = g.replay
    nat.check_errors(dev)
    rounds_of(graphs, args.window, 1)
    build_ms = {k: [v / reps for v in vs] for k, vs in rounds_of(graphs, args.window, args.rounds).items()}

    # ------------------------------------------------------------------ the step, four ways
    def make_step(feed_, edge_index, graph=True):
        torch.manual_seed(0)
        model = EncodeTransformDecode(args.mp, 15, 3, hidden_size=args.hidden, num_heads=args.heads,
                                      compute_dtype=torch.bfloat16)
        sim = Simulator(15, 0, 3, 0, 6, 0, 3, 6, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        b = Data(x=batch.x.clone(), y=batch.y.clone(), edge_index=edge_index, edge_attr=None)
        return TrainStep(sim, opt, sched, b, graph=graph, feed=feed_)

    fed = combined_feed()
    combined = make_step(fed, fed.edge_index)
    fed_off = combined_feed()
    fed_off.set_random_edges(False)
    off = make_step(fed_off, fed_off.edge_index)
    fed_dyn = ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp, dynamic_edges=de)
    dynamic = make_step(fed_dyn, fed_dyn.edge_index)
    host = make_step(None, feed.current_edge_index().clone(), graph=False)
    pairs = torch.zeros_like(feed.pairs)

    def host_loop():
        frames = torch.randint(0, T - 1, (B,)).tolist()
        xs, ys, eis = [], [], []
        for i, f in enumerate(frames):
            rows = slice(gp[i], gp[i + 1])
            d = Data(x=traj[f, rows].clone(), y=traj[f + 1, rows, 0:3].clone(), edge_index=mesh1, edge_attr=None)
            d = add_obstacles_next_pos(d, 0, 3, TYPE_INDEX + 3)
            d = add_noise(d, NOISE["noise_index_start"], NOISE["noise_index_end"], NOISE["noise_scale"],
                          NOISE["node_type_index"])
            d = add_world_edges(d, 0, 3, TYPE_INDEX + 3, radius=RADIUS)
            xs.append(d.x)
            ys.append(d.y)
            eis.append(d.edge_index + gp[i])
        pairs.random_(0, 2 ** 31 - 1)
        ei, _ = random_topology_torch(pairs, gp, torch.cat(eis, dim=1), R, cand_ptr=cand)
        host.batch = Data(x=torch.cat(xs), y=torch.cat(ys), edge_index=ei.contiguous(), edge_attr=None)
        return host()

    steps = {"combined": combined, "off": off, "dynamic": dynamic, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    nat.check_errors(dev)
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed_world_random_edges: a step's loss is not finite: {losses}")
    rounds_of(steps, args.window, 1)  # a process's first measurements run slow: one pass dropped
    step_ms = rounds_of(steps, args.window, args.rounds)
    nat.check_errors(dev)
    if combined.graph is None or off.graph is None or dynamic.graph is None:
        raise SystemExit("bench_feed_world_random_edges: a captured step lost its recording")

    best = {k: min(v) for k, v in step_ms.items()}
    bbest = {k: min(v) for k, v in build_ms.items()}
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "B": B, "N": N, "E_mesh": int(mesh.shape[1]), "max_neighbors": W, "ratio": args.ratio, "max_new": R,
           "num_candidates": cand[-1], "E_cap": int(mesh.shape[1]) + N * (W + R),
           "world_edges_first_last_drawn": world_counts, "random_edges_first_last_drawn": new_counts, "F": F, "T": T,
           "radius": RADIUS,
           "model": {"processor": "transformer", "mp": args.mp, "hidden": args.hidden, "heads": args.heads,
                     "dtype": "bf16"},
           "step_ms": {k: spread(v) for k, v in step_ms.items()},
           "combined_over_dynamic_ms": round(best["combined"] - best["dynamic"], 5),
           "off_over_dynamic_ms": round(best["off"] - best["dynamic"], 5),
           "host_loop_over_combined": round(best["host_loop"] / best["combined"], 3),
           "build_ms_in_graph": {k: spread(v) for k, v in build_ms.items()},
           "combined_build_minus_sum_of_both_ms": round(bbest["combined"] - bbest["world_alone"] - bbest["random_alone"],
                                                        5),
           "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
