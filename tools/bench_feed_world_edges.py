#!/usr/bin/env python
"""Times per-frame world edges inside the captured step (ResidentTrajectories(world_pos=..., dynamic_edges=...),
libmgn's mgn_world_topology_build) on one HIP device: plate.json's own model (EncodeTransformDecode, 10 blocks,
hidden size 64, 4 heads, bf16, no edge features) on 8 plates of meshes.plate_sample()'s default size (1,350 nodes
each), frame rows [world position, node type], T synthetic frames resident, radius 0.03.

    python tools/bench_feed_world_edges.py [--out profiles/feed_world_edges_bench.json] [--window 0.5]

"step": the training step, three ways, each with its own model and optimizer:
    dynamic    — (a) captured TrainStep(feed=dynamic feed): frames and noise drawn, the batch written and the topology
                 of mesh ∪ world edges rebuilt from the noisy x, all inside the one recorded graph;
    static     — (b) captured TrainStep(feed=world_pos= feed without dynamic_edges) on the same batch, its edge_index
                 the reference's of one frame, built once: what the parent commit trains on, and the floor;
    host_loop  — (c) what (a) replaces: per step and per graph a Data of the drawn frame through the package's
                 add_obstacles_next_pos, add_noise and add_world_edges (mgn_radius_pairs and mgn_coalesce, each with
                 a stream synchronisation), the graphs concatenated, a new edge_index and so a new GraphTopology,
                 then an EAGER TrainStep: a captured one would have to be recorded anew for every edge_index, which
                 costs more than the eager step.
"build": the build's three launches alone, 50 times in one hipGraph, per build: the host's launch cost is not in it.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; every round's window mean is kept, and the figures are the smallest and the largest of
them (the run-to-run spread) — at least --rounds (default 3, never fewer than 2) rounds. Before timing, the
dynamic topology of one fill is compared entry for entry with GraphTopology(edge_index of the torch rule on the
same x). Fails without a HIP device (no fallback)."""
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

NOISE = {"noise_index_start": 0, "noise_index_end": 3, "noise_scale": 0.003, "node_type_index": 6}
Y_COLUMNS, TYPE_INDEX, RADIUS = (0, 3), 3, 0.03


def rounds_of(fns, seconds, rounds):
    """{name: [ms per call of every round's window]}, the variants alternating."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            out[k].append(time_calls(f, seconds))
    return out


def spread(v):
    return {"min": round(min(v), 5), "max": round(max(v), 5), "rounds": [round(x, 5) for x in v]}


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
    args = ap.parse_args()
    args.rounds = max(args.rounds, 2)
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_world_edges: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.dataset.preprocessing import add_noise, add_obstacles_next_pos, add_world_edges
    from graphphysics.dataset.resident import ResidentTrajectories, world_topology_torch
    from graphphysics.models._engine import GraphTopology
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import graph_build, meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    dev = torch.device("cuda:0")
    B, T, W = args.batch, args.frames, args.max_neighbors
    s = meshes.plate_sample(seed=0)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
    N = n * B
    mesh1 = graph_build.face_to_edge(torch.from_numpy(s["cells"]).t().contiguous().to(dev), n)  # FaceToEdge + to_undirected
    mesh = torch.cat([mesh1 + i * n for i in range(B)], dim=1).contiguous()
    # synthetic trajectories: the sample's displacement x -> y walked further and further, so the obstacle sinks
    # into the plate and the contact set changes from frame to frame; each graph a little further than the last
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

    def dyn_feed():
        return ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp, dynamic_edges=de)

    # ------------------------------------------------------------------ the build against the torch rule
    feed = dyn_feed()
    batch = Data(x=torch.zeros(N, F + 3, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=feed.edge_index,
                 edge_attr=None)
    counts = []
    for frames in ([0] * B, [T - 2] * B, None):
        feed.set_frames("random" if frames is None else frames)
        feed.fill(batch)
        nat.check_errors(dev)
        want, _ = world_topology_torch(batch.x.cpu(), batch.x[:, TYPE_INDEX + 3].cpu(), gp, mesh.cpu(), RADIUS, W)
        E = int(feed.num_edges_dev.item())
        ref = GraphTopology(want.to(dev), N)
        ok = E == want.shape[1] and torch.equal(feed.edge_index[:, :E].cpu(), want)
        for k in ("csc_src", "csc_dst", "csc_eid", "row_perm"):
            ok = ok and torch.equal(getattr(feed.topology, k)[:E], getattr(ref, k)[:E])
        for k in ("col_ptr", "row_ptr"):
            ok = ok and torch.equal(getattr(feed.topology, k), getattr(ref, k))
        if not ok:
            raise SystemExit("bench_feed_world_edges: the dynamic topology and the torch rule disagree")
        counts.append(E - mesh.shape[1])
    static_ei = want.to(dev).contiguous()  # the reference's edge_index of the last drawn batch: the static feed's

    # ------------------------------------------------------------------ the build's launches without the host
    reps = 50
    x_fixed = batch.x.clone()
    kg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(kg):
        for _ in range(reps):
            feed.topology.build(x_fixed, x_fixed[:, TYPE_INDEX + 3])
    kg.replay()
    torch.cuda.synchronize()
    time_calls(kg.replay, args.window)
    build_ms = [v / reps for v in rounds_of({"k": kg.replay}, args.window, args.rounds)["k"]]

    # ------------------------------------------------------------------ the step, three ways
    def make_step(feed_, edge_index, graph=True):
        torch.manual_seed(0)
        model = EncodeTransformDecode(args.mp, 15, 3, hidden_size=args.hidden, num_heads=args.heads,
                                      compute_dtype=torch.bfloat16)
        sim = Simulator(15, 0, 3, 0, 6, 0, 3, 6, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        b = Data(x=batch.x.clone(), y=batch.y.clone(), edge_index=edge_index, edge_attr=None)
        return TrainStep(sim, opt, sched, b, graph=graph, feed=feed_)

    fed = dyn_feed()
    dynamic = make_step(fed, fed.edge_index)
    static = make_step(ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE, world_pos=wp), static_ei)
    host = make_step(None, static_ei, graph=False)

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
        host.batch = Data(x=torch.cat(xs), y=torch.cat(ys), edge_index=torch.cat(eis, dim=1), edge_attr=None)
        return host()

    steps = {"dynamic": dynamic, "static": static, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    nat.check_errors(dev)
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed_world_edges: a step's loss is not finite: {losses}")
    rounds_of(steps, args.window, 1)  # a process's first measurements run slow: one pass dropped
    step_ms = rounds_of(steps, args.window, args.rounds)
    nat.check_errors(dev)
    if dynamic.graph is None:
        raise SystemExit("bench_feed_world_edges: the dynamic step lost its recording")

    best = {k: min(v) for k, v in step_ms.items()}
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "B": B, "N": N, "E_mesh": int(mesh.shape[1]), "max_neighbors": W, "E_cap": int(mesh.shape[1]) + N * W,
           "world_edges_first_last_drawn": counts, "F": F, "T": T, "radius": RADIUS,
           "model": {"processor": "transformer", "mp": args.mp, "hidden": args.hidden, "heads": args.heads,
                     "dtype": "bf16"},
           "step_ms": {k: spread(v) for k, v in step_ms.items()},
           "dynamic_over_static_ms": round(best["dynamic"] - best["static"], 5),
           "dynamic_over_static_share_of_step": round((best["dynamic"] - best["static"]) / best["static"], 5),
           "host_loop_over_static_ms": round(best["host_loop"] - best["static"], 5),
           "build_ms_in_graph": spread(build_ms),
           "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
