#!/usr/bin/env python
"""Times random long-range edges inside the captured step (ResidentTrajectories(random_edges=...), libmgn's
mgn_random_topology_build) on one HIP device, at ratio 0.5 and max_new 16, in two configurations:
    cylinder — meshes.cylinder_batch(8) (8 CylinderFlow meshes, 15,384 nodes) with panels.json's transformer
               (15 blocks, hidden size 128, 4 heads, bf16), a plain feed of frame rows [velocity (2), node type];
    aneurysm — the mock aneurysm mesh (tests/golden/aneurysm_mesh.npz, 22,535 nodes, its 1-hop edges) with
               coarse-aneurysm.json's transformer (10 blocks, hidden size 64, 4 heads, bf16), an aneurysm= feed.

    python tools/bench_feed_random_edges.py [--out profiles/feed_random_edges_bench.json] [--window 0.5]

"step": the training step, four ways, each with its own model and optimizer:
    random     — (a) captured TrainStep(feed=random_edges feed): frames, noise and candidate pairs drawn, the batch
                 written and the topology of mesh ∪ random edges rebuilt, all inside the one recorded graph;
    off        — (b) the same kind of feed after set_random_edges(False): the same capacity and the same launches,
                 mesh edges only (the search finds its candidate range empty): the floor of (a);
    static     — (c) captured TrainStep(feed=the same feed without random_edges=) on the mesh edge_index: what the
                 parent commit trains on;
    host_loop  — (d) what (a) replaces: per step the pairs drawn, random_topology_torch on device tensors, a new
                 edge_index and so a new GraphTopology, then an EAGER TrainStep (a captured one would have to be
                 recorded anew for every edge_index, which costs more than the eager step).
"build": (e) the build's memset and five launches alone, 50 times in one hipGraph, per build: the host's launch cost is
not in it. (a) − (b) is the search plus the cost of attending over the extra edges; (b) − (c) what the fixed capacity,
the scan and the merge cost.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; every round's window mean is kept, and the figures are the smallest and the largest of
them (the run-to-run spread) — at least --rounds (default 3, never fewer than 2) rounds. Before timing, the topology
of one fill is compared entry for entry with the torch rule on the same pairs. Fails without a HIP device (no
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

from bench_feed import time_calls  # noqa: E402  (tools/bench_feed.py: one timing window)

ARRAYS = ("csc_src", "csc_dst", "csc_eid", "row_perm", "col_ptr", "row_ptr")


def rounds_of(fns, seconds, rounds):
    """{name: [ms per call of every round's window]}, the variants alternating."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            out[k].append(time_calls(f, seconds))
    return out


def spread(v):
    return {"min": round(min(v), 5), "max": round(max(v), 5), "rounds": [round(x, 5) for x in v]}


def sorted_mesh(ei, N):
    """edge_index sorted by (row, col), every edge once."""
    key = torch.unique(ei[0].to(torch.int64) * N + ei[1].to(torch.int64))
    return torch.stack([torch.div(key, N, rounding_mode="floor"), key % N]).contiguous()


def cylinder(args, dev):
    """(traj, node offsets, mesh, feed keywords, node-type column, width of y, (mp, hidden, heads))."""
    from graphphysics.utils import meshes

    mesh = meshes.load_cylinder_mesh()
    B, T = 8, args.frames
    b = meshes.cylinder_batch(B, jitter=0.01, mesh=mesh)
    n = b["nodes_per_graph"]
    N = n * B
    vel = torch.from_numpy(mesh["velocity"].astype(np.float32))
    nt = torch.from_numpy(mesh["node_type"].astype(np.float32))
    g = torch.Generator().manual_seed(0)
    amp = 1.0 + 0.05 * torch.randn(T, B, 1, 1, generator=g)
    v = (vel[torch.arange(T) % vel.shape[0]][:, None] * amp).reshape(T, N, 2)
    traj = torch.cat([v, nt.repeat(B)[None, :, None].expand(T, N, 1)], dim=2).contiguous().to(dev)
    noise = {"noise_index_start": 0, "noise_index_end": 2, "noise_scale": 0.02, "node_type_index": 2}
    return (traj, [i * n for i in range(B + 1)], sorted_mesh(torch.from_numpy(b["edge_index"]), N),
            dict(noise=noise), 2, 2, (15, 128, 4))


def aneurysm(args, dev):
    from graphphysics.utils import graph_build

    T = args.frames
    z = np.load(os.path.join(ROOT, "tests", "golden", "aneurysm_mesh.npz"))
    pos = torch.from_numpy(z["pos"].astype(np.float32)).contiguous().to(dev)
    tet = torch.from_numpy(z["tetra"].astype(np.int64)).t().contiguous().to(dev)
    N = pos.shape[0]
    mesh = sorted_mesh(graph_build.face_to_edge(tet, N).cpu(), N)  # k-hop 1
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(N, 3, generator=gen)
    phase = torch.sin(2 * np.pi * torch.arange(T, dtype=torch.float32) / 20.0)[:, None, None]
    vel = base[None] * (1.0 + 0.5 * phase) + 0.01 * torch.randn(T, N, 3, generator=gen)
    wall = (torch.rand(N, generator=gen) < 0.08).float()[None, :, None].expand(T, N, 1)
    traj = torch.cat([vel, wall], dim=2).contiguous().to(dev)
    noise = {"noise_index_start": [0, 1, 2, 4, 5, 6], "noise_index_end": [1, 2, 3, 5, 6, 7],
             "noise_scale": [10.0, 10.0, 1.0, 10.0, 10.0, 1.0], "node_type_index": 13}  # coarse-aneurysm.json
    return traj, [0, N], mesh, dict(noise=noise, aneurysm={"pos": pos}), 13, 3, (10, 64, 4)


def run(name, args, dev):
    from graphphysics import _native as nat
    from graphphysics.dataset.resident import ResidentTrajectories, random_topology_torch
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    traj, gp, mesh, kw, type_column, wy, (mp, hidden, heads) = {"cylinder": cylinder, "aneurysm": aneurysm}[name](args, dev)
    N, W = traj.shape[1], args.max_new
    re = {"edge_index": mesh, "ratio": args.ratio, "max_new": W}
    mesh_dev = mesh.to(dev)

    def make_feed(random=True):
        return ResidentTrajectories(traj, gp, (0, wy), type_column, random_edges=re if random else None, **kw)

    # ------------------------------------------------------------------ the build against the torch rule
    feed = make_feed()
    C, cand = feed.pairs.shape[0], feed.cand_ptr.tolist()
    batch = Data(x=torch.zeros(N, feed.Fx, device=dev), y=torch.zeros(N, wy, device=dev), edge_index=feed.edge_index,
                 edge_attr=None)
    live = []
    for _ in range(2):
        feed.fill(batch)
        want, arrays = random_topology_torch(feed.pairs, gp, mesh_dev, W, cand_ptr=cand)
        E = int(feed.num_edges_dev.item())
        ok = E == want.shape[1] and torch.equal(feed.edge_index[:, :E], want)
        for k in ARRAYS:
            n = N + 1 if k.endswith("_ptr") else E
            ok = ok and torch.equal(getattr(feed.topology, k)[:n], arrays[k])
        if not ok:
            raise SystemExit(f"bench_feed_random_edges ({name}): the topology and the torch rule disagree")
        live.append(E)

    # ------------------------------------------------------------------ (e) the build's launches without the host
    reps = 50
    kg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(kg):
        for _ in range(reps):
            feed.build_random_edges()
    kg.replay()
    torch.cuda.synchronize()
    time_calls(kg.replay, args.window)
    build_ms = [v / reps for v in rounds_of({"k": kg.replay}, args.window, args.rounds)["k"]]

    # ------------------------------------------------------------------ the step, four ways
    def make_step(feed_, edge_index, graph=True):
        torch.manual_seed(0)
        model = EncodeTransformDecode(mp, type_column + 9, wy, hidden_size=hidden, num_heads=heads,
                                      compute_dtype=torch.bfloat16)
        sim = Simulator(type_column + 9, 0, wy, 0, type_column, 0, wy, type_column, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        b = Data(x=batch.x.clone(), y=batch.y.clone(), edge_index=edge_index, edge_attr=None)
        return TrainStep(sim, opt, sched, b, graph=graph, feed=feed_)

    fed, fed_off = make_feed(), make_feed()
    fed_off.set_random_edges(False)
    random_step, off_step = make_step(fed, fed.edge_index), make_step(fed_off, fed_off.edge_index)
    static_step = make_step(make_feed(False), mesh_dev)
    host = make_step(make_feed(False), mesh_dev, graph=False)
    pairs = torch.zeros(C, 2, dtype=torch.int32, device=dev)

    def host_loop():
        pairs.random_(0, 2 ** 31 - 1)
        ei, _ = random_topology_torch(pairs, gp, mesh_dev, W, cand_ptr=cand)
        b = host.batch
        host.batch = Data(x=b.x, y=b.y, edge_index=ei.contiguous(), edge_attr=None)
        return host()

    steps = {"random": random_step, "off": off_step, "static": static_step, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    nat.check_errors(dev)
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed_random_edges ({name}): a step's loss is not finite: {losses}")
    if int(fed_off.num_edges_dev.item()) != mesh.shape[1] or int(fed.num_edges_dev.item()) <= mesh.shape[1]:
        raise SystemExit(f"bench_feed_random_edges ({name}): the switch does not do what it says")
    rounds_of(steps, args.window, 1)  # a process's first measurements run slow: one pass dropped
    step_ms = rounds_of(steps, args.window, args.rounds)
    nat.check_errors(dev)
    if random_step.graph is None or off_step.graph is None:
        raise SystemExit(f"bench_feed_random_edges ({name}): a captured step lost its recording")

    best = {k: min(v) for k, v in step_ms.items()}
    return {"N": N, "B": len(gp) - 1, "E_mesh": int(mesh.shape[1]), "candidates": C, "ratio": args.ratio, "max_new": W,
            "E_cap": int(mesh.shape[1]) + N * W, "live_edges_of_two_fills": live,
            "search_tests": int(sum((b - a) * (d - c) for a, b, c, d in zip(gp, gp[1:], cand, cand[1:]))),
            "model": {"processor": "transformer", "mp": mp, "hidden": hidden, "heads": heads, "dtype": "bf16"},
            "step_ms": {k: spread(v) for k, v in step_ms.items()},
            "build_ms_in_graph": spread(build_ms),
            "build_share_of_random_step": round(min(build_ms) / best["random"], 5),
            "random_minus_off_ms": round(best["random"] - best["off"], 5),
            "off_minus_static_ms": round(best["off"] - best["static"], 5),
            "random_minus_static_ms": round(best["random"] - best["static"], 5),
            "host_loop_over_random": round(best["host_loop"] / best["random"], 3),
            "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--max-new", type=int, default=16)
    ap.add_argument("--configs", default="cylinder,aneurysm")
    args = ap.parse_args()
    args.rounds = max(args.rounds, 2)
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed_random_edges: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds}
    for name in args.configs.split(","):
        out[name] = run(name, args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
