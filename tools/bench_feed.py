#!/usr/bin/env python
"""Times the resident-trajectory feed (dataset.resident.ResidentTrajectories, libmgn's mgn_feed_batch) on one
HIP device, at the benchmark workload's sizes (Cfg B: 8 CylinderFlow meshes, N = 15,384 nodes, F = 3 columns,
15 message-passing blocks, hidden size 128, bf16) with T = 600 synthetic frames resident.

    python tools/bench_feed.py [--out profiles/feed_bench.json] [--window 0.5]

(a) "fill": one batch's x and y.  kernel = the mgn_feed_batch call alone on given frames and normals;
    fill = ResidentTrajectories.fill (the frame draw, the normal draw and the launch); fill_torch = the same
    rule as torch ops on the same given frames and normals (dataset.resident.fill_torch).
(b) "step": the captured bf16 training step, three ways, each with its own model, optimizer and graph:
    fixed      — TrainStep on one fixed batch (what bench.py measures);
    feed       — TrainStep(feed=...): frames and noise drawn, and the batch written, inside the graph;
    host_loop  — today's way: per step a torch gather of the drawn frames into a new batch, the package's
                 add_noise on that copy, `step.batch = b` (TrainStep copies it into the recorded tensors), replay.
(c) "kernel": 50 launches recorded in one hipGraph and replayed, so that the host's launch cost is not in the
    figure; algorithmic_bytes is what the rule must move, computed from the shapes (frame t read, the y columns
    of frame t + 1 read, the normals read, x and y written) — a label for that count over the measured time, not
    a measurement of memory traffic.

All variants run in this process, alternating, each timed with device events over windows of at least --window
seconds after a warm-up; the figure is the best window's mean per call. Before timing, fill is compared with
fill_torch bit for bit. Fails without a HIP device (no fallback)."""
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

NOISE = {"noise_index_start": 0, "noise_index_end": 2, "noise_scale": 0.02, "node_type_index": 2}
Y_COLUMNS, TYPE_INDEX = (0, 2), 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--mp", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics import _native as nat
    from graphphysics.dataset.preprocessing import add_noise
    from graphphysics.dataset.resident import ResidentTrajectories, fill_torch
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    dev = torch.device("cuda:0")
    mesh = meshes.load_cylinder_mesh()
    b = meshes.cylinder_batch(args.batch, jitter=0.01, mesh=mesh)
    base = {k: torch.from_numpy(b[k]).to(dev) for k in ("x", "y", "edge_index", "edge_attr")}
    n, B, T = b["nodes_per_graph"], args.batch, args.frames
    N = n * B
    # synthetic trajectories: the mesh's 6 velocity frames cycled, each graph and frame scaled a little differently
    vel, nt = torch.from_numpy(mesh["velocity"].astype(np.float32)), torch.from_numpy(mesh["node_type"].astype(np.float32))
    g = torch.Generator().manual_seed(0)
    amp = 1.0 + 0.05 * torch.randn(T, B, 1, 1, generator=g)
    v = (vel[torch.arange(T) % vel.shape[0]][:, None] * amp).reshape(T, N, 2)
    traj = torch.cat([v, nt.repeat(B)[None, :, None].expand(T, N, 1)], dim=2).contiguous().to(dev)
    gp = [i * n for i in range(B + 1)]
    F = traj.shape[2]

    def data():
        return Data(x=base["x"].clone(), y=base["y"].clone(), edge_index=base["edge_index"], edge_attr=base["edge_attr"])

    # ------------------------------------------------------------------ (a) fill against fill_torch
    feed = ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE)
    batch = data()
    feed.fill(batch)
    wx, wy = fill_torch(traj, gp, feed.frame, Y_COLUMNS, TYPE_INDEX, feed.ranges, feed.scales, feed.z)
    torch.cuda.synchronize()
    if not (torch.equal(batch.x, wx) and torch.equal(batch.y, wy)):
        raise SystemExit("bench_feed: fill and fill_torch disagree")

    def kernel():
        nat.feed_batch(traj, feed.graph_ptr, feed.frame, Y_COLUMNS, TYPE_INDEX, feed.ranges, feed.scales, feed.z,
                       batch.x, batch.y)

    fills = {"kernel": kernel, "fill": lambda: feed.fill(batch),
             "fill_torch": lambda: fill_torch(traj, gp, feed.frame, Y_COLUMNS, TYPE_INDEX, feed.ranges, feed.scales,
                                              feed.z)}
    for f in fills.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    best_of(fills, args.window, 1)  # a process's first measurements run slow: one pass dropped
    fill_ms = best_of(fills, args.window, args.rounds)

    # ------------------------------------------------------------------ (c) the kernel without the host
    reps = 50
    kg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(kg):
        for _ in range(reps):
            kernel()
    kg.replay()
    torch.cuda.synchronize()
    kernel_ms = best_of({"k": kg.replay}, args.window, args.rounds)["k"] / reps
    W = feed.z.shape[1]
    wy_ = Y_COLUMNS[1] - Y_COLUMNS[0]
    alg_bytes = 4 * (N * F + N * wy_ + N * W + N * F + N * wy_)

    # ------------------------------------------------------------------ (b) the captured bf16 step, three ways
    def make_step(feed_=None):
        torch.manual_seed(0)
        model = EncodeProcessDecode(args.mp, 11, 3, 2, args.hidden, compute_dtype=torch.bfloat16)
        sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, model, dev)
        opt = FusedAdamW(list(sim.parameters()), lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.95))
        sched = CosineWarmupScheduler(opt, warmup=1000, max_iters=10 ** 6)
        return TrainStep(sim, opt, sched, data(), graph=True, feed=feed_)

    fixed = make_step()
    fed = make_step(ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, noise=NOISE))
    host = make_step()
    rows = torch.arange(N, device=dev)
    node_graph = torch.repeat_interleave(torch.arange(B, device=dev), n)

    def host_loop():
        t = torch.randint(0, T - 1, (B,), device=dev)[node_graph]
        d = Data(x=traj[t, rows], y=traj[t + 1, rows, Y_COLUMNS[0]:Y_COLUMNS[1]], edge_index=base["edge_index"],
                 edge_attr=base["edge_attr"])
        host.batch = add_noise(d, NOISE["noise_index_start"], NOISE["noise_index_end"], NOISE["noise_scale"],
                               NOISE["node_type_index"])
        return host()

    steps = {"fixed": fixed, "feed": fed, "host_loop": host_loop}
    losses = {}
    for k, f in steps.items():
        for _ in range(5):
            losses[k] = f()
    torch.cuda.synchronize()
    losses = {k: float(v.item()) for k, v in losses.items()}
    if not all(np.isfinite(list(losses.values()))):
        raise SystemExit(f"bench_feed: a step's loss is not finite: {losses}")
    best_of(steps, args.window, 1)
    step_ms = best_of(steps, args.window, args.rounds)

    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "B": B, "N": N, "F": F, "T": T, "mp": args.mp, "hidden": args.hidden, "dtype": "bf16",
           "fill_ms": {k: round(v, 5) for k, v in fill_ms.items()},
           "fill_torch_over_fill": round(fill_ms["fill_torch"] / fill_ms["fill"], 2),
           "kernel_ms_in_graph": round(kernel_ms, 6), "algorithmic_bytes": alg_bytes,
           "algorithmic_bytes_per_s": round(alg_bytes / (kernel_ms * 1e-3)),
           "step_ms": {k: round(v, 5) for k, v in step_ms.items()},
           "feed_over_fixed_ms": round(step_ms["feed"] - step_ms["fixed"], 5),
           "host_loop_over_fixed_ms": round(step_ms["host_loop"] - step_ms["fixed"], 5),
           "feed_faster_than_host_loop": bool(step_ms["feed"] < step_ms["host_loop"]),
           "loss_after_warmup": {k: round(v, 6) for k, v in losses.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
