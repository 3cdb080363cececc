#!/usr/bin/env python
"""Times the validation rollout (training.rollout.Rollout) on one HIP device: a bf16 EncodeProcessDecode (15
message-passing blocks, hidden size 128) on the cylinder mesh at B = 1 (N = 1,923, the size the reference
validates at) and B = 8, over T = 600 synthetic frames resident on the device (made as tools/bench_feed.py makes
them), that is 599 autoregressive steps per trajectory.

    python tools/bench_rollout.py [--out profiles/rollout_bench.json] [--window 0.5]

    existing        — Rollout(graph=True).rollout(frames), the per-frame batches prebuilt on the device (x a view
                      of the resident frame, y a contiguous copy made beforehand): per step the host's copies
                      into the static buffers, one replay, a clone and masked_mse;
    resident        — Rollout(graph=True, feed=...).rollout_resident(batch): one replay per step;
    resident_nokeep — the same with keep_predictions=False.

The three run in this process, alternating. The clock is the host's, around whole trajectories, each ended by a
device synchronise (the host's enqueue cost is what differs, device events alone would hide it); a window repeats
trajectories for at least --window seconds after a warm-up trajectory, the figure is the best of two windows, and
everything is measured twice ("runs") so the file shows the run-to-run spread next to the ratios. Before timing,
the resident predictions of the first 5 steps are compared with the existing path's bit for bit. Fails without a
HIP device (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def window(fn, steps, seconds):
    """Milliseconds per step over one window of whole trajectories lasting at least `seconds` (host clock)."""
    n, total = 0, 0.0
    while total < seconds:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        n += 1
    return total * 1e3 / (n * steps)


def measure(B, args, dev):
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    mesh = meshes.load_cylinder_mesh()
    b = meshes.cylinder_batch(B, jitter=0.01, mesh=mesh)
    ei, ea = torch.from_numpy(b["edge_index"]).to(dev), torch.from_numpy(b["edge_attr"]).to(dev)
    n, T = b["nodes_per_graph"], args.frames
    N, S = n * B, args.frames - 1
    vel = torch.from_numpy(mesh["velocity"].astype(np.float32))
    nt = torch.from_numpy(mesh["node_type"].astype(np.float32))
    g = torch.Generator().manual_seed(0)
    amp = 1.0 + 0.05 * torch.randn(T, B, 1, 1, generator=g)
    v = (vel[torch.arange(T) % vel.shape[0]][:, None] * amp).reshape(T, N, 2)
    traj = torch.cat([v, nt.repeat(B)[None, :, None].expand(T, N, 1)], dim=2).contiguous().to(dev)
    frames = [Data(x=traj[t], y=traj[t + 1, :, 0:2].contiguous(), edge_index=ei, edge_attr=ea) for t in range(S)]
    torch.manual_seed(0)
    sim = Simulator(11, 3, 2, 0, 2, 0, 2, 2, EncodeProcessDecode(args.mp, 11, 3, 2, args.hidden,
                                                                 compute_dtype=torch.bfloat16), dev)
    for f in frames[:2]:  # normaliser statistics
        with torch.no_grad():
            sim(f)
    sim.eval()
    gp = [i * n for i in range(B + 1)]
    batch = Data(x=traj[0].clone(), y=traj[1, :, 0:2].clone(), edge_index=ei, edge_attr=ea)
    old = Rollout(sim, 2, graph=True)
    new = Rollout(sim, 2, graph=True, feed=ResidentTrajectories(traj, gp, (0, 2), 2))
    lean = Rollout(sim, 2, graph=True, feed=ResidentTrajectories(traj, gp, (0, 2), 2))

    want, got = old.rollout(frames[:5]), new.rollout_resident(batch, 0, 5)
    torch.cuda.synchronize()
    if not torch.equal(want, got) or not torch.equal(torch.stack(old.losses), torch.stack(new.losses)):
        raise SystemExit(f"bench_rollout: the resident rollout differs from the existing one at B = {B}")

    def run_old():
        old.clear()
        old.rollout(frames)

    def run_new():
        new.clear()
        new.rollout_resident(batch, 0, S)

    def run_lean():
        lean.clear()
        lean.rollout_resident(batch, 0, S, keep_predictions=False)

    fns = {"existing": run_old, "resident": run_new, "resident_nokeep": run_lean}
    for f in fns.values():  # warm-up: one whole trajectory each (records the graphs)
        f()
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        best = {k: float("inf") for k in fns}
        for _ in range(2):
            for k, f in fns.items():
                best[k] = min(best[k], window(f, S, args.window))
        runs.append(best)
    ms = {k: min(r[k] for r in runs) for k in fns}
    spread = {k: abs(runs[0][k] - runs[1][k]) / min(runs[0][k], runs[1][k]) for k in fns}
    return {"B": B, "N": N, "steps_per_trajectory": S,
            "runs_ms_per_step": [{k: round(v, 5) for k, v in r.items()} for r in runs],
            "ms_per_step": {k: round(v, 5) for k, v in ms.items()},
            "run_to_run_spread": {k: round(v, 4) for k, v in spread.items()},
            "ratio_to_existing": {k: round(ms[k] / ms["existing"], 4) for k in fns},
            "resident_records": new.resident_records}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--mp", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "T": args.frames, "mp": args.mp,
           "hidden": args.hidden, "dtype": "bf16", "clock": "host, whole trajectories ending in a synchronise",
           "sizes": [measure(B, args, dev) for B in args.batches]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
