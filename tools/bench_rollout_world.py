#!/usr/bin/env python
"""Times the validation rollout on Lagrangian data (training.rollout.Rollout with a world_pos= feed) on one HIP
device, at Cfg C's size (DeformingPlate: meshes.plate_sample defaults, 8 graphs of 1,350 nodes, frame rows [world
position, node type], the static edges of meshes.plate_graph, 15 message-passing blocks, hidden size 128, bf16) over
one trajectory of T synthetic frames resident on the device (made as tools/bench_feed_world.py makes them), that is
T - 1 autoregressive steps.

    python tools/bench_rollout_world.py [--out profiles/rollout_world_bench.json] [--window 0.5]

    host_loop           — the way it replaces: per step and per graph a Data of the clean frame through the
                          package's add_obstacles_next_pos and add_world_pos_features, the graphs concatenated, then
                          Rollout(graph=True).step (the host's copies into the static buffers, one replay, a clone
                          and masked_mse);
    resident_frame      — Rollout(graph=True, feed=..., world_edges="frame").rollout_resident(batch): one replay
                          per step, the edge features from the clean frame (what host_loop computes);
    resident_prediction — the same with world_edges="prediction": the edge features from the fed-back positions.

The three run in this process, alternating. The clock is the host's, around whole trajectories, each ended by a
device synchronise (the host's enqueue cost is what differs, device events alone would hide it); a window repeats
trajectories for at least --window seconds after a warm-up trajectory, the figure is the best of two windows, and
everything is measured twice ("runs") so the file shows the run-to-run spread next to the ratios. Before timing,
the resident "frame" predictions of the first 3 steps are compared with the host loop's: not bit for bit — the host
loop's obstacle mean is torch.mean on the device, another summation order, and the model is bf16 — but to
1e-2·(1 + |ref|); the largest difference is recorded. Fails without a HIP device (no fallback)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_rollout import window  # noqa: E402  (tools/bench_rollout.py: the timing loop)

Y_COLUMNS, TYPE_INDEX, EA_START = (0, 3), 3, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--mp", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_world: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics.dataset.preprocessing import add_obstacles_next_pos, add_world_pos_features
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.models.processors import EncodeProcessDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data

    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames
    S = T - 1
    s = meshes.plate_sample(seed=0)
    g, _ = meshes.plate_graph(dev, seed=0)
    x0, y0 = torch.from_numpy(s["x"]), torch.from_numpy(s["y"])
    n = x0.shape[0]
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

    def host_batch(f):
        """Frame f of every graph as the dataset would hand it to validation_step."""
        xs, ys, eas = [], [], []
        for i in range(B):
            rows = slice(gp[i], gp[i + 1])
            d = Data(x=traj[f, rows].clone(), y=traj[f + 1, rows, 0:3].clone(), edge_index=ei1, edge_attr=mesh_ea)
            d = add_obstacles_next_pos(d, 0, 3, TYPE_INDEX + 3)
            d = add_world_pos_features(d, 0, 3)
            xs.append(d.x)
            ys.append(d.y)
            eas.append(d.edge_attr)
        return Data(x=torch.cat(xs), y=torch.cat(ys), edge_index=edge_index, edge_attr=torch.cat(eas))

    torch.manual_seed(0)
    sim = Simulator(15, 8, 3, 0, 6, 0, 3, 6, EncodeProcessDecode(args.mp, 15, 8, 3, args.hidden,
                                                                 compute_dtype=torch.bfloat16), dev)
    for f in (0, S // 2):  # normaliser statistics
        with torch.no_grad():
            sim(host_batch(f))
    sim.eval()
    batch = Data(x=torch.zeros(N, F + 3, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=edge_index,
                 edge_attr=base_ea.clone())
    old = Rollout(sim, TYPE_INDEX + 3, graph=True)
    res = {mode: Rollout(sim, TYPE_INDEX + 3, graph=True, world_edges=mode,
                         feed=ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_INDEX, world_pos=wp))
           for mode in ("frame", "prediction")}

    def run_old(steps=S):
        old.clear()
        return torch.stack([old.step(host_batch(f))[0] for f in range(steps)])

    want, got = run_old(3), res["frame"].rollout_resident(batch, 0, 3)
    torch.cuda.synchronize()
    diff = float((want - got).abs().max())
    if not bool(((want - got).abs() <= 1e-2 * (1 + want.abs())).all()):
        raise SystemExit(f"bench_rollout_world: the resident rollout differs from the host loop by {diff}")

    def resident(mode):
        def run():
            res[mode].clear()
            res[mode].rollout_resident(batch, 0, S)
        return run

    fns = {"host_loop": run_old, "resident_frame": resident("frame"), "resident_prediction": resident("prediction")}
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
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "B": B, "N": N,
           "E": int(edge_index.shape[1]), "F": F, "T": T, "steps_per_trajectory": S, "mp": args.mp,
           "hidden": args.hidden, "dtype": "bf16", "clock": "host, whole trajectories ending in a synchronise",
           "runs_ms_per_step": [{k: round(v, 5) for k, v in r.items()} for r in runs],
           "ms_per_step": {k: round(v, 5) for k, v in ms.items()},
           "run_to_run_spread": {k: round(v, 4) for k, v in spread.items()},
           "ratio_to_host_loop": {k: round(ms[k] / ms["host_loop"], 4) for k in fns},
           "max_abs_difference_to_host_loop_3_steps": diff,
           "resident_records": {k: r.resident_records for k, r in res.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
