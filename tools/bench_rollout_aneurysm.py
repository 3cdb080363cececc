#!/usr/bin/env python
"""Times the validation rollout on aneurysm data (training.rollout.Rollout with an aneurysm= feed) on one HIP
device: the mock aneurysm mesh (tests/golden/aneurysm_mesh.npz, 22,535 nodes, its 1-hop edges; 193 of its nodes lie
on the inflow face), coarse-aneurysm.json's own model (transformer, 10 message-passing blocks, hidden size 64, 4
heads, bf16) and one trajectory of T synthetic frames [velocity (3), wall flag] resident on the device (made as
tools/bench_feed_aneurysm.py makes them), that is T - 2 autoregressive steps from frame 1.

    python tools/bench_rollout_aneurysm.py [--out profiles/rollout_aneurysm_bench.json] [--window 0.5]

    host_loop_prediction — the way it replaces: per step a Data of the clean frame, its predecessor and its successor
                           through external.aneurysm.build_features (which has a unique(): a synchronisation with
                           the host), then Rollout(graph=True, use_previous_data=True, 4, 7).step (the host's copies
                           into the static buffers, one replay, a clone and masked_mse);
    host_loop_frame      — the same with use_previous_data=False;
    resident_prediction  — Rollout(graph=True, feed=..., acceleration="prediction").rollout_resident(batch, 1): one
                           replay per step;
    resident_frame       — the same with acceleration="frame".

The measurement is made twice ("runs"), each in a child process of its own under its own time limit (--run-timeout
seconds; this process never opens the device, and a run that fails or overruns ends the tool without starting
another), so the file shows the run-to-run spread next to the ratios. Inside a run the four variants alternate. The
clock is the host's, around whole trajectories, each ended by a device synchronise (the host's enqueue cost is what
differs, device events alone would hide it); a window repeats trajectories for at least --window seconds after a
warm-up trajectory, and a run's figure is the best of two windows. Before timing, the resident predictions of the
first 3 steps are compared with the host loop's in both modes, to 1e-2·(1 + |ref|) (the model is bf16); the largest
difference is recorded. A run fails without a HIP device (no fallback)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

F, Y_COLUMNS = 4, (0, 3)
TYPE_COLUMN = F + 9
MODES = ("prediction", "frame")


def measure(args):
    """One run, in this process: {variant: ms per step}, the comparison with the host loop, and the sizes."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_aneurysm: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from bench_rollout import window  # tools/bench_rollout.py: the timing loop
    from graphphysics.dataset.resident import ResidentTrajectories
    from graphphysics.external.aneurysm import build_features
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.rollout import Rollout
    from graphphysics.utils import graph_build
    from graphphysics.utils.data import Data

    dev = torch.device("cuda:0")
    T = args.frames
    S = T - 2
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

    def host_batch(f):
        """Frame f as the dataset would hand it to validation_step."""
        d = build_features(Data(x=traj[f].clone(), y=traj[f + 1, :, 0:3].clone(), pos=pos,
                                previous_data=traj[f - 1, :, 0:3]))
        return Data(x=d.x, y=d.y, edge_index=edge_index, edge_attr=None)

    torch.manual_seed(0)
    model = EncodeTransformDecode(args.mp, TYPE_COLUMN + 9, 3, hidden_size=args.hidden, num_heads=4,
                                  compute_dtype=torch.bfloat16)
    sim = Simulator(TYPE_COLUMN + 9, 0, 3, 0, TYPE_COLUMN, 0, 3, TYPE_COLUMN, model, dev)
    for f in (1, S // 2):  # normaliser statistics
        with torch.no_grad():
            sim(host_batch(f))
    sim.eval()
    batch = Data(x=torch.zeros(N, F + 10, device=dev), y=torch.zeros(N, 3, device=dev), edge_index=edge_index,
                 edge_attr=None)
    prev = dict(use_previous_data=True, previous_data_start=F, previous_data_end=F + 3)
    old = {"prediction": Rollout(sim, TYPE_COLUMN, graph=True, **prev), "frame": Rollout(sim, TYPE_COLUMN, graph=True)}
    res = {mode: Rollout(sim, TYPE_COLUMN, graph=True, acceleration=mode,
                         feed=ResidentTrajectories(traj, gp, Y_COLUMNS, TYPE_COLUMN, aneurysm={"pos": pos}))
           for mode in MODES}
    n_inflow = int((res["frame"].feed.node_type == 4).sum())

    def host_loop(mode):
        def run(steps=S):
            old[mode].clear()
            return torch.stack([old[mode].step(host_batch(1 + s))[0] for s in range(steps)])
        return run

    def resident(mode):
        def run():
            res[mode].clear()
            res[mode].rollout_resident(batch, 1, S)
        return run

    diff = {}
    for mode in MODES:
        want, got = host_loop(mode)(3), res[mode].rollout_resident(batch, 1, 3)
        torch.cuda.synchronize()
        diff[mode] = float((want - got).abs().max())
        if not bool(((want - got).abs() <= 1e-2 * (1 + want.abs())).all()):
            raise SystemExit(f"bench_rollout_aneurysm: the resident rollout ({mode}) differs from the host loop by "
                             f"{diff[mode]}")

    fns = {}
    for mode in MODES:
        fns["host_loop_" + mode], fns["resident_" + mode] = host_loop(mode), resident(mode)
    for f in fns.values():  # warm-up: one whole trajectory each (records the graphs)
        f()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(2):
        for k, f in fns.items():
            best[k] = min(best[k], window(f, S, args.window))
    return {"ms_per_step": best, "max_abs_difference_to_host_loop_3_steps": diff,
            "resident_records": {k: r.resident_records for k, r in res.items()},
            "device": torch.cuda.get_device_name(0), "N": N, "E": int(edge_index.shape[1]), "inflow_nodes": n_inflow}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--mp", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--run-timeout", type=float, default=240.0, help="time limit of one run (a child process), seconds")
    ap.add_argument("--child", action="store_true", help="one run in this process; prints its JSON (used by the tool)")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return
    runs = []
    for i in range(2):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--window", str(args.window), "--frames",
               str(args.frames), "--mp", str(args.mp), "--hidden", str(args.hidden)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.run_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_rollout_aneurysm: run {i} exceeded {args.run_timeout} s; no further run is started")
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"bench_rollout_aneurysm: run {i} ended with status {p.returncode}; no further run is "
                             "started")
        runs.append(json.loads(lines[-1][len("RESULT "):]))
    keys = list(runs[0]["ms_per_step"])
    per_run = [r["ms_per_step"] for r in runs]
    ms = {k: min(r[k] for r in per_run) for k in keys}
    spread = {k: abs(per_run[0][k] - per_run[1][k]) / min(per_run[0][k], per_run[1][k]) for k in keys}
    ratio = {m: ms["resident_" + m] / ms["host_loop_" + m] for m in MODES}
    # faster beyond the spread: the slower of the resident's two runs against the faster of the host loop's
    beyond = {m: bool(max(r["resident_" + m] for r in per_run) < min(r["host_loop_" + m] for r in per_run))
              for m in MODES}
    first = runs[0]
    out = {"device": first["device"], "window_s": args.window, "B": 1, "N": first["N"], "E": first["E"], "F": F,
           "batch_row": F + 10, "T": args.frames, "steps_per_trajectory": args.frames - 2,
           "inflow_nodes": first["inflow_nodes"], "mp": args.mp, "hidden": args.hidden, "heads": 4, "dtype": "bf16",
           "clock": "host, whole trajectories ending in a synchronise; each run a process of its own",
           "runs_ms_per_step": [{k: round(v, 5) for k, v in r.items()} for r in per_run],
           "ms_per_step": {k: round(v, 5) for k, v in ms.items()},
           "run_to_run_spread": {k: round(v, 4) for k, v in spread.items()},
           "resident_over_host_loop": {m: round(v, 4) for m, v in ratio.items()},
           "resident_faster_than_host_loop_in_both_runs": beyond,
           "max_abs_difference_to_host_loop_3_steps": [r["max_abs_difference_to_host_loop_3_steps"] for r in runs],
           "resident_records": first["resident_records"]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
