#!/usr/bin/env python
"""Times libmgn's fused gated-MLP kernels (dense="libmgn") against the torch composition (dense="torch",
x + gated_mlp(norm2(x)) as Transformer.forward runs it) on one HIP device.

    python tools/bench_gated_mlp.py [--out profiles/gated_mlp_bench.json] [--window 0.5]

(a) op level: forward (no_grad) and forward+backward of the dense half of one block, N = 15,384 and 22,535
    rows, hidden 64 and 128, fp32 and bf16.
(b) step level: a captured TrainStep of EncodeTransformDecode at the plate config's sizes (MP = 10, h = 64,
    H = 4) and the panels config's (MP = 15, h = 128, H = 4) on meshes.cylinder_batch(8), dense="torch"
    against dense="libmgn", milliseconds per replayed step.
Both implementations run in this process, alternating, each timed with device events over a window of at
least --window seconds after a warm-up, everything twice; a figure is the mean of the two windows and
"spread" the larger of the two variants' run-to-run differences, relative. A difference between the variants
counts only where it exceeds the spread ("verdict"). The op-level figures time the whole autograd call on
either side (Python, allocator, the backward's plumbing, the launches). "*_kernels_ms" times the library
calls alone — mgn_gated_mlp_forward, or _forward with saves followed by _backward, on preallocated buffers —
and "algorithmic_flop_per_s" is a label over THAT time, not a measurement: 18 h² N (forward) or
18 + 36 + 12 h² N (forward + backward with the recomputed u, v). Fails without a HIP device (no fallback)."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def compare(impls, window, rounds=2):
    """{name: [ms per window]} with the variants alternating, then (means, spread)."""
    for f in impls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    runs = {k: [] for k in impls}
    for _ in range(rounds):
        for k, f in impls.items():
            runs[k].append(time_calls(f, window))
    mean = {k: sum(v) / len(v) for k, v in runs.items()}
    spread = max((max(v) - min(v)) / min(v) for v in runs.values())
    return mean, spread, runs


def verdict(torch_ms, kernel_ms, spread):
    r = torch_ms / kernel_ms
    if abs(r - 1) <= spread:
        return "within spread"
    return "libmgn faster" if r > 1 else "libmgn slower"


def library_calls(m, x, gy, dt):
    """(forward, forward + backward) closures over mgn_gated_mlp_forward / _backward on preallocated buffers."""
    from graphphysics import _native as nat

    N, h = x.shape
    g = m.gated_mlp
    ps = [p.detach() for p in (g[1].linear1.weight, g[1].linear1.bias, g[1].linear2.weight, g[1].linear2.bias,
                               g[2].weight, g[2].bias, m.norm2.scale, g[0].scale)]
    desc = nat.gated_mlp_desc(h, nat.mgn_dtype(dt), *ps)
    L, d, dev = nat.lib(), ctypes.byref(desc), x.device
    xs = x.detach()
    y, dx = torch.empty_like(xs), torch.empty_like(xs)
    saved = torch.empty(int(L.mgn_gated_mlp_saved_bytes(d, N)), dtype=torch.uint8, device=dev)
    wsb = int(L.mgn_gated_mlp_backward_workspace_bytes(d, N))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    G = torch.empty(sum(p.numel() for p in ps), device=dev)
    st = nat.stream_ptr(dev)

    def fwd():
        nat.check(L.mgn_gated_mlp_forward(d, nat.ptr(xs), h, N, nat.ptr(y), h, None, st))

    def fwd_bwd():
        nat.check(L.mgn_gated_mlp_forward(d, nat.ptr(xs), h, N, nat.ptr(y), h, nat.ptr(saved), st))
        nat.check(L.mgn_gated_mlp_backward(d, nat.ptr(xs), h, N, nat.ptr(saved), nat.ptr(gy), h, nat.ptr(dx),
                                           nat.ptr(G), nat.ptr(ws), wsb, st))

    fwd.keep = fwd_bwd.keep = (desc, ps, xs, y, dx, saved, ws, G)  # the buffers live as long as the closures
    return fwd, fwd_bwd


def op_rows(dev, window):
    from graphphysics.models.layers import Transformer

    for N in (15384, 22535):
        for h in (64, 128):
            for dt in (torch.float32, torch.bfloat16):
                torch.manual_seed(0)
                m = Transformer(h, h, 4, compute_dtype=dt, dense="libmgn").to(dev)
                x = torch.randn(N, h, device=dev).requires_grad_(True)
                gy = torch.randn(N, h, device=dev)

                def composed():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                        return x + m.gated_mlp(m.norm2(x))

                impls = {"torch": composed, "libmgn": lambda: m._dense_half(x)}

                def fwd(f):
                    with torch.no_grad():
                        f()

                def fwd_bwd(f):
                    x.grad = None
                    m.zero_grad(set_to_none=True)
                    f().backward(gy)

                row = {"N": N, "hidden": h, "dtype": str(dt).replace("torch.", "")}
                lib_calls = dict(zip(("fwd", "fwd_bwd"), library_calls(m, x, gy, dt)))
                for mode, run, flop in (("fwd", fwd, 18), ("fwd_bwd", fwd_bwd, 66)):
                    mean, spread, runs = compare({k: (lambda f=f: run(f)) for k, f in impls.items()}, window)
                    kmean, kspread, kruns = compare({"kernels": lib_calls[mode]}, window)
                    row.update({f"{mode}_torch_ms": round(mean["torch"], 4), f"{mode}_libmgn_ms": round(mean["libmgn"], 4),
                                f"{mode}_windows_ms": {k: [round(t, 4) for t in v] for k, v in runs.items()},
                                f"{mode}_spread": round(spread, 4),
                                f"{mode}_speedup": round(mean["torch"] / mean["libmgn"], 3),
                                f"{mode}_verdict": verdict(mean["torch"], mean["libmgn"], spread),
                                f"{mode}_kernels_ms": round(kmean["kernels"], 4),
                                f"{mode}_kernels_windows_ms": [round(t, 4) for t in kruns["kernels"]],
                                f"{mode}_algorithmic_flop_per_s": round(flop * h * h * N / (kmean["kernels"] * 1e-3))})
                yield row


def step_rows(dev, window):
    from graphphysics.models.processors import EncodeTransformDecode
    from graphphysics.models.simulator import Simulator
    from graphphysics.training.optim import FusedAdamW
    from graphphysics.training.step import TrainStep
    from graphphysics.utils import meshes
    from graphphysics.utils.data import Data
    from graphphysics.utils.scheduler import CosineWarmupScheduler

    b = meshes.cylinder_batch(8, jitter=0.01)
    for name, mp, h in (("plate sizes", 10, 64), ("panels sizes", 15, 128)):
        for dt in (torch.float32, torch.bfloat16):
            steps = {}
            for dense in ("torch", "libmgn"):
                data = Data(edge_attr=None, **{k: torch.from_numpy(b[k]).to(dev) for k in ("x", "y", "edge_index")})
                torch.manual_seed(0)
                m = EncodeTransformDecode(mp, 11, 2, hidden_size=h, num_heads=4, compute_dtype=dt, dense=dense)
                sim = Simulator(11, 0, 2, 0, 2, 0, 2, 2, m, dev)
                opt = FusedAdamW(sim.parameters(), lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.95))
                sch = CosineWarmupScheduler(opt, warmup=5, max_iters=100000)
                steps[dense] = TrainStep(sim, opt, sch, data, graph=True)
            mean, spread, runs = compare(steps, window)
            torch.cuda.synchronize()
            yield {"config": name, "MP": mp, "hidden": h, "heads": 4, "N": int(b["x"].shape[0]),
                   "dtype": str(dt).replace("torch.", ""), "step_torch_ms": round(mean["torch"], 4),
                   "step_libmgn_ms": round(mean["libmgn"], 4),
                   "windows_ms": {k: [round(t, 4) for t in v] for k, v in runs.items()}, "spread": round(spread, 4),
                   "speedup": round(mean["torch"] / mean["libmgn"], 3),
                   "share_removed": round(1 - mean["libmgn"] / mean["torch"], 4),
                   "verdict": verdict(mean["torch"], mean["libmgn"], spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--skip-steps", action="store_true", help="table (a) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_mlp: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "op": [], "step": []}
    for row in op_rows(dev, args.window):
        print(json.dumps(row), flush=True)
        out["op"].append(row)
    if not args.skip_steps:
        for row in step_rows(dev, args.window):
            print(json.dumps(row), flush=True)
            out["step"].append(row)
    out["spread_max"] = max([r[f"{m}_spread"] for r in out["op"] for m in ("fwd", "fwd_bwd")] +
                            [r["spread"] for r in out["step"]])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("op", "step")}))


if __name__ == "__main__":
    main()
