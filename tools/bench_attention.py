#!/usr/bin/env python
"""Times libmgn's graph-attention kernels against the torch composition (sparse_attention_torch) — the
only thing a user without DGL could run instead — forward and forward+backward, on one HIP device.

    python tools/bench_attention.py [--out profiles/attention_bench.json] [--window 0.5]

Sizes: meshes.cylinder_batch(8) (N = 15,384, E = 88,560) and the aneurysm 2-hop mesh of
tests/test_configs_gpu.py (about 1.4M edges); (hidden, heads) = (64, 4) and (128, 4); fp32 and bf16.
Both implementations run in this process, alternating, each timed with device events over windows of
at least --window seconds after a warm-up; the figure is the best window's mean per call. "bytes" is
what the algorithm must move, computed from the shapes (not measured): the q, k, v, y rows once plus the
gathered k and v rows for the forward, and for the backward q, y, dy, dq, dk, dv once, the gathered k, v
(pass 1) and q, dy (pass 2) rows and the 2H-float edge workspace written and read once;
"algorithmic_bytes_per_s" is that count over the kernels' time — a label for this count, not a
measurement of memory traffic. Fails without a HIP device (no fallback)."""
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


def graphs(dev):
    from graphphysics.utils import graph_build as G
    from graphphysics.utils import meshes

    b = meshes.cylinder_batch(8)
    yield "cylinder_batch(8)", b["x"].shape[0], torch.from_numpy(b["edge_index"]).to(dev)
    z = np.load(os.path.join(ROOT, "tests", "golden", "aneurysm_mesh.npz"))
    tet = torch.from_numpy(z["tetra"].astype(np.int64)).t().contiguous().to(dev)
    n = z["pos"].shape[0]
    yield "aneurysm 2-hop", n, G.k_hop_edge_index(G.face_to_edge(tet, n), 2, n).contiguous()


def algorithmic_bytes(N, E, h, H, size):
    row = h * size
    fwd = 4 * N * row + 2 * E * row + N * H * 4
    bwd = 6 * N * row + 4 * E * row + 2 * E * 2 * H * 4 + N * H * 4
    return fwd, fwd + bwd


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics.models.layers import graph_attention, sparse_attention_torch

    dev = torch.device("cuda:0")
    rows = []
    for name, N, ei in graphs(dev):
        E = ei.shape[1]
        for h, H in ((64, 4), (128, 4)):
            for dt in (torch.float32, torch.bfloat16):
                g = torch.Generator(device="cpu").manual_seed(0)
                qkv = torch.randn(N, 3 * h, generator=g).to(dev, dt).requires_grad_(True)
                gy = torch.randn(N, h, generator=g).to(dev, dt)
                q, k, v = qkv[:, :h], qkv[:, h:2 * h], qkv[:, 2 * h:]
                impls = {"kernel": lambda: graph_attention(q, k, v, ei, H),
                         "torch": lambda: sparse_attention_torch(q, k, v, ei, H)}

                def fwd(f):
                    with torch.no_grad():
                        f()

                def fwd_bwd(f):
                    qkv.grad = None
                    f().backward(gy)

                res = {}
                for mode, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                    for f in impls.values():  # warm-up: topology cache, allocator
                        for _ in range(3):
                            run(f)
                    torch.cuda.synchronize()
                    best = {k_: float("inf") for k_ in impls}
                    for _ in range(args.rounds):  # alternate the two implementations
                        for k_, f in impls.items():
                            best[k_] = min(best[k_], time_calls(lambda: run(f), args.window))
                    for k_ in impls:
                        res[f"{mode}_{k_}_ms"] = round(best[k_], 4)
                bf, bfb = algorithmic_bytes(N, E, h, H, qkv.element_size())
                row = {"graph": name, "N": N, "E": E, "hidden": h, "heads": H, "dtype": str(dt).replace("torch.", ""),
                       **res, "fwd_speedup": round(res["fwd_torch_ms"] / res["fwd_kernel_ms"], 2),
                       "fwd_bwd_speedup": round(res["fwd_bwd_torch_ms"] / res["fwd_bwd_kernel_ms"], 2),
                       "fwd_algorithmic_bytes": bf, "fwd_bwd_algorithmic_bytes": bfb,
                       "fwd_algorithmic_bytes_per_s": round(bf / (res["fwd_kernel_ms"] * 1e-3)),
                       "fwd_bwd_algorithmic_bytes_per_s": round(bfb / (res["fwd_bwd_kernel_ms"] * 1e-3))}
                print(json.dumps(row), flush=True)
                rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "kernel_faster_everywhere": all(r["fwd_speedup"] > 1 and r["fwd_bwd_speedup"] > 1 for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}))


if __name__ == "__main__":
    main()
