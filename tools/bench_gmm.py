#!/usr/bin/env python
"""Times the mixture-density head's loss and sampler on libmgn (mgn_gmm_nll_diag / _backward,
mgn_gmm_sample_diag) against their torch compositions (utils.loss.masked_gmm_nll_torch,
models.simulator.sample_gmm_diagonal_torch: what runs where the kernels do not apply), on one HIP device.

    python tools/bench_gmm.py [--out profiles/gmm_bench.json] [--window 0.5]

Sizes: N in {2k, 16k, 128k} nodes, K = 3 components, d = 3 outputs (21 parameters per node), node types a
strided column of a wider x, masks NORMAL and OUTFLOW. "nll_fwd_bwd": masked_gmm_nll and its backward to
the gradient of the network output; "sample": one draw per node from given noise (u, z), so both
implementations do the same work. Both implementations run in this process, alternating, each timed with
device events over windows of at least --window seconds after a warm-up; the figure is the best window's
mean per call and includes the launches' host cost (at 2k nodes that is all there is to measure). The first
size is run once more beforehand and that pass dropped (a process's first measurements run slow).
"algorithmic_bytes" is what the algorithm must move, computed from the shapes (not measured): loss —
parameters, targets and node types read by the forward and again by the backward, the gradient written;
sampler — parameters, u, z read, the sample written. "algorithmic_bytes_per_s" is that count over the
kernels' time: a label for this count, not a measurement of memory traffic. Before timing, the two
implementations' results are compared on the benchmark's inputs. Fails without a HIP device (no fallback)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "graph-physics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, D = 3, 3
MASKS = [0, 5]
TEMPERATURE = 1.0


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 16384, 131072])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gmm: needs a HIP device (there is no CPU fallback)")
    import __graft_entry__ as ge

    ge.build()
    from graphphysics.models.simulator import sample_gmm_diagonal, sample_gmm_diagonal_torch
    from graphphysics.utils.loss import masked_gmm_nll, masked_gmm_nll_torch

    dev = torch.device("cuda:0")
    P = K * (2 * D + 1)
    rows = []
    # the first size is measured twice and its first pass dropped: whatever a process measures first runs
    # slower for a few seconds (both implementations, whichever size comes first)
    for i, N in enumerate(args.sizes[:1] + args.sizes):
        g = torch.Generator(device="cpu").manual_seed(N)
        net = torch.randn(N, P, generator=g).to(dev).requires_grad_(True)
        target = torch.randn(N, D, generator=g).to(dev)
        x = torch.zeros(N, 8, device=dev)
        x[:, 2] = torch.randint(0, 7, (N,), generator=g).float().to(dev)
        nt = x[:, 2]
        u, z = torch.rand(N, generator=g).to(dev), torch.randn(N, D, generator=g).to(dev)
        one = torch.ones((), device=dev)

        def nll(f):
            net.grad = None
            f(target, net, nt, MASKS, D, K, TEMPERATURE).backward(one)
            return net.grad

        def sample(f):
            with torch.no_grad():
                return f(net, D, K, TEMPERATURE, u, z)

        modes = {"nll_fwd_bwd": (nll, {"kernel": masked_gmm_nll, "torch": masked_gmm_nll_torch}),
                 "sample": (sample, {"kernel": sample_gmm_diagonal, "torch": sample_gmm_diagonal_torch})}
        res, agree = {}, {}
        for mode, (run, impls) in modes.items():
            a, b = run(impls["kernel"]).clone(), run(impls["torch"]).clone()
            agree[mode] = float((a - b).abs().max() / b.abs().max())
            for f in impls.values():  # warm-up: allocator, code objects
                for _ in range(5):
                    run(f)
            torch.cuda.synchronize()
            best = {k_: float("inf") for k_ in impls}
            for _ in range(args.rounds):  # alternate the two implementations
                for k_, f in impls.items():
                    best[k_] = min(best[k_], time_calls(lambda: run(f), args.window))
            for k_ in impls:
                res[f"{mode}_{k_}_ms"] = round(best[k_], 5)
        nll_bytes = 2 * (N * P + N * D + N) * 4 + N * P * 4
        smp_bytes = (N * P + N + N * D) * 4 + N * D * 4
        row = {"N": N, "K": K, "d": D, **res,
               "nll_fwd_bwd_speedup": round(res["nll_fwd_bwd_torch_ms"] / res["nll_fwd_bwd_kernel_ms"], 2),
               "sample_speedup": round(res["sample_torch_ms"] / res["sample_kernel_ms"], 2),
               "nll_fwd_bwd_algorithmic_bytes": nll_bytes, "sample_algorithmic_bytes": smp_bytes,
               "nll_fwd_bwd_algorithmic_bytes_per_s": round(nll_bytes / (res["nll_fwd_bwd_kernel_ms"] * 1e-3)),
               "sample_algorithmic_bytes_per_s": round(smp_bytes / (res["sample_kernel_ms"] * 1e-3)),
               "max_rel_difference_kernel_vs_torch": {k_: float(f"{v:.3g}") for k_, v in agree.items()}}
        if i == 0:
            continue
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds,
           "kernel_faster_everywhere": all(r["nll_fwd_bwd_speedup"] > 1 and r["sample_speedup"] > 1 for r in rows),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}))


if __name__ == "__main__":
    main()
