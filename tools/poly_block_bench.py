#!/usr/bin/env python3
"""Times K blocks, diagonals and their modulator gradients from the walk operator (needs an MI355X).

Workload: the headline C4 graph (Erdos-Renyi, N = 100k, 1M undirected edges), L = 8, diffusion modulator
f_l = (-beta)^l / l! with beta = 1, and x = 256 and 8192 training nodes: K(x, x) (GRFEngine.poly_kernel_block),
diag K[x] (poly_kernel_diag) and the backward pass of <g, K(x, x)> (poly_kernel_grad, g random).

Byte model: every step gathers nnz(G) rows of S x 8 bytes, S = min(|x|, 256) columns per
block, B = ceil(|x| / 256) column blocks.  A block costs 2 (n_f - 1) B steps, a diagonal (n_f - 1) B, a backward
pass 2 B (n_f - 1) chain steps and 2 B (n_f - 1) Krylov steps.  The model time is those bytes at the gather rate
section 12 measured for the chain at S = 64 (6.3 TB/s); the achieved rate is the same bytes over the measured time.
There is no pass or fail figure.

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each timed call,
synchronised; median and range of the repeats.  One JSON line at the end.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GATHER_TBS = 6.3   # the chain's gather rate at S = 64


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--x", type=int, nargs="+", default=[256, 8192])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("poly_block_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import get_engine
    from grf_amd.graphs import er_graph_exact_edges

    eng = get_engine("cuda:0")
    dev = eng.device
    A = er_graph_exact_edges(args.n, args.edges, seed=0)
    op = GraphPreprocessor(A, max_walk_length=args.length, use_tqdm=False).walk_operator()
    L = args.length
    f = torch.tensor([(-args.beta) ** l / math.factorial(l) for l in range(L)], dtype=torch.float64, device=dev)
    nnz = op.G.nnz
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "edges": args.edges, "L": L, "beta": args.beta,
           "nnz_G": nnz, "model_gather_TBs": GATHER_TBS, "cases": []}
    perm = np.random.default_rng(0).permutation(args.n)
    print(f"nnz(G) = {nnz}; model rate {GATHER_TBS} TB/s", flush=True)
    print(f"{'x':>6} {'call':>9} {'steps':>6} {'model GB':>9} {'model ms':>9} {'median ms':>10} {'min':>8} {'max':>8} "
          f"{'TB/s':>6}", flush=True)
    for n_x in args.x:
        x = torch.from_numpy(perm[:n_x].copy()).to(dev)
        g = torch.randn(n_x, n_x, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
        S, B = min(n_x, 256), -(-n_x // 256)
        step_bytes = nnz * S * 8
        calls = [("block", 2 * (L - 1) * B, lambda: eng.poly_kernel_block(op, f, x, x)),
                 ("diagonal", (L - 1) * B, lambda: eng.poly_kernel_diag(op, f, x)),
                 ("backward", 4 * (L - 1) * B, lambda: eng.poly_kernel_grad(op, f, g, x, x))]
        for name, steps, fn in calls:
            t = timed(fn, args.warmup, args.repeats)
            model_bytes = steps * step_bytes
            row = {"x": n_x, "call": name, "steps": steps, "model_bytes": model_bytes,
                   "model_ms": model_bytes / (GATHER_TBS * 1e12) * 1e3,
                   "achieved_TBs": model_bytes / (t["median_ms"] * 1e-3) / 1e12, **t}
            out["cases"].append(row)
            print(f"{n_x:>6} {name:>9} {steps:>6} {model_bytes / 1e9:>9.2f} {row['model_ms']:>9.2f} "
                  f"{t['median_ms']:>10.2f} {t['min_ms']:>8.2f} {t['max_ms']:>8.2f} {row['achieved_TBs']:>6.2f}",
                  flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
