#!/usr/bin/env python3
"""Times one value-plus-gradient evaluation of the matrix-free marginal likelihood (needs an MI355X).

Workload: the headline C4 graph (Erdos-Renyi, N = 100k, 1M undirected edges, 128 walks, L = 8,
p_halt = 0.1), diffusion modulator, noise 0.01, t = 64 Gaussian probes, CG tolerance 1e-2 -- the
reference's training settings (max_cholesky_size = 0, cg_tolerance = 1e-2, num_trace_samples = 64).

  1. grf_marginal_log_likelihood(...).backward() with all 100k nodes as training rows, and with 8192.
  2. At 8192 the dense route the package offered before: grf_kernel's dense K[train, train] ->
     torch.linalg.cholesky -> backward.
  3. grf_steps_frob_f64 against the unfused form: L spmm calls into an (n_train x S) buffer plus a
     torch multiply-sum.

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each
timed call, synchronised; the median and the spread of the repeats are printed.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=128)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--small", type=int, default=8192, help="training rows of the dense comparison")
    ap.add_argument("--tolerance", type=float, default=1e-2)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense K + Cholesky route")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mll_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import get_engine
    from grf_amd.features import StepMatrices, grf_kernel, grf_marginal_log_likelihood
    from grf_amd.graphs import er_graph_exact_edges

    eng = get_engine("cuda:0")
    dev = eng.device
    t0 = time.perf_counter()
    A = er_graph_exact_edges(args.n, args.edges, seed=0)
    pre = GraphPreprocessor(A, walks_per_node=args.walks, p_halt=args.p_halt, max_walk_length=args.length,
                            random_walk_seed=42, use_tqdm=False)
    steps = StepMatrices(pre.preprocess_graph(), eng)
    torch.cuda.synchronize()
    L = steps.L
    import math
    f0 = torch.tensor([(-1.0) ** l / (2 ** l * math.factorial(l)) for l in range(L)], dtype=torch.float32, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "edges": args.edges, "walks": args.walks, "L": L,
           "p_halt": args.p_halt, "probes": args.probes, "tolerance": args.tolerance, "noise": args.noise,
           "nnz_steps": steps.nnz_sum, "setup_s": time.perf_counter() - t0}
    print(f"setup {out['setup_s']:.1f} s: {L} step matrices, {steps.nnz_sum} entries", flush=True)
    perm = np.random.default_rng(0).permutation(args.n)
    S = 1 + args.probes

    for name, n_tr in (("all", args.n), ("small", min(args.small, args.n))):
        tr = torch.from_numpy(np.sort(perm[:n_tr])).to(dev)
        y = torch.randn(n_tr, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
        Z = torch.randn(n_tr, args.probes, device=dev, dtype=torch.float64,
                        generator=torch.Generator(dev).manual_seed(6))
        last = {}

        def mll_step():
            f = f0.clone().requires_grad_(True)
            s2 = torch.tensor([args.noise], dtype=torch.float64, device=dev, requires_grad=True)
            info = {}
            v = grf_marginal_log_likelihood(f, s2, steps, tr, y, probes=Z, tolerance=args.tolerance, info=info)
            v.backward()
            last.update(value=float(v.item()), grad_f=f.grad.tolist(), grad_noise=float(s2.grad.item()),
                        iters=info["cg_iterations"])

        r = timed(mll_step, args.warmup, args.repeats)
        r.update(n_train=n_tr, **last)
        out[f"mll_{name}"] = r
        print(f"matrix-free MLL + gradients, n_train = {n_tr}: {r['median_ms']:.2f} ms "
              f"[{r['min_ms']:.2f}, {r['max_ms']:.2f}], {last['iters']} CG iterations, "
              f"value/n = {last['value']:.6f}", flush=True)

        # the contraction alone, fused against L spmm calls + a multiply-sum
        g = torch.Generator(dev).manual_seed(7)
        Am, Bm = (torch.randn(n_tr, S, device=dev, dtype=torch.float64, generator=g) for _ in range(2))
        WA, WB = (torch.randn(args.n, S, device=dev, dtype=torch.float64, generator=g) for _ in range(2))
        wt = torch.randn(S, device=dev, dtype=torch.float64, generator=g)
        buf = torch.empty(n_tr, S, device=dev, dtype=torch.float64)
        res = {}

        def fused():
            res["fused"] = eng.steps_frob(steps, tr, Am, WA, Bm, WB, wt)

        def unfused():
            o = torch.empty(L, device=dev, dtype=torch.float64)
            for l, M in enumerate(steps.steps):
                o[l] = (Am * eng.spmm(M, WB, tr, out=buf) * wt).sum() + (Bm * eng.spmm(M, WA, tr, out=buf) * wt).sum()
            res["unfused"] = o

        rf, ru = timed(fused, args.warmup, args.repeats), timed(unfused, args.warmup, args.repeats)
        rel = float(((res["fused"] - res["unfused"]).abs().max() / res["unfused"].abs().max()).item())
        out[f"frob_{name}"] = {"n_train": n_tr, "S": S, "fused": rf, "unfused": ru, "max_rel_difference": rel}
        print(f"steps_frob, n_train = {n_tr}, S = {S}: fused {rf['median_ms']:.2f} ms [{rf['min_ms']:.2f}, "
              f"{rf['max_ms']:.2f}]  unfused {ru['median_ms']:.2f} ms [{ru['min_ms']:.2f}, {ru['max_ms']:.2f}]  "
              f"(results differ by {rel:.1e} relative)", flush=True)

        if name == "small" and not args.no_dense:
            def dense_step():
                f = f0.clone().requires_grad_(True)
                K = grf_kernel(f, steps, tr, tr).to(torch.float64)
                K = K + args.noise * torch.eye(n_tr, device=dev, dtype=torch.float64)
                C = torch.linalg.cholesky(K)
                a = torch.cholesky_solve(y[:, None], C)[:, 0]
                v = (-0.5 * (y @ a) - torch.log(torch.diagonal(C)).sum() - 0.5 * n_tr * math.log(2 * math.pi)) / n_tr
                v.backward()
                last.update(dense_value=float(v.item()))

            try:
                r = timed(dense_step, 1, max(2, args.repeats // 2))
                r.update(n_train=n_tr, value=last["dense_value"])
                print(f"dense K + Cholesky + backward, n_train = {n_tr}: {r['median_ms']:.2f} ms "
                      f"[{r['min_ms']:.2f}, {r['max_ms']:.2f}], value/n = {last['dense_value']:.6f}", flush=True)
            except RuntimeError as e:  # (a torch build without a device Cholesky)
                r = {"n_train": n_tr, "error": str(e).splitlines()[0][:200]}
                print(f"dense K + Cholesky route not available: {r['error']}", flush=True)
            out["dense_small"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
