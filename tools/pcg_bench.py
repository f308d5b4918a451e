#!/usr/bin/env python3
"""Times the diagonally preconditioned solves against the plain ones (needs an MI355X).

Workload: the headline C4 graph (Erdos-Renyi, N = 100k, 1M undirected edges, 128 walks, L = 8,
p_halt = 0.1), diffusion modulator, noise 0.01, CG tolerance 1e-2 -- the settings of tools/mll_bench.py and
tools/posterior_bench.py.  Every part runs with preconditioner=None and "jacobi" in the same run.

  1. grf_marginal_log_likelihood(...).backward() (t = 64 Gaussian probes) with all 100k nodes as training
     rows, and with 8192: CG iterations and time per evaluation.
  2. One predict_f chunk: posterior_moments of 256 test nodes on 60k training nodes.
  3. The recurrence alone: cg_solve of 65 columns for a fixed 20 iterations (tolerance 0), plain against
     preconditioned, per iteration; and the Jacobi kernel (grf_gram_jacobi_f64) on its own.

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each
timed call, synchronised; the median and the spread of the repeats are printed.  One JSON line at the end.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = (None, "jacobi")


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


def fmt(r):
    return f"{r['median_ms']:.2f} ms [{r['min_ms']:.2f}, {r['max_ms']:.2f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=128)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--small", type=int, default=8192, help="the second training-set size of part 1")
    ap.add_argument("--n-train", type=int, default=60_000, help="training nodes of the predict_f chunk")
    ap.add_argument("--tolerance", type=float, default=1e-2)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--iterations", type=int, default=20, help="fixed iterations of part 3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pcg_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import get_engine
    from grf_amd.features import StepMatrices, grf_marginal_log_likelihood
    from grf_amd.graphs import er_graph_exact_edges

    eng = get_engine("cuda:0")
    dev = eng.device
    t0 = time.perf_counter()
    A = er_graph_exact_edges(args.n, args.edges, seed=0)
    pre = GraphPreprocessor(A, walks_per_node=args.walks, p_halt=args.p_halt, max_walk_length=args.length,
                            random_walk_seed=42, use_tqdm=False)
    steps = StepMatrices(pre.preprocess_graph(), eng)
    L = steps.L
    f0 = torch.tensor([(-1.0) ** l / (2 ** l * math.factorial(l)) for l in range(L)], dtype=torch.float32, device=dev)
    phi = steps.phi(f0)
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "edges": args.edges, "walks": args.walks, "L": L,
           "p_halt": args.p_halt, "probes": args.probes, "tolerance": args.tolerance, "noise": args.noise,
           "nnz_phi": phi.nnz, "setup_s": time.perf_counter() - t0}
    print(f"setup {out['setup_s']:.1f} s: {L} step matrices, Phi has {phi.nnz} entries", flush=True)
    perm = np.random.default_rng(0).permutation(args.n)

    # 1. the marginal likelihood with its gradients
    for name, n_tr in (("all", args.n), ("small", min(args.small, args.n))):
        tr = torch.from_numpy(np.sort(perm[:n_tr])).to(dev)
        y = torch.randn(n_tr, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
        Z = torch.randn(n_tr, args.probes, device=dev, dtype=torch.float64,
                        generator=torch.Generator(dev).manual_seed(6))
        for mode in MODES:
            last = {}

            def mll_step():
                f = f0.clone().requires_grad_(True)
                s2 = torch.tensor([args.noise], dtype=torch.float64, device=dev, requires_grad=True)
                info = {}
                v = grf_marginal_log_likelihood(f, s2, steps, tr, y, probes=Z, tolerance=args.tolerance, info=info,
                                                preconditioner=mode)
                v.backward()
                last.update(value=float(v.item()), grad_f=f.grad.tolist(), grad_noise=float(s2.grad.item()),
                            iters=info["cg_iterations"])

            r = timed(mll_step, args.warmup, args.repeats)
            r.update(n_train=n_tr, **last)
            out[f"mll_{name}_{mode}"] = r
            print(f"MLL + gradients, n_train = {n_tr}, preconditioner = {mode}: {fmt(r)}, {last['iters']} CG "
                  f"iterations, value/n = {last['value']:.6f}", flush=True)

    # 2. one predict_f chunk
    n_tr = min(args.n_train, args.n)
    r = np.random.default_rng(0)
    tr = torch.from_numpy(np.sort(perm[:n_tr])).to(dev)
    te = torch.from_numpy(r.integers(0, args.n, eng.POSTERIOR_CHUNK)).to(dev)
    y = torch.randn(n_tr, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
    ref = {}
    for mode in MODES:
        last = {}

        def moments():
            info = {}
            last["mean"], last["var"] = eng.posterior_moments(phi, tr, te, y, args.noise, tolerance=args.tolerance,
                                                              info=info, preconditioner=mode)
            last["info"] = info

        rm = timed(moments, args.warmup, args.repeats)
        info = last["info"]
        ref[mode] = (last["mean"], last["var"])
        out[f"predict_f_chunk_{mode}"] = dict(rm, n_train=n_tr, n_test=int(te.numel()),
                                              cg_iterations=info["cg_iterations"],
                                              alpha_iterations=info["alpha_iterations"])
        print(f"predict_f chunk ({te.numel()} nodes, n_train = {n_tr}), preconditioner = {mode}: {fmt(rm)}, CG "
              f"iterations {info['cg_iterations']} (mean solve {info['alpha_iterations']})", flush=True)
    dv = float(((ref[None][1] - ref["jacobi"][1]).abs() / ref[None][1].abs()).max().item())
    out["predict_f_var_max_rel_difference"] = dv
    print(f"variances of the two runs differ by at most {dv:.1e} relative (both stopped at the tolerance)", flush=True)

    # 3. the recurrence alone, a fixed number of iterations
    n_tr = args.n
    tr = torch.from_numpy(np.sort(perm[:n_tr])).to(dev)
    S = 1 + args.probes
    B = torch.randn(n_tr, S, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(8))
    phi_t = eng.csr_transpose(phi, tr)
    rj = timed(lambda: eng.gram_jacobi(phi, tr, args.noise), args.warmup, args.repeats)
    out["gram_jacobi"] = dict(rj, n_sel=n_tr)
    print(f"grf_gram_jacobi_f64, {n_tr} rows: {rj['median_ms']:.3f} ms [{rj['min_ms']:.3f}, {rj['max_ms']:.3f}]",
          flush=True)
    dinv = eng.gram_jacobi(phi, tr, args.noise)
    per = {}
    for mode, pre_vec in ((None, None), ("jacobi", dinv)):
        its = {}

        def solve():
            _, its["n"] = eng.cg_solve(phi, B, args.noise, tr, phi_t, tolerance=0.0, max_iter=args.iterations,
                                       precond=pre_vec)

        rs = timed(solve, args.warmup, args.repeats)
        per[mode] = rs["median_ms"] / max(its["n"], 1)
        out[f"recurrence_{mode}"] = dict(rs, iterations=its["n"], ms_per_iteration=per[mode], n_train=n_tr, S=S)
        print(f"cg_solve, {its['n']} iterations, S = {S}, n_train = {n_tr}, preconditioner = {mode}: {fmt(rs)}, "
              f"{per[mode]:.3f} ms per iteration", flush=True)
    out["recurrence_overhead"] = per["jacobi"] / per[None] - 1.0
    print(f"the preconditioned iteration costs {100 * out['recurrence_overhead']:+.1f} % of a plain one", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
