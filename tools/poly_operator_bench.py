#!/usr/bin/env python3
"""Times the exact kernel as a matrix-free operator (WalkPolynomial) against the Phi-based solve (needs an MI355X).

Workload: the headline C4 graph (Erdos-Renyi, N = 100k, 1M undirected edges), 60k training rows, S = 65 columns
(y and 64 probes; 64 samples for predict), L = 8, diffusion modulator f_l = (-beta)^l / l! with beta = 1,
noise 0.01.  For one marginal-likelihood evaluation (value and gradients) and one predict it reports the CG
iteration count, the time of the CG solve alone per iteration, and the total time -- on the operator
(Phi = sum_l f_l G^l, never formed) and, in the same run, on the walks' step matrices (Phi = sum_l f_l M_l,
128 walks, p_halt = 0.1).  The two solve different matrices (the exact kernel against its estimate), so their
iteration counts need not agree.  There is no pass or fail figure.

Timing discipline of bench.py: a warm-up call of the same shapes first, then device events around each timed
call, synchronised; the median of the repeats is printed.  One JSON line at the end.
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
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--train", type=int, default=60_000)
    ap.add_argument("--test", type=int, default=10_000)
    ap.add_argument("--walks", type=int, default=128)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--tolerance", type=float, default=1e-2)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-walks", action="store_true", help="skip the comparison base on the walks' step matrices")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("poly_operator_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import get_engine
    from grf_amd.features import StepMatrices
    from grf_amd.graphs import er_graph_exact_edges

    eng = get_engine("cuda:0")
    dev = eng.device
    t0 = time.perf_counter()
    A = er_graph_exact_edges(args.n, args.edges, seed=0)
    pre = GraphPreprocessor(A, walks_per_node=args.walks, p_halt=args.p_halt, max_walk_length=args.length,
                            random_walk_seed=42, use_tqdm=False)
    op = pre.walk_operator()
    L = args.length
    f = torch.tensor([(-args.beta) ** l / math.factorial(l) for l in range(L)], dtype=torch.float64, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "edges": args.edges, "n_train": args.train,
           "n_test": args.test, "L": L, "beta": args.beta, "noise": args.noise, "tolerance": args.tolerance,
           "probes": args.probes, "nnz_G": op.G.nnz}
    paths = [("operator", op)]
    if not args.no_walks:
        steps = StepMatrices(pre.preprocess_graph(), eng)
        out["nnz_steps"] = steps.nnz_sum
        paths.append(("walks", steps))
    torch.cuda.synchronize()
    out["setup_s"] = time.perf_counter() - t0
    print(f"setup {out['setup_s']:.1f} s: nnz(G) = {op.G.nnz}", flush=True)

    perm = np.random.default_rng(0).permutation(args.n)
    tr = torch.from_numpy(perm[:args.train].copy()).to(dev)
    te = torch.from_numpy(perm[args.train:args.train + args.test].copy()).to(dev)
    g = torch.Generator(dev).manual_seed(5)
    y = torch.randn(args.train, device=dev, dtype=torch.float64, generator=g)
    Z = torch.randn(args.train, args.probes, device=dev, dtype=torch.float64, generator=g)
    rhs = torch.cat([y[:, None], Z], dim=1).contiguous()
    e1 = torch.randn(args.probes, args.n, device=dev, dtype=torch.float64, generator=g)
    e2 = math.sqrt(args.noise) * torch.randn(args.probes, args.train, device=dev, dtype=torch.float64, generator=g)
    Bp = torch.randn(args.train, args.probes, device=dev, dtype=torch.float64, generator=g)

    for name, obj in paths:
        is_op = name == "operator"
        if not is_op:
            phi = obj.phi(f)
            phi_t = eng.csr_transpose(phi, tr)
        last = {}

        def solve(B):
            if is_op:
                last["iters"] = eng.cg_solve_poly(obj, f, B, args.noise, tr, args.tolerance, args.max_iter)[1]
            else:
                last["iters"] = eng.cg_solve(phi, B, args.noise, tr, phi_t, args.tolerance, args.max_iter)[1]

        def mll():
            last["mll"] = eng.marginal_log_likelihood(obj, f, tr, y, args.noise, Z, args.tolerance, args.max_iter)

        def predict():
            last["pred"] = eng.pathwise_predict(obj if is_op else phi, tr, te, y, args.noise, e1, e2, args.tolerance,
                                                args.max_iter, **({"f": f} if is_op else {}))

        res = {}
        for what, B in (("mll", rhs), ("predict", Bp)):
            ms = timed(lambda: solve(B), args.warmup, args.repeats)
            res[f"{what}_cg_ms"] = ms
            res[f"{what}_cg_iters"] = last["iters"]
            res[f"{what}_cg_ms_per_iter"] = ms / max(last["iters"], 1)
        res["mll_total_ms"] = timed(mll, args.warmup, args.repeats)
        res["mll_iters"] = last["mll"][3]
        res["mll_value_per_datum"] = last["mll"][0] / args.train
        res["predict_total_ms"] = timed(predict, args.warmup, args.repeats)
        res["predict_iters"] = last["pred"][1]
        out[name] = res
        print(f"{name}: MLL {res['mll_total_ms']:.1f} ms total, {res['mll_iters']} CG iterations, "
              f"{res['mll_cg_ms_per_iter']:.2f} ms per iteration (S = {rhs.shape[1]}); predict "
              f"{res['predict_total_ms']:.1f} ms total, {res['predict_iters']} iterations, "
              f"{res['predict_cg_ms_per_iter']:.2f} ms per iteration (S = {Bp.shape[1]})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
