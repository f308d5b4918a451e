#!/usr/bin/env python3
"""Times the exact posterior mean and variance (GRFEngine.posterior_moments; needs an MI355X).

Workload: the headline C4 graph (Erdos-Renyi, N = 100k, 1M undirected edges, 128 walks, L = 8,
p_halt = 0.1), diffusion modulator, noise 0.01, 60k training nodes, 4096 test nodes (16 chunks of 256),
CG tolerance 1e-2 (gpytorch's eval_cg_tolerance).

  1. posterior_moments: ms per 256-node chunk, CG iterations per chunk.
  2. The two kernels of csrc/grf_posterior.hip alone at the chunk's shapes -- grf_posterior_rhs_f64 and
     grf_posterior_reduce_f64 -- their share of a chunk's time, and the reduce kernel's achieved bandwidth
     (16 n S bytes read once) against the 8 TB/s peak.
  3. The only route there was before: 64 pathwise samples (pathwise_predict) and their .std(0), its time and
     its error against the exact standard deviations on the same nodes.

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

PEAK_BYTES_PER_S = 8.0e12


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
    return f"{r['median_ms']:.3f} ms [{r['min_ms']:.3f}, {r['max_ms']:.3f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=128)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--n-train", type=int, default=60_000)
    ap.add_argument("--n-test", type=int, default=4096)
    ap.add_argument("--tolerance", type=float, default=1e-2)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("posterior_bench: no GPU (timings are taken on the device or not at all)")

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
    steps = StepMatrices(pre.preprocess_graph(), eng)
    L = steps.L
    f0 = torch.tensor([(-1.0) ** l / (2 ** l * math.factorial(l)) for l in range(L)], dtype=torch.float32, device=dev)
    phi = steps.phi(f0)
    torch.cuda.synchronize()
    n_tr, n_te = min(args.n_train, args.n), args.n_test
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "edges": args.edges, "walks": args.walks, "L": L,
           "p_halt": args.p_halt, "n_train": n_tr, "n_test": n_te, "tolerance": args.tolerance, "noise": args.noise,
           "nnz_phi": phi.nnz, "setup_s": time.perf_counter() - t0}
    print(f"setup {out['setup_s']:.1f} s: Phi has {phi.nnz} entries", flush=True)
    r = np.random.default_rng(0)
    perm = r.permutation(args.n)
    tr = torch.from_numpy(np.sort(perm[:n_tr])).to(dev)
    te = torch.from_numpy(r.integers(0, args.n, n_te)).to(dev)
    y = torch.randn(n_tr, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
    chunks = -(-n_te // eng.POSTERIOR_CHUNK)
    last = {}

    # 1. the whole call
    def moments():
        info = {}
        last["mean"], last["var"] = eng.posterior_moments(phi, tr, te, y, args.noise, tolerance=args.tolerance,
                                                          info=info)
        last["info"] = info

    rm = timed(moments, args.warmup, args.repeats)
    per_chunk = rm["median_ms"] / max(chunks, 1)
    it = last["info"]["cg_iterations"]
    out["posterior_moments"] = dict(rm, chunks=chunks, ms_per_chunk=per_chunk, cg_iterations=it,
                                    alpha_iterations=last["info"]["alpha_iterations"],
                                    min_var=float(last["var"].min().item()))
    print(f"posterior_moments, n_train = {n_tr}, n_test = {n_te}: {fmt(rm)}, {per_chunk:.3f} ms per 256-node chunk, "
          f"CG iterations per chunk {min(it)}..{max(it)} (mean solve {last['info']['alpha_iterations']})", flush=True)

    # 2. the two kernels alone at a chunk's shapes
    S = min(eng.POSTERIOR_CHUNK, n_te)
    nodes = te[:S]
    E = torch.empty((phi.n_cols, S), dtype=torch.float64, device=dev)
    prior = torch.empty(S, dtype=torch.float64, device=dev)
    r_rhs = timed(lambda: eng.posterior_rhs(phi, nodes, E, prior), args.warmup + 1, args.repeats + 2)
    B = eng.spmm(phi, E, tr)
    X, _ = eng.cg_solve(phi, B, args.noise, tr, tolerance=args.tolerance)
    alpha = torch.randn(n_tr, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(6))
    var, mean = (torch.empty(S, dtype=torch.float64, device=dev) for _ in range(2))
    r_red = timed(lambda: eng.posterior_reduce(B, X, prior, alpha, 0.0, var, mean), args.warmup + 1, args.repeats + 2)
    gbs = 16.0 * n_tr * S / (r_red["median_ms"] * 1e-3)
    share = (r_rhs["median_ms"] + r_red["median_ms"]) / per_chunk if per_chunk else 0.0
    out["rhs_kernel"] = dict(r_rhs, S=S, n_cols=phi.n_cols)
    out["reduce_kernel"] = dict(r_red, S=S, n=n_tr, bytes=16 * n_tr * S, bytes_per_s=gbs,
                                fraction_of_peak=gbs / PEAK_BYTES_PER_S)
    out["new_kernels_share_of_chunk"] = share
    print(f"grf_posterior_rhs_f64 (E {phi.n_cols} x {S}): {fmt(r_rhs)}", flush=True)
    print(f"grf_posterior_reduce_f64 (n = {n_tr}, S = {S}): {fmt(r_red)}, {gbs / 1e12:.2f} TB/s = "
          f"{100 * gbs / PEAK_BYTES_PER_S:.0f} % of the 8 TB/s peak", flush=True)
    print(f"the two kernels' share of a chunk's time: {100 * share:.1f} %", flush=True)

    # 3. the route there was before: 64 pathwise samples and their spread
    # (at predict's default CG tolerance of 1, and at the tolerance of the exact moments)
    exact_std = last["var"].clamp_min(0).sqrt()
    out["pathwise_samples"] = {}
    for tol in (1.0, args.tolerance):
        def samples():
            g = torch.Generator(dev).manual_seed(7)
            e1 = torch.randn(args.samples, args.n, device=dev, generator=g)
            e2 = math.sqrt(args.noise) * torch.randn(args.samples, n_tr, device=dev, generator=g)
            smp, its = eng.pathwise_predict(phi, tr, te, y, args.noise, e1, e2, tolerance=tol)
            last["s_mean"], last["s_std"], last["s_iters"] = smp.mean(0), smp.std(0), its

        rs = timed(samples, args.warmup, args.repeats)
        rel = ((last["s_std"] - exact_std).abs() / exact_std)
        mean_err = (last["s_mean"] - last["mean"]).abs() / exact_std
        out["pathwise_samples"][f"tolerance_{tol:g}"] = dict(
            rs, samples=args.samples, cg_iterations=last["s_iters"], std_rel_error_median=float(rel.median().item()),
            std_rel_error_mean=float(rel.mean().item()), std_rel_error_max=float(rel.max().item()),
            mean_error_in_std_median=float(mean_err.median().item()))
        print(f"{args.samples} pathwise samples + .mean(0)/.std(0), CG tolerance {tol:g}: {fmt(rs)} "
              f"({last['s_iters']} CG iterations); std against the exact one: relative error median "
              f"{100 * float(rel.median()):.1f} %, mean {100 * float(rel.mean()):.1f} %, max {100 * float(rel.max()):.1f} % "
              f"(1/sqrt(2*63) = 8.9 %); mean off by a median {float(mean_err.median()):.3f} posterior std", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
