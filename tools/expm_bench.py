#!/usr/bin/env python3
"""Times the exact diffusion kernel exp(-beta L) and the fp64 product under it (needs an MI355X).

1. The kernel's yardstick: one squaring P <- P P in the symmetric mode of GRFEngine.gemm_nt_f64 (just over half the
   tiles computed, both triangles written) at n = 2708 and n = 8192, against torch.matmul(P, P) in fp64 on the same
   tensor, and both as a fraction of the fp64 matrix-core ceiling (--ceiling-tflops: the figure
   tools/mfma_f64_ceiling measured on this box; AMD's specification for the card is 78.6).  Flops are counted as
   2 n^3 for both, so the symmetric mode's figure is an effective rate.
2. End to end: api.diffusion_kernel_exact (Laplacian, 17 + s products, the copy to the host) on Cora (n = 2708,
   bench.py --workload c3's graph) and on C2's graph (Erdos-Renyi, n = 10 000) at beta = 2, with the product count,
   the device-only time of GRFEngine.diffusion_expm, and for Cora the time of scipy.linalg.expm on the host.

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each timed call,
synchronised; median and range of the repeats.  There is no pass or fail figure.  One JSON line at the end; the
printed lines are also written to --out (default profiles/expm_bench.txt).
"""
import argparse
import builtins
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
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2708, 8192])
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--ceiling-tflops", type=float, default=78.6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--skip-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("expm_bench: no GPU (timings are taken on the device or not at all)")

    import bench
    from grf_amd import api
    from grf_amd.engine import get_engine

    eng = get_engine("cuda:0")
    dev = eng.device
    log = open(args.out, "w")

    def print(*a, **k):  # (every line goes to the terminal and to --out)
        k.pop("flush", None)
        builtins.print(*a, flush=True, **k)
        builtins.print(*a, file=log, flush=True, **k)

    out = {"device": torch.cuda.get_device_name(0), "beta": args.beta, "ceiling_tflops": args.ceiling_tflops,
           "squaring": [], "end_to_end": []}
    print(f"{'n':>6} {'call':>22} {'median ms':>10} {'min':>8} {'max':>8} {'TF/s (2n^3)':>12} {'of ceiling':>10}", flush=True)
    for n in args.sizes:
        # a symmetric matrix with its spectrum in (0, 1], as every squaring's input has
        g = torch.Generator(dev).manual_seed(n)
        Q = torch.rand((n, n), dtype=torch.float64, device=dev, generator=g)
        P = (Q + Q.T) / (2.0 * n)
        C = torch.empty_like(P)
        T = torch.empty_like(P)
        flops = 2.0 * n ** 3
        for name, fn in (("gemm_nt_f64 symmetric", lambda: eng.gemm_nt_f64(P, P, out=C, symmetric=True)),
                         ("gemm_nt_f64 general", lambda: eng.gemm_nt_f64(P, P, out=C)),
                         ("torch.matmul fp64", lambda: torch.matmul(P, P, out=T))):
            t = timed(fn, args.warmup, args.repeats)
            tf = flops / (t["median_ms"] * 1e-3) / 1e12
            out["squaring"].append({"n": n, "call": name, "tflops_2n3": tf, "of_ceiling": tf / args.ceiling_tflops, **t})
            print(f"{n:>6} {name:>22} {t['median_ms']:>10.3f} {t['min_ms']:>8.3f} {t['max_ms']:>8.3f} {tf:>12.2f} "
                  f"{tf / args.ceiling_tflops:>10.3f}", flush=True)
        err = float((C - T).abs().max() / T.abs().max())
        print(f"{n:>6} max |gemm - matmul| / max |matmul| = {err:.2e}", flush=True)
        del Q, P, C, T
    if not args.skip_end_to_end:
        for wl in ("c3", "c2"):
            W, desc, _ = bench.dense_workload(wl)
            n = W.shape[0]
            L, radius = api.dense_laplacian_device(W, True, dev)
            rho = args.beta * radius
            products = 17 + eng.expm_squarings(rho)
            t_dev = timed(lambda: eng.diffusion_expm(L, args.beta, rho), args.warmup, args.repeats)
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                K = api.diffusion_kernel_exact(W, args.beta)
                wall.append((time.perf_counter() - t0) * 1e3)
            row = {"workload": wl, "n": n, "products": products, "expm_device": t_dev,
                   "api_wall_ms_median": float(np.median(wall)),
                   "tflops_device": products * 2.0 * n ** 3 / (t_dev["median_ms"] * 1e-3) / 1e12}
            if wl == "c3" and not args.skip_scipy:
                import scipy.linalg
                Lh = L.cpu().numpy()
                t0 = time.perf_counter()
                S = scipy.linalg.expm(-args.beta * Lh)
                row["scipy_expm_ms"] = (time.perf_counter() - t0) * 1e3
                row["scipy_threads"] = os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else \
                    int(os.environ["OMP_NUM_THREADS"])
                row["max_abs_diff_vs_scipy"] = float(np.abs(K - S).max())
            out["end_to_end"].append(row)
            print(f"{desc}: {products} products, diffusion_expm {t_dev['median_ms']:.2f} ms "
                  f"[{t_dev['min_ms']:.2f}, {t_dev['max_ms']:.2f}] ({row['tflops_device']:.2f} TF/s effective), "
                  f"api.diffusion_kernel_exact {row['api_wall_ms_median']:.1f} ms wall"
                  + (f", scipy.linalg.expm {row['scipy_expm_ms']:.0f} ms on {row['scipy_threads']} threads, "
                     f"max |diff| {row['max_abs_diff_vs_scipy']:.2e}" if "scipy_expm_ms" in row else ""), flush=True)
            del L, K
    print(json.dumps(out))


if __name__ == "__main__":
    main()
