#!/usr/bin/env python3
"""Times GRFEngine.exact_steps on the two low-degree graphs of the reference's sparse experiments (needs an
MI355X): a 1000 x 1000 grid at L = 5 and a 2^20-node ring at L = 3.

Beside it, on the same graph: the walk preprocessing (Philox walks -> step matrices) at m = 128 and at the
reference's m = 1000 walks per node, and scipy's chain M_l = M_{l-1} @ L on the host (scipy's SpGEMM runs on
one thread; the thread count of the box is printed with it).  Device timings use device events around each
call after warm-up calls of the same shapes; the median and [min, max] of the repeats are printed.  exact_steps
reads each power's nnz on the host, so its time includes those synchronisations.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd"), os.path.join(ROOT, "tools")):
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


def show(name, r):
    print(f"  {name}: {r['median_ms']:.2f} ms [{r['min_ms']:.2f}, {r['max_ms']:.2f}]", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1000, help="side of the grid")
    ap.add_argument("--ring", type=int, default=1 << 20, help="nodes of the ring")
    ap.add_argument("--walks", default="128,1000")
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exact_steps_bench: no GPU (timings are taken on the device or not at all)")
    import scipy.sparse as sp
    from grf_amd import _lib as C
    from grf_amd.engine import get_engine
    from grf_error import grid, ring

    eng = get_engine("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "host_threads": os.cpu_count(), "cases": []}
    for name, A, L in ((f"grid {args.grid}x{args.grid}", grid(args.grid, args.grid), 5),
                       (f"ring {args.ring}", ring(args.ring), 3)):
        G = eng.laplacian(A)
        torch.cuda.synchronize()
        case = {"graph": name, "n": A.shape[0], "L": L}
        print(f"{name}: n = {A.shape[0]}, L = {L}", flush=True)
        last = {}

        def exact():
            last["steps"] = eng.exact_steps(G, L)

        case["exact_steps"] = timed(exact, args.warmup, args.repeats)
        case["nnz"] = [M.nnz for M in last["steps"]]
        show(f"exact_steps (nnz {case['nnz']})", case["exact_steps"])
        last.clear()
        for m in (int(x) for x in args.walks.split(",")):
            def walk():
                slots = eng.walk(G, m, args.p_halt, L, rng=C.RNG_PHILOX, seed=42)
                last["steps"] = eng.step_matrices(eng.steps(slots, C.NORM_MUL_RECIP))

            try:
                r = timed(walk, args.warmup, max(2, args.repeats // 2))
                r["nnz"] = [M.nnz for M in last["steps"]]
                show(f"walk preprocessing, m = {m} (nnz {r['nnz']})", r)
            except (RuntimeError, ValueError) as e:  # (the visit slots of m = 1000 may not fit)
                r = {"error": str(e).splitlines()[0][:200]}
                print(f"  walk preprocessing, m = {m}: {r['error']}", flush=True)
            case[f"walk_m{m}"] = r
            last.clear()
            torch.cuda.empty_cache()
        if not args.no_scipy:
            Ls = G.to_scipy()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                M = sp.identity(A.shape[0], format="csr")
                for _l in range(1, L):
                    M = M @ Ls
                t.append((time.perf_counter() - t0) * 1e3)
            case["scipy_chain"] = {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t), "repeats": 3}
            show(f"scipy chain on the host ({os.cpu_count()} threads visible, SpGEMM uses one)", case["scipy_chain"])
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
