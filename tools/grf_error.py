#!/usr/bin/env python3
"""Relative Frobenius error of the GRF kernel against the exact kernel it estimates (needs an MI355X).

For a graph and a modulator f, the exact K = Phi Phi^T with Phi = sum_l f_l L^l comes from the device SpGEMM's
exact step matrices (GRFEngine.exact_steps); the GRF K from the Philox walks at each --walks value (the
benchmarked fused path where m L <= 4096, the walk / features path above).  Printed per walks-per-node value:
||K_grf - K_exact||_F / ||K_exact||_F, mean and spread over --seeds walk seeds -- the paper's figure of merit.
Both K are formed in fp64 from the fp64 features (dense: keep the graph at ~10^4 nodes).  One JSON line at the end.

--operator takes the exact K from the walk operator instead (GRFEngine.poly_kernel_block on a WalkPolynomial:
Horner chains with L itself, no power of it formed), so the tool also runs on graphs whose exact step matrices
fill in -- Erdos-Renyi graphs, where exact_steps raises.

--truth expm measures against the closed form exp(-beta L) instead (GRFEngine.diffusion_expm: scaling and squaring
on the fp64 matrix cores) and splits the GRF kernel's error in two: the truncation error of the walk-power series
(the exact walk-power K against exp(-beta L), independent of the walks) and the Monte-Carlo error (the GRF K against
the walk-power K); the total is the GRF K against exp(-beta L).  All three relative to ||exp(-beta L)||_F.
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


def grid(rows, cols):
    import scipy.sparse as sp
    idx = np.arange(rows * cols).reshape(rows, cols)
    e = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                        np.stack([idx[:-1].ravel(), idx[1:].ravel()])], axis=1)
    A = sp.coo_matrix((np.ones(e.shape[1]), (e[0], e[1])), shape=(rows * cols,) * 2)
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def ring(n):
    import scipy.sparse as sp
    i = np.arange(n)
    A = sp.coo_matrix((np.ones(2 * n), (np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i - 1) % n]))),
                      shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.data[:] = 1.0
    A.sort_indices()
    return A


def dense64(eng, M):
    """A DeviceCSR's fp64 values as a dense matrix on the device."""
    D = torch.zeros((M.n_rows, M.n_cols), dtype=torch.float64, device=eng.device)
    r = torch.repeat_interleave(torch.arange(M.n_rows, device=eng.device), M.ptr[1:] - M.ptr[:-1], output_size=M.nnz)
    D[r, M.idx[:M.nnz].long()] = M.val[:M.nnz]
    return D


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="grid:100x100", help="grid:RxC, ring:N or er:N:EDGES")
    ap.add_argument("--walks", default="16,64,256,1000", help="walks-per-node values, comma separated")
    ap.add_argument("--length", type=int, default=5)
    ap.add_argument("--p-halt", type=float, default=0.1)
    ap.add_argument("--beta", type=float, default=1.0, help="diffusion modulator (-beta/2)^l / l!")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--operator", action="store_true",
                    help="the exact K from the walk operator (no step matrices: works where they fill in)")
    ap.add_argument("--truth", choices=("pofm", "expm"), default="pofm",
                    help="pofm: against the exact walk-power K; expm: against exp(-beta L), truncation and "
                         "Monte-Carlo error apart")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grf_error: no GPU")
    from grf_amd import _lib as C
    from grf_amd.engine import WalkPolynomial, get_engine
    from grf_amd.graphs import er_graph_exact_edges

    kind, _, spec = args.graph.partition(":")
    if kind == "grid":
        r, c = (int(x) for x in spec.split("x"))
        A = grid(r, c)
    elif kind == "ring":
        A = ring(int(spec))
    elif kind == "er":
        n, m = (int(x) for x in spec.split(":"))
        A = er_graph_exact_edges(n, m, seed=0)
    else:
        sys.exit(f"grf_error: unknown graph {args.graph!r}")
    eng = get_engine("cuda:0")
    L = args.length
    f = np.array([(-args.beta / 2.0) ** l / math.factorial(l) for l in range(L)])
    G = eng.laplacian(A)
    out = {"graph": args.graph, "n": A.shape[0], "L": L, "p_halt": args.p_halt, "beta": args.beta, "rows": []}
    if args.operator:
        K = eng.poly_kernel_block(WalkPolynomial(G, L, engine=eng), torch.from_numpy(f))
        out["exact_from"] = "operator"
        what = f"exact K from the operator, nnz(L) = {G.nnz}"
    else:
        steps = eng.exact_steps(G, L)
        Phi = sum(fl * dense64(eng, M) for fl, M in zip(f, steps))
        K = Phi @ Phi.T
        out["nnz_exact_steps"] = [M.nnz for M in steps]
        what = f"exact steps nnz = {out['nnz_exact_steps']}"
    k_norm = float(torch.linalg.norm(K))
    print(f"{args.graph}: n = {A.shape[0]}, {what}, ||K||_F = {k_norm:.6g}")
    E = None
    if args.truth == "expm":
        # the scipy-semantics normalised Laplacian of non-negative weights: spectrum in [0, 2]
        rho = 2.0 * args.beta
        E = eng.diffusion_expm(dense64(eng, G), args.beta, rho)
        e_norm = float(torch.linalg.norm(E))
        out["truth"] = "expm"
        out["expm_products"] = 17 + eng.expm_squarings(rho)
        out["truncation"] = float(torch.linalg.norm(K - E)) / e_norm
        print(f"exp(-beta L): {out['expm_products']} dense products, ||E||_F = {e_norm:.6g}; truncation error "
              f"||K_pofm - E||_F / ||E||_F = {out['truncation']:.4e}")
        print(f"{'walks':>8} {'total (vs expm)':>18} {'Monte-Carlo (vs pofm)':>24} {'truncation':>14}")
    else:
        print(f"{'walks':>8} {'rel Frobenius error':>22} {'[min, max]':>26}")
    for m in (int(x) for x in args.walks.split(",")):
        errs, totals = [], []
        for seed in range(args.seeds):
            if m * L <= 4096:
                rows = eng.walk_phi(G, m, args.p_halt, L, f, seed=100 + seed, norm=C.NORM_MUL_RECIP)
            else:
                slots = eng.walk(G, m, args.p_halt, L, rng=C.RNG_PHILOX, seed=100 + seed)
                rows = eng.features(slots, f, C.NORM_MUL_RECIP)
            P = dense64(eng, eng.compact(rows))
            Kg = P @ P.T
            errs.append(float(torch.linalg.norm(Kg - K)) / (k_norm if E is None else e_norm))
            if E is not None:
                totals.append(float(torch.linalg.norm(Kg - E)) / e_norm)
            del P, rows, Kg
        if E is not None:
            out["rows"].append({"walks": m, "total": float(np.mean(totals)), "monte_carlo": float(np.mean(errs)),
                                "truncation": out["truncation"], "total_min": min(totals), "total_max": max(totals)})
            print(f"{m:>8} {np.mean(totals):>18.4e} {np.mean(errs):>24.4e} {out['truncation']:>14.4e}", flush=True)
            continue
        out["rows"].append({"walks": m, "mean": float(np.mean(errs)), "min": min(errs), "max": max(errs)})
        print(f"{m:>8} {np.mean(errs):>22.4e} {'[%.4e, %.4e]' % (min(errs), max(errs)):>26}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
