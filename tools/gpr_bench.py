#!/usr/bin/env python3
"""Times the dense exact GPR's device path (needs an MI355X): GRFEngine.cholesky (grf_potrf_f64), one
gpr_log_marginal_likelihood forward plus backward, and GPR.predict_f, at Cora's n = 2485 and at n = 10 000, each
against torch.linalg.cholesky / cholesky_solve / solve_triangular on the same tensors.

The matrix is K = Phi Phi^T / k + I (Phi random n x k, fp64), the shape of a kernel matrix plus noise; Y has two
columns; predict_f runs on 1000 test nodes through a kernel object that gathers from a fixed K.  The share of the
factorisation spent in potf2's serial columns is estimated as (number of diagonal blocks) x (the time of
cholesky at n = 128, which is one potf2 launch and the copy) / (the time of cholesky at n).

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each timed call,
synchronised; median and range of the repeats.  There is no pass or fail figure.  One JSON line at the end; the
printed lines are also written to --out (default profiles/gpr_bench.txt).
"""
import argparse
import builtins
import json
import os
import sys

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


class FixedKernel(torch.nn.Module):
    """K_torch gathers from a fixed matrix (what the dense kernels' K_torch does with their cached K)."""

    def __init__(self, K):
        super().__init__()
        self.Kfull = K

    def K_torch(self, X1, X2=None):
        i1 = torch.as_tensor(X1).reshape(-1).long().to(self.Kfull.device)
        i2 = i1 if X2 is None else torch.as_tensor(X2).reshape(-1).long().to(self.Kfull.device)
        return self.Kfull[i1][:, i2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2485, 10000])
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpr_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpr_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp.models import GPR
    from grf_amd.engine import get_engine
    from grf_amd.features import gpr_log_marginal_likelihood

    eng = get_engine()
    dev = eng.device
    log = open(args.out, "w")

    def print(*a, **k):  # (every line goes to the terminal and to --out)
        k.pop("flush", None)
        builtins.print(*a, flush=True, **k)
        builtins.print(*a, file=log, flush=True, **k)

    out = {"device": torch.cuda.get_device_name(0), "rows": []}
    I2 = torch.eye(128, dtype=torch.float64, device=dev) * 2.0
    one_block = timed(lambda: eng.cholesky(I2), args.warmup, args.repeats)
    print(f"cholesky at n = 128 (one potf2 block and the copy): {one_block['median_ms']:.4f} ms "
          f"[{one_block['min_ms']:.4f}, {one_block['max_ms']:.4f}]")
    out["potf2_block"] = one_block
    print(f"{'n':>6} {'call':>34} {'median ms':>10} {'min':>9} {'max':>9}")

    def row(n, name, t, **extra):
        out["rows"].append({"n": n, "call": name, **t, **extra})
        print(f"{n:>6} {name:>34} {t['median_ms']:>10.3f} {t['min_ms']:>9.3f} {t['max_ms']:>9.3f}")

    def torch_row(n, name, fn):
        """A torch baseline; one that torch cannot run at this size (its solver's own allocation) is recorded so."""
        try:
            row(n, name, timed(fn, args.warmup, args.repeats))
            return True
        except RuntimeError as e:
            out["rows"].append({"n": n, "call": name, "failed": str(e).splitlines()[0]})
            print(f"{n:>6} {name:>34} failed in torch: {str(e).splitlines()[0]}")
            torch.cuda.empty_cache()
            return False

    for n in args.sizes:
        g = torch.Generator(dev).manual_seed(n)
        k = 64
        Phi = torch.randn((n + args.n_test, k), dtype=torch.float64, device=dev, generator=g)
        Kall = Phi @ Phi.T / k
        K = Kall[:n, :n].contiguous()
        Y = torch.randn((n, 2), dtype=torch.float64, device=dev, generator=g)
        noise = torch.tensor(1.0, dtype=torch.float64, device=dev)
        Kh = K + torch.eye(n, dtype=torch.float64, device=dev)

        t = timed(lambda: eng.cholesky(Kh), args.warmup, args.repeats)
        blocks = -(-n // 128)
        share = blocks * one_block["median_ms"] / t["median_ms"]
        row(n, "GRFEngine.cholesky", t, potf2_share=share)
        row(n, "torch.linalg.cholesky", timed(lambda: torch.linalg.cholesky(Kh), args.warmup, args.repeats))
        F, logdet, info = eng.cholesky(Kh)
        Lt = torch.linalg.cholesky(Kh)
        err = float((torch.tril(F) - Lt).abs().max() / Lt.abs().max())
        print(f"{n:>6} info {int(info.item())}, max |L - torch L| / max |L| = {err:.2e}; potf2's serial columns: "
              f"{blocks} blocks x {one_block['median_ms']:.4f} ms = {100 * share:.1f} % of the factorisation")

        def lml_ours():
            Kg = K.detach().requires_grad_(True)
            ng = noise.detach().requires_grad_(True)
            v, _ = gpr_log_marginal_likelihood(Kg, ng, Y, engine=eng)
            v.backward()
            return v

        def lml_torch():
            Kg = K.detach().requires_grad_(True)
            ng = noise.detach().requires_grad_(True)
            L = torch.linalg.cholesky(Kg + ng * torch.eye(n, dtype=torch.float64, device=dev))
            a = torch.cholesky_solve(Y, L)
            v = -0.5 * (Y * a).sum() - 2 * torch.log(L.diagonal()).sum() - n * np.log(2 * np.pi)
            v.backward()
            return v

        row(n, "gpr_log_marginal_likelihood f+b", timed(lml_ours, args.warmup, args.repeats))
        if torch_row(n, "torch cholesky lml f+b", lml_torch):
            a, b = float(lml_ours().item()), float(lml_torch().item())
            print(f"{n:>6} lml {a!r} vs torch {b!r} (relative difference {abs(a - b) / abs(b):.2e})")

        kernel = FixedKernel(Kall)
        X = torch.arange(n, device=dev)
        Xs = torch.arange(n, n + args.n_test, device=dev)
        model = GPR(data=(X, Y), kernel=kernel, noise_variance=1.0)
        model.predict_f(Xs)  # (the factor is cached from here on, as it is after a training step)

        def predict_torch():
            Ksx = Kall[n:, :n]
            A = torch.linalg.solve_triangular(Lt, Ksx.T, upper=False)
            V = torch.linalg.solve_triangular(Lt, Y, upper=False)
            return A.T @ V, Kall.diagonal()[n:] - (A * A).sum(dim=0)

        row(n, f"GPR.predict_f ({args.n_test} nodes)", timed(lambda: model.predict_f(Xs), args.warmup, args.repeats))
        if torch_row(n, "torch solve_triangular predict", predict_torch):
            m1, v1 = model.predict_f(Xs)
            m2, v2 = predict_torch()
            print(f"{n:>6} predict_f vs torch: max |mean diff| {float((m1 - m2).abs().max()):.2e}, "
                  f"max |var diff| {float((v1[:, 0] - v2).abs().max()):.2e}")
        del Phi, Kall, K, Kh, F, Lt, kernel, model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
