#!/usr/bin/env python3
"""Times the sparse variational GP's device path (needs an MI355X) at the Cora notebooks' shape: N = 1988 training
nodes, M = 994 inducing nodes, P = 7 classes.  One SVGP.training_loss forward plus backward (a step of the
notebooks' Adam loop without the optimiser) and SVGP.predict_y on 497 nodes, each against the same expression
written with torch.linalg.cholesky, solve_triangular and torch.special.erf autograd on the same device; then the
pieces of a step one by one, to say where the time goes.

The kernel matrix is synthetic and well conditioned, K = s (Phi Phi^T / k + I) (Phi random n x k, fp64) with a
trainable scale s, so that the backward reaches K[Z, Z] as it does with a graph kernel's modulator; labels are
random.

Timing discipline of bench.py: warm-up calls of the same shapes first, then device events around each timed call,
synchronised; median and range of the repeats.  There is no pass or fail figure.  One JSON line at the end; the
printed lines are also written to --out (default profiles/svgp_bench.txt).
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


class ScaledKernel(torch.nn.Module):
    """K_torch gathers from a fixed matrix times a trainable scale."""

    def __init__(self, K):
        super().__init__()
        self.Kfull = K
        self.scale = torch.nn.Parameter(torch.ones((), dtype=torch.float64, device=K.device))

    def K_torch(self, X1, X2=None):
        i1 = torch.as_tensor(X1).reshape(-1).long().to(self.Kfull.device)
        i2 = i1 if X2 is None else torch.as_tensor(X2).reshape(-1).long().to(self.Kfull.device)
        return self.scale * self.Kfull[i1][:, i2]


def torch_conditional(Kmm, Knm, Knn, q_mu, q_sqrt, jitter):
    M = Kmm.shape[0]
    Lm = torch.linalg.cholesky(Kmm + jitter * torch.eye(M, dtype=Kmm.dtype, device=Kmm.device))
    A = torch.linalg.solve_triangular(Lm, Knm.t(), upper=False)
    Lq = torch.tril(q_sqrt)
    fmean = A.t() @ q_mu
    base = Knn - (A * A).sum(dim=0)
    fvar = torch.stack([base + ((A.t() @ Lq[p]) ** 2).sum(dim=1) for p in range(Lq.shape[0])], dim=1)
    return fmean, fvar, Lq


def torch_prob(mu, var, y, gx, w):
    """RobustMax.prob_is_largest on torch.special.erf for the labels y (n,)."""
    P = mu.shape[1]
    x = mu.gather(1, y[:, None]) + gx[None, :] * torch.sqrt(torch.clamp(2.0 * var.gather(1, y[:, None]), min=1e-10))
    d = (x[:, None, :] - mu[:, :, None]) / torch.sqrt(torch.clamp(var, min=1e-10))[:, :, None]
    cdfs = 0.5 * (1.0 + torch.special.erf(d / np.sqrt(2.0))) * (1 - 2e-4) + 1e-4
    on = torch.nn.functional.one_hot(y, P).to(mu.dtype)[:, :, None]
    return torch.prod(cdfs * (1.0 - on) + on, dim=1) @ w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1988)
    ap.add_argument("--m", type=int, default=994)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--n-test", type=int, default=497)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgp_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("svgp_bench: no GPU (timings are taken on the device or not at all)")

    from efficient_graph_gp.likelihoods import MultiClass
    from efficient_graph_gp.models import SVGP
    from grf_amd.engine import get_engine

    eng = get_engine()
    dev = eng.device
    log = open(args.out, "w")

    def print(*a, **k):  # (every line goes to the terminal and to --out)
        k.pop("flush", None)
        builtins.print(*a, flush=True, **k)
        builtins.print(*a, file=log, flush=True, **k)

    N, M, P, NT, eps, jitter = args.n, args.m, args.classes, args.n_test, 1e-3, 1e-6
    out = {"device": torch.cuda.get_device_name(0), "N": N, "M": M, "P": P, "n_test": NT, "rows": []}
    print(f"SVGP at N = {N}, M = {M}, P = {P}; predict_y on {NT} nodes; {args.repeats} repeats after {args.warmup} "
          f"warm-up calls; {out['device']}")
    print(f"{'call':>58} {'median ms':>10} {'min':>9} {'max':>9}")

    def row(name, t):
        out["rows"].append({"call": name, **t})
        print(f"{name:>58} {t['median_ms']:>10.3f} {t['min_ms']:>9.3f} {t['max_ms']:>9.3f}")

    g = torch.Generator(dev).manual_seed(N)
    k = 64
    Phi = torch.randn((N + NT, k), dtype=torch.float64, device=dev, generator=g)
    Kall = Phi @ Phi.T / k + torch.eye(N + NT, dtype=torch.float64, device=dev)
    kernel = ScaledKernel(Kall)
    X = torch.arange(N, device=dev)
    Z = torch.arange(0, N, N // M, device=dev)[:M]
    Xs = torch.arange(N, N + NT, device=dev)
    Y = torch.randint(0, P, (N,), device=dev, generator=g).to(torch.int32)
    q_mu = 0.1 * torch.randn((M, P), dtype=torch.float64, device=dev, generator=g)
    model = SVGP(kernel, MultiClass(P), Z, num_latent_gps=P, q_mu=q_mu, jitter=jitter)
    data = (X, Y)
    gx, gw = np.polynomial.hermite.hermgauss(20)
    gx_t = torch.as_tensor(gx, device=dev)
    w_t = torch.as_tensor(gw / np.sqrt(np.pi), device=dev)
    Yl = Y.long()

    def touch():
        """What an optimiser step does to the caches: the kernel's parameter gets a new version, so the factor of
        K[Z, Z] is computed again, as in every step of a training loop."""
        with torch.no_grad():
            kernel.scale.mul_(1.0)

    def step_ours():
        touch()
        model.zero_grad(set_to_none=True)
        loss = model.training_loss(data)
        loss.backward()
        return loss

    def loss_torch():
        Kb = kernel.K_torch(torch.cat([Z, X]), Z)
        Knn = kernel.K_torch(X, X).diagonal()
        fmean, fvar, Lq = torch_conditional(Kb[:M], Kb[M:], Knn, model.q_mu, model.q_sqrt, jitter)
        p = torch_prob(fmean, fvar, Yl, gx_t, w_t)
        ve = p * np.log(1.0 - eps) + (1.0 - p) * np.log(eps / (P - 1))
        kl = 0.5 * ((model.q_mu ** 2).sum() - P * M - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum()
                    + (Lq * Lq).sum())
        return kl - ve.sum()

    def step_torch():
        model.zero_grad(set_to_none=True)
        loss = loss_torch()
        loss.backward()
        return loss

    row("SVGP.training_loss forward + backward", timed(step_ours, args.warmup, args.repeats))
    a = float(step_ours().item())
    g_ours = [model.q_mu.grad.clone(), model.q_sqrt.grad.clone(), kernel.scale.grad.clone()]
    row("torch cholesky / solve_triangular / erf forward + backward", timed(step_torch, args.warmup, args.repeats))
    b = float(step_torch().item())
    g_torch = [model.q_mu.grad.clone(), model.q_sqrt.grad.clone(), kernel.scale.grad.clone()]
    print(f"loss {a!r} vs torch {b!r} (relative difference {abs(a - b) / abs(b):.2e}); gradients, max |diff| / max "
          "|value|: " + ", ".join(f"{n} {float((x - y).abs().max() / y.abs().max()):.2e}"
                                  for n, x, y in zip(("q_mu", "q_sqrt", "kernel scale"), g_ours, g_torch)))
    with torch.no_grad():
        row("SVGP.training_loss forward only (factor included)",
            timed(lambda: (touch(), model.training_loss(data)), args.warmup, args.repeats))

    @torch.no_grad()
    def predict_torch():
        Kb = kernel.K_torch(torch.cat([Z, Xs]), Z)
        fmean, fvar, _ = torch_conditional(Kb[:M], Kb[M:], kernel.K_torch(Xs, Xs).diagonal(), model.q_mu,
                                           model.q_sqrt, jitter)
        cols = []
        for c in range(P):
            p = torch_prob(fmean, fvar, torch.full((NT,), c, device=dev), gx_t, w_t)
            cols.append(p * (1.0 - eps) + (1.0 - p) * (eps / (P - 1)))
        ps = torch.stack(cols, dim=1)
        return ps, ps - ps * ps

    model.predict_y(Xs)  # (the factor is cached from here on, as it is after a training step)
    row(f"SVGP.predict_y ({NT} nodes, factor cached)", timed(lambda: model.predict_y(Xs), args.warmup, args.repeats))
    row("torch predict_y (factors K[Z, Z] each call)", timed(predict_torch, args.warmup, args.repeats))
    print(f"predict_y vs torch: max |ps diff| {float((model.predict_y(Xs)[0] - predict_torch()[0]).abs().max()):.2e}")

    # ---- the pieces of one step, on the step's own shapes
    print("the pieces of one step:")
    with torch.no_grad():
        Kmm = Kall[Z][:, Z].contiguous()
        Knm = Kall[X][:, Z].contiguous()
        Kh = Kmm + jitter * torch.eye(M, dtype=torch.float64, device=dev)
        F, _, _ = eng.cholesky(Kh)
        Lq = torch.tril(model.q_sqrt.detach())
        B = Lq.transpose(1, 2).reshape(P * M, M)
        AT = eng.cholesky_solve(F, Knm)
        A = AT.t().contiguous()
        T = eng.gemm_nt_f64(AT, B)
        fmean = eng.gemm_nt_f64(AT, model.q_mu.detach().t().contiguous())
        fvar = eng.rows_sqsum(T, P, Kall.diagonal()[X] - eng.rows_sqsum(AT, 1)[:, 0])
        W = torch.randn((N, P * M), dtype=torch.float64, device=dev, generator=g)
        Wt = W.t().contiguous()
        Cq = Lq.permute(1, 0, 2).reshape(M, P * M)
        Mm = torch.randn((M, M), dtype=torch.float64, device=dev, generator=g)
        pieces = [
            ("cholesky of K[Z, Z] (M)", lambda: eng.cholesky(Kh)),
            ("forward solve, N right-hand sides", lambda: eng.cholesky_solve(F, Knm, transposed=False)),
            ("T = AT [Lq_1 .. Lq_P] (N x P M, k = M)", lambda: eng.gemm_nt_f64(AT, B)),
            ("rows_sqsum(T, P) + rows_sqsum(AT, 1)", lambda: (eng.rows_sqsum(T, P), eng.rows_sqsum(AT, 1))),
            ("robustmax_ve with gradients (the quadrature)", lambda: eng.robustmax_ve(fmean, fvar, Y)),
            ("robustmax_ve forward only", lambda: eng.robustmax_ve(fmean, fvar, Y, with_grad=False)),
            ("backward: W = 2 Gv o T and its transpose", lambda: (W * 2.0).t().contiguous()),
            ("backward: d/dLq = W^T A (P M x M, k = N)", lambda: eng.gemm_nt_f64(Wt, A)),
            ("backward: sum_p W_p Lq_p^T (N x M, k = P M)", lambda: eng.gemm_nt_f64(W, Cq)),
            ("backward: transposed solve, N right-hand sides", lambda: eng.cholesky_solve(F, Knm, transposed=True)),
            ("backward: Kmn_bar A^T and Lm^T L_bar (two M x M products)",
             lambda: (eng.gemm_nt_f64(A, A), eng.gemm_nt_f64(Mm, Mm))),
            ("backward: two transposed solves, M right-hand sides",
             lambda: eng.cholesky_solve(F, eng.cholesky_solve(F, Mm, transposed=True), transposed=True)),
            ("K_torch gathers (K[Z + X, Z], diag K[X, X])",
             lambda: (kernel.K_torch(torch.cat([Z, X]), Z), kernel.K_torch(X, X).diagonal())),
        ]
        for name, fn in pieces:
            row(name, timed(fn, args.warmup, args.repeats))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
