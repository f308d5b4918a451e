"""numpy fp64 restatement of the diagonally preconditioned linear_cg (TEST INFRASTRUCTURE ONLY).

* :func:`pcg_lanczos` is ``mll_reference.cg_lanczos`` (``oracle.cg.linear_cg`` with the coefficients recorded)
  run the way linear_operator's linear_cg runs with a ``preconditioner`` closure z = dinv . r:
      init:  r = b / ||b||, p = z = dinv . r, x = 0, rz = sum r.z
      step:  alpha = rz / p.Ap (0 where p.Ap < eps or the column has converged); r -= alpha Ap; x += alpha p;
             z = dinv . r; beta = rz_new / rz_old (0 where rz_old < eps); p = z + beta p.
  The residual norm behind has_converged and the stopping rule stays the unpreconditioned ||r||.  The same
  operations in the same order as linear_cg: with dinv = 1 every product with it is exact, so the iterates
  are linear_cg's bit for bit.
* :func:`jacobi_dinv`: dinv[r] = 1 / (sum_e Phi[r, e]^2 + noise), the squares added one by one in the row's
  stored order (the engine's order rule); 1 where the sum plus noise is not positive.
* :func:`estimate`: ``mll_reference.estimate`` with the Jacobi preconditioner.  With D = diag(K^) and the
  caller's probes g_i the solve's columns are [y | D^1/2 g_i]; the preconditioned coefficients are the Lanczos
  coefficients of D^-1/2 K^ D^-1/2 started at g_i / ||g_i||, so
      log det K^ ~ sum_r log d_r + slq_logdet(coef, iters, ||g_i||^2),
  and with z_i = D^1/2 g_i, u_i = K^-1 z_i the trace terms pair u_i with D^-1 z_i = D^-1/2 g_i.  The noise
  gradient's a.a (a = K^-1 y) is of second order in the iterate's error under plain CG but of first order under a
  preconditioner, so it is taken as a_k.a_k + 2 w.r_k with r_k = y - K^ a_k and w ~ K^-1 a_k from one more
  one-column preconditioned solve: y^T K^-1 a_k = a_k.a_k + w.r_k and a_k.(a - a_k) = w.r_k, each up to a product
  of two solve errors.
"""
import numpy as np
import scipy.sparse as sp

import mll_reference as R


def pcg_lanczos(matmul, rhs, dinv, tolerance=1.0, eps=1e-10, stop_updating_after=1e-10, max_iter=1000):
    """(solution, iterations run, alpha [max_iter x S], beta [max_iter x S], final residual norms [S])."""
    dtype = np.float64
    rhs = np.asarray(rhs, dtype)
    dinv = np.asarray(dinv, dtype).reshape(-1, 1)
    rhs_norm = np.linalg.norm(rhs, axis=0, keepdims=True).astype(dtype)
    rhs_is_zero = rhs_norm < eps
    rhs_norm = np.where(rhs_is_zero, dtype(1), rhs_norm)
    rhs = rhs / rhs_norm
    result = np.zeros_like(rhs)
    residual = rhs - matmul(result)
    residual_norm = np.linalg.norm(residual, axis=0, keepdims=True)
    has_converged = residual_norm < stop_updating_after
    n_iter = 0 if has_converged.all() else max_iter
    z = dinv * residual
    p = z.copy()
    rz = np.sum(residual * z, axis=0, keepdims=True)
    alphas = np.zeros((max_iter, rhs.shape[1]))
    betas = np.zeros((max_iter, rhs.shape[1]))
    k_done = 0
    residual_norm = np.where(rhs_is_zero, dtype(0), residual_norm)
    for k in range(n_iter):
        mvms = matmul(p)
        pap = np.sum(p * mvms, axis=0, keepdims=True)
        zero = pap < eps
        alpha = np.where(zero, dtype(0), rz / np.where(zero, dtype(1), pap))
        alpha = np.where(has_converged, dtype(0), alpha)
        residual = residual - alpha * mvms
        result = result + alpha * p
        z = dinv * residual
        rz_new = np.sum(residual * z, axis=0, keepdims=True)
        zero = rz < eps
        beta = np.where(zero, dtype(0), rz_new / np.where(zero, dtype(1), rz))
        rz = rz_new
        p = p * beta + z
        alphas[k], betas[k] = alpha[0], beta[0]
        residual_norm = np.linalg.norm(residual, axis=0, keepdims=True)
        residual_norm = np.where(rhs_is_zero, dtype(0), residual_norm)
        has_converged = residual_norm < stop_updating_after
        k_done = k + 1
        if k >= min(10, max_iter - 1) and residual_norm.mean() < tolerance:
            break
    return result * rhs_norm, k_done, alphas, betas, residual_norm[0]


def jacobi_dinv(phi, noise, rows=None):
    """phi: scipy CSR (the engine's fp32 values, any dtype); rows: the selected rows (repeats allowed)."""
    phi = sp.csr_matrix(phi)
    rows = np.arange(phi.shape[0]) if rows is None else np.asarray(rows)
    out = np.ones(len(rows))
    for i, r in enumerate(rows):
        v = phi.data[phi.indptr[r]:phi.indptr[r + 1]].astype(np.float32).astype(np.float64)
        acc = 0.0
        for sq in v * v:                                # (exact products; one rounding per addition)
            acc += sq
        d = acc + float(noise)
        out[i] = 1.0 / d if d > 0.0 else 1.0
    return out


def estimate(Pt, Ms, y, noise, G, tolerance=1.0, max_iter=1000, dinv=None):
    """``mll_reference.estimate`` with the Jacobi preconditioner (dinv: another fixed positive diagonal's
    inverse).  G: the caller's probes (n x t).  Same dict."""
    Pt = sp.csr_matrix(Pt, dtype=np.float64)
    y = np.asarray(y, np.float64).ravel()
    G = np.asarray(G, np.float64)
    n, t = G.shape
    if dinv is None:
        dinv = 1.0 / (np.asarray(Pt.multiply(Pt).sum(axis=1)).ravel() + noise)
    sq = np.sqrt(dinv)[:, None]                          # D^-1/2
    Z = G / sq                                           # z_i = D^1/2 g_i
    rhs = np.concatenate([y[:, None], Z], axis=1)
    X, iters, al, be, _ = pcg_lanczos(R._khat_matmul(Pt, noise), rhs, dinv, tolerance=tolerance, max_iter=max_iter)
    a, U = X[:, 0], X[:, 1:]
    logdet = -float(np.sum(np.log(dinv))) + R.slq_logdet(al[:, 1:], be[:, 1:], iters, G)
    value = -0.5 * float(y @ a) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
    V = G * sq                                           # D^-1 z_i
    mm = R._khat_matmul(Pt, noise)
    w = pcg_lanczos(mm, a[:, None], dinv, tolerance=tolerance, max_iter=max_iter)[0][:, 0]
    aa = float(a @ a) + 2.0 * float(w @ (y - mm(a)))     # a.a to second order (see the module docstring)
    grad_noise = 0.5 * aa - 0.5 / t * float(np.sum(U * V))
    Wa, WU, WV = Pt.T @ a, Pt.T @ U, Pt.T @ V
    grad_f = np.zeros(len(Ms))
    for l, M in enumerate(Ms):
        M = sp.csr_matrix(M, dtype=np.float64)
        quad = float(a @ (M @ Wa))
        trace = float(np.sum(U * (M @ WV)) + np.sum(V * (M @ WU)))
        grad_f[l] = quad - 0.5 / t * trace
    return dict(value=value, grad_f=grad_f, grad_noise=grad_noise, logdet=logdet, iters=iters, alpha=al, beta=be,
                X=X)


CORA_F = [1.0, -0.5, 0.125, -1.0 / 48.0]                 # f_l = (-1)^l / (2^l l!), l < 4


def cora_phi(golden):
    """Phi = sum_{l<4} f_l M_l on the golden Cora m16 step matrices (fp32 values widened), all 2708 rows."""
    from golden_util import csr
    d = golden("cora")
    n = int(d["n"]) if "n" in d.files else len(d["m16_l0_indptr"]) - 1
    return R.phi_from_steps([csr(d, f"m16_l{l}", n) for l in range(4)], CORA_F)


def moments(Pm, train, test, y, noise, tolerance=1e-2, max_iter=1000, full_cov=False):
    """``posterior_reference.moments`` with every solve (alpha and each chunk of <= 256 test nodes) preconditioned
    by the one Jacobi diagonal of K^: the same dict.  Pm: scipy sparse or dense Phi."""
    import posterior_reference as PO
    train, test = np.asarray(train, np.int64), np.asarray(test, np.int64)
    Pt = Pm[train]
    Px = PO._rows(Pm, test)
    n, ns = len(train), len(test)
    y = np.asarray(y, np.float64).ravel()
    Ptd = PO._rows(Pm, train)
    dinv = 1.0 / (np.sum(Ptd * Ptd, axis=1) + noise)

    def matmul(v):
        return Pt @ (Pt.T @ v) + noise * v

    alpha, it_alpha, _, _, _ = pcg_lanczos(matmul, y[:, None], dinv, tolerance=tolerance, max_iter=max_iter)
    alpha = alpha[:, 0]
    mean, var, prior = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    cov = np.zeros((ns, ns)) if full_cov else None
    B_all = np.zeros((n, ns))
    Xs, iters = [], []
    for c0 in range(0, ns, PO.CHUNK):
        c1 = min(c0 + PO.CHUNK, ns)
        E = Px[c0:c1].T
        prior[c0:c1] = np.sum(E * E, axis=0)
        B = np.asarray(Pt @ E)
        X, it, _, _, _ = pcg_lanczos(matmul, B, dinv, tolerance=tolerance, max_iter=max_iter)
        iters.append(it)
        var[c0:c1] = prior[c0:c1] - np.sum((2.0 * B - matmul(X)) * X, axis=0)
        mean[c0:c1] = B.T @ alpha
        B_all[:, c0:c1] = B
        Xs.append(X)
    if full_cov:
        for (c0, X) in zip(range(0, ns, PO.CHUNK), Xs):
            cov[:, c0:c0 + X.shape[1]] = Px @ Px[c0:c0 + X.shape[1]].T - B_all.T @ X
        cov = 0.5 * (cov + cov.T)
        cov[np.diag_indices(ns)] = var
    return dict(mean=mean, var=var, cov=cov, prior=prior, iters=iters, alpha_iters=it_alpha)
