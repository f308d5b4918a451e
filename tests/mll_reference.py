"""numpy fp64 restatement of the matrix-free marginal likelihood (TEST INFRASTRUCTURE ONLY).

    MLL(f, s2) = -1/2 y^T K^-1 y - 1/2 log det K^ - n/2 log 2 pi,   K^ = Phi_T Phi_T^T + s2 I,
    Phi = sum_l f_l M_l,  T = the training rows.

* :func:`cg_lanczos` is ``oracle.cg.linear_cg`` (the same operations in the same order) that also
  records every iteration's per-column alpha and beta.
* :func:`tridiagonal` / :func:`slq_logdet`: a column's Lanczos tridiagonal from its CG coefficients
  (T[k,k] = 1/alpha_k + beta_{k-1}/alpha_{k-1}, T[k,k+1] = sqrt(beta_k)/alpha_k over the iterations
  before its first zero alpha) and log det ~ (1/t) sum_i ||z_i||^2 sum_j V_i[0,j]^2 log lambda_ij.
* :func:`estimate`: value and gradients by gpytorch's estimators,
  1/2 a^T dK a - 1/(2t) sum_i u_i^T dK z_i with a = K^-1 y, u_i = K^-1 z_i, both from one CG solve.
* :func:`dense_truth`: the same quantities from the dense K^ (Cholesky log det, K^-1, exact traces).

Both take Phi_T and the M_l[T] as scipy matrices of fp64 values (the engine's fp32 values widened), so
they differ only by the estimator, never by the inputs.
"""
import numpy as np
import scipy.sparse as sp


def phi_from_steps(mats, f):
    """Phi = sum_l f_l M_l as the engine forms it: fp64 sums in step order, rounded once to fp32 (then
    widened back); f holds the modulator's fp32 values."""
    f = [float(np.float32(v)) for v in np.asarray(f).ravel()]
    phi = None
    for fl, M in zip(f, mats):
        term = sp.csr_matrix(M, dtype=np.float64) * fl
        phi = term if phi is None else phi + term
    phi = sp.csr_matrix(phi.astype(np.float32).astype(np.float64))
    phi.eliminate_zeros()
    return phi


def cg_lanczos(matmul, rhs, tolerance=1.0, eps=1e-10, stop_updating_after=1e-10, max_iter=1000):
    """(solution, iterations run, alpha [max_iter x S], beta [max_iter x S]); rows past the iterations
    run stay zero."""
    dtype = np.float64
    rhs = np.asarray(rhs, dtype)
    rhs_norm = np.linalg.norm(rhs, axis=0, keepdims=True).astype(dtype)
    rhs_is_zero = rhs_norm < eps
    rhs_norm = np.where(rhs_is_zero, dtype(1), rhs_norm)
    rhs = rhs / rhs_norm
    result = np.zeros_like(rhs)
    residual = rhs - matmul(result)
    residual_norm = np.linalg.norm(residual, axis=0, keepdims=True)
    has_converged = residual_norm < stop_updating_after
    n_iter = 0 if has_converged.all() else max_iter
    p = residual.copy()
    rr = np.sum(residual * residual, axis=0, keepdims=True)
    alphas = np.zeros((max_iter, rhs.shape[1]))
    betas = np.zeros((max_iter, rhs.shape[1]))
    k_done = 0
    for k in range(n_iter):
        mvms = matmul(p)
        pap = np.sum(p * mvms, axis=0, keepdims=True)
        zero = pap < eps
        alpha = np.where(zero, dtype(0), rr / np.where(zero, dtype(1), pap))
        alpha = np.where(has_converged, dtype(0), alpha)
        residual = residual - alpha * mvms
        result = result + alpha * p
        rr_new = np.sum(residual * residual, axis=0, keepdims=True)
        zero = rr < eps
        beta = np.where(zero, dtype(0), rr_new / np.where(zero, dtype(1), rr))
        rr = rr_new
        p = p * beta + residual
        alphas[k], betas[k] = alpha[0], beta[0]
        residual_norm = np.linalg.norm(residual, axis=0, keepdims=True)
        residual_norm = np.where(rhs_is_zero, dtype(0), residual_norm)
        has_converged = residual_norm < stop_updating_after
        k_done = k + 1
        if k >= min(10, max_iter - 1) and residual_norm.mean() < tolerance:
            break
    return result * rhs_norm, k_done, alphas, betas


def lanczos_length(alpha, iters):
    """Iterations before the column's first zero alpha, or the iterations run."""
    zero = np.flatnonzero(np.asarray(alpha)[:iters] == 0.0)
    return int(zero[0]) if zero.size else int(iters)


def tridiagonal(alpha, beta, iters):
    m = lanczos_length(alpha, iters)
    T = np.zeros((m, m))
    for k in range(m):
        T[k, k] = 1.0 / alpha[k] + (beta[k - 1] / alpha[k - 1] if k > 0 else 0.0)
        if k + 1 < m:
            T[k, k + 1] = T[k + 1, k] = np.sqrt(beta[k]) / alpha[k]
    return T


def slq_logdet(alphas, betas, iters, Z):
    """alphas / betas: the probe columns' coefficients [max_iter x t]; Z the probes [n x t]."""
    t = Z.shape[1]
    total = 0.0
    for c in range(t):
        T = tridiagonal(alphas[:, c], betas[:, c], iters)
        if T.shape[0] == 0:
            continue
        lam, V = np.linalg.eigh(T)
        total += float(Z[:, c] @ Z[:, c]) * float(np.sum(V[0] ** 2 * np.log(lam)))
    return total / t


def _khat_matmul(Pt, noise):
    return lambda v: Pt @ (Pt.T @ v) + noise * v


def estimate(Pt, Ms, y, noise, Z, tolerance=1.0, max_iter=1000):
    """The matrix-free estimate.  Pt = Phi[T] (n x N), Ms = [M_l[T]] (n x N each), Z = probes (n x t).
    Returns a dict: value, grad_f (L,), grad_noise, logdet, iters, alpha / beta ([max_iter x (1 + t)])."""
    Pt = sp.csr_matrix(Pt, dtype=np.float64)
    y = np.asarray(y, np.float64).ravel()
    Z = np.asarray(Z, np.float64)
    n, t = Z.shape
    rhs = np.concatenate([y[:, None], Z], axis=1)
    X, iters, al, be = cg_lanczos(_khat_matmul(Pt, noise), rhs, tolerance=tolerance, max_iter=max_iter)
    a, U = X[:, 0], X[:, 1:]
    logdet = slq_logdet(al[:, 1:], be[:, 1:], iters, Z)
    value = -0.5 * float(y @ a) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
    grad_noise = 0.5 * float(a @ a) - 0.5 / t * float(np.sum(U * Z))
    Wa, WU, WZ = Pt.T @ a, Pt.T @ U, Pt.T @ Z
    grad_f = np.zeros(len(Ms))
    for l, M in enumerate(Ms):
        M = sp.csr_matrix(M, dtype=np.float64)
        quad = float(a @ (M @ Wa))                                   # 1/2 a^T dK_l a = a^T M_l Phi_T^T a
        trace = float(np.sum(U * (M @ WZ)) + np.sum(Z * (M @ WU)))   # sum_i u_i^T dK_l z_i
        grad_f[l] = quad - 0.5 / t * trace
    return dict(value=value, grad_f=grad_f, grad_noise=grad_noise, logdet=logdet, iters=iters, alpha=al, beta=be,
                X=X)


def dense_truth(Pt, Ms, y, noise):
    """The exact value and gradients from the dense K^ (dict: value, grad_f, grad_noise, logdet)."""
    P = sp.csr_matrix(Pt, dtype=np.float64).toarray()
    y = np.asarray(y, np.float64).ravel()
    n = P.shape[0]
    K = P @ P.T + noise * np.eye(n)
    C = np.linalg.cholesky(K)
    logdet = 2.0 * float(np.sum(np.log(np.diag(C))))
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    a = np.linalg.solve(K, y)
    value = -0.5 * float(y @ a) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
    grad_noise = 0.5 * float(a @ a) - 0.5 * float(np.trace(Kinv))
    grad_f = np.zeros(len(Ms))
    for l, M in enumerate(Ms):
        Md = sp.csr_matrix(M, dtype=np.float64).toarray()
        dK = Md @ P.T + P @ Md.T
        grad_f[l] = 0.5 * float(a @ dK @ a) - 0.5 * float(np.sum(Kinv * dK))
    return dict(value=value, grad_f=grad_f, grad_noise=grad_noise, logdet=logdet)


def identity_probes(n):
    """Z = sqrt(n) I: the Hutchinson trace is exact, and SLQ is exact once Lanczos has run out."""
    return np.sqrt(float(n)) * np.eye(n)
