"""numpy fp64 restatement of the exact posterior moments (TEST INFRASTRUCTURE ONLY).

For training nodes T, K = Phi Phi^T, K^ = K[T,T] + s2 I, alpha = K^-1 y and test nodes x_c with b_c = K[T, x_c]:

    mean_c = b_c^T alpha,   var_c = K[x_c, x_c] - b_c^T K^-1 b_c,   cov = K[x,x] - B^T K^-1 B.

* :func:`moments` is the chunked, matrix-free form the engine runs: alpha from one ``oracle.cg.linear_cg`` solve
  of y, then per chunk of <= 256 test nodes E = Phi[x]^T, B = Phi[T] E, one batched linear_cg solve X, and the
  column sums prior - sum X (2 B - K^ X) and B^T alpha; with ``full_cov`` cov[:, chunk] = Phi[x] E - B_all^T X,
  symmetrised as (C + C^T) / 2, its diagonal the variances.  The variance's quadratic form is the energy form
  x^T (2 b - K^ x) = b^T K^-1 b - ||x - x_k||^2_K: below b^T K^-1 b for any x, where b^T x alone is only while CG
  keeps its residual orthogonal to the Krylov space (it equals b^T K^-1 b - ||x - x_k||^2_K - x_k^T r_k).
* :func:`dense_truth` forms K^ and solves by Cholesky.

Phi is a scipy sparse matrix (the walk's Phi: the engine's fp32 values widened) or a dense array (the operator
path's p(G)); both functions see the same one, so they differ only by the solver.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import cg as OCG

CHUNK = 256


def _rows(P, idx):
    R = P[np.asarray(idx, np.int64)]
    return R.toarray() if sp.issparse(R) else np.asarray(R, np.float64)


def moments(P, train, test, y, noise, tolerance=1e-2, max_iter=1000, full_cov=False, add_noise=False, chunk=CHUNK):
    """dict: mean (n*,), var (n*,), cov (n* x n*, or None), prior (n*,), iters (one count per chunk)."""
    train, test = np.asarray(train, np.int64), np.asarray(test, np.int64)
    Pt = P[train]                                   # stays sparse when P is
    Px = _rows(P, test)
    n, ns = len(train), len(test)
    y = np.asarray(y, np.float64).ravel()

    def matmul(v):
        return Pt @ (Pt.T @ v) + noise * v

    alpha, it_alpha = OCG.linear_cg(matmul, y[:, None], tolerance=tolerance, max_iter=max_iter)
    alpha = alpha[:, 0]
    mean, var, prior = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    cov = np.zeros((ns, ns)) if full_cov else None
    B_all = np.zeros((n, ns))
    Xs, iters = [], []
    for c0 in range(0, ns, chunk):
        c1 = min(c0 + chunk, ns)
        E = Px[c0:c1].T                             # (N x S)
        prior[c0:c1] = np.sum(E * E, axis=0)
        B = np.asarray(Pt @ E)
        X, it = OCG.linear_cg(matmul, B, tolerance=tolerance, max_iter=max_iter)
        iters.append(it)
        var[c0:c1] = prior[c0:c1] - np.sum((2.0 * B - matmul(X)) * X, axis=0)
        mean[c0:c1] = B.T @ alpha
        B_all[:, c0:c1] = B
        Xs.append(X)
    if full_cov:
        for (c0, X) in zip(range(0, ns, chunk), Xs):
            c1 = c0 + X.shape[1]
            cov[:, c0:c1] = Px @ Px[c0:c1].T - B_all.T @ X
        cov = 0.5 * (cov + cov.T)
    if add_noise:
        var = var + noise
    if full_cov:
        cov[np.diag_indices(ns)] = var
    return dict(mean=mean, var=var, cov=cov, prior=prior, iters=iters, alpha_iters=it_alpha)


def dense_truth(P, train, test, y, noise):
    """dict: mean, var, cov, prior from the dense K^ (Cholesky)."""
    Pt, Px = _rows(P, train), _rows(P, test)
    y = np.asarray(y, np.float64).ravel()
    Khat = Pt @ Pt.T + noise * np.eye(len(Pt))
    B = Pt @ Px.T
    c = sla.cho_factor(Khat, lower=True)
    Kxx = Px @ Px.T
    cov = Kxx - B.T @ sla.cho_solve(c, B)
    cov = 0.5 * (cov + cov.T)
    return dict(mean=B.T @ sla.cho_solve(c, y), var=np.diag(cov).copy(), cov=cov, prior=np.diag(Kxx).copy(), B=B)


def stopped_solve_bounds(B, y, noise, tolerance, chunk=CHUNK):
    """What a solve that stopped by linear_cg's rule (mean normalised residual norm < tolerance) can be off by,
    from lambda_min(K^) >= s2 alone.  The y column is a batch of one, so ||r|| < tolerance ||y|| and
        |mean_c - truth| = |b_c^T K^-1 r| <= ||b_c|| tolerance ||y|| / s2.
    In a chunk of S columns each normalised residual is below S tolerance (their mean is below tolerance), so
        0 <= var_c - truth = r_c^T K^-1 r_c <= (S tolerance ||b_c||)^2 / s2.
    Returns (mean_bound, var_bound), one value per test node."""
    nb = np.linalg.norm(B, axis=0)
    S = np.array([min(chunk, B.shape[1] - chunk * (c // chunk)) for c in range(B.shape[1])], np.float64)
    return nb * tolerance * np.linalg.norm(y) / noise, (S * tolerance * nb) ** 2 / noise


def errors(got, truth, full_cov=False):
    """max |got - truth| relative to the largest prior variance, for mean, var (and cov)."""
    scale = float(np.max(truth["prior"])) if len(truth["prior"]) else 1.0
    out = {}
    for q in ("mean", "var") + (("cov",) if full_cov else ()):
        g, t = np.asarray(got[q], np.float64), np.asarray(truth[q], np.float64)
        out[q] = float(np.max(np.abs(g - t))) / scale if g.size else 0.0
    return out


def nlpd(y_true, y_mean, y_std):
    """The mean negative log density of y_true under N(y_mean, y_std^2): the quantity the reference's
    compute_nlpd returns (experiments/graph_bo/scripts/wind_experiment.py:319-324)."""
    z = (np.asarray(y_true, np.float64) - y_mean) / y_std
    return float(np.mean(0.5 * np.log(2.0 * np.pi * y_std * y_std) + 0.5 * z * z))


def identity_closed_form(f0, noise, train, test, y):
    """Phi = f0 I: var = f0^2 - f0^4 / (f0^2 + s2) and mean = f0^2 / (f0^2 + s2) y on training nodes, var = f0^2
    and mean = 0 elsewhere."""
    k = f0 * f0
    pos = {int(t): i for i, t in enumerate(np.asarray(train))}
    mean = np.array([k / (k + noise) * y[pos[int(x)]] if int(x) in pos else 0.0 for x in test])
    var = np.array([k - k * k / (k + noise) if int(x) in pos else k for x in test])
    return mean, var
