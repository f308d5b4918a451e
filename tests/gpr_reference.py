"""numpy restatement of the dense exact GPR: the blocked fp64 Cholesky factorisation and triangular solves of
include/grf_dense_solve.h (grf_potrf_f64, grf_trsm_f64), the dense formulas of gpflow.models.GPR
(log_marginal_likelihood, its gradients in K and the noise, predict_f / predict_y), and an np.longdouble truth
for each.

The restatement follows the library's block structure (block edge NB, right-looking, the panel as right-hand
sides, the trailing update subtracted block step by block step; in a block the substitution recurrence with one
chain in ascending k).  The products of the updates use numpy's own summation order, which the bounds allow:
Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Thm 10.3 and Thm 8.5 hold for any order.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u)), all evaluated in np.longdouble:
    |A - L L^T| <= gamma_{n+1} |L| |L^T|     on the lower triangle   (factor_residual)
    |b - T x|   <= gamma_n |T| |x|           for T = L and T = L^T   (solve_residual)
Both are stated as comparisons (excess = lhs - rhs <= 0), never as quotients: zero entries occur.
"""
import numpy as np

NB = 128
U = np.longdouble(2.0) ** -53
LD = np.longdouble


def gamma(k):
    k = LD(k)
    return k * U / (LD(1) - k * U)


# ------------------------------------------------------------------ the fp64 restatement
def potf2(S):
    """The column recurrence on the b x b block S (lower triangle read): the lower factor L."""
    b = S.shape[0]
    L = np.zeros((b, b))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(b):
            s = np.zeros(b - j)
            p = 0.0
            for k in range(j):
                a = L[j, k]
                s = s + L[j:, k] * a
                p = p + a * a
            piv = np.sqrt(S[j, j] - p)
            L[j, j] = piv
            L[j + 1:, j] = (S[j + 1:, j] - s[1:]) / piv
    return L


def trsm_block(T, X, transposed):
    """Rows of X solve T x = b (T lower, b x b) or T^T x = b, by substitution in order (in a copy)."""
    X = X.copy()
    b = T.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        if not transposed:
            for i in range(b):
                s = np.zeros(X.shape[0])
                for k in range(i):
                    s = s + T[i, k] * X[:, k]
                X[:, i] = (X[:, i] - s) / T[i, i]
        else:
            for i in range(b - 1, -1, -1):
                s = np.zeros(X.shape[0])
                for k in range(i + 1, b):
                    s = s + T[k, i] * X[:, k]
                X[:, i] = (X[:, i] - s) / T[i, i]
    return X


def potrf(A, nb=NB):
    """(F, logdet, info) as grf_potrf_f64: F holds L below and L^T mirrored above."""
    n = A.shape[0]
    W = np.tril(A) + np.tril(A, -1).T
    F = np.zeros((n, n))
    logdet, info = 0.0, 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for j0 in range(0, n, nb):
            j1 = min(j0 + nb, n)
            L11 = potf2(W[j0:j1, j0:j1])
            F[j0:j1, j0:j1] = L11 + np.tril(L11, -1).T
            for r in range(j1 - j0):
                piv = L11[r, r]
                if info == 0 and not (piv > 0.0 and np.isfinite(piv)):
                    info = j0 + r + 1
                logdet = logdet + 2.0 * np.log(piv)
            if j1 == n:
                break
            L21 = trsm_block(L11, W[j1:, j0:j1], False)
            F[j1:, j0:j1] = L21
            F[j0:j1, j1:] = L21.T
            W[j1:, j1:] = -1.0 * (L21 @ L21.T) + W[j1:, j1:]
    return F, (np.nan if info else logdet), info


def trsm(F, B, transposed, nb=NB):
    """Rows of B solve L x = b or L^T x = b as grf_trsm_f64 (B: nrhs x n; a copy is returned)."""
    B = np.array(B, dtype=np.float64)
    n = F.shape[0]
    starts = list(range(0, n, nb))
    for j0 in (reversed(starts) if transposed else starts):
        j1 = min(j0 + nb, n)
        X = trsm_block(np.tril(F[j0:j1, j0:j1]), B[:, j0:j1], transposed)
        B[:, j0:j1] = X
        if transposed and j0 > 0:
            B[:, :j0] = -1.0 * (X @ F[:j0, j0:j1].T) + B[:, :j0]
        elif not transposed and j1 < n:
            B[:, j1:] = -1.0 * (X @ F[j1:, j0:j1].T) + B[:, j1:]
    return B


# ------------------------------------------------------------------ the longdouble truth
def potrf_truth(A):
    """The lower Cholesky factor of the symmetric matrix given by A's lower triangle, in np.longdouble."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def trsm_truth(L, B, transposed):
    """Rows of B solve L x = b / L^T x = b in np.longdouble."""
    L = np.asarray(L, dtype=LD)
    X = np.array(B, dtype=LD)
    n = L.shape[0]
    if not transposed:
        for i in range(n):
            X[:, i] = (X[:, i] - X[:, :i] @ L[i, :i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[:, i] = (X[:, i] - X[:, i + 1:] @ L[i + 1:, i]) / L[i, i]
    return X


# ------------------------------------------------------------------ the bounds, as comparisons
def factor_residual_excess(A, L):
    """max over the lower triangle of |A - L L^T| - gamma_{n+1} |L| |L^T| (<= 0: the bound holds)."""
    A, L = np.asarray(A, dtype=LD), np.tril(np.asarray(L, dtype=LD))
    n = A.shape[0]
    lhs = np.abs(A - L @ L.T)
    rhs = gamma(n + 1) * (np.abs(L) @ np.abs(L).T)
    low = np.tril(np.ones((n, n), dtype=bool))
    return (lhs - rhs)[low].max()


def solve_residual_excess(T, X, B):
    """max of |b - T x| - gamma_n |T| |x| over the rows (x, b) of (X, B); T is the triangular matrix itself."""
    T, X, B = np.asarray(T, dtype=LD), np.asarray(X, dtype=LD), np.asarray(B, dtype=LD)
    n = T.shape[0]
    lhs = np.abs(B - X @ T.T)
    rhs = gamma(n) * (np.abs(X) @ np.abs(T).T)
    return (lhs - rhs).max()


def logdet_ascending(F, dtype=np.float64):
    """2 sum_i log F_ii as grf_potrf_f64 states it: the terms RN(2 log F_ii) added in ascending i, in fp64 (the order
    and the roundings are the statement; in np.longdouble the same loop is the truth of the GPR formulas)."""
    s = dtype(0)
    for d in np.diag(np.asarray(F, dtype=dtype)):
        s = s + dtype(2) * np.log(d)
    return s


def spd_matrix(n, seed, density=0.05, shift=0.1):
    """A = Phi Phi^T + shift I with Phi a random `density`-dense n x 3n matrix (fp64, exactly symmetric)."""
    r = np.random.default_rng(seed)
    Phi = r.standard_normal((n, 3 * n)) * (r.random((n, 3 * n)) < density)
    A = Phi @ Phi.T
    A = np.tril(A) + np.tril(A, -1).T
    return A + shift * np.eye(n)


# ------------------------------------------------------------------ the dense GPR formulas
def _factor(Kh, dtype):
    if dtype is LD:
        L = potrf_truth(Kh)
        return L, logdet_ascending(L, LD), 0
    F, logdet, info = potrf(np.asarray(Kh, dtype=np.float64))
    return F, logdet, info


def _solve(L, B, transposed, dtype):
    return trsm_truth(L, B, transposed) if dtype is LD else trsm(L, B, transposed)


def gpr(K, noise, Y, Ksx=None, Kss=None, dtype=np.float64):
    """gpflow.models.GPR on a given K = K[X, X] (n x n), noise variance and Y (n x p), zero mean:
        lml, dK = dL/dK, dnoise = dL/dsigma^2, and with Ksx = K[X*, X] (n* x n) and Kss = K[X*, X*]:
        mean (n* x p), var (n*), cov (n* x n*) of predict_f (predict_y adds the noise to var / cov's diagonal).
    dtype np.float64: the library's algorithm (blocked factorisation, substitution); np.longdouble: the truth."""
    dt = LD if dtype in (LD, np.longdouble) else np.float64
    K, Y = np.asarray(K, dtype=dt), np.asarray(Y, dtype=dt)
    n, p = Y.shape
    Kh = K + dt(noise) * np.eye(n, dtype=dt)
    L, logdet, info = _factor(Kh, dt)
    alpha_t = _solve(L, _solve(L, Y.T, False, dt), True, dt)                      # p x n
    lml = -dt(0.5) * (Y.T * alpha_t).sum() - dt(0.5 * p) * logdet - dt(0.5 * n * p) * np.log(dt(8) * np.arctan(dt(1)))
    Kinv = _solve(L, _solve(L, np.eye(n, dtype=dt), False, dt), True, dt)
    Kinv = np.triu(Kinv) + np.triu(Kinv, 1).T                                       # (the product reads Z's upper half)
    dK = dt(0.5) * (alpha_t.T @ alpha_t) + dt(-0.5 * p) * Kinv
    out = dict(lml=lml, dK=dK, dnoise=np.trace(dK), info=info)
    if Ksx is not None:
        A = _solve(L, np.asarray(Ksx, dtype=dt), False, dt)                         # n* x n: rows L^-1 k_*
        V = _solve(L, Y.T, False, dt)                                               # p x n
        out["mean"] = A @ V.T
        if Kss is not None:
            Kss = np.asarray(Kss, dtype=dt)
            out["var"] = np.diag(Kss) - (A * A).sum(axis=1)
            out["cov"] = Kss - A @ A.T
    return out
