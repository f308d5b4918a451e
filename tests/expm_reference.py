"""A numpy restatement of grf_expm_sym_f64 (include/grf.h, "grf_expm_sym_f64", order rule) with its analytic
gradients, a truth from numpy.linalg.eigh, and the seeded cases the CPU and GPU tests share.

The restatement follows the entry step by step: the same s = max(0, ceil(log2 rho)), the same scaled matrix
X = RN(-beta 2^-s L), the same Horner recurrence on the degree-18 Taylor polynomial (H_18 = I + RN(1/18) X,
H_k = I + RN(1/k) (X H_{k+1}), 17 products), the same s squarings, and after every product the symmetric mode's
write-out (the upper triangle mirrored).  Only the order of the sums inside a product differs (numpy's matmul
against the matrix cores' k-tiles).

Measured error of the restatement against the eigh truth, max |E - truth| over the entries (E's entries lie in
[-1, 1]); the tests assert 10x these figures, for the restatement and for the device alike (MEASURED holds the
same numbers per case).  n = 300; "norm": rho = 2 beta, "comb": rho = beta ||L||_inf; s in brackets:

    graph / Laplacian     beta = 0.1     beta = 2       beta = 10      beta = 50      beta = 400
    er            norm    1.67e-15 [0]   7.77e-16 [2]   6.16e-17 [5]   4.77e-17 [7]   2.45e-16 [10]
    er            comb    7.77e-15 [3]   3.46e-15 [7]   1.72e-16 [9]   5.96e-16 [12]  3.63e-15 [15]
    star          norm    7.08e-15 [0]   1.10e-14 [2]   7.44e-15 [5]   2.01e-13 [7]   1.60e-12 [10]
    star          comb    8.50e-14 [6]   5.27e-13 [11]  4.73e-14 [13]  5.88e-14 [15]  4.54e-13 [18]
    ring_isolated norm    1.78e-15 [0]   9.99e-16 [2]   1.17e-15 [5]   8.62e-16 [7]   1.13e-15 [10]
    ring_isolated comb    2.00e-15 [0]   1.22e-15 [3]   1.30e-15 [6]   2.55e-15 [8]   2.84e-15 [11]
    weighted      norm    1.67e-15 [0]   6.94e-16 [2]   6.94e-17 [5]   1.39e-16 [7]   1.13e-15 [10]
    weighted      comb    2.78e-15 [4]   2.36e-16 [8]   6.72e-16 [10]  2.62e-15 [13]  2.02e-14 [16]

scipy.linalg.expm (the reference's own function) lies within the same figures of the truth (at most 1.0e-12, the
normalised star at beta = 400; the star's truth itself carries the eigensolver's error on a 299-fold eigenvalue).

Gradient error: the analytic gradients on the restatement's E against central differences of the truth, relative
to the sum of the absolute values of the gradient's terms (sigma_f^2 sum |G| |L| |E| for beta, 2 sigma_f sum |G| |E|
for sigma_f).  The figures (MEASURED_GRAD, at most 7.8e-11 / 4.9e-12) are those of the difference quotient
(h = 1e-5 relative: truncation ~ h^2, rounding ~ 2^-53 / h), not of the analytic side; 10x is asserted.
"""
import math

import numpy as np

DEGREE = 18
N = 300
BETAS = (0.1, 2.0, 10.0, 50.0, 400.0)
GRAPHS = ("er", "star", "ring_isolated", "weighted")


def squarings(rho: float) -> int:
    """grf_expm_squarings: max(0, ceil(log2 rho)), exactly."""
    if not math.isfinite(rho):
        return -1
    if not rho > 1.0:
        return 0
    m, e = math.frexp(rho)
    return e - 1 if m == 0.5 else e


def graph(name: str, n: int = N) -> np.ndarray:
    """Seeded symmetric adjacency matrices with a zero diagonal."""
    W = np.zeros((n, n))
    if name == "er":
        rng = np.random.default_rng(11)
        W = np.triu((rng.random((n, n)) < 0.03).astype(np.float64), 1)
    elif name == "star":
        W[0, 1:] = 1.0
    elif name == "ring_isolated":
        m = n - 5  # a ring, then five isolated nodes
        idx = np.arange(m)
        W[idx, (idx + 1) % m] = 1.0
        W = np.triu(W + W.T > 0, 1).astype(np.float64)
    elif name == "weighted":
        rng = np.random.default_rng(12)
        W = np.triu((rng.random((n, n)) < 0.05) * rng.uniform(0.1, 3.0, (n, n)), 1)
    else:
        raise KeyError(name)
    return W + W.T


def laplacian(W: np.ndarray, normalize: bool) -> np.ndarray:
    """graph_kernels/utils.py:22-26 (a degree-0 node keeps the row e_i) or D - W."""
    W = np.asarray(W, dtype=np.float64)
    deg = W.sum(axis=1)
    if not normalize:
        return np.diag(deg) - W
    d = np.zeros_like(deg)
    d[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return np.eye(W.shape[0]) - (d[:, None] * W) * d[None, :]


def rho_bound(W: np.ndarray, L: np.ndarray, beta: float, normalize: bool) -> float:
    """The Python layer's bound on the spectral radius of beta L."""
    if normalize and (np.asarray(W) >= 0).all():
        return 2.0 * beta
    return beta * float(np.abs(L).sum(axis=1).max())


def _sym(C: np.ndarray) -> np.ndarray:
    """The symmetric mode's write-out: entries j >= i kept, mirrored below."""
    U = np.triu(C)
    return U + np.triu(C, 1).T


def expm_restated(L: np.ndarray, beta: float, rho: float) -> np.ndarray:
    if not (math.isfinite(beta) and beta > 0 and math.isfinite(rho)):
        raise ValueError("beta must be positive and finite, rho finite")
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    s = squarings(rho)
    I = np.eye(n)
    X = math.ldexp(-beta, -s) * L
    H = (1.0 / DEGREE) * X + I
    for k in range(DEGREE - 1, 0, -1):
        H = _sym((1.0 / k) * (X @ H.T) + I)
    for _ in range(s):
        H = _sym(H @ H.T)
    return H


def product_count(rho: float) -> int:
    return DEGREE - 1 + squarings(rho)


def expm_truth(L: np.ndarray, beta: float) -> np.ndarray:
    lam, V = np.linalg.eigh(np.asarray(L, dtype=np.float64))
    return (V * np.exp(-beta * lam)[None, :]) @ V.T


def kernel_value(E: np.ndarray, sigma_f: float, x1, x2, G: np.ndarray) -> float:
    """<G, sigma_f^2 E[x1, x2]>"""
    return float(sigma_f ** 2 * (G * E[np.ix_(x1, x2)]).sum())


def kernel_grads(L: np.ndarray, E: np.ndarray, sigma_f: float, x1, x2, G: np.ndarray):
    """(d/dbeta, d/dsigma_f, scale_beta, scale_sigma) of <G, sigma_f^2 E[x1, x2]>:
    d/dbeta = -sigma_f^2 <G, (L E)[x1, x2]> (E is symmetric: E[:, x2] = E[x2, :]^T), d/dsigma_f = 2 sigma_f <G, E[x1, x2]>;
    the scales are the sums of the absolute values of the terms."""
    LE = L[x1, :] @ E[x2, :].T
    d_beta = -sigma_f ** 2 * float((G * LE).sum())
    d_sigma = 2.0 * sigma_f * float((G * E[np.ix_(x1, x2)]).sum())
    scale_beta = sigma_f ** 2 * float((np.abs(G) * (np.abs(L[x1, :]) @ np.abs(E[x2, :]).T)).sum())
    scale_sigma = 2.0 * sigma_f * float((np.abs(G) * np.abs(E[np.ix_(x1, x2)])).sum())
    return d_beta, d_sigma, scale_beta, scale_sigma


def cases():
    """(key, graph name, normalize, beta) of every forward case."""
    for g in GRAPHS:
        for normalize in (True, False):
            for beta in BETAS:
                yield f"{g}-{'norm' if normalize else 'comb'}-{beta:g}", g, normalize, beta


GRAD_BETAS = (0.1, 2.0)
GRAD_SIGMA = 1.3


def grad_cases():
    for g in GRAPHS:
        for normalize in (True, False):
            for beta in GRAD_BETAS:
                yield f"{g}-{'norm' if normalize else 'comb'}-{beta:g}", g, normalize, beta


def grad_inputs(n: int = N):
    """Seeded x1 (with repeats), x2 (unsorted, != x1) and cotangent G."""
    rng = np.random.default_rng(13)
    x1 = rng.integers(0, n, 37)
    x1[5] = x1[0]
    x2 = rng.permutation(n)[:23]
    x2[7] = x2[2]
    G = rng.standard_normal((x1.size, x2.size))
    return x1, x2, G


_cache = {}


def case_data(g: str, normalize: bool, beta: float):
    """(W, L, rho, truth) of a case; graphs, Laplacians and truths are computed once and shared (read-only)."""
    if (g, normalize) not in _cache:
        W = graph(g)
        L = laplacian(W, normalize)
        lam, V = np.linalg.eigh(L)
        for a in (W, L, lam, V):
            a.setflags(write=False)
        _cache[(g, normalize)] = (W, L, lam, V)
    W, L, lam, V = _cache[(g, normalize)]
    key = (g, normalize, beta)
    if key not in _cache:
        T = (V * np.exp(-beta * lam)[None, :]) @ V.T
        T.setflags(write=False)
        _cache[key] = T
    return W, L, rho_bound(W, L, beta, normalize), _cache[key]


def fd_grads(g: str, normalize: bool, beta: float, sigma_f: float, x1, x2, G):
    """Central differences of the truth's <G, sigma_f^2 E[x1, x2]> in beta and sigma_f (h = 1e-5 relative:
    truncation h^2 / 6 ~ 2e-11 relative, rounding 1e-16 / h ~ 1e-11)."""
    case_data(g, normalize, beta)
    _, _, lam, V = _cache[(g, normalize)]
    V1, V2 = V[x1, :], V[x2, :]

    def val(b, sg):
        return float(sg ** 2 * (G * ((V1 * np.exp(-b * lam)[None, :]) @ V2.T)).sum())

    hb, hs = 1e-5 * beta, 1e-5 * sigma_f
    return ((val(beta + hb, sigma_f) - val(beta - hb, sigma_f)) / (2 * hb),
            (val(beta, sigma_f + hs) - val(beta, sigma_f - hs)) / (2 * hs))


# max |restatement - truth| per forward case, measured by tests/test_expm_reference.py::test_print_measured
MEASURED = {
    "er-norm-0.1": 1.67e-15, "er-norm-2": 7.77e-16, "er-norm-10": 6.16e-17, "er-norm-50": 4.77e-17,
    "er-norm-400": 2.45e-16,
    "er-comb-0.1": 7.77e-15, "er-comb-2": 3.46e-15, "er-comb-10": 1.72e-16, "er-comb-50": 5.96e-16,
    "er-comb-400": 3.63e-15,
    "star-norm-0.1": 7.08e-15, "star-norm-2": 1.10e-14, "star-norm-10": 7.44e-15, "star-norm-50": 2.01e-13,
    "star-norm-400": 1.60e-12,
    "star-comb-0.1": 8.50e-14, "star-comb-2": 5.27e-13, "star-comb-10": 4.73e-14, "star-comb-50": 5.88e-14,
    "star-comb-400": 4.54e-13,
    "ring_isolated-norm-0.1": 1.78e-15, "ring_isolated-norm-2": 9.99e-16, "ring_isolated-norm-10": 1.17e-15,
    "ring_isolated-norm-50": 8.62e-16, "ring_isolated-norm-400": 1.13e-15,
    "ring_isolated-comb-0.1": 2.00e-15, "ring_isolated-comb-2": 1.22e-15, "ring_isolated-comb-10": 1.30e-15,
    "ring_isolated-comb-50": 2.55e-15, "ring_isolated-comb-400": 2.84e-15,
    "weighted-norm-0.1": 1.67e-15, "weighted-norm-2": 6.94e-16, "weighted-norm-10": 6.94e-17,
    "weighted-norm-50": 1.39e-16, "weighted-norm-400": 1.13e-15,
    "weighted-comb-0.1": 2.78e-15, "weighted-comb-2": 2.36e-16, "weighted-comb-10": 6.72e-16,
    "weighted-comb-50": 2.62e-15, "weighted-comb-400": 2.02e-14,
}
# (|analytic - central difference| / scale) per gradient case for (beta, sigma_f)
MEASURED_GRAD = {
    "er-norm-0.1": (5.25e-11, 4.93e-12), "er-norm-2": (3.16e-12, 5.76e-14),
    "er-comb-0.1": (7.54e-12, 7.94e-13), "er-comb-2": (7.25e-15, 1.23e-13),
    "star-norm-0.1": (7.77e-11, 3.76e-12), "star-norm-2": (6.52e-12, 2.25e-13),
    "star-comb-0.1": (5.46e-12, 3.41e-12), "star-comb-2": (3.93e-13, 8.71e-13),
    "ring_isolated-norm-0.1": (1.81e-11, 3.98e-12), "ring_isolated-norm-2": (3.61e-12, 1.66e-12),
    "ring_isolated-comb-0.1": (2.64e-12, 3.31e-12), "ring_isolated-comb-2": (7.16e-13, 7.72e-13),
    "weighted-norm-0.1": (5.30e-11, 3.54e-12), "weighted-norm-2": (4.33e-12, 7.74e-13),
    "weighted-comb-0.1": (3.17e-12, 9.56e-13), "weighted-comb-2": (6.02e-15, 9.68e-14),
}
