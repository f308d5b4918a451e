"""numpy / scipy fp64 restatement of the walk polynomial operator (TEST INFRASTRUCTURE ONLY).

    Phi = p(G) = sum_{l < n_f} f_l G^l,  n_f = min(len(f), L),   K^ = Phi[T] Phi[T]^T + s2 I.

* :func:`horner` is the operator's Horner chain by the order rule of include/grf.h: every output element
  starts from +0.0, adds the row's products one entry at a time in the row's order, then the f_l X addend,
  then the noise addend.  numpy has no fused multiply-add, so products are rounded before they are added: on
  integer-valued inputs (every partial sum below 2^53) both are exact and the device result must be these
  bits; on real inputs :func:`horner` also returns the bound ``2 D 2^-53 sum|terms|`` per step (D = the row
  length + 2: its additions plus the folded scale, once for each side), propagated through the chain.
* :func:`dense_poly`, :func:`dense_khat`, :func:`dense_grad`: the same quantities from dense matrix powers.
* :func:`krylov_grad`: the gradient contraction as the device computes it (Krylov blocks of G^T).
* seeded case generators.
"""
import numpy as np
import scipy.sparse as sp

U53 = 2.0 ** -53


def n_terms(f, L):
    return min(len(f), int(L))


def _rows_product(A, X, Xabs_err):
    """(A X, |A| |X|, |A| err, row lengths): row sums accumulated one entry at a time in CSR order."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    ptr, idx, val = A.indptr, A.indices, A.data
    lens = np.diff(ptr)
    acc = np.zeros((n, X.shape[1]))
    mag = np.zeros_like(acc)
    err = np.zeros_like(acc)
    for j in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > j)
        e = ptr[rows] + j
        acc[rows] = acc[rows] + val[e, None] * X[idx[e]]
        mag[rows] += np.abs(val[e, None]) * np.abs(X[idx[e]])
        err[rows] += np.abs(val[e, None]) * Xabs_err[idx[e]]
    return acc, mag, err, lens


def scatter_rows(X, in_idx, n):
    """S^T X: the n-row block whose rows in_idx are X's rows, the others zero."""
    if in_idx is None:
        return np.asarray(X, np.float64)
    out = np.zeros((n, X.shape[1]))
    out[np.asarray(in_idx)] = X
    return out


def horner(A, f, L, X, in_idx=None, out_idx=None, P=None, noise=0.0, Xerr=None):
    """(Y, bound): Y = (p(A) S_in^T X)[out_idx] (+ noise P) by the order rule, and the error bound of a
    device result against it.  Xerr: a bound of the device's own error in X (a chain fed by a chain)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    f = np.asarray(f, np.float64).ravel()
    nf = n_terms(f, L)
    Xf = scatter_rows(np.asarray(X, np.float64), in_idx, n)
    H = None
    err0 = np.zeros_like(Xf) if Xerr is None else scatter_rows(np.asarray(Xerr, np.float64), in_idx, n)
    err = np.abs(f[nf - 1]) * err0
    for l in range(max(nf - 2, 0), -1, -1):
        if nf == 1:
            acc, mag, perr, lens = np.zeros_like(Xf), np.zeros_like(Xf), np.zeros_like(Xf), np.zeros(n, np.int64)
        elif H is None:
            acc, mag, perr, lens = _rows_product(A, f[nf - 1] * Xf, err)
        else:
            acc, mag, perr, lens = _rows_product(A, H, err)
        H = acc + f[l] * Xf
        mag = mag + np.abs(f[l]) * np.abs(Xf)
        err = perr + np.abs(f[l]) * err0 + 2.0 * (lens[:, None] + 2) * U53 * mag
    rows = np.arange(n) if out_idx is None else np.asarray(out_idx)
    Y, mag, err = H[rows], mag[rows], err[rows]
    if P is not None:
        Y = Y + noise * np.asarray(P, np.float64)
        err = err + 2.0 * U53 * np.abs(noise) * np.abs(P) * (np.diff(A.indptr)[rows][:, None] + 2)
    return Y, err


def dense_poly(G, f, L):
    """p(G) from numpy.linalg.matrix_power."""
    Gd = sp.csr_matrix(G, dtype=np.float64).toarray()
    f = np.asarray(f, np.float64).ravel()
    return sum(f[l] * np.linalg.matrix_power(Gd, l) for l in range(n_terms(f, L)))


def dense_khat(G, f, L, T, noise):
    Pt = dense_poly(G, f, L)[np.asarray(T)]
    return Pt @ Pt.T + noise * np.eye(len(T))


def dense_grad(G, f, L, T, A, B, wt):
    """out[l] = sum_c wt[c] a_c^T (G^l[T] Phi[T]^T + Phi[T] G^l[T]^T) b_c."""
    Gd = sp.csr_matrix(G, dtype=np.float64).toarray()
    T = np.asarray(T)
    Pt = dense_poly(G, f, L)[T]
    out = np.zeros(n_terms(f, L))
    for l in range(out.size):
        Ml = np.linalg.matrix_power(Gd, l)[T]
        dK = Ml @ Pt.T + Pt @ Ml.T
        out[l] = float(np.sum(np.asarray(wt) * np.sum(A * (dK @ B), axis=0)))
    return out


def krylov_grad(G, f, L, T, A, B, wt):
    """(out, bound, mag): out[l] = sum_c wt[c] (<U_l, W_B> + <V_l, W_A>)[c] with U_l = (G^T)^l S_T^T A,
    V_l = (G^T)^l S_T^T B, W_A = p(G^T) S_T^T A, W_B likewise -- the device's algorithm; the bound is
    2 D 2^-53 sum|terms| of every sum involved, mag the largest sum|terms| of the final sums (integer cases
    assert it stays below 2^53: every partial sum is then exact in any order)."""
    Gt = sp.csr_matrix(sp.csr_matrix(G, dtype=np.float64).T)
    Gt.sort_indices()
    n = Gt.shape[0]
    nf = n_terms(f, L)
    wt = np.asarray(wt, np.float64)
    WA, eA = horner(Gt, f, L, A, in_idx=T)
    WB, eB = horner(Gt, f, L, B, in_idx=T)
    U, V = scatter_rows(A, T, n), scatter_rows(B, T, n)
    eU, eV = np.zeros_like(U), np.zeros_like(V)
    out, bound = np.zeros(nf), np.zeros(nf)
    mag_max = 0.0
    S = U.shape[1]
    for l in range(nf):
        if l:
            U, mU, pU, lens = _rows_product(Gt, U, eU)
            V, mV, pV, _ = _rows_product(Gt, V, eV)
            eU = pU + 2.0 * (lens[:, None] + 2) * U53 * mU
            eV = pV + 2.0 * (lens[:, None] + 2) * U53 * mV
        terms = wt * (U * WB + V * WA)
        out[l] = float(np.sum(terms))
        mag = np.abs(wt) * (np.abs(U) * np.abs(WB) + np.abs(V) * np.abs(WA))
        prop = np.abs(wt) * (eU * (np.abs(WB) + eB) + np.abs(U) * eB + eV * (np.abs(WA) + eA) + np.abs(V) * eA)
        bound[l] = float(np.sum(prop)) + 2.0 * (2 * n * S + 2) * U53 * float(np.sum(mag))
        mag_max = max(mag_max, float(np.sum(mag)))
    return out, bound, mag_max


# ------------------------------------------------------------------------------------ case generators
def directed_graph(n, seed, integer, long_rows=(0, 1, 63, 64, 65, 200), degree=3, weights=(-2.0, -1.0, 1.0, 2.0)):
    """A directed, weighted n x n CSR (sorted columns): rows of `degree` random entries, and -- where n allows --
    one row of each length in long_rows.  integer: weights drawn from `weights`; else uniform in +-[0.05, 0.25]."""
    r = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    special = {}
    if long_rows and n > max(long_rows):
        for q, ln in zip(r.choice(n, len(long_rows), replace=False), long_rows):
            special[int(q)] = ln
    for i in range(n):
        k = special.get(i, min(degree, n))
        c = np.sort(r.choice(n, k, replace=False))
        v = r.choice(list(weights), k) if integer else r.uniform(0.05, 0.25, k) * r.choice([-1.0, 1.0], k)
        rows += [i] * k
        cols += list(c)
        vals += list(v)
    G = sp.csr_matrix((vals, (rows, cols)), shape=(n, n), dtype=np.float64)
    G.sort_indices()
    return G


def modulator(n_f, seed, integer):
    r = np.random.default_rng(1000 + seed)
    if integer:
        return r.choice([-1.0, 1.0, 2.0], n_f)
    return r.uniform(0.3, 1.0, n_f) * r.choice([-1.0, 1.0], n_f) / np.arange(1, n_f + 1)


def block(n_rows, S, seed, integer):
    r = np.random.default_rng(2000 + seed)
    if integer:
        return r.integers(-2, 3, (n_rows, S)).astype(np.float64)
    return r.standard_normal((n_rows, S))


def abs_chain_max(G, f, L, X, in_idx=None):
    """max over the chain of sum|terms| (the integer cases assert it stays below 2^53)."""
    Y, _ = horner(abs(sp.csr_matrix(G)), np.abs(f), L, np.abs(X), in_idx=in_idx)
    return float(Y.max()) if Y.size else 0.0


def well_conditioned_system(n, n_sys, seed, n_f=4, noise=0.5):
    """(G, f, T, noise) with cond(K^) <= 5, asserted here: a weak directed G (|row sums| <= 0.15) under a
    modulator led by f_0 = 1, so Phi is a small perturbation of the identity."""
    G = directed_graph(n, seed, integer=False, long_rows=(0, 1, 63, 64, 65) if n > 65 else ())
    G = sp.csr_matrix(sp.diags(0.15 / np.maximum(np.asarray(abs(G).sum(1)).ravel(), 1e-300)) @ G)
    G.sort_indices()
    f = np.array([1.0, 0.5, -0.25, 0.125, 0.0625, -0.03, 0.015, 0.007])[:n_f]
    T = np.random.default_rng(3000 + seed).permutation(n)[:n_sys]  # (unsorted, like x_train.int())
    K = dense_khat(G, f, n_f, T, noise)
    cond = float(np.linalg.cond(K))
    assert cond <= 5.0, cond
    return G, f, T, noise
