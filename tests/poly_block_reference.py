"""numpy fp64 restatement of the walk operator's K blocks, diagonals and modulator gradients (TEST
INFRASTRUCTURE ONLY), on top of tests/poly_reference.py so that the order rule is stated once.

    Psi_i = p(G^T) S_i^T,   K[x1, x2] = Psi_1^T Psi_2,   diag K[x]_c = sum_r Psi[r, c]^2,
    d<g, K[x1, x2]>/df_l = sum_c <((G^T)^l S_1^T g)[:, c], Psi_2[:, c]> + sum_r <((G^T)^l S_2^T g^T)[:, r], Psi_1[:, r]>,
    d<g, diag K[x]>/df_l = 2 sum_c g_c <(G^T)^l e_{x_c}, Psi[:, c]>.

Every chain is :func:`poly_reference.horner` on the unit columns (an index list may repeat and be unsorted: an
entry is a column).  On integer-valued inputs with every sum|terms| below 2^53 all of it is exact in any order,
so the device must return these bits.  On real inputs each function also returns a bound of a device result
against it: the chains carry horner's ``2 D 2^-53 sum|terms|`` per step through both chains, and the column
reductions add the same form with D = :func:`reduction_depth`, the longest chain of additions in the kernels'
fixed-order reduction (a wave's rows, the xor tree, the four waves, the blocks, the column-block contributions).
"""
import numpy as np
import scipy.sparse as sp

import poly_reference as PR

U53 = PR.U53
KRYLOV_BLOCKS = 512   # csrc/grf_poly.hip kKrylovBlocks
MAX_COLS = 256        # the operator's column limit: one column block


def nodes(x, n):
    return np.arange(n) if x is None else np.asarray(x, np.int64).ravel()


def unit_columns(x, n):
    """S^T as a dense block: column c is e_{x[c]}."""
    x = nodes(x, n)
    E = np.zeros((n, x.size))
    E[x, np.arange(x.size)] = 1.0
    return E


def transpose(G):
    Gt = sp.csr_matrix(sp.csr_matrix(G, dtype=np.float64).T)
    Gt.sort_indices()
    return Gt


def reduction_depth(n, cols_per_lane=1, contributions=1):
    """The longest chain of additions one output of the kernels' reductions goes through: a wave's rows (times the
    columns a lane owns, when columns are summed too), 6 xor steps, 3 wave additions, the block partials and the
    column-block contributions."""
    blocks = max(1, min(-(-n // 4), KRYLOV_BLOCKS))
    return -(-n // (4 * blocks)) * cols_per_lane + 6 + 3 + blocks + contributions


def psi(G, f, L, x):
    """(Psi, bound): p(G^T) on the unit columns of x, all n rows."""
    n = G.shape[0]
    return PR.horner(transpose(G), f, L, unit_columns(x, n))


def kernel_block(G, f, L, x1=None, x2=None):
    """(K[x1, x2], bound): chain 1 with G^T from the unit columns of x2, chain 2 with G on the rows x1."""
    n = G.shape[0]
    W, eW = psi(G, f, L, x2)
    return PR.horner(G, f, L, W, out_idx=nodes(x1, n), Xerr=eW)


def kernel_diag(G, f, L, x=None):
    """(diag K[x], bound)."""
    n = G.shape[0]
    W, eW = psi(G, f, L, x)
    d = np.sum(W * W, axis=0)
    bound = np.sum(2.0 * np.abs(W) * eW + eW * eW, axis=0) + 2.0 * reduction_depth(n) * U53 * d
    return d, bound


def _krylov_half(G, f, L, U0, xb, eU0=None):
    """(out, bound, mag): out[l] = sum_c <(G^T)^l U0[:, c], Psi_b[:, c]> for the unit columns of xb.  eU0: a
    bound of the device's own error in U0."""
    Gt = transpose(G)
    n = Gt.shape[0]
    nf = PR.n_terms(f, L)
    W, eW = psi(G, f, L, xb)
    U, eU = U0, np.zeros_like(U0) if eU0 is None else eU0
    out, bound = np.zeros(nf), np.zeros(nf)
    mag_max = 0.0
    n_blocks = max(1, -(-U0.shape[1] // MAX_COLS))
    depth = reduction_depth(n, cols_per_lane=MAX_COLS // 64, contributions=2 * n_blocks)
    for l in range(nf):
        if l:
            U, mU, pU, lens = PR._rows_product(Gt, U, eU)
            eU = pU + 2.0 * (lens[:, None] + 2) * U53 * mU
        out[l] = float(np.sum(U * W))
        mag = float(np.sum(np.abs(U) * np.abs(W)))
        bound[l] = float(np.sum(eU * (np.abs(W) + eW) + np.abs(U) * eW)) + 2.0 * depth * U53 * mag
        mag_max = max(mag_max, mag)
    return out, bound, mag_max


def kernel_grad(G, f, L, g, x1=None, x2=None):
    """(out, bound, mag): the modulator gradient of <g, K[x1, x2]> as the device computes it; mag is the largest
    sum|terms| of the final sums (integer cases assert it stays below 2^53)."""
    n = G.shape[0]
    x1, x2 = nodes(x1, n), nodes(x2, n)
    g = np.asarray(g, np.float64)
    U1, A1 = np.zeros((n, x2.size)), np.zeros((n, x2.size))
    np.add.at(U1, x1, g)            # S_1^T g (repeated nodes add up)
    np.add.at(A1, x1, np.abs(g))
    U2, A2 = np.zeros((n, x1.size)), np.zeros((n, x1.size))
    np.add.at(U2, x2, g.T)          # S_2^T g^T
    np.add.at(A2, x2, np.abs(g.T))
    # a repeated node's cotangents are added in no fixed order, along both axes, before the kernel reads them
    m = 2.0 * (np.bincount(x1).max(initial=1) + np.bincount(x2).max(initial=1)) * U53
    a, ba, ma = _krylov_half(G, f, L, U1, x2, m * A1)
    b, bb, mb = _krylov_half(G, f, L, U2, x1, m * A2)
    return a + b, ba + bb + 2.0 * U53 * (np.abs(a) + np.abs(b)), ma + mb


def kernel_diag_grad(G, f, L, g, x=None):
    """(out, bound, mag): the modulator gradient of <g, diag K[x]>."""
    n = G.shape[0]
    x = nodes(x, n)
    U0 = unit_columns(x, n) * np.asarray(g, np.float64).ravel()[None, :]
    out, bound, mag = _krylov_half(G, f, L, U0, x)
    return 2.0 * out, 2.0 * bound, 2.0 * mag


# ------------------------------------------------------------------------------------ dense truth
def dense_block(G, f, L, x1=None, x2=None):
    """p(G)[x1] p(G)[x2]^T from numpy.linalg.matrix_power."""
    n = G.shape[0]
    P = PR.dense_poly(G, f, L)
    return P[nodes(x1, n)] @ P[nodes(x2, n)].T


def dense_grad(G, f, L, g, x1=None, x2=None):
    """out[l] = <g, G^l[x1] Phi[x2]^T + Phi[x1] G^l[x2]^T>."""
    n = G.shape[0]
    x1, x2 = nodes(x1, n), nodes(x2, n)
    Gd = sp.csr_matrix(G, dtype=np.float64).toarray()
    P = PR.dense_poly(G, f, L)
    out = np.zeros(PR.n_terms(f, L))
    for l in range(out.size):
        Ml = np.linalg.matrix_power(Gd, l)
        out[l] = float(np.sum(np.asarray(g) * (Ml[x1] @ P[x2].T + P[x1] @ Ml[x2].T)))
    return out


def dense_diag_grad(G, f, L, g, x=None):
    n = G.shape[0]
    x = nodes(x, n)
    Gd = sp.csr_matrix(G, dtype=np.float64).toarray()
    P = PR.dense_poly(G, f, L)
    return np.array([2.0 * float(np.sum(np.asarray(g).ravel() * np.sum(np.linalg.matrix_power(Gd, l)[x] * P[x], axis=1)))
                     for l in range(PR.n_terms(f, L))])


def index_list(n, count, seed):
    """`count` node indices in [0, n): unsorted, and with repeats whenever count > 1."""
    r = np.random.default_rng(4000 + seed)
    x = r.integers(0, n, count)
    if count > 1:
        x[-1] = x[0]
    return x.astype(np.int64)
