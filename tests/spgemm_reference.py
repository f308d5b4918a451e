"""numpy restatement of the device SpGEMM's result contract (include/grf.h grf_spgemm_csr_*), the chain of
exact step matrices built on it, and the seeded cases the CPU and GPU tests share.

The rule: row i's pattern is the union of the patterns of B's rows k over the stored entries (i, k) of A,
columns ascending, exact-zero sums kept; c_ij starts from +0.0 and adds RN(a_ik b_kj) one product at a time
in the order of A's row entries (ascending k), multiply and add rounded separately.  numpy's elementwise
``*`` and ``+`` on float64 arrays are exactly those two roundings (no fused multiply-add).
"""
import numpy as np
import scipy.sparse as sp


def _csr(M):
    M = sp.csr_matrix(M)
    return (np.asarray(M.indptr, np.int64), np.asarray(M.indices, np.int64), np.asarray(M.data, np.float64),
            M.shape)


def spgemm(A, B) -> sp.csr_matrix:
    """C = A B by the rule above (stored zeros kept: build, do not ``eliminate_zeros``)."""
    ap, ai, av, (n_rows, n_mid) = _csr(A)
    bp, bi, bv, (n_mid_b, n_cols) = _csr(B)
    assert n_mid == n_mid_b
    lens = bp[ai + 1] - bp[ai]                      # products of each A entry
    total = int(lens.sum())
    a_of = np.repeat(np.arange(len(ai)), lens)      # product -> A entry; products are in sequence order
    start = np.cumsum(lens) - lens
    b_of = bp[ai][a_of] + (np.arange(total) - start[a_of])
    row = np.repeat(np.arange(n_rows), np.diff(ap))[a_of]
    col = bi[b_of]
    prod = av[a_of] * bv[b_of]                      # RN(a_ik b_kj)
    order = np.argsort(row * np.int64(max(n_cols, 1)) + col, kind="stable")  # by (row, column), sequence kept
    row, col, prod = row[order], col[order], prod[order]
    head = np.ones(total, bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    first = np.flatnonzero(head)
    seg_len = np.diff(np.append(first, total))
    out = np.zeros(len(first))                      # +0.0
    for t in range(int(seg_len.max()) if len(first) else 0):
        live = seg_len > t
        out[live] = out[live] + prod[first[live] + t]
    ptr = np.zeros(n_rows + 1, np.int64)
    np.add.at(ptr, row[first] + 1, 1)
    ptr = np.cumsum(ptr)
    C = sp.csr_matrix((n_rows, n_cols))
    C.indptr, C.indices, C.data = ptr, col[first].astype(np.int32), out
    return C


def exact_steps(G, max_walk_length: int):
    """[I, G, G^2, ...] (max_walk_length matrices) chained as M_l = M_{l-1} G, the reference's
    compute_pstep_walk_matrix indexing (general_kernel_pofm.py:7-42)."""
    n = G.shape[0]
    M = sp.csr_matrix((np.ones(n), np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, n))
    out = [M]
    for _ in range(1, max_walk_length):
        M = spgemm(M, G)
        out.append(M)
    return out


def gamma(n: int) -> float:
    u = n * 2.0 ** -53
    return u / (1.0 - u)


def chain_bound(Ld: np.ndarray, l: int) -> np.ndarray:
    """Elementwise bound between two differently ordered fp64 evaluations of L^l (n x n):
    2 ((1 + gamma_n)^l - 1) (|L|^l)_ij."""
    n = Ld.shape[0]
    return 2.0 * ((1.0 + gamma(n)) ** l - 1.0) * np.linalg.matrix_power(np.abs(Ld), l)


def same_bits(C, R) -> bool:
    """Pattern equal and value bits identical (explicit zeros and their signs included)."""
    return (C.shape == R.shape and np.array_equal(np.asarray(C.indptr, np.int64), np.asarray(R.indptr, np.int64))
            and np.array_equal(np.asarray(C.indices, np.int64), np.asarray(R.indices, np.int64))
            and np.array_equal(np.asarray(C.data, np.float64).view(np.uint64),
                               np.asarray(R.data, np.float64).view(np.uint64)))


# ------------------------------------------------------------------------------------------- graphs
def grid_adjacency(rows: int, cols: int) -> sp.csr_matrix:
    idx = np.arange(rows * cols).reshape(rows, cols)
    e = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                        np.stack([idx[:-1].ravel(), idx[1:].ravel()])], axis=1)
    A = sp.coo_matrix((np.ones(e.shape[1]), (e[0], e[1])), shape=(rows * cols,) * 2)
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def er_adjacency(n: int, p: float, seed: int) -> sp.csr_matrix:
    rng = np.random.default_rng(seed)
    U = np.triu(rng.random((n, n)) < p, 1)
    A = sp.csr_matrix((U | U.T).astype(np.float64))
    A.sort_indices()
    return A


def normalized_laplacian(A) -> sp.csr_matrix:
    """I - D^-1/2 A D^-1/2 (isolated nodes: the diagonal 1 alone), sorted CSR."""
    A = sp.csr_matrix(A, dtype=np.float64)
    deg = np.asarray(A.sum(axis=1)).ravel()
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    L = (sp.identity(A.shape[0], format="csr") - sp.diags(dinv) @ A @ sp.diags(dinv)).tocsr()
    L.sort_indices()
    return L


# -------------------------------------------------------------------------------------------- cases
def csr_from_rows(rows, n_cols: int, rng, values="normal") -> sp.csr_matrix:
    """rows: per row either a length (that many random distinct columns) or an array of columns."""
    ptr, idx = [0], []
    for r in rows:
        cols = np.sort(rng.choice(n_cols, int(r), replace=False)) if np.isscalar(r) else np.sort(np.asarray(r))
        idx.append(cols.astype(np.int64))
        ptr.append(ptr[-1] + len(cols))
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    if values == "normal":
        val = rng.standard_normal(len(idx))
    else:  # small integers (zero included: a stored zero times a negative value is a -0.0 product)
        val = rng.integers(-2, 3, len(idx)).astype(np.float64)
    M = sp.csr_matrix((len(rows), n_cols))
    M.indptr, M.indices, M.data = np.asarray(ptr, np.int64), idx.astype(np.int32), val
    return M


A_LENS = (0, 1, 2, 63, 64, 65, 200)
B_LENS = (0, 1, 5, 64, 65, 1000)


def case_mixed(n_rows: int, seed: int = 0):
    """A rows of 0 ... 200 entries over B rows of 0 ... 1000 entries; rectangular (n_mid 300, n_cols 3000)."""
    rng = np.random.default_rng(seed)
    n_mid, n_cols = 300, 3000
    B = csr_from_rows([B_LENS[k % len(B_LENS)] for k in range(n_mid)], n_cols, rng)
    # (a single row: the 200-entry one; else the lengths in turn, from the row of 2)
    lens = [200] if n_rows == 1 else [A_LENS[(r + 2) % len(A_LENS)] for r in range(n_rows)]
    return csr_from_rows(lens, n_mid, rng), B


def case_thresholds(thresholds, seed: int = 1):
    """For every threshold T and d in (-1, 0, +1): one output row with T + d products (two B rows of random
    columns) and one with exactly T + d distinct columns (two B rows of disjoint ranges and a third inside
    the first's range, so sums have two terms).  Returns A, B and the (products, distinct) of each row."""
    rng = np.random.default_rng(seed)
    n_cols = max(thresholds) + 1500
    b_rows, a_rows, want = [], [], []
    for T in thresholds:
        for d in (-1, 0, 1):
            k = len(b_rows)
            b_rows += [T - 40, 40 + d]
            a_rows.append([k, k + 1])
            want.append(("products", T + d))
            k = len(b_rows)
            b_rows += [np.arange(T - 40), np.arange(T - 40, T + d), rng.choice(T - 40, 100, replace=False)]
            a_rows.append([k, k + 1, k + 2])
            want.append(("distinct", T + d))
    B = csr_from_rows(b_rows, n_cols, rng)
    A = csr_from_rows(a_rows, len(b_rows), rng)
    return A, B, want


def case_hub(seed: int = 2):
    """One output row far past one LDS accumulator at n_cols = 70 000 (80 B rows of 1000 entries: about
    48 000 distinct columns), beside four short rows."""
    rng = np.random.default_rng(seed)
    n_mid, n_cols = 120, 70000
    B = csr_from_rows([1000] * 80 + [5] * 40, n_cols, rng)
    A = csr_from_rows([2, np.arange(80), 0, 3, 1], n_mid, rng)
    return A, B


def case_full_overlap(seed: int = 3):
    """Every B row has the same 64-column pattern: distinct columns = 64 whatever the product count."""
    rng = np.random.default_rng(seed)
    n_mid, n_cols = 260, 500
    pat = np.sort(rng.choice(n_cols, 64, replace=False))
    B = csr_from_rows([pat] * n_mid, n_cols, rng)
    A = csr_from_rows([A_LENS[r % len(A_LENS)] for r in range(21)] + [16, 17], n_mid, rng)  # 16 x 64 = 1024
    return A, B


def case_no_overlap(seed: int = 4):
    """B's rows have disjoint column ranges (row k: columns 37 k ... 37 k + 36): distinct = products."""
    rng = np.random.default_rng(seed)
    n_mid = 220
    B = csr_from_rows([np.arange(37 * k, 37 * k + 37) for k in range(n_mid)], 37 * n_mid, rng)
    A = csr_from_rows([A_LENS[r % len(A_LENS)] for r in range(14)] + [27, 28, 110, 111], n_mid, rng)
    return A, B


def case_cancelling(seed: int = 5):
    """Small-integer values (zeros stored): exact cancellations (stored +0.0) and -0.0 products; a last row
    whose only products are -0.0 (the sum from +0.0 stays +0.0)."""
    rng = np.random.default_rng(seed)
    n_mid, n_cols = 90, 40
    B = csr_from_rows([int(x) for x in rng.integers(0, 30, n_mid - 1)] + [np.arange(6)], n_cols, rng, "int")
    B.data[B.indptr[-2]:] = 0.0
    A = csr_from_rows([int(x) for x in rng.integers(0, 70, 60)] + [[n_mid - 1]], n_mid, rng, "int")
    A.data[-1] = -1.0
    return A, B


def case_wide(seed: int = 6):
    """n_cols = 2^31 - 1 with the columns at the top of the range; ten large rows (more than the big path's
    smallest wave count) and three short ones."""
    rng = np.random.default_rng(seed)
    n_mid, n_cols = 40, 2 ** 31 - 1
    b_rows = [n_cols - 1 - np.sort(rng.choice(5000, 300 if k < 30 else 4, replace=False)) for k in range(n_mid)]
    B = csr_from_rows(b_rows, n_cols, rng)
    A = csr_from_rows([np.arange(r, r + 12) for r in range(10)] + [[30, 31], [39], []], n_mid, rng)
    return A, B
