"""numpy restatements of the feature-algebra and dense-step kernels (TEST INFRASTRUCTURE ONLY).

References (plain numpy, fp64; no GPU, no torch.cuda):

* :func:`phi_steps_ref`: ``grf_phi_steps_csr_count / _fill`` -- per row and column the steps
  ``l < min(n_f, L)`` that hold the column, in ascending ``l``: ``acc = 0.0 + f_l v_l`` for the first, then
  ``acc = acc + f_l v_l`` (``v`` the fp32 value widened; one rounding per product and per sum), entries
  whose ``acc == 0.0`` dropped.  An explicit loop over the steps on a dense accumulator with a "touched"
  mask, so a row's pattern is ``touched & (acc != 0)``.
* :func:`dense_phi_ref`: ``grf_dense_steps_phi`` -- ``acc = 0.0; acc = acc + F[..., l] * f[l]``.
* :func:`rowdot_ref`, :func:`rows_dot_cols_ref`, :func:`dense_grad_ref`: the three contractions, each with
  the sum of the magnitudes of its terms (what a first-order rounding bound is relative to).

Case generators (seeded): :func:`steps_case`, :func:`steps_modulators`, :func:`rows_case`,
:func:`rowdot_case`, :func:`dense_case`.  ``kind = "int"`` gives integers in [-4, 4] (every product and
partial sum of the kernels is then an integer far below 2^53, so any summation order gives the same fp64
and the GPU comparison is bitwise); ``kind = "real"`` gives standard normals rounded to fp32.
"""
import functools

import numpy as np
import scipy.sparse as sp

KINDS = ("int", "real")
LONG_ROW = 200  # entries of the long rows (more than three trips of a 64-lane loop)


# ------------------------------------------------------------------------------------------ references
def _v64(M):
    """The matrix's values as the kernels read them: fp32, widened."""
    return np.asarray(M.data).astype(np.float32).astype(np.float64)


def phi_steps_ref(mats, f, n_f):
    """(indptr int64, indices int32, values fp64, values fp32) of Phi = sum_{l < min(n_f, L)} f_l M_l."""
    L = len(mats)
    Lf = min(int(n_f), L)
    n_rows, n_cols = mats[0].shape
    f = np.asarray(f, np.float64).ravel()
    acc = np.zeros((n_rows, n_cols), np.float64)
    touched = np.zeros((n_rows, n_cols), bool)
    for l in range(Lf):  # (a step holds a (row, column) at most once, so the indexed update is one sum each)
        M = mats[l]
        r = np.repeat(np.arange(n_rows), np.diff(M.indptr))
        c = M.indices
        acc[r, c] = acc[r, c] + f[l] * _v64(M)  # (0.0 + t for the entry's first step)
        touched[r, c] = True
    keep = touched & (acc != 0.0)
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(keep.sum(1), out=indptr[1:])
    idx = np.nonzero(keep)[1].astype(np.int32)  # (row-major: each row's columns ascending)
    val = acc[keep]
    return indptr, idx, val, val.astype(np.float32)


def dense_phi_ref(F, f):
    """Phi[i, j] = sum_l F[i, j, l] f_l, l ascending from acc = 0.0, one rounding per product and per sum."""
    F = np.asarray(F, np.float64)
    f = np.asarray(f, np.float64).ravel()
    acc = np.zeros(F.shape[:2], np.float64)
    for l in range(F.shape[2]):
        acc = acc + F[..., l] * f[l]
    return acc


def _row(M, r):
    s, e = M.indptr[r], M.indptr[r + 1]
    return M.indices[s:e], _v64(M)[s:e]


def rowdot_ref(A, rows_a, B, rows_b, n_pairs):
    """out[r] = A[rows_a[r]] . B[rows_b[r]] and sum |a||b| (None rows: the identity)."""
    out, mag = np.zeros(n_pairs), np.zeros(n_pairs)
    for r in range(n_pairs):
        ca, va = _row(A, r if rows_a is None else int(rows_a[r]))
        cb, vb = _row(B, r if rows_b is None else int(rows_b[r]))
        _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
        t = va[ia] * vb[ib]
        out[r], mag[r] = t.sum(), np.abs(t).sum()
    return out, mag


def rows_dot_cols_ref(M, rows, Z, n_sel):
    """out[r] = sum_e M[rows[r], e] Z[col_e, r] and sum |v||Z| (None rows: the identity)."""
    Z = np.asarray(Z, np.float64)
    out, mag = np.zeros(n_sel), np.zeros(n_sel)
    for r in range(n_sel):
        c, v = _row(M, r if rows is None else int(rows[r]))
        t = v * Z[c, r]
        out[r], mag[r] = t.sum(), np.abs(t).sum()
    return out, mag


def dense_grad_ref(F, Phi, G):
    """grad_l = <F_l, (G + G^T) Phi> and sum_ij |F_ijl| ((|G| + |G|^T) |Phi|)_ij."""
    F, Phi, G = (np.asarray(x, np.float64) for x in (F, Phi, G))
    H = (G + G.T) @ Phi
    Ha = (np.abs(G) + np.abs(G).T) @ np.abs(Phi)
    return np.einsum("ijl,ij->l", F, H), np.einsum("ijl,ij->l", np.abs(F), Ha)


def dense_grad_depth(n):
    """The summation depth of grf_dense_steps_grad: 1 (S = G + G^T) + n + 1 (the MFMA k-sum) + 1 + 16 (a
    lane's epilogue) + 6 (wave_sum) + 3 (the four waves) + ceil(nblk / 64) + 6 (the reduce kernel)."""
    nblk = (-(-n // 64)) ** 2
    return n + 34 + -(-nblk // 64)


def dot_depth(length):
    """csr_rowdot / csr_rows_dot_cols: ceil(len / 64) sums per lane + the 6-level xor tree."""
    return -(-int(length) // 64) + 6


# --------------------------------------------------------------------------------------------- values
def _values(r, kind, size, zeros=False):
    """fp32 values of the kind; no zeros unless asked."""
    if kind == "int":
        v = r.integers(-4, 5, size).astype(np.float32)
        if not zeros:
            v[v == 0] = r.choice(np.array([-4, -3, -2, -1, 1, 2, 3, 4], np.float32), int((v == 0).sum()))
        return v
    if kind != "real":
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    v = r.standard_normal(size).astype(np.float32)
    v[v == 0] = np.float32(1.0)
    return v


def _csr_from_rows(rows, n_cols):
    """rows: a list of {column: value} -> CSR with sorted columns, fp32 values, stored zeros kept."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    idx, val = [], []
    for i, row in enumerate(rows):
        cols = sorted(row)
        idx.extend(cols)
        val.extend(row[c] for c in cols)
        indptr[i + 1] = len(idx)
    M = sp.csr_matrix((np.asarray(val, np.float32), np.asarray(idx, np.int32), indptr), shape=(len(rows), n_cols))
    M.has_sorted_indices = True
    return M


# ---------------------------------------------------------------------------------------- step matrices
STEP_ROWS, STEP_COLS, STEP_LS = (1, 3, 4, 5, 257), 300, (1, 2, 5, 63, 64)


@functools.lru_cache(maxsize=None)
def steps_case(n_rows, n_cols, L, kind, seed=0, empty_step=False, stored_zero=True):
    """L step matrices (scipy CSR, fp32 values, sorted duplicate-free columns).

    Row 0 is the rich row.  Step 0 holds ``LONG_ROW`` entries of it, the first and the last column among
    them; column 7 is held by every step (a full ballot); step l alone holds column 100 + l (disjoint
    columns); steps 0 and 1, and no other, hold column 9 with the same value (they cancel under
    f = (1, -1, ...)); with ``stored_zero`` the last step stores a 0.0 at column 11.  Row 1 is empty in
    every step; row 2 is held by one step only (the last).  The rows after them are random: up to 12
    entries per step out of a pool of 40 columns (so columns meet), and every 64th also has ``LONG_ROW``
    entries in step ``(row // 64) % L`` (the next one if that is the empty step).  ``empty_step`` (L >= 2):
    step ``L // 2`` has nnz = 0, so the full ballot is of the other steps, and with L = 2 the cancelling
    pair and the stored zero are absent.  Needs n_cols >= 280."""
    if n_cols < 280 or L > 64 or (empty_step and L < 2):
        raise ValueError("steps_case: n_cols >= 280, L <= 64, empty_step needs L >= 2")
    r = np.random.default_rng([seed, n_rows, n_cols, L, KINDS.index(kind), int(empty_step)])
    hole = L // 2 if empty_step else -1
    rows = [[dict() for _ in range(n_rows)] for _ in range(L)]

    def put(l, row, cols):
        if l == hole:
            return
        cols = np.asarray(cols).ravel()
        for c, v in zip(cols, _values(r, kind, cols.size)):
            rows[l][row][int(c)] = v

    # row 0: columns 0, 7, 9, 11, 100 .. 163 and n_cols - 1 are placed by hand, the rest of the long row at random
    free = np.setdiff1d(np.arange(1, n_cols - 1), np.r_[7, 9, 11, np.arange(100, 164)])
    cancel = L >= 2 and hole != 1
    put(0, 0, np.r_[0, n_cols - 1, r.choice(free, LONG_ROW - 4 - int(cancel) - int(stored_zero and L == 1),
                                            replace=False)])
    for l in range(L):
        put(l, 0, [7, 100 + l])
    if cancel:
        put(0, 0, [9])
        rows[1][0][9] = rows[0][0][9]
    if stored_zero and L - 1 != hole:
        rows[L - 1][0][11] = np.float32(0.0)
    if n_rows > 2:  # (row 1 stays empty)
        put(L - 1 if L - 1 != hole else 0, 2, [0, 5, n_cols - 1])
    for row in range(3, n_rows):
        pool = r.choice(n_cols, 40, replace=False)
        for l in range(L):
            if r.random() < 0.6:
                put(l, row, r.choice(pool, int(r.integers(0, 13)), replace=False))
        if row % 64 == 3:
            ll = (row // 64) % L
            ll = (ll + 1) % L if ll == hole else ll
            rows[ll][row].clear()
            put(ll, row, r.choice(n_cols, LONG_ROW, replace=False))
    return [_csr_from_rows(rows[l], n_cols) for l in range(L)]


def steps_modulators(L, kind, seed=0):
    """Two modulators of length L: (1, -1, 0, random...) -- the cancelling pair and an f_l = 0 -- and a
    random one whose last entry is 0."""
    r = np.random.default_rng([seed, L, KINDS.index(kind)])

    def rand():
        return r.integers(-3, 4, L).astype(np.float64) if kind == "int" else r.standard_normal(L)

    fa, fb = rand(), rand()
    fa[:3] = [1.0, -1.0, 0.0][:L]
    fb[fb == 0] = 2.0
    fb[L - 1] = 0.0
    return fa, fb


# --------------------------------------------------------------------------------- rows of given lengths
ROW_LENGTHS = (0, 1, 63, 64, 65, LONG_ROW)


def rows_case(lengths, n_cols, kind, seed=0):
    """A CSR matrix whose row i has lengths[i] entries at random sorted columns."""
    r = np.random.default_rng([seed, len(lengths), n_cols, KINDS.index(kind)])
    rows = []
    for n in lengths:
        cols = r.choice(n_cols, int(n), replace=False)
        rows.append(dict(zip(cols.tolist(), _values(r, kind, int(n)))))
    return _csr_from_rows(rows, n_cols)


def dotcols_lengths(n_rows=131):
    """Row lengths of the rows_dot_cols matrix: 0, 64, 65 and LONG_ROW first, then 1, 63 and random ones."""
    r = np.random.default_rng(n_rows)
    return (0, 64, 65, LONG_ROW, 1, 63) + tuple(int(x) for x in r.integers(0, 90, n_rows - 6))


def selection(n_sel, n_rows=len(ROW_LENGTHS)):
    """n_sel row numbers in descending order with repeats; the last row (the longest of ROW_LENGTHS) first."""
    order = list(range(n_rows - 1, -1, -1))
    picks = [order[i % n_rows] for i in range(n_sel - 1)] + [order[0]]
    return np.sort(np.asarray(picks, np.int64))[::-1].copy()


ROWDOT_TEMPLATES = 7  # pair r of the matched rows has template r % 7 (rowdot_case)


def rowdot_case(n_cols, kind, seed=0, n_a=131, n_b=137):
    """(A, B, perm): two different CSR matrices of n_a and n_b rows and a map perm[i] (i < n_a) such that
    (A row i, B row perm[i]) is a pair of template i % 7; perm[i] = i for i < 7.  The templates:
    0 both long (130 and LONG_ROW entries, half of A's columns in B), 1 identical rows, 2 disjoint rows,
    3 A empty, 4 B empty, 5 a single common column, B's first, 6 a single common column, B's last.
    B's rows that pair with no A row are random."""
    r = np.random.default_rng([seed, n_cols, KINDS.index(kind), n_a, n_b])
    perm = np.r_[np.arange(7), 7 + r.permutation(n_a - 7)]

    def rnd(cols):
        cols = np.asarray(cols).ravel()
        return dict(zip(cols.tolist(), _values(r, kind, cols.size)))

    a_rows, b_rows = [None] * n_a, [None] * n_b
    for i in range(n_a):
        t = i % ROWDOT_TEMPLATES
        p = r.permutation(n_cols)
        if t == 0:
            ra, rb = rnd(p[:130]), rnd(np.r_[p[:65], p[130:130 + LONG_ROW - 65]])
        elif t == 1:
            ra = rnd(p[:int(r.integers(1, 90))])
            rb = dict(ra)
        elif t == 2:
            ra, rb = rnd(p[:70]), rnd(p[70:150])
        elif t == 3:
            ra, rb = {}, rnd(p[:20])
        elif t == 4:
            ra, rb = rnd(p[:20]), {}
        else:
            cb = np.sort(p[:66])
            common = cb[0] if t == 5 else cb[-1]
            others = np.setdiff1d(np.arange(n_cols), cb)
            ra, rb = rnd(np.r_[common, r.choice(others, 40, replace=False)]), rnd(cb)
        a_rows[i], b_rows[int(perm[i])] = ra, rb
    for j in range(n_b):
        if b_rows[j] is None:
            b_rows[j] = rnd(r.choice(n_cols, int(r.integers(0, 30)), replace=False))
    return _csr_from_rows(a_rows, n_cols), _csr_from_rows(b_rows, n_cols), perm


def dense_matrix(shape, kind, seed=0):
    """A dense fp32 matrix of the kind (the Z operand of rows_dot_cols)."""
    r = np.random.default_rng([seed, KINDS.index(kind)] + list(shape))
    return _values(r, kind, shape, zeros=True)


# ------------------------------------------------------------------------------------ dense step tensors
DENSE_NS, DENSE_LS = (1, 15, 17, 64, 65, 130), (1, 7, 8, 9, 17)


def dense_case(n, L, kind, seed=0):
    """(F (n, n, L) fp64 with about half its entries zero, f (L,), G (n, n) non-symmetric)."""
    r = np.random.default_rng([seed, n, L, KINDS.index(kind)])
    if kind == "int":
        F = r.integers(-4, 5, (n, n, L)).astype(np.float64)
        f = r.integers(-3, 4, L).astype(np.float64)
        G = r.integers(-4, 5, (n, n)).astype(np.float64)
    else:
        F, f, G = r.standard_normal((n, n, L)), r.standard_normal(L), r.standard_normal((n, n))
    F = F * (r.random((n, n, L)) < 0.5)
    f[f == 0] = 1.0
    if n > 1:
        G[0, n - 1], G[n - 1, 0] = 3.0, -2.0  # (never symmetric)
    return F, f, G


# ------------------------------------------------------------------------- the module surface's step set
def hub_steps_case(n=300, L=4, hubs=12, seed=0):
    """(mats, hub rows): L step matrices (n x n) with positive fp32 loads; ``hubs`` rows hold 130 to
    LONG_ROW entries in every step (out of one pool of LONG_ROW columns per row, so Phi's row stays within
    LONG_ROW), every other row 0 to 7 (every 25th none in any step)."""
    r = np.random.default_rng([seed, n, L, hubs])
    hub_rows = np.sort(r.choice(n, hubs, replace=False))
    pools = {int(h): r.choice(n, LONG_ROW, replace=False) for h in hub_rows}
    mats = []
    for _ in range(L):
        rows = []
        for i in range(n):
            if i in pools:
                cols = r.choice(pools[i], int(r.integers(130, LONG_ROW + 1)), replace=False)
            else:
                cols = r.choice(n, int(r.integers(0, 8)) if i % 25 != 1 else 0, replace=False)
            rows.append(dict(zip(cols.tolist(), r.uniform(0.05, 1.0, cols.size).astype(np.float32))))
        mats.append(_csr_from_rows(rows, n))
    return mats, hub_rows


def steps_cases():
    """Every (n_rows, L, kind, empty_step) the phi_steps tests run."""
    out = [(n, L, kind, False) for n in STEP_ROWS for L in STEP_LS for kind in KINDS]
    out += [(n, L, kind, True) for n in (5, 257) for L in STEP_LS if L >= 2 for kind in KINDS]
    return out
