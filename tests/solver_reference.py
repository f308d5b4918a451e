"""numpy restatements of the solver-side kernels (TEST INFRASTRUCTURE ONLY): grf_cg.hip's SpMM, CSR transpose
and CG, and grf_mll.hip's steps_frob.

References (plain numpy / scipy, fp64; no GPU, no torch):

* :func:`spmm_ref`: ``Y = M[rows] X (+ zc Z)`` with the sum of the terms' magnitudes; :func:`spmm_depth` the
  number of roundings a term of ``spmm_kernel`` passes through.
* :func:`transpose_ref`: ``grf_csr_transpose`` -- the selected rows' entries in position order, sorted stably by
  column, the fp32 values carried as bit patterns.
* :func:`frob_ref`: ``grf_steps_frob_f64`` with the sum of the terms' magnitudes; :func:`frob_depth` its depth.
* :func:`cg_oracle`: ``oracle.cg`` / ``mll_reference.cg_lanczos`` on a :class:`CgCase`.
* :func:`spmm_tile_rows` / :func:`cg_workspace_bytes`: the column-tile width and the CG workspace layout of
  grf_cg.hip restated, so a test can tell from ``grf_cg_workspace_bytes`` that the tiles it was built for are
  the tiles the library runs.

Case generators (seeded, cached): :func:`edge_csr`, :func:`small_cg_case` / :func:`small_cg_cases`,
:func:`tiled_cg_case`, :func:`frob_case`.  ``kind = "int"`` gives integers in [-4, 4] (every product and partial
sum is an integer far below 2^24, so any summation order gives the same fp32 / fp64 and the GPU comparison is
bitwise); ``kind = "real"`` gives standard normals rounded to fp32.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import feature_reference as R
import mll_reference as MR

KINDS = R.KINDS
EDGE_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
EDGE_ROWS = 2 * len(EDGE_LENGTHS)
TILE_BYTES = 8 << 20  # grf_cg.hip's default GRF_SPMM_TILE_BYTES


# ------------------------------------------------------------------------------------------------ SpMM
def _abs(M):
    A = M.copy().astype(np.float64)
    A.data = np.abs(A.data)
    return A


def _take(M, rows):
    return sp.csr_matrix(M, dtype=np.float64) if rows is None else sp.csr_matrix(M, dtype=np.float64)[np.asarray(rows)]


def spmm_ref(M, rows, X, Z=None, zc=0.0):
    """(Y, mag): Y = M[rows] X (+ zc Z) in fp64 and mag = |M[rows]| |X| (+ |zc| |Z|) (None rows: all)."""
    X = np.asarray(X, np.float64)
    Ms = _take(M, rows)
    Y, mag = Ms @ X, _abs(Ms) @ np.abs(X)
    if Z is not None:
        Y = Y + zc * np.asarray(Z, np.float64)
        mag = mag + abs(zc) * np.abs(np.asarray(Z, np.float64))
    return Y, mag


def spmm_groups(S):
    """(SG, G) of spmm_dispatch: SG lanes per column group, G = 64 / SG groups that split a row's entries."""
    SG = 64 if S >= 48 else 16 if S >= 12 else 4 if S >= 3 else 1
    return SG, 64 // SG


def spmm_depth(length, S):
    """The roundings a term of spmm_kernel's row sum passes through, at most.

    A row of ``length`` entries is read in batches of 64; in a batch of cnt entries group g takes the entries
    g, g + G, ... -- ceil(cnt / G) of them for the fullest group, every one a single fma into the group's
    accumulator (the product is not rounded on its own), and the accumulator is carried from batch to batch.
    The G accumulators are then added by a log2(G)-level xor tree.  So
        D = sum_batches ceil(cnt_b / G) + log2(G),
    which for S >= 48 (G = 1) is the row's length: one lane sums the whole row in sequence.  (The first fma
    adds to 0.0 and rounds only the product, so D overstates an entry's roundings by at most one.)"""
    _, G = spmm_groups(S)
    length = int(length)
    full, rest = divmod(length, 64)
    return full * (64 // G) + -(-rest // G) + int(np.log2(G))


# ------------------------------------------------------------------------------------------- transpose
def transpose_ref(M, rows, n_cols):
    """(t_ptr int64 [n_cols + 1], t_idx int32, t_val uint32 bit patterns) of (M[rows])^T: every column lists
    the selection positions that hold it in ascending order (a row selected twice is two positions)."""
    rows = np.arange(M.shape[0]) if rows is None else np.asarray(rows, np.int64)
    lens = np.diff(M.indptr)[rows] if rows.size else np.zeros(0, np.int64)
    pos = np.repeat(np.arange(rows.size), lens)
    ent = np.concatenate([np.arange(M.indptr[r], M.indptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)])
    ent = ent.astype(np.int64)
    col = np.asarray(M.indices)[ent]
    bits = np.ascontiguousarray(np.asarray(M.data, np.float32)).view(np.uint32)[ent]
    order = np.argsort(col, kind="stable")
    t_ptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n_cols), out=t_ptr[1:])
    return t_ptr, pos[order].astype(np.int32), bits[order]


def with_subnormal(M):
    """A copy of M whose last stored value is the fp32 subnormal 1e-40 (for the bit-exact transpose)."""
    M = M.copy()
    M.data[-1] = np.float32(1e-40)
    assert 0 < M.data[-1] < np.finfo(np.float32).tiny
    return M


# ------------------------------------------------------------------------------------------ steps_frob
def frob_ref(mats, rows, A, WA, B, WB, wt):
    """(out, mag) per step: out[l] = sum_c wt[c] sum_r (A[r,c] (M_l[rows[r]] WB)[c] + B[r,c] (M_l[rows[r]] WA)[c])
    and the same sum over the absolute values of every factor."""
    A, WA, B, WB, wt = (np.asarray(x, np.float64) for x in (A, WA, B, WB, wt))
    rows = np.arange(A.shape[0]) if rows is None else np.asarray(rows, np.int64)
    out, mag = np.zeros(len(mats)), np.zeros(len(mats))
    for l, M in enumerate(mats):
        M = sp.csr_matrix(M, dtype=np.float64)
        TA, TB = (M @ WA)[rows], (M @ WB)[rows]            # (per distinct row, then indexed)
        out[l] = float(((A * TB + B * TA) @ wt).sum())
        Ma = _abs(M)
        TA, TB = (Ma @ np.abs(WA))[rows], (Ma @ np.abs(WB))[rows]
        mag[l] = float(((np.abs(A) * TB + np.abs(B) * TA) @ np.abs(wt)).sum())
    return out, mag


def frob_row_blocks(n_sel):
    return max(1, min(-(-int(n_sel) // 4), 512))


def frob_depth(max_len, n_sel, S):
    """The roundings a term of steps_frob_kernel passes through, at most.

    An entry's term is s = fma(v, fma(a, xb, b * xa), s): the product b * xa, the inner fma and the outer fma
    round once each -- three roundings, the last of which is the first of the row's sequential sum; the row's
    later entries (up to max_len - 1) add one each: max_len + 2.  acc = fma(wgt_i, s_i, acc) over the lane's
    NC = ceil(S / 64) column chunks and the wave's rows in sequence (a wave takes ceil(n_sel / (4 nb)) rows,
    nb = min(ceil(n_sel / 4), 512) blocks): NC ceil(n_sel / (4 nb)).  Then the 6-level xor tree, three adds
    for the four waves, and the last block's sum of the nb partials in block order: 6 + 3 + nb."""
    nb = frob_row_blocks(n_sel)
    nc = -(-int(S) // 64)
    rows_per_wave = -(-int(n_sel) // (4 * nb))
    return int(max_len) + 2 + nc * rows_per_wave + 6 + 3 + nb


# ------------------------------------------------------------------------------ tiles and CG workspace
def _al256(x):
    return (int(x) + 255) & ~255


def spmm_tile_rows(n_in, S, elem, budget=TILE_BYTES):
    """grf_cg.hip's spmm_tile_rows: the X rows per column tile (a power of two), 0 = untiled."""
    if budget <= 0:
        return 0
    tw = 64
    while tw * 2 * S * elem <= budget:
        tw *= 2
    while -(-n_in // tw) > 16:
        tw *= 2
    return 0 if tw >= n_in else tw


def cg_tiles(n_sys, n_cols, S, elem):
    """(tw1, nt1, tw2, nt2): the tiles of Phi_t^T (over the n_sys rows of P) and of Phi_t (over the n_cols of W)."""
    tw1, tw2 = spmm_tile_rows(n_sys, S, elem), spmm_tile_rows(n_cols, S, elem)
    return tw1, (-(-n_sys // tw1) if tw1 else 1), tw2, (-(-n_cols // tw2) if tw2 else 1)


def cg_workspace_bytes(n_sys, n_cols, S):
    """grf_cg_workspace_bytes restated (the larger of the fp32 and the fp64 layout)."""
    def total(elem):
        tw1, nt1, tw2, nt2 = cg_tiles(n_sys, n_cols, S, elem)
        o = 4 * _al256(n_sys * S * elem) + _al256(n_cols * S * elem)
        o += _al256(256 * S * 8) + _al256(5 * S * 8) + _al256((2 * S + 8) * 4)
        o += _al256((nt1 + 1) * n_cols * 8) if tw1 else 0
        o += _al256((nt2 + 1) * n_sys * 8) if tw2 else 0
        return o
    return max(total(4), total(8))


# ---------------------------------------------------------------------------------------------- edge_csr
@functools.lru_cache(maxsize=None)
def edge_csr(kind, n_cols, seed=0):
    """EDGE_ROWS = 32 rows whose lengths cycle twice through EDGE_LENGTHS (they straddle every G = 1, 4, 16,
    64 and both unroll depths, 4 and 8, of spmm_kernel).  The first cycle's rows use the inner columns only,
    except row 1, whose one entry is in column 0; in the second cycle every row of two or more entries holds
    both the first and the last column and row 17's one entry is in the last column.  So rows 0 and 2..15
    (:data:`EDGE_NO_FIRST_COLUMN`) never hold column 0.  ``"int"``: row 3 stores a 0.0 and row 5 a -0.0.
    Needs n_cols >= 202."""
    if n_cols < 202:
        raise ValueError("edge_csr: n_cols >= 202")
    r = np.random.default_rng([seed, n_cols, KINDS.index(kind)])
    rows = []
    for i in range(EDGE_ROWS):
        n = EDGE_LENGTHS[i % len(EDGE_LENGTHS)]
        if i < len(EDGE_LENGTHS):
            cols = [0] if i == 1 else r.choice(np.arange(1, n_cols - 1), n, replace=False).tolist()
        elif n == 1:
            cols = [n_cols - 1]
        elif n >= 2:
            cols = [0, n_cols - 1] + r.choice(np.arange(1, n_cols - 1), n - 2, replace=False).tolist()
        else:
            cols = []
        rows.append(dict(zip(cols, R._values(r, kind, len(cols)))))
    if kind == "int":
        rows[3][min(rows[3])] = np.float32(0.0)
        rows[5][min(rows[5])] = np.float32(-0.0)
    return R._csr_from_rows(rows, n_cols)


EDGE_NO_FIRST_COLUMN = np.array([0] + list(range(2, len(EDGE_LENGTHS))))


def edge_dense(shape, kind, seed=0, dtype=np.float64):
    """A dense operand of the kind (fp32-representable values, zeros allowed)."""
    r = np.random.default_rng([seed, KINDS.index(kind)] + list(shape))
    return R._values(r, kind, shape, zeros=True).astype(dtype)


# ------------------------------------------------------------------------------------------------- CG
CgCase = namedtuple("CgCase", "phi train n_cols S noise B")
# phi: scipy CSR (fp32 values); train: the row map (int64); B: (len(train) x S) fp64 of fp32-representable values

SMALL_N_SYS = (1, 2, 3, 5, 64, 1025)
SMALL_S = (1, 3, 5, 85, 86, 255, 256)
SMALL_COLS = 300
ZERO_COLUMN = 1  # the zero rhs column of the cases with S >= 3
MAX_ITERS = (1, 2, 3, 4)


def sigma_max(P):
    """The largest singular value of a scipy matrix."""
    if min(P.shape) <= 512:
        return float(np.linalg.norm(P.toarray().astype(np.float64), 2)) if P.nnz else 0.0
    import scipy.sparse.linalg as spl
    return float(spl.svds(P.astype(np.float64), k=1, v0=np.ones(min(P.shape)), tol=1e-12,
                          return_singular_vectors=False)[0])


def cg_noise(Pt):
    """noise = max(1, ceil(sigma_max(Phi_T)^2 / 4)): the eigenvalues of K^ lie in [noise, 5 noise]."""
    return float(max(1.0, np.ceil(sigma_max(Pt) ** 2 / 4.0)))


def _rhs(r, n, S):
    B = r.standard_normal((n, S)).astype(np.float32).astype(np.float64)
    if S >= 3:
        B[:, ZERO_COLUMN] = 0.0
    return B


@functools.lru_cache(maxsize=None)
def small_cg_case(n_sys, S, seed=0):
    """Phi has n_sys + 2 rows of ROW_LENGTHS cycled (0, 1, 63, 64, 65, 200 entries; real values) over 300
    columns; the training rows are n_sys, n_sys - 1, ..., 1 (a descending row map that skips the first and the
    last row); one zero rhs column where S >= 3."""
    lengths = tuple(R.ROW_LENGTHS[(i + 1) % len(R.ROW_LENGTHS)] for i in range(n_sys + 2))  # (row 1 is not empty)
    phi = R.rows_case(lengths, SMALL_COLS, "real", seed=seed + 17)
    train = np.arange(n_sys, 0, -1).astype(np.int64)
    r = np.random.default_rng([seed, n_sys, S])
    return CgCase(phi, train, SMALL_COLS, S, cg_noise(phi[train]), _rhs(r, n_sys, S))


def small_cg_cases():
    return [(n, S) for n in SMALL_N_SYS for S in SMALL_S]


# the column tile of a 256-column fp64 solve at the default budget: spmm_tile_rows(., 256, 8) = 4096 (its loop
# doubles the width while the DOUBLED width still fits the budget, so a tile is 8 MiB of X, not 4)
TILED_S = 256
TILED_TW = 4096
TILED_ROWS, TILED_TRAIN, TILED_COLS = TILED_TW + 52, TILED_TW + 1, 3 * TILED_TW + 1
TILED_LENGTHS = (0, 1, 2, 7, 17, 63, 64, 65, 130, 200)
TILED_LEADING = 6
TILED_HUB = 10


def tiled_leading_rows(tw=TILED_TW):
    """The column sets of the six leading rows of tiled_cg_case."""
    return [
        [],                                                          # empty
        [3 * tw],                                                    # one entry, in the last column
        [tw - 1, tw, 2 * tw - 1, 2 * tw, 3 * tw - 1, 3 * tw],        # exactly on every tile edge
        list(range(tw - 64, tw + 66)),                               # 130: entry 63 ends tile 0, entry 64 starts tile 1
        [3, 77, tw - 2, 2 * tw + 1, 2 * tw + 500, 3 * tw - 1, 3 * tw],  # tiles 0, 2 and 3 only
        list(range(tw + 100, tw + 100 + 2 * R.LONG_ROW, 2)),         # 200 entries, all inside tile 1
    ]


@functools.lru_cache(maxsize=None)
def tiled_cg_case(seed=0):
    """The column-tiled solve: Phi has TILED_TW + 52 rows over 3 TILED_TW + 1 columns, TILED_TW + 1 training rows,
    S = 256.  With tw = spmm_tile_rows = 4096 for fp64 that is 4 tiles of Phi_t, the last one column wide, and 2
    tiles of Phi_t^T, the last one row wide; for fp32 (tw = 8192) 2 tiles of Phi_t and Phi_t^T untiled.  The six
    leading rows (tiled_leading_rows) are training positions 0..5; the other rows are random with lengths
    from TILED_LENGTHS, never use the 70 columns 5000..5069 (empty rows of Phi_t^T), and every fourth of two or
    more entries holds column TILED_HUB (a row of Phi_t^T of many 64-entry batches over both its tiles); position
    TILED_TW (the one-row tile of Phi_t^T) holds entries."""
    tw = TILED_TW
    r = np.random.default_rng([seed, tw])
    pool = np.setdiff1d(np.arange(TILED_COLS), np.arange(5000, 5070))
    rows = []
    for cols in tiled_leading_rows(tw):
        rows.append(dict(zip(cols, R._values(r, "real", len(cols)))))
    lens = r.choice(TILED_LENGTHS, TILED_ROWS - TILED_LEADING)
    for i, n in enumerate(lens):
        cols = r.choice(pool, int(n), replace=False).tolist()
        if i % 4 == 0 and n >= 2 and TILED_HUB not in cols:
            cols[0] = TILED_HUB                                      # (a column of about 900 entries of Phi_t)
        rows.append(dict(zip(cols, R._values(r, "real", len(cols)))))
    phi = R._csr_from_rows(rows, TILED_COLS)
    rest = TILED_LEADING + r.permutation(TILED_ROWS - TILED_LEADING)
    train = np.r_[np.arange(TILED_LEADING), rest][:TILED_TRAIN].astype(np.int64)
    if phi.indptr[train[tw] + 1] == phi.indptr[train[tw]]:           # (position tw must hold entries)
        j = next(j for j in range(TILED_LEADING, tw) if phi.indptr[train[j] + 1] - phi.indptr[train[j]] >= 63)
        train[[j, tw]] = train[[tw, j]]
    B = _rhs(np.random.default_rng([seed, 1]), TILED_TRAIN, TILED_S)
    return CgCase(phi, train, TILED_COLS, TILED_S, cg_noise(phi[train]), B)


def khat_matmul(case, dtype=np.float64):
    Pt = case.phi[case.train].astype(dtype)
    PtT = Pt.T.tocsr()
    noise = dtype(case.noise)
    return lambda v: Pt @ (PtT @ v) + noise * v


@functools.lru_cache(maxsize=None)
def _oracle(key, max_iter):
    case = small_cg_case(*key[1:]) if key[0] == "small" else tiled_cg_case()
    return MR.cg_lanczos(khat_matmul(case), case.B, max_iter=max_iter)


def cg_oracle(key, max_iter):
    """(X, iterations, alpha, beta) of mll_reference.cg_lanczos -- oracle.cg.linear_cg's operations with the
    coefficients recorded -- for ("small", n_sys, S) or ("tiled",), cached."""
    return _oracle(tuple(key), int(max_iter))


def column_rel(X, Xo):
    """max over the columns of max_r |X - Xo| / max_r |Xo| (columns that are zero in Xo must be zero in X)."""
    X, Xo = np.asarray(X, np.float64), np.asarray(Xo, np.float64)
    scale = np.abs(Xo).max(0)
    err = np.abs(X - Xo).max(0)
    if np.any(err[scale == 0] != 0):
        return np.inf
    return float((err[scale > 0] / scale[scale > 0]).max(initial=0.0))


# --------------------------------------------------------------------------------------------- frob_case
FROB_LENGTHS = (0, 1, 2, 63, 64, 65, R.LONG_ROW)
FROB_ROWS, FROB_COLS = 2 * len(FROB_LENGTHS), 300
# (L, S, n_sel, map): every L, S, n_sel and the NULL map at least once
FROB_CASES = ((1, 1, 1, "map"), (1, 63, 5, "map"), (5, 64, FROB_ROWS, "null"), (5, 65, 2049, "map"),
              (5, 128, 5, "map"), (5, 129, 1, "map"), (64, 192, 5, "map"), (5, 193, FROB_ROWS, "null"),
              (5, 256, 2049, "map"), (64, 64, 2049, "map"), (64, 256, 1, "map"))


@functools.lru_cache(maxsize=None)
def frob_steps(L, kind, seed=0):
    """L step matrices of 14 rows over 300 columns: row i of step l has FROB_LENGTHS[(i + l) % 7] entries (so
    every row is 0, 1, 2, 63, 64, 65 and 200 entries long in some step); with L >= 2 step L // 2 is empty."""
    mats = []
    for l in range(L):
        lengths = tuple(0 if (L >= 2 and l == L // 2) else FROB_LENGTHS[(i + l) % len(FROB_LENGTHS)]
                        for i in range(FROB_ROWS))
        mats.append(R.rows_case(lengths, FROB_COLS, kind, seed=seed + 100 + l))
    return mats


def frob_rows(n_sel, which):
    """The row map: None; [6] (200 entries in step 0); descending with repeats; a cycle with a repeat."""
    if which == "null":
        assert n_sel == FROB_ROWS
        return None
    if n_sel == 1:
        return np.array([6], np.int64)
    if n_sel == 5:
        return np.array([13, 6, 6, 3, 0], np.int64)
    rows = np.arange(n_sel, dtype=np.int64) % FROB_ROWS
    rows[1] = rows[0]
    return rows


@functools.lru_cache(maxsize=None)
def frob_case(L, S, n_sel, which, kind, seed=0):
    """(mats, rows, A, WA, B, WB, wt): A, B (n_sel x S), WA, WB (300 x S), wt (S,) of the kind (integers in
    [-4, 4], or normals rounded to fp32)."""
    r = np.random.default_rng([seed, L, S, n_sel, KINDS.index(kind)])
    gen = lambda shape: R._values(r, kind, shape, zeros=True).astype(np.float64)
    return (frob_steps(L, kind), frob_rows(n_sel, which), gen((n_sel, S)), gen((FROB_COLS, S)), gen((n_sel, S)),
            gen((FROB_COLS, S)), gen((S,)))
