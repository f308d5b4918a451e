"""CPU: the numpy references and case generators of tests/solver_reference.py.

* Every reference is pinned to a dense ``np.longdouble`` evaluation on its small cases: ``spmm_ref`` and
  ``frob_ref`` to ``(terms + 1) 2^-53 magnitude`` (the fp64 sums' own first-order bound; integer cases: equal),
  ``transpose_ref`` to the dense transpose (values, bit patterns, ascending positions, repeated rows).
* ``spmm_depth`` and ``frob_depth`` are checked against their closed forms at the lengths where a batch, a
  group or the grid stride turns over.
* For every integer case the largest magnitude sum is below 2^24 (SpMM, fp32 and fp64 alike) or 2^53
  (steps_frob): every partial sum of the kernels, in any order, is then an exact integer, which is what makes
  the bitwise assertions of tests/test_gpu_solver_kernels.py legitimate.
* Every generated case holds the rows the GPU tests rely on, so an edit to a generator cannot silently drop an
  edge; the tile widths the tiled case was built for are the ones ``spmm_tile_rows`` gives.
* CG conditioning: ``noise = max(1, ceil(sigma_max^2 / 4))`` bounds cond(K^) by 5, and on every CG case
  ``oracle.cg.linear_cg`` in fp64 agrees with itself in ``np.longdouble`` to 1e-12 (per-column max-norm
  relative) at every ``max_iter`` the GPU tests use, with equal iteration counts -- so the GPU tolerance of 1e-10
  sits two orders above this bound and (measured: at most 8e-15 here) four above the reference's own error.
"""
import numpy as np
import pytest

import feature_reference as R
import solver_reference as SR
from oracle import cg as OCG

LD = np.longdouble
U = 2.0 ** -53


def _dense(M):
    return M.toarray().astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("kind", R.KINDS)
def test_spmm_ref_against_long_double(kind):
    M = SR.edge_csr(kind, 300)
    D = _dense(M).astype(LD)
    for S in (1, 5, 65):
        X = SR.edge_dense((300, S), kind)
        Z = SR.edge_dense((7, S), kind, seed=1)
        for rows in (None, np.arange(SR.EDGE_ROWS)[::-1], R.selection(7, SR.EDGE_ROWS)):
            Y, mag = SR.spmm_ref(M, rows, X)
            sel = np.arange(SR.EDGE_ROWS) if rows is None else rows
            exact, amag = D[sel] @ X.astype(LD), np.abs(D[sel]) @ np.abs(X).astype(LD)
            assert np.allclose(mag, amag.astype(np.float64), rtol=1e-13, atol=0)
            lens = np.diff(M.indptr)[sel][:, None]
            if kind == "int":
                assert np.array_equal(Y, exact.astype(np.float64))
            else:
                assert np.all(np.abs(Y.astype(LD) - exact) <= (lens + 1) * U * mag)
        rows = R.selection(7, SR.EDGE_ROWS)
        Y, mag = SR.spmm_ref(M, rows, X, Z, -2.5)
        exact = D[rows] @ X.astype(LD) + LD(-2.5) * Z.astype(LD)
        lens = np.diff(M.indptr)[rows][:, None]
        assert np.all(np.abs(Y.astype(LD) - exact) <= (lens + 3) * U * mag + 1e-300)


def test_spmm_depth_closed_forms():
    for S, (SG, G) in ((1, (1, 64)), (2, (1, 64)), (3, (4, 16)), (11, (4, 16)), (12, (16, 4)), (47, (16, 4)),
                       (48, (64, 1)), (256, (64, 1))):
        assert SR.spmm_groups(S) == (SG, G)
        lg = int(np.log2(G))
        assert SR.spmm_depth(0, S) == lg
        for n in SR.EDGE_LENGTHS:
            batches = [64] * (n // 64) + ([n % 64] if n % 64 else [])
            assert SR.spmm_depth(n, S) == sum(-(-c // G) for c in batches) + lg
        assert SR.spmm_depth(200, S) == (200 if G == 1 else 3 * (64 // G) + -(-8 // G) + lg)


@pytest.mark.parametrize("n_cols", [256, 300, 4096])
def test_transpose_ref_against_dense(n_cols):
    M = SR.with_subnormal(SR.edge_csr("int", n_cols))
    D = _dense(M)
    for rows in (None, R.selection(40, SR.EDGE_ROWS), np.zeros(0, np.int64), np.array([16, 0, 0])):
        t_ptr, t_idx, t_val = SR.transpose_ref(M, rows, n_cols)
        sel = np.arange(SR.EDGE_ROWS) if rows is None else rows
        assert t_ptr.dtype == np.int64 and t_idx.dtype == np.int32 and t_val.dtype == np.uint32
        assert t_ptr.shape == (n_cols + 1,) and t_ptr[0] == 0 and t_ptr[-1] == t_idx.size == t_val.size
        assert t_ptr[-1] == int(np.diff(M.indptr)[sel].sum())
        T = np.zeros((n_cols, len(sel)))
        for c in range(n_cols):
            p = t_idx[t_ptr[c]:t_ptr[c + 1]]
            assert np.all(np.diff(p) > 0)                         # ascending positions, each once
            T[c, p] = t_val[t_ptr[c]:t_ptr[c + 1]].view(np.float32)
        assert np.array_equal(T, D[sel].T.reshape(n_cols, len(sel)))
    full = SR.transpose_ref(M, None, n_cols)[2]
    assert np.uint32(0x80000000) in full and np.uint32(0) in full  # the -0.0 and the 0.0, by their bits
    assert np.float32(1e-40).view(np.uint32) in full               # the subnormal
    rep = SR.transpose_ref(M, np.array([31, 31]), n_cols)          # a repeated row: positions 0 and 1 per column
    assert np.array_equal(rep[1], np.tile([0, 1], 200)) and np.array_equal(rep[2][0::2], rep[2][1::2])


def test_transpose_ref_single_column():
    M = R._csr_from_rows([{0: np.float32(2)}, {}, {0: np.float32(-3)}, {0: np.float32(5)}, {}], 1)
    t_ptr, t_idx, t_val = SR.transpose_ref(M, np.array([3, 1, 0, 0]), 1)
    assert t_ptr.tolist() == [0, 3] and t_idx.tolist() == [0, 2, 3]
    assert t_val.view(np.float32).tolist() == [5.0, 2.0, 2.0]


@pytest.mark.parametrize("kind", R.KINDS)
def test_frob_ref_against_long_double_and_integer_bounds(kind):
    for (L, S, n_sel, which) in SR.FROB_CASES:
        mats, rows, A, WA, B, WB, wt = SR.frob_case(L, S, n_sel, which, kind)
        out, mag = SR.frob_ref(mats, rows, A, WA, B, WB, wt)
        assert out.shape == mag.shape == (L,)
        if kind == "int":
            assert mag.max() < 2.0 ** 53 and all(np.all(x == np.rint(x)) for x in (A, WA, B, WB, wt))
            assert np.array_equal(out, np.rint(out))
        if n_sel > SR.FROB_ROWS:
            continue                                               # (the dense long double pass: small cases)
        sel = np.arange(n_sel) if rows is None else rows
        for l, M in enumerate(mats):
            D = _dense(M).astype(LD)[sel]
            exact = (((A.astype(LD) * (D @ WB.astype(LD)) + B.astype(LD) * (D @ WA.astype(LD))) @ wt.astype(LD))).sum()
            terms = int(np.diff(M.indptr).max()) + S + n_sel + 3
            assert abs(LD(out[l]) - exact) <= terms * U * mag[l], (L, S, n_sel, l)
            if kind == "int":
                assert out[l] == float(exact)
    assert np.abs(out).max() > 0


def test_frob_depth_closed_forms():
    assert SR.frob_depth(200, 1, 1) == 202 + 1 + 9 + 1
    assert SR.frob_depth(65, 5, 129) == 67 + 3 + 9 + 2
    assert SR.frob_depth(200, 2048, 256) == 202 + 4 + 9 + 512       # one row per wave
    assert SR.frob_depth(200, 2049, 256) == 202 + 8 + 9 + 512       # past 4 x 512: a wave's second row
    assert SR.frob_row_blocks(2049) == 512 and SR.frob_row_blocks(1) == 1


# -------------------------------------------------------------------------------------- edges are present
@pytest.mark.parametrize("n_cols", [256, 300, 4096])
def test_edge_csr_holds_its_edges(n_cols):
    for kind in R.KINDS:
        M = SR.edge_csr(kind, n_cols)
        lens = np.diff(M.indptr)
        assert M.shape == (SR.EDGE_ROWS, n_cols) and lens.tolist() == list(SR.EDGE_LENGTHS) * 2
        assert all(np.all(np.diff(M.indices[M.indptr[i]:M.indptr[i + 1]]) > 0) for i in range(SR.EDGE_ROWS))
        assert 0 in M.indices and n_cols - 1 in M.indices
        for i in range(17, SR.EDGE_ROWS):                           # both ends in one row
            row = M.indices[M.indptr[i]:M.indptr[i + 1]]
            assert row[-1] == n_cols - 1 and (lens[i] == 1 or row[0] == 0)
        for i in SR.EDGE_NO_FIRST_COLUMN:
            assert 0 not in M.indices[M.indptr[i]:M.indptr[i + 1]]
        assert set(lens[SR.EDGE_NO_FIRST_COLUMN]) == set(SR.EDGE_LENGTHS) - {1}
        bits = np.ascontiguousarray(M.data).view(np.uint32)
        if kind == "int":
            assert (bits == 0).sum() == 1 and (bits == 0x80000000).sum() == 1
            assert np.all(M.data == np.rint(M.data)) and np.abs(M.data).max() <= 4
        else:
            assert not np.any(M.data == 0)


@pytest.mark.parametrize("S", [1, 2, 3, 11, 12, 47, 48, 64, 65, 130, 256])
def test_spmm_integer_cases_stay_below_2_24(S):
    M = SR.edge_csr("int", 300)
    X = SR.edge_dense((300, S), "int")
    Y, mag = SR.spmm_ref(M, None, X)
    assert np.all(X == np.rint(X)) and mag.max() < 2.0 ** 24 and np.array_equal(Y, np.rint(Y))
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X) and np.abs(Y).max() > 0


def test_tiled_case_holds_its_structure():
    c = SR.tiled_cg_case()
    tw = SR.TILED_TW
    assert c.phi.shape == (tw + 52, 3 * tw + 1) and c.train.size == tw + 1 and c.S == 256 and c.B.shape == (tw + 1, 256)
    assert SR.cg_tiles(tw + 1, 3 * tw + 1, 256, 8) == (tw, 2, tw, 4)      # fp64: Phi_t^T 2 tiles, Phi_t 4
    assert SR.cg_tiles(tw + 1, 3 * tw + 1, 256, 4) == (0, 1, 2 * tw, 2)   # fp32: Phi_t 2 tiles
    assert np.array_equal(c.train[:6], np.arange(6)) and np.unique(c.train).size == c.train.size
    row = lambda i: c.phi.indices[c.phi.indptr[i]:c.phi.indptr[i + 1]]
    assert row(0).size == 0 and row(1).tolist() == [3 * tw]
    assert row(2).tolist() == [tw - 1, tw, 2 * tw - 1, 2 * tw, 3 * tw - 1, 3 * tw]
    assert row(3).size == 130 and row(3)[63] == tw - 1 and row(3)[64] == tw
    t4 = set((row(4) // tw).tolist())
    assert t4 == {0, 2, 3}
    assert row(5).size == 200 and set((row(5) // tw).tolist()) == {1}
    lens = np.diff(c.phi.indptr)
    assert set(lens[6:]) == set(SR.TILED_LENGTHS)
    Pt = c.phi[c.train]
    assert (np.bincount(Pt.indices, minlength=c.n_cols) == 0).sum() >= 64  # empty rows of Phi_t^T
    assert lens[c.train[tw]] > 0                                            # the one-row tile of Phi_t^T
    t_ptr, t_idx, _ = SR.transpose_ref(c.phi, c.train, c.n_cols)
    assert np.any(t_idx == tw) and np.diff(t_ptr)[SR.TILED_HUB] > 640       # and a column of many batches
    assert np.all(c.B[:, SR.ZERO_COLUMN] == 0) and np.all(np.abs(c.B).max(0)[[0, 2, 255]] > 0)


def test_small_cases_hold_their_rows():
    for n_sys, S in SR.small_cg_cases():
        c = SR.small_cg_case(n_sys, S)
        lens = np.diff(c.phi.indptr)[c.train]
        assert c.train.tolist() == list(range(n_sys, 0, -1)) and c.B.shape == (n_sys, S) and lens[-1] == 63
        if n_sys >= 64:
            assert set(lens) == set(R.ROW_LENGTHS)
        assert (S < 3) == bool(np.all(np.abs(c.B).max(0) > 0))
        assert S < 3 or not c.B[:, SR.ZERO_COLUMN].any()
        assert np.array_equal(c.B.astype(np.float32).astype(np.float64), c.B)


def test_workspace_restatement_matches_the_tiles():
    tw = SR.TILED_TW
    assert SR.spmm_tile_rows(3 * tw + 1, 256, 8) == tw and SR.spmm_tile_rows(tw + 1, 256, 8) == tw
    assert SR.spmm_tile_rows(tw, 256, 8) == 0 and SR.spmm_tile_rows(300, 1, 8) == 0
    assert SR.spmm_tile_rows(3000, 200, 8) == 0                     # (test_gpu_cg.py's largest solve is untiled)
    assert SR.spmm_tile_rows(1 << 24, 64, 4) == 1 << 20             # at most 16 tiles
    untiled = 4 * SR._al256(5 * 3 * 8) + SR._al256(300 * 3 * 8) + SR._al256(256 * 3 * 8) + 256 + 256
    assert SR.cg_workspace_bytes(5, 300, 3) == untiled


# ----------------------------------------------------------------------------------------- conditioning
def _check_conditioning(key, case, worst):
    Pt = case.phi[case.train]
    smax = SR.sigma_max(Pt)
    assert case.noise == max(1.0, np.ceil(smax ** 2 / 4.0)) and (case.noise + smax ** 2) / case.noise <= 5.0
    mm64, mmld = SR.khat_matmul(case), SR.khat_matmul(case, LD)
    for mi in SR.MAX_ITERS:
        X, it = OCG.linear_cg(mm64, case.B, max_iter=mi)
        Xl, itl = OCG.linear_cg(mmld, case.B.astype(LD), max_iter=mi, dtype=LD)
        assert Xl.dtype == LD and it == itl == mi
        rel = SR.column_rel(X, Xl.astype(np.float64))
        worst[0] = max(worst[0], rel)
        assert rel <= 1e-12, (key, mi, rel)
        Xc, itc, al, be = SR.cg_oracle(key, mi)                      # the recorded run is the same run
        assert itc == it and np.array_equal(Xc, X) and al.shape == be.shape == (mi, case.S)


@pytest.mark.parametrize("n_sys", SR.SMALL_N_SYS)
def test_small_cg_cases_are_well_conditioned_and_the_oracle_is_accurate(n_sys):
    worst = [0.0]
    for S in SR.SMALL_S:
        _check_conditioning(("small", n_sys, S), SR.small_cg_case(n_sys, S), worst)
    print(f"n_sys={n_sys}: fp64 oracle vs long double, worst per-column relative error {worst[0]:.1e}")


def test_tiled_cg_case_is_well_conditioned_and_the_oracle_is_accurate():
    worst = [0.0]
    _check_conditioning(("tiled",), SR.tiled_cg_case(), worst)
    print(f"tiled: fp64 oracle vs long double, worst per-column relative error {worst[0]:.1e}")
