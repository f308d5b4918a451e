"""CPU: the numpy references and case generators of tests/feature_reference.py.

* Every reference is pinned to an independent formula on every generated case.
  - ``phi_steps_ref`` against ``sum_l f_l M_l`` formed densely in ``np.longdouble``.  Integer cases: equal.
    Real cases: compared in long double (so no second rounding enters), entry by entry, against the bound
    of the restated arithmetic itself: k steps meeting at an entry are k rounded products and k - 1 rounded
    sums, ``|ref - exact| <= (2k - 1) 2^-53 sum_l |f_l v_l|`` to first order (+ the long double sum's own
    2k eps_ld).  With one step that is half an ulp: the reference is the correctly rounded product.  (Two
    rounded products summed are NOT in general the rounded exact sum, so plain equality holds for one step
    and for the integer kind only.)  The pattern must be equal after dropping zeros.
  - the dot references against dense ``@``; ``dense_phi_ref`` against ``F @ f``; ``dense_grad_ref`` against
    the two traces ``<F_l, G Phi> + <F_l, G^T Phi>`` formed separately.
* For every integer case the largest magnitude sum is below 2^53: every partial sum of the kernels, in any
  order, is then an exact integer, which is what makes the bitwise assertions of
  tests/test_gpu_feature_kernels.py legitimate.
* Every generated case holds the rows the GPU tests rely on (a row longer than a wave, an empty row, a
  full-ballot column, a cancelling pair, ...), so an edit to a generator cannot silently drop an edge.
"""
import numpy as np
import pytest

import feature_reference as R

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
U = 2.0 ** -53


def _dense(M):
    return M.toarray().astype(np.float32).astype(np.float64)


def _pattern(M):
    """Stored entries (explicit zeros included) as a dense 0 / 1 array."""
    P = np.zeros(M.shape, np.int64)
    for r in range(M.shape[0]):
        P[r, M.indices[M.indptr[r]:M.indptr[r + 1]]] = 1
    return P


def _phi_dense(ref, shape):
    ptr, idx, v64, v32 = ref
    D = np.zeros(shape)
    for r in range(shape[0]):
        D[r, idx[ptr[r]:ptr[r + 1]]] = v64[ptr[r]:ptr[r + 1]]
    return D


# --------------------------------------------------------------------------------------- phi_steps_ref
@pytest.mark.parametrize("n_rows,L", [(n, L) for n in R.STEP_ROWS for L in R.STEP_LS])
def test_phi_steps_ref_against_long_double_sum(n_rows, L):
    for (n, l, kind, hole) in [c for c in R.steps_cases() if c[0] == n_rows and c[1] == L]:
        mats = R.steps_case(n, R.STEP_COLS, L, kind, empty_step=hole)
        dense = [_dense(M) for M in mats]
        pats = [_pattern(M) for M in mats]
        for f in R.steps_modulators(L, kind):
            for n_f in sorted({0, 1, L - 1, L}):
                ref = R.phi_steps_ref(mats, f, n_f)
                ptr, idx, v64, v32 = ref
                assert ptr.dtype == np.int64 and idx.dtype == np.int32 and v64.dtype == np.float64
                assert np.array_equal(v32, v64.astype(np.float32)) and not np.any(v64 == 0.0)
                assert all(np.all(np.diff(idx[ptr[r]:ptr[r + 1]]) > 0) for r in range(n))
                exact = np.zeros((n, R.STEP_COLS), LD)
                mag = np.zeros((n, R.STEP_COLS))
                k = np.zeros((n, R.STEP_COLS), np.int64)
                for l_ in range(min(n_f, L)):
                    exact += LD(f[l_]) * dense[l_].astype(LD)
                    mag += np.abs(f[l_]) * np.abs(dense[l_])
                    k += pats[l_]
                got = _phi_dense(ref, exact.shape)
                assert np.array_equal(got != 0, exact != 0), (kind, hole, n_f)
                if kind == "int":
                    assert np.array_equal(got, exact.astype(np.float64)), (kind, hole, n_f)
                    assert mag.max(initial=0.0) < 2.0 ** 53
                else:
                    err = np.abs(got.astype(LD) - exact).astype(np.float64)
                    bound = ((2 * k - 1).clip(0) * U * (1 + 2.0 ** -50) + 2 * k * EPS_LD) * mag
                    assert np.all(err <= bound), (kind, hole, n_f, float((err - bound).max()))


@pytest.mark.parametrize("case", R.steps_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{'hole' if c[3] else 'full'}")
def test_steps_case_holds_its_rows(case):
    n_rows, L, kind, hole = case
    n_cols = R.STEP_COLS
    mats = R.steps_case(n_rows, n_cols, L, kind, empty_step=hole)
    assert len(mats) == L and all(M.shape == (n_rows, n_cols) for M in mats)
    for M in mats:
        assert M.data.dtype == np.float32 and M.indices.dtype == np.int32
        assert all(np.all(np.diff(M.indices[M.indptr[r]:M.indptr[r + 1]]) > 0) for r in range(n_rows))
        if kind == "int":
            assert np.array_equal(M.data, np.round(M.data)) and np.abs(M.data).max(initial=0) <= 4
    pats = np.stack([_pattern(M) for M in mats])  # (L, rows, cols), stored zeros included
    held = pats.sum(0)
    lens = np.stack([np.diff(M.indptr) for M in mats])
    live = L - int(hole)
    assert lens.max() == R.LONG_ROW and lens[0, 0] == R.LONG_ROW           # a row of 200 entries
    assert held[0, 0] >= 1 and held[0, n_cols - 1] >= 1                    # first and last column
    assert (held == live).any() and held[0, 7] == live                     # a column held by all the steps
    assert all(held[0, 100 + l] == (l != (L // 2 if hole else -1)) and pats[l, 0, 100 + l] == held[0, 100 + l]
               for l in range(L))                                          # disjoint columns across steps
    assert (sum(int(M.nnz == 0) for M in mats) == 1) == bool(hole)         # a whole step with nnz = 0
    zeros = [(l, r, c) for l, M in enumerate(mats) for r in range(n_rows)
             for c, v in zip(M.indices[M.indptr[r]:M.indptr[r + 1]], M.data[M.indptr[r]:M.indptr[r + 1]]) if v == 0]
    assert zeros == ([(L - 1, 0, 11)] if not (hole and L == 2) else [])    # a stored 0.0 (and no other)
    if L >= 2 and not (hole and L == 2):                                   # a pair that cancels under (1, -1)
        assert held[0, 9] == 2 and pats[0, 0, 9] and pats[1, 0, 9]
        assert _dense(mats[0])[0, 9] == _dense(mats[1])[0, 9] != 0
        fa, _ = R.steps_modulators(L, kind)
        assert fa[0] == 1.0 and fa[1] == -1.0
        ptr, idx, _, _ = R.phi_steps_ref(mats, fa, L)
        assert 9 not in idx[ptr[0]:ptr[1]]
    fa, fb = R.steps_modulators(L, kind)
    assert (L < 3 or fa[2] == 0.0) and fb[L - 1] == 0.0                     # an f_l = 0
    if n_rows >= 3:
        assert held[1].sum() == 0                                          # empty in every step
        assert (lens[:, 2] > 0).sum() == 1                                 # present in one step only
    if n_rows == 257:
        assert (lens.sum(0) > 64).sum() >= 4 and (held >= min(live, 2)).sum() > 50   # long rows; columns that meet


# --------------------------------------------------------------------------------- the dot references
@pytest.mark.parametrize("kind", R.KINDS)
def test_rowdot_ref_and_case(kind):
    A, B, perm = R.rowdot_case(300, kind)
    assert A.shape[0] != B.shape[0] and np.array_equal(perm[:7], np.arange(7))
    assert sorted(perm.tolist()) == list(range(A.shape[0]))
    la, lb = np.diff(A.indptr), np.diff(B.indptr)
    Ad, Bd = _dense(A), _dense(B)
    Ap, Bp = _pattern(A), _pattern(B)
    for i in range(A.shape[0]):
        j, t = int(perm[i]), i % R.ROWDOT_TEMPLATES
        common = np.flatnonzero(Ap[i] & Bp[j])
        cb = B.indices[B.indptr[j]:B.indptr[j + 1]]
        if t == 0:
            assert la[i] == 130 and lb[j] == R.LONG_ROW and common.size == 65
        elif t == 1:
            assert la[i] > 0 and np.array_equal(Ad[i], Bd[j]) and np.array_equal(Ap[i], Bp[j])
        elif t == 2:
            assert la[i] > 64 and lb[j] > 64 and common.size == 0
        elif t == 3:
            assert la[i] == 0 and lb[j] > 0
        elif t == 4:
            assert la[i] > 0 and lb[j] == 0
        elif t == 5:
            assert common.tolist() == [cb[0]] and lb[j] > 64
        else:
            assert common.tolist() == [cb[-1]] and lb[j] > 64
    n = A.shape[0]
    sel = np.arange(n)[::-1] // 2
    for ra, rb in [(None, None), (None, perm), (sel, None), (sel, perm[sel])]:
        out, mag = R.rowdot_ref(A, ra, B, rb, n)
        ia = np.arange(n) if ra is None else ra
        ib = np.arange(n) if rb is None else rb
        want = np.einsum("ij,ij->i", Ad[ia], Bd[ib])
        wmag = np.einsum("ij,ij->i", np.abs(Ad[ia]), np.abs(Bd[ib]))
        assert np.allclose(mag, wmag, rtol=1e-14, atol=0)
        if kind == "int":
            assert np.array_equal(out, want) and mag.max() < 2.0 ** 53
        else:
            assert np.all(np.abs(out - want) <= 2 * 300 * U * wmag)
    assert mag.max() > 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_rows_dot_cols_ref_and_case(kind):
    lengths = R.dotcols_lengths()
    assert lengths[:4] == (0, 64, 65, R.LONG_ROW) and len(lengths) > 130
    M = R.rows_case(lengths, 300, kind)
    assert np.array_equal(np.diff(M.indptr), lengths) and M.data.dtype == np.float32
    assert not np.any(M.data == 0)
    Md = _dense(M)
    for n_sel in (1, 5, 130):
        Z = R.dense_matrix((300, n_sel), kind)
        assert Z.dtype == np.float32
        for rows in (None, R.selection(n_sel)):
            out, mag = R.rows_dot_cols_ref(M, rows, Z, n_sel)
            ir = np.arange(n_sel) if rows is None else rows
            want = np.einsum("rk,kr->r", Md[ir], Z.astype(np.float64))
            wmag = np.einsum("rk,kr->r", np.abs(Md[ir]), np.abs(Z.astype(np.float64)))
            assert np.allclose(mag, wmag, rtol=1e-14, atol=0)
            if kind == "int":
                assert np.array_equal(out, want) and mag.max() < 2.0 ** 53
            else:
                assert np.all(np.abs(out - want) <= 2 * 300 * U * wmag)


def test_selection_is_descending_with_repeats():
    for n_sel in (1, 3, 5, 255, 256, 257):
        s = R.selection(n_sel)
        assert s.size == n_sel and np.all(np.diff(s) <= 0) and s[0] == len(R.ROW_LENGTHS) - 1
        assert n_sel == 1 or np.any(np.diff(s) == 0)
        assert n_sel < 255 or set(s.tolist()) == set(range(len(R.ROW_LENGTHS)))
    assert R.ROW_LENGTHS == (0, 1, 63, 64, 65, 200)
    for kind in R.KINDS:
        assert np.array_equal(np.diff(R.rows_case(R.ROW_LENGTHS, 300, kind).indptr), R.ROW_LENGTHS)


# ------------------------------------------------------------------------------ the dense references
@pytest.mark.parametrize("n", R.DENSE_NS)
def test_dense_refs_and_case(n):
    for L in R.DENSE_LS:
        for kind in R.KINDS:
            F, f, G = R.dense_case(n, L, kind)
            assert F.shape == (n, n, L) and f.shape == (L,) and G.shape == (n, n)
            assert n == 1 or not np.array_equal(G, G.T)
            assert (F == 0).any() or n * n * L < 8
            Phi = R.dense_phi_ref(F, f)
            want = F @ f
            pmag = np.abs(F) @ np.abs(f)
            grad, gmag = R.dense_grad_ref(F, Phi, G)
            two = np.einsum("ijl,ij->l", F, G @ Phi) + np.einsum("ijl,ij->l", F, G.T @ Phi)
            if kind == "int":
                assert np.array_equal(Phi, want) and np.array_equal(grad, two)
                assert np.array_equal(F, np.round(F)) and np.array_equal(G, np.round(G))
                assert pmag.max() < 2.0 ** 53 and gmag.max() < 2.0 ** 53
            else:
                assert np.all(np.abs(Phi - want) <= 2 * L * U * pmag)
                assert np.all(np.abs(grad - two) <= 2 * (n + n * n + 2) * U * gmag)  # (plain numpy sums)
    assert R.dense_grad_depth(130) == 130 + 34 + 1 and R.dense_grad_depth(1) == 1 + 34 + 1


def test_hub_steps_case():
    mats, hubs = R.hub_steps_case()
    assert len(mats) == 4 and hubs.size == 12 and all(M.shape == (300, 300) for M in mats)
    lens = np.stack([np.diff(M.indptr) for M in mats])
    assert np.all(lens[:, hubs] >= 130) and np.all(lens[:, hubs] <= R.LONG_ROW)
    rest = np.setdiff1d(np.arange(300), hubs)
    assert lens[:, rest].max() < 8 and (lens[:, rest].sum(0) == 0).any()
    union = sum(_pattern(M) for M in mats)[hubs]
    assert np.all((union > 0).sum(1) <= R.LONG_ROW) and np.all((union > 0).sum(1) >= 130)
    assert all(M.data.min() > 0 and M.data.dtype == np.float32 for M in mats)
