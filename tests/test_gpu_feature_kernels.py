"""GPU: the feature-algebra kernels (grf_features.hip: grf_phi_steps_csr_count / _fill, grf_csr_row_lengths,
grf_csr_gather_rows, grf_csr_rowdot, grf_csr_rows_dot_cols) and the dense-step kernels (grf_dense_steps.hip:
grf_dense_steps_phi, grf_dense_steps_grad) called directly at edge shapes, against the numpy restatements
of tests/feature_reference.py (pinned on the CPU by tests/test_feature_reference.py).

Two kinds of assertion:
  * integer-valued inputs: bitwise equality.  Every product and partial sum is an integer below 2^53
    (asserted per case by tests/test_feature_reference.py), so any summation order gives the same fp64 and
    no tolerance hides an indexing, tail or stride error.
  * real-valued inputs: ``|got - ref| <= 2 D 2^-53 magnitude + 1e-300`` with D the kernel's own summation
    depth and magnitude the sum of the terms' absolute values; the factor 2 covers the fp64 reference's
    own rounding.  Nothing is measured:
      csr_rowdot          D = ceil(len_A / 64) + 6 (the fp32 x fp32 products are exact in fp64)
      csr_rows_dot_cols   D = ceil(len / 64) + 6
      dense_steps_grad    D = n + 34 + ceil(nblk / 64), nblk = ceil(n / 64)^2: 1 (S = G + G^T) + n + 1 (the
                          MFMA k-sum) + 1 + 16 (a lane's epilogue) + 6 (wave_sum) + 3 (the four waves) +
                          ceil(nblk / 64) + 6 (the reduce kernel)
    and a second call must return the same bits (the kernels sum in a fixed order).
  grf_phi_steps_csr and grf_dense_steps_phi are exact for both kinds: the references restate their
  arithmetic operation by operation (-ffp-contract=off).

Largest error / bound measured on an MI355X over the real-valued cases (information, not asserted; each
test prints its own): csr_rowdot 0.235 (n_pairs = 130; 0.014 at 1), csr_rows_dot_cols 0.132 (n_sel = 130;
0.022 at 1, 0.031 at 5), dense_steps_grad 0.004 (n = 15; 0.002 at 17, 0.001 at 64, 65 and 130).  The whole
file runs in under 6 s, its slowest test (257 rows x 64 steps) in 0.6 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import feature_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_COLS = R.STEP_COLS


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _dev(M, eng):
    """scipy CSR (fp32 values) -> DeviceCSR with the fp32 values the kernels read."""
    from grf_amd.engine import DeviceCSR
    D = DeviceCSR.from_scipy(M, eng.device)
    D.val32 = D.val.float()
    return D


def _step_set(mats, eng):
    from grf_amd.features import StepMatrices
    ts = [torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)),
                                  torch.from_numpy(M.indices.astype(np.int64)),
                                  torch.from_numpy(M.data.astype(np.float32)), M.shape, dtype=torch.float32)
          for M in mats]
    return StepMatrices(ts, eng)


def _t(a, eng, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(eng.device)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


def _within(got, ref, mag, depth):
    """The real-valued bound: (held, the largest error / bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = 2.0 * np.asarray(depth, np.float64) * U * mag + 1e-300
    return bool(np.all(err <= bound)), float((err / bound).max())


# ------------------------------------------------------------------------------------ grf_phi_steps_csr
SENT_I, PAD = -77, 9


def _phi_raw(sm, f, n_f, want64, want32=True):
    """count -> scan -> fill as StepMatrices.phi calls them, with n_f, NULL outputs and the buffers'
    sizes (ptr[-1] + PAD, sentinel-filled) under the test's control."""
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    e = sm.engine
    n = sm.shape[0]
    ft = _t(np.asarray(f, np.float64), e)
    cnt = torch.full((n,), SENT_I, dtype=torch.int32, device=e.device)
    C.check(e.lib.grf_phi_steps_csr_count(n, sm.L, sm._ptrs[0], sm._ptrs[1], sm._ptrs[2], _p(ft), n_f, _p(cnt),
                                          e.stream), "grf_phi_steps_csr_count")
    ptr = e._empty(n + 1, torch.int64)
    ws = e._ws(e.lib.grf_scan_workspace_bytes(n))
    C.check(e.lib.grf_scan_counts(n, _p(cnt), _p(ptr), _p(ws), ws.numel(), e.stream), "grf_scan_counts")
    total = int(ptr[-1].item())
    idx = torch.full((total + PAD,), SENT_I, dtype=torch.int32, device=e.device)
    v64 = torch.full((total + PAD,), float("nan"), dtype=torch.float64, device=e.device) if want64 else None
    v32 = torch.full((total + PAD,), float("nan"), dtype=torch.float32, device=e.device) if want32 else None
    C.check(e.lib.grf_phi_steps_csr_fill(n, sm.L, sm._ptrs[0], sm._ptrs[1], sm._ptrs[2], _p(ft), n_f, _p(ptr),
                                         _p(idx), _p(v64), _p(v32), e.stream), "grf_phi_steps_csr_fill")
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(cnt), host(ptr), host(idx), host(v64), host(v32)


def _check_phi(out, ref, tag):
    cnt, ptr, idx, v64, v32 = out
    rptr, ridx, r64, r32 = ref
    total = int(rptr[-1])
    assert np.array_equal(ptr, rptr), tag
    assert np.array_equal(cnt, np.diff(rptr)) and int(cnt.sum()) == int(ptr[-1]), tag  # count and fill agree
    assert np.array_equal(idx[:total], ridx), tag
    assert np.all(idx[total:] == SENT_I) and idx.size == total + PAD, tag                # nothing past ptr[-1]
    if v64 is not None:
        assert _same_bits(v64[:total], r64), tag
        assert np.all(np.isnan(v64[total:])), tag
    if v32 is not None:
        assert _same_bits(v32[:total], r32) and _same_bits(r32, r64.astype(np.float32)), tag
        assert np.all(np.isnan(v32[total:])), tag


@pytest.mark.parametrize("n_rows,L", [(n, L) for n in R.STEP_ROWS for L in R.STEP_LS])
def test_phi_steps_csr_exact(eng, n_rows, L):
    """Phi's indptr, indices, fp64 values and their fp32 casts bit-equal to phi_steps_ref for every case of
    the shape (both kinds, with and without an empty step), both modulators, n_f in {0, 1, L - 1, L}, with
    and without the fp64 output; the public wrapper StepMatrices.phi gives the same CSR."""
    for (_, _, kind, hole) in [c for c in R.steps_cases() if c[0] == n_rows and c[1] == L]:
        mats = R.steps_case(n_rows, N_COLS, L, kind, empty_step=hole)
        sm = _step_set(mats, eng)
        assert sm.L == L and sm.nnz_sum == sum(M.nnz for M in mats)
        for fi, f in enumerate(R.steps_modulators(L, kind)):
            for n_f in sorted({0, 1, L - 1, L}):
                ref = R.phi_steps_ref(mats, f, n_f)
                for want64 in (True, False):
                    _check_phi(_phi_raw(sm, f, n_f, want64), ref, (kind, hole, fi, n_f, want64))
                if n_f == L:
                    _check_phi(_phi_raw(sm, f, n_f, True, want32=False), ref, (kind, hole, fi, "no fp32"))
                if n_f >= 1:  # the wrapper: the modulator's length is n_f
                    phi = sm.phi(torch.from_numpy(f[:n_f].copy()), want64=True)
                    total = int(ref[0][-1])
                    assert phi.nnz == total and np.array_equal(phi.ptr.cpu().numpy(), ref[0])
                    assert np.array_equal(phi.idx[:total].cpu().numpy(), ref[1])
                    assert _same_bits(phi.val[:total].cpu().numpy(), ref[2])
                    assert _same_bits(phi.val32[:total].cpu().numpy(), ref[3])


def test_phi_steps_csr_argument_edges(eng):
    """n_rows == 0 is OK (no output needed); 65 step matrices are refused (GRF_EUNSUPPORTED) before any
    launch; a modulator longer than L uses its first L entries."""
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    mats = R.steps_case(4, N_COLS, 2, "int")
    sm = _step_set(mats, eng)
    null = ctypes.c_void_p(0)
    f = _t(np.array([1.0, -1.0]), eng)
    C.check(eng.lib.grf_phi_steps_csr_count(0, 2, sm._ptrs[0], sm._ptrs[1], sm._ptrs[2], _p(f), 2, null, eng.stream),
            "grf_phi_steps_csr_count")
    C.check(eng.lib.grf_phi_steps_csr_fill(0, 2, sm._ptrs[0], sm._ptrs[1], sm._ptrs[2], _p(f), 2, null, null, null,
                                           null, eng.stream), "grf_phi_steps_csr_fill")
    arrs = [(ctypes.c_void_p * 65)(*[getattr(sm.steps[0], a).data_ptr()] * 65) for a in ("ptr", "idx", "val32")]
    p65 = [ctypes.cast(a, ctypes.c_void_p) for a in arrs]
    f65 = _t(np.ones(65), eng)
    cnt = torch.full((4,), SENT_I, dtype=torch.int32, device=eng.device)
    with pytest.raises(NotImplementedError):
        C.check(eng.lib.grf_phi_steps_csr_count(4, 65, p65[0], p65[1], p65[2], _p(f65), 65, _p(cnt), eng.stream),
                "grf_phi_steps_csr_count")
    with pytest.raises(NotImplementedError):
        C.check(eng.lib.grf_phi_steps_csr_fill(4, 65, p65[0], p65[1], p65[2], _p(f65), 65, _p(cnt), _p(cnt), null,
                                               _p(f65), eng.stream), "grf_phi_steps_csr_fill")
    assert np.all(cnt.cpu().numpy() == SENT_I)
    ref = R.phi_steps_ref(mats, [2.0, 3.0], 2)
    phi = sm.phi(torch.tensor([2.0, 3.0, 5.0, 7.0], dtype=torch.float64), want64=True)
    assert np.array_equal(phi.ptr.cpu().numpy(), ref[0]) and _same_bits(phi.val[:phi.nnz].cpu().numpy(), ref[2])


# ------------------------------------------------------------- grf_csr_row_lengths / grf_csr_gather_rows
@pytest.mark.parametrize("n_sel", [1, 3, 5, 255, 256, 257])
def test_csr_row_lengths_and_gather_rows_exact(eng, n_sel):
    """Rows of 0, 1, 63, 64, 65 and 200 entries selected in descending order with repeats: lengths (with a
    row map and with NULL), indices and values bit-equal, nothing written past the last entry."""
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    from grf_amd.features import gather_rows
    for kind in R.KINDS:
        A = R.rows_case(R.ROW_LENGTHS, N_COLS, kind)
        Ad = _dev(A, eng)
        rows = R.selection(n_sel)
        rmap = _t(rows, eng, torch.int32)
        lens = np.diff(A.indptr)
        want = A[rows]
        want.sort_indices()
        total = int(want.nnz)
        cnt = torch.full((n_sel + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
        C.check(eng.lib.grf_csr_row_lengths(n_sel, _p(Ad.ptr), _p(rmap), _p(cnt), eng.stream), "grf_csr_row_lengths")
        cnt = cnt.cpu().numpy()
        assert np.array_equal(cnt[:n_sel], lens[rows]) and np.all(cnt[n_sel:] == SENT_I)
        m = min(n_sel, A.shape[0])  # NULL row_map: the first m rows
        cnt0 = torch.full((m + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
        C.check(eng.lib.grf_csr_row_lengths(m, _p(Ad.ptr), ctypes.c_void_p(0), _p(cnt0), eng.stream),
                "grf_csr_row_lengths")
        cnt0 = cnt0.cpu().numpy()
        assert np.array_equal(cnt0[:m], lens[:m]) and np.all(cnt0[m:] == SENT_I)
        optr = _t(np.asarray(want.indptr, np.int64), eng)
        oidx = torch.full((total + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
        oval = torch.full((total + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        C.check(eng.lib.grf_csr_gather_rows(n_sel, _p(Ad.ptr), _p(Ad.idx), _p(Ad.val32), _p(rmap), _p(optr), _p(oidx),
                                            _p(oval), eng.stream), "grf_csr_gather_rows")
        oidx, oval = oidx.cpu().numpy(), oval.cpu().numpy()
        assert np.array_equal(oidx[:total], want.indices) and np.all(oidx[total:] == SENT_I), kind
        assert _same_bits(oval[:total], want.data.astype(np.float32)) and np.all(np.isnan(oval[total:])), kind
        Gd = gather_rows(eng, Ad, torch.from_numpy(rows))  # the wrapper (lengths + scan + gather)
        assert Gd.n_rows == n_sel and np.array_equal(Gd.ptr.cpu().numpy(), want.indptr)
        assert np.array_equal(Gd.idx[:total].cpu().numpy(), want.indices)
        assert _same_bits(Gd.val32[:total].cpu().numpy(), want.data.astype(np.float32))


# ------------------------------------------------------------------------------------- grf_csr_rowdot
def _rowdot_rows(n_pairs):
    """rows_a of the explicit-map calls: descending with repeats; at 130 every template many times over."""
    if n_pairs == 1:
        return np.array([7])  # (template 0 behind the permutation: 130 and 200 entries)
    if n_pairs == 5:
        return np.array([6, 5, 5, 1, 0])
    return np.sort(np.r_[np.arange(40, 131), np.arange(30), [130, 130, 64, 64, 3, 3, 0, 0, 7]])[::-1].copy()


@pytest.mark.parametrize("n_pairs", [1, 5, 130])
def test_csr_rowdot(eng, n_pairs):
    """A[rows_a[r]] . B[rows_b[r]] for two different matrices (131 and 137 rows): pairs of rows of 130 and
    200 entries, identical, disjoint, A empty, B empty, one common column that is B's first / B's last; all
    four NULL / non-NULL combinations of the row maps.  Integer kind bitwise, real kind within
    D = ceil(len_A / 64) + 6; a second call gives the same bits."""
    from grf_amd.features import rowdot
    worst = 0.0
    for kind in R.KINDS:
        A, B, perm = R.rowdot_case(N_COLS, kind)
        Ad, Bd = _dev(A, eng), _dev(B, eng)
        inv = np.argsort(perm)  # B row j < 131 pairs with A row inv[j]
        sel = _rowdot_rows(n_pairs)
        assert sel.size == n_pairs
        combos = [(None, None), (None, perm[:n_pairs]), (inv[:n_pairs], None), (sel, perm[sel])]
        for ra, rb in combos:
            ref, mag = R.rowdot_ref(A, ra, B, rb, n_pairs)
            ta = None if ra is None else torch.from_numpy(np.asarray(ra, np.int64))
            tb = None if rb is None else torch.from_numpy(np.asarray(rb, np.int64))
            out = rowdot(eng, Ad, ta, Bd, tb, n_pairs)
            got = out.cpu().numpy()
            assert _same_bits(rowdot(eng, Ad, ta, Bd, tb, n_pairs).cpu().numpy(), got)
            tag = (kind, ra is None, rb is None)
            if kind == "int":
                assert _same_bits(got, ref + 0.0), tag
            else:
                la = np.diff(A.indptr)[np.arange(n_pairs) if ra is None else ra]
                ok, ratio = _within(got, ref, mag, [R.dot_depth(x) for x in la])
                worst = max(worst, ratio)
                assert ok, (tag, ratio)
        assert np.abs(ref).max() > 0
    print(f"csr_rowdot n_pairs={n_pairs}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------ grf_csr_rows_dot_cols
def _rows_dot_cols_raw(eng, Md, rmap, Z, n_sel, ldz):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    out = torch.full((n_sel + PAD,), float("nan"), dtype=torch.float64, device=eng.device)
    C.check(eng.lib.grf_csr_rows_dot_cols(n_sel, _p(Md.ptr), _p(Md.idx), _p(Md.val32), _p(rmap), _p(Z), ldz, _p(out),
                                          eng.stream), "grf_csr_rows_dot_cols")
    out = out.cpu().numpy()
    assert np.all(np.isnan(out[n_sel:]))
    return out[:n_sel]


@pytest.mark.parametrize("n_sel", [1, 5, 130])
def test_csr_rows_dot_cols(eng, n_sel):
    """out[r] = sum_e M[rows[r], e] Z[col_e, r] with Z a column slice of a wider NaN-filled fp32 matrix
    (ldz > n_sel): rows of 0, 64, 65 and 200 entries, NULL row map and a map with repeats; ldz < n_sel is
    refused.  Integer kind bitwise, real kind within D = ceil(len / 64) + 6; a second call, same bits."""
    from grf_amd.features import rows_dot_cols
    worst = 0.0
    lengths = R.dotcols_lengths()
    for kind in R.KINDS:
        M = R.rows_case(lengths, N_COLS, kind)
        Md = _dev(M, eng)
        Zh = R.dense_matrix((N_COLS, n_sel), kind)
        wide = torch.full((N_COLS, n_sel + 11), float("nan"), dtype=torch.float32, device=eng.device)
        Z = wide[:, 3:3 + n_sel]
        Z.copy_(_t(Zh, eng))
        assert Z.stride(0) == n_sel + 11 and Z.data_ptr() != wide.data_ptr()
        rep = R.selection(n_sel)  # (within the first six rows: 0, 64, 65, 200, 1, 63 entries)
        for rows in (None, rep):
            ref, mag = R.rows_dot_cols_ref(M, rows, Zh, n_sel)
            rmap = None if rows is None else _t(rows, eng, torch.int32)
            got = _rows_dot_cols_raw(eng, Md, rmap, Z, n_sel, Z.stride(0))
            assert _same_bits(_rows_dot_cols_raw(eng, Md, rmap, Z, n_sel, Z.stride(0)), got)
            if rows is not None:  # the wrapper passes Z's own stride
                assert _same_bits(rows_dot_cols(eng, Md, torch.from_numpy(rows), Z).cpu().numpy(), got)
            if kind == "int":
                assert _same_bits(got, ref + 0.0), (kind, rows is None)
            else:
                ln = np.asarray(lengths)[np.arange(n_sel) if rows is None else rows]
                ok, ratio = _within(got, ref, mag, [R.dot_depth(x) for x in ln])
                worst = max(worst, ratio)
                assert ok, (kind, rows is None, ratio)
        with pytest.raises(ValueError):
            _rows_dot_cols_raw(eng, Md, None, Z, n_sel, n_sel - 1)
    print(f"csr_rows_dot_cols n_sel={n_sel}: worst error / bound = {worst:.3f}")


# --------------------------------------------------------------------------------- grf_dense_steps_phi
def _dense_phi_raw(eng, F, f, n, L, lda32, want64):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    phi32 = torch.full((n, lda32), float("nan"), dtype=torch.float32, device=eng.device)
    phi64 = torch.full((n, n), float("nan"), dtype=torch.float64, device=eng.device) if want64 else None
    C.check(eng.lib.grf_dense_steps_phi(n, L, _p(F), _p(f), _p(phi64), _p(phi32), lda32, eng.stream),
            "grf_dense_steps_phi")
    return (None if phi64 is None else phi64.cpu().numpy()), phi32.cpu().numpy()


@pytest.mark.parametrize("n", R.DENSE_NS)
def test_dense_steps_phi_exact(eng, n):
    """Phi = F f bit-equal to dense_phi_ref (both kinds), the fp32 image its cast with the padding columns
    [n, lda32) written 0.0 over a NaN-filled buffer, at lda32 = 64 ceil(n / 64) and a larger one, with and
    without the fp64 output; DenseSteps.phi gives the same bits."""
    from grf_amd.features import DenseSteps
    for L in R.DENSE_LS:
        for kind in R.KINDS:
            Fh, fh, _ = R.dense_case(n, L, kind)
            ref = R.dense_phi_ref(Fh, fh)
            F, f = _t(Fh, eng), _t(fh, eng)
            lda = 64 * -(-n // 64)
            for lda32 in (lda, lda + 80):
                for want64 in (True, False):
                    p64, p32 = _dense_phi_raw(eng, F, f, n, L, lda32, want64)
                    tag = (L, kind, lda32, want64)
                    assert p64 is None or _same_bits(p64, ref), tag
                    assert _same_bits(p32[:, :n], ref.astype(np.float32)), tag
                    assert p32.shape == (n, lda32) and _same_bits(p32[:, n:], np.zeros((n, lda32 - n), np.float32)), tag
            assert _same_bits(DenseSteps(F, eng).phi(f).cpu().numpy(), ref), (L, kind)


# -------------------------------------------------------------------------------- grf_dense_steps_grad
def _dense_grad_raw(eng, F, phi, G, ldg, n, L, short=0):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    need = int(eng.lib.grf_dense_steps_grad_workspace_bytes(n, L))
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=eng.device)  # (dirty: NaN bit patterns)
    grad = torch.full((L + PAD,), float("nan"), dtype=torch.float64, device=eng.device)
    C.check(eng.lib.grf_dense_steps_grad(n, L, _p(F), _p(phi), _p(G), ldg, _p(grad), _p(ws), need - short,
                                         eng.stream), "grf_dense_steps_grad")
    grad = grad.cpu().numpy()
    assert np.all(np.isnan(grad[L:]))
    return grad[:L]


@pytest.mark.parametrize("n", R.DENSE_NS)
def test_dense_steps_grad(eng, n):
    """dL/df_l = <F_l, (G + G^T) Phi> with a non-symmetric G that is a view of a wider NaN-filled matrix
    (ldg > n), L in {1, 7, 8, 9, 17} (the second and third group of eight steps of the epilogue): integer
    kind bitwise, real kind within D = n + 34 + ceil(nblk / 64); a second call gives the same bits; a
    contiguous G (ldg == n) gives the same bits as the view; a workspace one byte short is refused."""
    worst = 0.0
    for L in R.DENSE_LS:
        for kind in R.KINDS:
            Fh, fh, Gh = R.dense_case(n, L, kind)
            Ph = R.dense_phi_ref(Fh, fh)
            ref, mag = R.dense_grad_ref(Fh, Ph, Gh)
            F, phi = _t(Fh, eng), _t(Ph, eng)
            wide = torch.full((n, n + 13), float("nan"), dtype=torch.float64, device=eng.device)
            G = wide[:, 5:5 + n]
            G.copy_(_t(Gh, eng))
            assert G.stride(0) == n + 13
            got = _dense_grad_raw(eng, F, phi, G, G.stride(0), n, L)
            assert _same_bits(_dense_grad_raw(eng, F, phi, G, G.stride(0), n, L), got), (L, kind)
            assert _same_bits(_dense_grad_raw(eng, F, phi, _t(Gh, eng), n, n, L), got), (L, kind)
            if kind == "int":
                assert _same_bits(got, ref + 0.0), (L, kind, got, ref)
            else:
                ok, ratio = _within(got, ref, mag, R.dense_grad_depth(n))
                worst = max(worst, ratio)
                assert ok, (L, kind, ratio)
    with pytest.raises(ValueError):
        _dense_grad_raw(eng, F, phi, G, G.stride(0), n, L, short=1)
    print(f"dense_steps_grad n={n}: worst error / bound = {worst:.3f}")


def test_dense_steps_grad_of_an_empty_tensor_is_zero(eng):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    null = ctypes.c_void_p(0)
    grad = torch.full((9 + PAD,), float("nan"), dtype=torch.float64, device=eng.device)
    C.check(eng.lib.grf_dense_steps_grad(0, 9, null, null, null, 0, _p(grad), null, 0, eng.stream),
            "grf_dense_steps_grad")
    grad = grad.cpu().numpy()
    assert _same_bits(grad[:9], np.zeros(9)) and np.all(np.isnan(grad[9:]))


# --------------------------------------------------------------------------------- the module surface
def _close(got, ref, absbound):
    """The K / diag tolerance of tests/test_gpu_features.py."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return bool(np.all(err <= 3e-5 * absbound + 1e-7 * max(np.abs(ref).max(), 1e-30))), float(err.max())


def test_sparse_grf_kernel_on_hub_rows(eng):
    """SparseGRFKernel over a synthetic step set (n = 300, L = 4, 12 hub rows of 130 to 200 entries):
    K[x1, x2], diag=True and both backward paths with x1, x2 holding hub rows, short rows, an empty row and
    repeats, against the fp64 restatement with the tolerances tests/test_gpu_features.py states (K and diag:
    3e-5 (|Phi||Phi|^T) + 1e-7 max|K|; gradients rtol 1e-4).  The loads, the modulator and the weights are
    positive, so no cancellation stands between the relative tolerance and the fp32 operands' rounding."""
    from efficient_graph_gp_sparse.gptorch_kernels_sparse import SparseGRFKernel
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from efficient_graph_gp_sparse.utils_sparse.sparse_lo import SparseLinearOperator
    mats, hubs = R.hub_steps_case()
    L = len(mats)
    dense = [M.toarray().astype(np.float32).astype(np.float64) for M in mats]
    kern = SparseGRFKernel(L, [SparseLinearOperator(GraphPreprocessor.from_scipy_csr(M).to("cuda")) for M in mats])
    kern = kern.cuda()
    with torch.no_grad():
        kern.raw_modulator_vector.copy_(torch.tensor([1.0, 0.5, 0.25, 0.125]))
    f = kern.modulator_vector.detach().cpu().numpy().astype(np.float64)
    Phi = sum(fl * M for fl, M in zip(f, dense))
    empty = int(np.flatnonzero(np.abs(Phi).sum(1) == 0)[0])
    short = [i for i in range(300) if i not in set(hubs.tolist())][:3]
    i1 = [int(hubs[0]), short[0], int(hubs[5]), int(hubs[0]), empty, int(hubs[11]), short[1]]
    i2 = [int(hubs[5]), int(hubs[5]), short[2], int(hubs[1]), int(hubs[3]), empty, int(hubs[11])]
    x1, x2 = torch.tensor(i1, device="cuda"), torch.tensor(i2, device="cuda")
    K = kern(x1, x2)
    ok, e = _close(K.detach().cpu().numpy(), Phi[i1] @ Phi[i2].T, np.abs(Phi[i1]) @ np.abs(Phi[i2]).T)
    assert ok, e
    Kd = kern(x1, x2, diag=True)
    ok, e = _close(Kd.detach().cpu().numpy(), np.einsum("ij,ij->i", Phi[i1], Phi[i2]),
                   np.einsum("ij,ij->i", np.abs(Phi[i1]), np.abs(Phi[i2])))
    assert ok, e
    W = np.random.default_rng(1).uniform(0.5, 1.5, (7, 7))
    (kern(x1, x2) * torch.tensor(W, device="cuda", dtype=torch.float32)).sum().backward()
    gref = [np.sum(W * (dense[l][i1] @ Phi[i2].T + Phi[i1] @ dense[l][i2].T)) for l in range(L)]
    np.testing.assert_allclose(kern.raw_modulator_vector.grad.cpu().numpy(), gref, rtol=1e-4)
    kern.raw_modulator_vector.grad = None
    w = np.random.default_rng(2).uniform(0.5, 1.5, 7)
    (kern(x1, x2, diag=True) * torch.tensor(w, device="cuda", dtype=torch.float32)).sum().backward()
    gref = [np.sum(w * (np.einsum("ij,ij->i", dense[l][i1], Phi[i2]) + np.einsum("ij,ij->i", Phi[i1], dense[l][i2])))
            for l in range(L)]
    np.testing.assert_allclose(kern.raw_modulator_vector.grad.cpu().numpy(), gref, rtol=1e-4)
