"""GPU: the solver-side kernels called directly through the C ABI at edge shapes -- grf_csr_transpose,
grf_spmm_csr / _f64, grf_cg_gram_solve / _f64 / _lanczos_f64 (grf_cg.hip) and grf_steps_frob_f64 (grf_mll.hip)
-- against the numpy restatements of tests/solver_reference.py (pinned on the CPU by
tests/test_solver_reference.py).  Leading dimensions, nnz bounds, NULL pointers, buffer sizes and the
workspaces (zero-filled, sized by the library's own *_workspace_bytes) are the test's.

Assertions:
  * integer-valued inputs: bitwise equality (every product and partial sum is an integer below 2^24 / 2^53,
    asserted per case on the CPU, so any summation order gives the same bits);
  * real-valued inputs: ``|got - ref| <= 2 D u magnitude + 1e-300``, u = 2^-24 (fp32) or 2^-53 (fp64), D the
    kernel's own depth (solver_reference.spmm_depth / frob_depth), magnitude the sum of the terms' absolute
    values; the factor 2 covers the second-order terms and the fp64 reference's own rounding;
  * the CSR transpose is exact: t_ptr over all n_cols + 1 entries, t_idx and t_val's bits over the real entries;
  * CG: iteration counts equal to the oracle's, X within 1e-10 (fp64) / 1e-4 (fp32) of it per column in the
    max norm (the bounds tests/test_gpu_cg.py uses for early iterates; the fp64 oracle is itself within 1e-14 of
    its long double run on these cases, cond(K^) <= 5), the Lanczos rows within 1e-10 of the row's largest
    coefficient + 1e-20 (a beta below 1e-20 is the squared residual of a column under linear_cg's own stop
    threshold 1e-10: a solve of n_sys <= 3 rows ends exactly, and what is left there is rounding noise);
  * a second call returns the same bits; buffers are NaN-filled with PAD elements past their end, and neither
    the padding columns nor the tail may change.
Nothing measured is asserted; each test prints its largest error / bound.

Measured on an MI355X (information, not asserted; each test prints its own).  Largest error / bound over the
real-valued cases: SpMM fp32 0.48 (S >= 48, where one lane sums a whole row; 0.07 to 0.24 below), fp64 0.19 (exactly
0 for S >= 48: the products of fp32-representable factors are exact in fp64 and the lane adds them in scipy's
order), grid stride 0.11; steps_frob 0.0008 (its depth is dominated by the worst-case block sum).  CG: x within
7.0e-15 of the oracle in fp64 (1.3e-15 up to n_sys = 64, 4.9e-15 at 1025, 7.0e-15 tiled) and 3.6e-7 in fp32, the
Lanczos coefficients at most 1.1e-3 of their bound.  The whole file runs in under 5 s, its slowest test (the
column-tiled solve) in 0.7 s.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import feature_reference as R
import solver_reference as SR

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53
PAD, SENT_I, SENT_L = 9, -77, -7777
N_COLS = 300
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _t(a, eng, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(eng.device)


def _csr(M, eng):
    """(ptr int64, idx int32, val fp32) device tensors of a scipy CSR, the fp32 bits kept."""
    return (_t(np.asarray(M.indptr, np.int64), eng), _t(np.asarray(M.indices, np.int32), eng),
            _t(np.asarray(M.data, np.float32), eng))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


def _within(got, ref, mag, depth, u):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = 2.0 * np.asarray(depth, np.float64) * u * mag + 1e-300
    return bool(np.all(err <= bound)), float((err / bound).max(initial=0.0))


def _padded(a, ld, eng, dtype):
    """a (n x S) in the leading S columns of an (n x ld) NaN matrix followed by PAD NaN elements; returns
    (flat device buffer, n, ld)."""
    n, S = a.shape
    host = np.full(n * ld + PAD, np.nan, dtype)
    host[:n * ld].reshape(n, ld)[:, :S] = a
    return _t(host, eng)


def _nan_out(n, ld, eng, dtype):
    return torch.full((n * ld + PAD,), float("nan"), dtype=dtype, device=eng.device)


def _unpad(buf, n, S, ld, what):
    """The (n x S) block of a padded output; the padding columns and the PAD tail must still be NaN."""
    host = buf.cpu().numpy()
    body = host[:n * ld].reshape(n, ld)
    assert np.all(np.isnan(body[:, S:])) and np.all(np.isnan(host[n * ld:])), f"{what}: padding overwritten"
    return body[:, :S].copy()


def _zero_ws(nbytes, eng):
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=eng.device)


# ------------------------------------------------------------------------------------- grf_csr_transpose
def _transpose_raw(eng, dev, rmap, n_sel, n_cols, nnz_arg, null_entries=False):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    ptr, idx, val = dev
    t_ptr = torch.full((n_cols + 1 + PAD,), SENT_L, dtype=torch.int64, device=eng.device)
    t_idx = torch.full((nnz_arg + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    t_val = torch.full((nnz_arg + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
    ws = _zero_ws(eng.lib.grf_csr_transpose_workspace_bytes(n_sel, n_cols, nnz_arg), eng)
    ent = (NULL,) * 4 if null_entries else (_p(idx), _p(val), _p(t_idx), _p(t_val))
    C.check(eng.lib.grf_csr_transpose(n_sel, _p(ptr), ent[0], ent[1], _p(rmap), n_cols, nnz_arg, _p(t_ptr), ent[2],
                                      ent[3], _p(ws), ws.numel(), eng.stream), "grf_csr_transpose")
    return t_ptr.cpu().numpy(), t_idx.cpu().numpy(), t_val.cpu().numpy()


def _check_transpose(eng, M, rows, n_cols, tag):
    ref_ptr, ref_idx, ref_val = SR.transpose_ref(M, rows, n_cols)
    total = int(ref_ptr[-1])
    dev = _csr(M, eng)
    n_sel = M.shape[0] if rows is None else len(rows)
    rmap = None if rows is None else _t(np.asarray(rows, np.int32), eng)
    for extra in (0, 1, 300):
        nnz_arg = total + extra
        t_ptr, t_idx, t_val = _transpose_raw(eng, dev, rmap, n_sel, n_cols, nnz_arg)
        assert np.array_equal(t_ptr[:n_cols + 1], ref_ptr) and t_ptr[n_cols] == total, (tag, extra)
        assert np.all(t_ptr[n_cols + 1:] == SENT_L), (tag, extra)
        assert np.array_equal(t_idx[:total], ref_idx), (tag, extra)
        assert np.array_equal(_bits(t_val[:total]), ref_val), (tag, extra)
        assert np.all(t_idx[nnz_arg:] == SENT_I) and np.all(np.isnan(t_val[nnz_arg:])), (tag, extra)  # nothing past nnz
        again = _transpose_raw(eng, dev, rmap, n_sel, n_cols, nnz_arg)
        assert np.array_equal(again[1][:total], t_idx[:total]) and _same_bits(again[2][:total], t_val[:total])
    if total == 0:  # no entries: the entry arrays may be NULL
        t_ptr, _, _ = _transpose_raw(eng, dev, rmap, n_sel, n_cols, 0, null_entries=True)
        assert not t_ptr[:n_cols + 1].any() and np.all(t_ptr[n_cols + 1:] == SENT_L), tag


@pytest.mark.parametrize("n_cols", [256, 300, 4096])
def test_csr_transpose_exact(eng, n_cols):
    """(M[rows])^T for the 32 edge rows (0 to 200 entries, a stored 0.0, a -0.0 and a subnormal) at n_cols = 256
    and 4096 (powers of two: the pad key n_cols needs one bit more than the columns) and 300; row_map NULL,
    descending with repeats (40 positions), empty (n_sel = 0) and of empty rows only (NULL entry arrays); nnz
    exact and an upper bound (+1, +300).  Exact, and nothing is written past nnz."""
    M = SR.with_subnormal(SR.edge_csr("int", n_cols))
    for tag, rows in (("null", None), ("repeats", R.selection(40, SR.EDGE_ROWS)), ("none", np.zeros(0, np.int64)),
                      ("empty rows", np.array([16, 0, 0, 16]))):
        _check_transpose(eng, M, rows, n_cols, (n_cols, tag))


def test_csr_transpose_single_column(eng):
    """Five rows over one column (key_bits = 1, the pad key 1): every selection of the edge-row test."""
    M = R._csr_from_rows([{0: np.float32(2)}, {}, {0: np.float32(-0.0)}, {0: np.float32(1e-40)}, {}], 1)
    for tag, rows in (("null", None), ("repeats", R.selection(7, 5)), ("none", np.zeros(0, np.int64)),
                      ("empty rows", np.array([4, 1, 1]))):
        _check_transpose(eng, M, rows, 1, (1, tag))


# ------------------------------------------------------------------------------------------ grf_spmm_csr
def _spmm_raw(eng, dev, rmap, n_out, Xbuf, ldx, S, ldy, dtype):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    Y = _nan_out(n_out, ldy, eng, dtype)
    fn = eng.lib.grf_spmm_csr if dtype == torch.float32 else eng.lib.grf_spmm_csr_f64
    C.check(fn(n_out, _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(rmap), _p(Xbuf), ldx, S, _p(Y), ldy, eng.stream),
            "grf_spmm_csr")
    return Y


def _spmm_selections():
    """(tag, rows): NULL, reversed and repeated maps at n_out in {1, 3, 4, 5, all}."""
    out = []
    for n in (1, 3, 4, 5, SR.EDGE_ROWS):
        out.append((f"null{n}", None, n))
        out.append((f"rev{n}", np.arange(SR.EDGE_ROWS)[::-1][:n].copy(), n))
        out.append((f"rep{n}", R.selection(n if n < SR.EDGE_ROWS else 40, SR.EDGE_ROWS), n if n < SR.EDGE_ROWS else 40))
    return out


@pytest.mark.parametrize("S", [1, 2, 3, 11, 12, 47, 48, 64, 65, 130, 256])
def test_spmm_edge_rows(eng, S):
    """Y = M[rows] X for the 32 edge rows (0 to 200 entries: the second and third 64-entry batch, every group
    count's tail, both unroll depths), fp32 and fp64, ldx = S + 3 and ldy = S + 5 over NaN, row_map NULL /
    reversed / with repeats, n_out in {1, 3, 4, 5, all}.  Integer kind bitwise, real kind within spmm_depth; the
    same bits twice.  And with X's row 0 NaN the rows that do not hold column 0 give the same bits as before:
    a lane past a row's end must not gather the row of its filler index 0."""
    worst = {torch.float32: 0.0, torch.float64: 0.0}
    lens_all = np.diff(SR.edge_csr("int", N_COLS).indptr)
    for kind in R.KINDS:
        M = SR.edge_csr(kind, N_COLS)
        dev = _csr(M, eng)
        for dtype, npdt, u in ((torch.float32, np.float32, U32), (torch.float64, np.float64, U64)):
            Xh = SR.edge_dense((N_COLS, S), kind, dtype=npdt)
            Xbuf = _padded(Xh, S + 3, eng, npdt)
            ref_all, mag_all = SR.spmm_ref(M, None, Xh)
            for tag, rows, n_out in _spmm_selections():
                sel = np.arange(n_out) if rows is None else rows
                rmap = None if rows is None else _t(rows.astype(np.int32), eng)
                Y = _spmm_raw(eng, dev, rmap, n_out, Xbuf, S + 3, S, S + 5, dtype)
                got = _unpad(Y, n_out, S, S + 5, (kind, dtype, tag))
                Y2 = _spmm_raw(eng, dev, rmap, n_out, Xbuf, S + 3, S, S + 5, dtype)
                assert torch.equal(Y[:n_out * (S + 5)].view(torch.uint8), Y2[:n_out * (S + 5)].view(torch.uint8))
                ref, mag = ref_all[sel], mag_all[sel]
                if kind == "int":
                    assert _same_bits(got, (ref + 0.0).astype(npdt)), (kind, dtype, tag)
                else:
                    depth = np.array([SR.spmm_depth(x, S) for x in lens_all[sel]])[:, None]
                    ok, ratio = _within(got, ref, mag, depth, u)
                    worst[dtype] = max(worst[dtype], ratio)
                    assert ok, (kind, dtype, tag, ratio)
            # X's row 0 poisoned: the rows without column 0 are unchanged
            Xp = Xh.copy()
            Xp[0] = np.nan
            sel = SR.EDGE_NO_FIRST_COLUMN
            rmap = _t(sel.astype(np.int32), eng)
            clean = _unpad(_spmm_raw(eng, dev, rmap, sel.size, Xbuf, S + 3, S, S + 5, dtype), sel.size, S, S + 5, "clean")
            poisoned = _unpad(_spmm_raw(eng, dev, rmap, sel.size, _padded(Xp, S + 3, eng, npdt), S + 3, S, S + 5, dtype),
                              sel.size, S, S + 5, "poisoned")
            assert _same_bits(poisoned, clean), (kind, dtype, "row 0 of X gathered by a lane past the row's end")
    print(f"spmm S={S}: worst error / bound fp32 {worst[torch.float32]:.3f}, fp64 {worst[torch.float64]:.3f}")


def test_spmm_nothing_to_do_writes_nothing(eng):
    """n_out = 0 and S = 0 return OK and leave Y untouched."""
    M = SR.edge_csr("int", N_COLS)
    dev = _csr(M, eng)
    for dtype, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        Xbuf = _padded(SR.edge_dense((N_COLS, 4), "int", dtype=npdt), 7, eng, npdt)
        for n_out, S in ((0, 4), (5, 0)):
            from grf_amd import _lib as C
            from grf_amd.engine import _p
            Y = torch.full((64,), float("nan"), dtype=dtype, device=eng.device)
            fn = eng.lib.grf_spmm_csr if dtype == torch.float32 else eng.lib.grf_spmm_csr_f64
            C.check(fn(n_out, _p(dev[0]), _p(dev[1]), _p(dev[2]), NULL, _p(Xbuf), 7, S, _p(Y), 9, eng.stream),
                    "grf_spmm_csr")
            assert bool(torch.isnan(Y).all()), (dtype, n_out, S)


def test_spmm_grid_stride(eng):
    """n_out = 4 * 65536 + 5 output rows (one more trip of the grid-stride loop for the first five waves), the
    map cycling over the 32 edge rows, S = 3, fp32 and fp64: integer kind bitwise, real kind within
    spmm_depth."""
    n_out, S = 4 * 65536 + 5, 3
    rows = (np.arange(n_out) % SR.EDGE_ROWS).astype(np.int32)
    worst = 0.0
    for kind in R.KINDS:
        M = SR.edge_csr(kind, N_COLS)
        dev = _csr(M, eng)
        rmap = _t(rows, eng)
        lens = np.diff(M.indptr)
        for dtype, npdt, u in ((torch.float32, np.float32, U32), (torch.float64, np.float64, U64)):
            Xh = SR.edge_dense((N_COLS, S), kind, dtype=npdt)
            ref, mag = SR.spmm_ref(M, None, Xh)                     # per distinct row, then indexed
            Y = _spmm_raw(eng, dev, rmap, n_out, _padded(Xh, S + 3, eng, npdt), S + 3, S, S + 5, dtype)
            got = _unpad(Y, n_out, S, S + 5, (kind, dtype))
            if kind == "int":
                assert _same_bits(got, (ref + 0.0).astype(npdt)[rows]), (kind, dtype)
            else:
                depth = np.array([SR.spmm_depth(x, S) for x in lens])[:, None]
                bound = (2.0 * depth * u * mag + 1e-300)[rows]
                err = np.abs(got.astype(np.float64) - ref[rows])
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (kind, dtype)
    print(f"spmm grid stride: worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- CG
class _CgDevice:
    """A CgCase on the device: Phi, the row map and Phi_t^T (from transpose_ref, so the solve's check does not
    lean on grf_csr_transpose)."""

    def __init__(self, case, eng):
        self.case, self.eng = case, eng
        self.n_sys = int(case.train.size)
        self.phi = _csr(case.phi, eng)
        self.rmap = _t(case.train.astype(np.int32), eng)
        t_ptr, t_idx, t_val = SR.transpose_ref(case.phi, case.train, case.n_cols)
        self.t = (_t(t_ptr, eng), _t(t_idx, eng), _t(t_val.view(np.float32), eng))
        self.ws_bytes = int(eng.lib.grf_cg_workspace_bytes(self.n_sys, case.n_cols, case.S))
        assert self.ws_bytes == SR.cg_workspace_bytes(self.n_sys, case.n_cols, case.S)  # the tiles are as restated
        self.rhs = {}

    def solve(self, max_iter, dtype=torch.float64, lanczos=False):
        """(X (n_sys x S), iterations, alpha, beta) through ld_rhs = S + 3 and ldx = S + 5 over NaN."""
        from grf_amd import _lib as C
        from grf_amd.engine import _p
        e, c, S, n = self.eng, self.case, self.case.S, self.n_sys
        npdt = np.float32 if dtype == torch.float32 else np.float64
        if dtype not in self.rhs:
            self.rhs[dtype] = _padded(c.B.astype(npdt), S + 3, e, npdt)
        X = _nan_out(n, S + 5, e, dtype)
        ws = _zero_ws(self.ws_bytes, e)
        iters = ctypes.c_int32(-1)
        head = (n, _p(self.phi[0]), _p(self.phi[1]), _p(self.phi[2]), _p(self.rmap), c.n_cols, _p(self.t[0]),
                _p(self.t[1]), _p(self.t[2]), float(c.noise), _p(self.rhs[dtype]), S + 3, S, 1.0, int(max_iter), _p(X),
                S + 5, _p(ws), ws.numel(), ctypes.byref(iters), NULL)
        al = be = None
        if lanczos:
            coef = torch.full((2 * max_iter * (S + 2) + PAD,), float("nan"), dtype=torch.float64, device=e.device)
            C.check(e.lib.grf_cg_gram_solve_lanczos_f64(*head, _p(coef), S + 2, e.stream), "grf_cg_gram_solve_lanczos_f64")
            host = coef.cpu().numpy()  # (the solve zeroes all 2 max_iter x ld_coef elements, then fills S per row)
            rows = host[:2 * max_iter * (S + 2)].reshape(2 * max_iter, S + 2)
            assert not rows[:, S:].any() and np.all(np.isnan(host[2 * max_iter * (S + 2):])), "coef: written past its end"
            al, be = rows[:max_iter, :S].copy(), rows[max_iter:, :S].copy()
        else:
            fn = e.lib.grf_cg_gram_solve if dtype == torch.float32 else e.lib.grf_cg_gram_solve_f64
            C.check(fn(*head, e.stream), "grf_cg_gram_solve")
        return _unpad(X, n, S, S + 5, "x"), int(iters.value), al, be


def _check_cg(dev, key, max_iters32=(1, 2, 3), fp32=False):
    """fp64 + Lanczos at max_iter 1..4 against the oracle (and fp32 at 1..3 to 1e-4 when asked); returns the
    largest relative errors (x fp64, coefficients, x fp32)."""
    S = dev.case.S
    worst = [0.0, 0.0, 0.0]
    for mi in SR.MAX_ITERS:
        Xo, ito, alo, beo = SR.cg_oracle(key, mi)
        X, it, _, _ = dev.solve(mi)
        Xl, itl, al, be = dev.solve(mi, lanczos=True)
        assert it == itl == ito == mi, (key, mi, it, itl, ito)
        assert _same_bits(Xl, X), (key, mi, "the Lanczos entry point gives another x")
        rel = SR.column_rel(X, Xo)
        worst[0] = max(worst[0], rel)
        assert rel <= 1e-10, (key, mi, rel)
        if S >= 3:
            assert not X[:, SR.ZERO_COLUMN].any() and not al[:, SR.ZERO_COLUMN].any()
        for k in range(mi):
            for got, ref in ((al[k], alo[k]), (be[k], beo[k])):
                err = float(np.abs(got - ref).max())
                tol = 1e-10 * float(np.abs(ref).max()) + 1e-20
                worst[1] = max(worst[1], err / tol)
                assert err <= tol, (key, mi, k, err, tol)
        assert al.shape == (mi, S) and not al[it:].any() and not be[it:].any()
    if fp32:
        for mi in max_iters32:
            Xo, ito, _, _ = SR.cg_oracle(key, mi)
            X, it, _, _ = dev.solve(mi, dtype=torch.float32)
            assert X.dtype == np.float32 and it == ito == mi
            rel = SR.column_rel(X, Xo)
            worst[2] = max(worst[2], rel)
            assert rel <= 1e-4, (key, mi, rel)
            if S >= 3:
                assert not X[:, SR.ZERO_COLUMN].any()
    return worst


@pytest.mark.parametrize("n_sys", SR.SMALL_N_SYS)
def test_cg_small_and_odd_shapes(eng, n_sys):
    """linear_cg on n_sys in {1, 2, 3, 5, 64, 1025} rows (fewer rows than a block's waves; above 4 x 256 a wave
    of cg_reduce_kernel takes a second row) x S in {1, 3, 5, 85, 86, 255, 256} (tpc = 256 / S threads per column
    in the last block: 256, 85, 51, 3, 2, 1, 1) with a zero rhs column, a descending row map, ld_rhs = S + 3 and
    ldx = S + 5 over NaN, max_iter 1..4.  n_sys = 1, 2, 3 end exactly after n_sys steps, so the later iterations
    run through the eps / conv guards.  fp32 at n_sys in {3, 1025}, S in {5, 86}, max_iter 1..3."""
    worst = [0.0, 0.0, 0.0]
    for S in SR.SMALL_S:
        dev = _CgDevice(SR.small_cg_case(n_sys, S), eng)
        w = _check_cg(dev, ("small", n_sys, S), fp32=(n_sys in (3, 1025) and S in (5, 86)))
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"cg n_sys={n_sys}: x fp64 {worst[0]:.1e} (bound 1e-10), coefficients error / bound {worst[1]:.1e}, "
          f"x fp32 {worst[2]:.1e} (bound 1e-4)")


def test_cg_column_tiled(eng):
    """The column-tiled solve (tiled_cg_case: 4097 training rows over 12289 columns, S = 256): 4 tiles of Phi_t,
    the last one column wide, and 2 tiles of Phi_t^T, the last one row wide, in fp64; 2 tiles of Phi_t in fp32.
    Rows that are empty, skip tiles, lie on every tile edge and straddle one at a batch boundary.  The library's
    workspace size must be the restated layout's (the tiles engage as built for), which needs the default tile
    budget.  max_iter 1..4 (fp32 1..3) against the oracle, the Lanczos coefficients, the same bits twice."""
    assert "GRF_SPMM_TILE_BYTES" not in os.environ, \
        "GRF_SPMM_TILE_BYTES is set: this test is built for the default tile budget (8 MiB); unset it"
    case = SR.tiled_cg_case()
    n, tw = case.train.size, SR.TILED_TW
    assert SR.cg_tiles(n, case.n_cols, case.S, 8) == (tw, 2, tw, 4) and SR.cg_tiles(n, case.n_cols, case.S, 4)[2:] == (2 * tw, 2)
    dev = _CgDevice(case, eng)
    worst = _check_cg(dev, ("tiled",), fp32=True)
    X, _, al, be = dev.solve(4, lanczos=True)
    X2, _, al2, be2 = dev.solve(4, lanczos=True)
    assert _same_bits(X, X2) and _same_bits(al, al2) and _same_bits(be, be2)
    X32, X32b = dev.solve(3, dtype=torch.float32)[0], dev.solve(3, dtype=torch.float32)[0]
    assert _same_bits(X32, X32b)
    print(f"cg tiled: x fp64 {worst[0]:.1e} (bound 1e-10), coefficients error / bound {worst[1]:.1e}, "
          f"x fp32 {worst[2]:.1e} (bound 1e-4)")


# ------------------------------------------------------------------------------------ grf_steps_frob_f64
def _frob_raw(eng, steps, rmap, n_sel, bufs, S, L):
    from grf_amd import _lib as C
    from grf_amd.engine import _p
    A, WA, B, WB, wt = bufs
    out = torch.full((L + PAD,), float("nan"), dtype=torch.float64, device=eng.device)
    ws = _zero_ws(eng.lib.grf_steps_frob_workspace_bytes(n_sel, L), eng)
    sp = steps._ptrs
    C.check(eng.lib.grf_steps_frob_f64(n_sel, L, sp[0], sp[1], sp[2], _p(rmap), _p(A), _p(B), S + 3, _p(WA), _p(WB),
                                       S + 5, _p(wt), S, _p(out), _p(ws), ws.numel(), eng.stream), "grf_steps_frob_f64")
    out = out.cpu().numpy()
    assert np.all(np.isnan(out[L:]))
    return out[:L]


@pytest.mark.parametrize("L,S,n_sel,which", SR.FROB_CASES)
def test_steps_frob_edge_shapes(eng, L, S, n_sel, which):
    """out[l] = sum_c wt[c] sum_r (A (M_l[rows] WB) + B (M_l[rows] WA))[r, c] over step matrices whose rows hold
    0, 1, 2, 63, 64, 65 and 200 entries (the 64-entry batches, the odd tail after the two-in-flight loop) with one
    empty step, L in {1, 5, 64}, every column-chunk count's edge S, n_sel in {1, 5, 2049} (past 4 x 512: the grid
    stride) or the NULL map, ld = S + 3 and ldw = S + 5 over NaN.  Integer kind bitwise, real kind within
    frob_depth; the same bits twice."""
    from grf_amd.features import StepMatrices
    worst = 0.0
    for kind in R.KINDS:
        mats, rows, A, WA, B, WB, wt = SR.frob_case(L, S, n_sel, which, kind)
        ts = [torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)),
                                      torch.from_numpy(M.indices.astype(np.int64)),
                                      torch.from_numpy(M.data.astype(np.float32)), M.shape, dtype=torch.float32)
              for M in mats]
        steps = StepMatrices(ts, eng)
        assert steps.L == L
        rmap = None if rows is None else _t(rows.astype(np.int32), eng)
        bufs = (_padded(A, S + 3, eng, np.float64), _padded(WA, S + 5, eng, np.float64),
                _padded(B, S + 3, eng, np.float64), _padded(WB, S + 5, eng, np.float64), _t(wt, eng))
        got = _frob_raw(eng, steps, rmap, n_sel, bufs, S, L)
        assert _same_bits(_frob_raw(eng, steps, rmap, n_sel, bufs, S, L), got), kind
        ref, mag = SR.frob_ref(mats, rows, A, WA, B, WB, wt)
        if L >= 2:
            assert got[L // 2] == 0.0 and mag[L // 2] == 0.0         # the empty step
        if kind == "int":
            assert _same_bits(got, ref + 0.0), (kind, got, ref)
        else:
            depth = [SR.frob_depth(int(np.diff(M.indptr).max(initial=0)), n_sel, S) for M in mats]
            ok, ratio = _within(got, ref, mag, depth, U64)
            worst = max(worst, ratio)
            assert ok, (kind, ratio)
    print(f"steps_frob L={L} S={S} n_sel={n_sel} {which}: worst error / bound = {worst:.4f}")
