"""CPU: the walk polynomial operator's entry points are an additive part of ABI 9 -- declared in the header
with the reference lines they serve, listed in the binding, exported by the built library -- and their
arguments are checked before anything touches a device."""
import ctypes
import os
import re

import abi_contract

NEW = ["grf_poly_workspace_bytes", "grf_poly_apply_f64", "grf_cg_poly_workspace_bytes", "grf_cg_poly_solve_f64",
       "grf_cg_poly_solve_lanczos_f64", "grf_poly_grad_workspace_bytes", "grf_poly_grad_f64"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grf.h")


def _header() -> str:
    with open(HEADER) as fh:
        return fh.read()


def test_header_declares_the_entry_points_with_their_reference_lines_and_the_order_rule():
    text = _header()
    for name in NEW:
        assert re.search(r"\b(size_t|int32_t)\s+" + name + r"\s*\(", text), name
    section = text[text.index("the exact walk-power kernel as a matrix-free operator"):]
    for cite in ("general_kernel_pofm.py:7-42", "general_kernel_pofm.py:45-96", "models/sparse_grf_model.py:21-45"):
        assert cite in section, cite
    assert "Order rule" in section and "+0.0" in section
    assert re.search(r"#define\s+GRF_ABI_VERSION\s+9\b", text)


def test_symbols_are_bound_and_exported_and_the_abi_is_still_9():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_workspace_sizes():
    from grf_amd import _lib
    lib = _lib.load()
    assert lib.grf_poly_workspace_bytes(1000, 1, 65) == 0 == lib.grf_poly_workspace_bytes(1000, 2, 65)
    assert lib.grf_poly_workspace_bytes(1000, 3, 65) >= 2 * 1000 * 65 * 8
    assert lib.grf_poly_workspace_bytes(1000, 8, 65) == lib.grf_poly_workspace_bytes(1000, 3, 65)
    # R, P, Y, X of the recurrence and three n x S blocks of the chains
    assert lib.grf_cg_poly_workspace_bytes(600, 1000, 65) >= (4 * 600 + 3 * 1000) * 65 * 8
    assert lib.grf_poly_grad_workspace_bytes(1000, 65) >= 6 * 1000 * 65 * 8 + 256


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    d = ctypes.c_void_p(8)  # (never dereferenced: every call below is refused by its argument checks)
    EINVAL, EUNSUP = _lib.GRF_EINVAL, _lib.GRF_EUNSUPPORTED

    need = lib.grf_poly_workspace_bytes(10, 4, 3)

    def apply(n=10, ptr=d, f=d, n_f=4, row_map=d, n_out=5, X=d, ldx=3, n_rhs=3, Y=d, ldy=3, ws=d, ws_bytes=need):
        return lib.grf_poly_apply_f64(n, ptr, d, d, f, n_f, None, row_map, n_out, X, ldx, n_rhs, Y, ldy, ws,
                                      ws_bytes, None)

    assert apply(n=0) == EINVAL and apply(ptr=None) == EINVAL and apply(f=None) == EINVAL
    assert apply(n_f=0) == EINVAL and apply(X=None) == EINVAL and apply(Y=None) == EINVAL
    assert apply(row_map=None, n_out=5) == EINVAL      # (all rows: n_out must be n)
    assert apply(n=1 << 31) == EUNSUP
    assert apply(n_rhs=0) == EUNSUP and apply(n_rhs=257, ldx=300, ldy=300) == EUNSUP
    assert apply(ldx=2) == EINVAL and apply(ldy=2) == EINVAL
    assert apply(ws=None) == EINVAL and apply(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()

    cneed = lib.grf_cg_poly_workspace_bytes(5, 10, 3)

    def solve(lanczos, n_sys=5, n=10, g=d, gt=d, f=d, n_f=4, row_map=d, inv_map=d, rhs=d, ld_rhs=3, n_rhs=3,
              max_iter=4, x=d, ldx=3, ws=d, ws_bytes=cneed, coef=d, ld_coef=3):
        head = (n_sys, n, g, d, d, gt, d, d, f, n_f, row_map, inv_map, 0.1, rhs, ld_rhs, n_rhs, 1.0, max_iter, x,
                ldx, ws, ws_bytes, None, None)
        if lanczos:
            return lib.grf_cg_poly_solve_lanczos_f64(*head, coef, ld_coef, None)
        return lib.grf_cg_poly_solve_f64(*head, None)

    for lz in (False, True):
        assert solve(lz, n_sys=0) == EINVAL and solve(lz, n=0) == EINVAL
        assert solve(lz, g=None) == EINVAL and solve(lz, gt=None) == EINVAL and solve(lz, f=None) == EINVAL
        assert solve(lz, n_f=0) == EINVAL and solve(lz, row_map=None) == EINVAL and solve(lz, inv_map=None) == EINVAL
        assert solve(lz, rhs=None) == EINVAL and solve(lz, x=None) == EINVAL
        assert solve(lz, n=1 << 31) == EUNSUP
        assert solve(lz, n_rhs=257, ld_rhs=300, ldx=300, ld_coef=300) == EUNSUP and solve(lz, n_rhs=0) == EUNSUP
        assert solve(lz, ld_rhs=2) == EINVAL and solve(lz, ldx=2) == EINVAL and solve(lz, max_iter=-1) == EINVAL
        assert solve(lz, ws=None) == EINVAL and solve(lz, ws_bytes=cneed - 1) == EINVAL
        assert b"workspace" in lib.grf_last_error()
    assert solve(True, coef=None) == EINVAL and solve(True, ld_coef=2) == EINVAL

    gneed = lib.grf_poly_grad_workspace_bytes(10, 3)

    def grad(n=10, gt=d, f=d, n_f=4, n_sel=5, inv_map=d, A=d, B=d, ld=3, wt=d, n_rhs=3, out=d, ws=d, ws_bytes=gneed):
        return lib.grf_poly_grad_f64(n, gt, d, d, f, n_f, n_sel, inv_map, A, B, ld, wt, n_rhs, out, ws, ws_bytes,
                                     None)

    assert grad(n=0) == EINVAL and grad(n_sel=0) == EINVAL and grad(gt=None) == EINVAL and grad(f=None) == EINVAL
    assert grad(n_f=0) == EINVAL and grad(inv_map=None) == EINVAL and grad(A=None) == EINVAL
    assert grad(B=None) == EINVAL and grad(wt=None) == EINVAL and grad(out=None) == EINVAL
    assert grad(n=1 << 31) == EUNSUP
    assert grad(n_rhs=0) == EUNSUP and grad(n_rhs=257, ld=300) == EUNSUP
    assert grad(ld=2) == EINVAL
    assert grad(ws=None) == EINVAL and grad(ws_bytes=gneed - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()
