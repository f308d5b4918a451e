"""CPU: the walk operator's K-block entry points are an additive part of ABI 9 -- declared in the header with the
reference lines they serve, listed in the binding, exported by the built library -- and their arguments are
checked before anything touches a device."""
import ctypes
import os
import re

import abi_contract

NEW = ["grf_poly_kernel_block_workspace_bytes", "grf_poly_kernel_block_f64", "grf_poly_kernel_diag_workspace_bytes",
       "grf_poly_kernel_diag_f64", "grf_poly_kernel_grad_workspace_bytes", "grf_poly_kernel_grad_f64"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grf.h")


def test_header_declares_the_entry_points_under_the_unchanged_order_rule():
    with open(HEADER) as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\b(size_t|int32_t)\s+" + name + r"\s*\(", text), name
    section = text[text.index("K blocks, diagonals and their modulator gradients from the operator"):]
    assert "general_kernel_pofm.py:45-96" in section and "Unit columns" in section and "bit-identical" in section
    assert text.count("Order rule.") == 1   # (stated once; the new entry points follow it unchanged)
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
    blk = 1000 * 256 * 8
    # Psi, and the chains' two intermediates from n_f = 3 on; a block of min(n2, 256) columns
    assert blk <= lib.grf_poly_kernel_block_workspace_bytes(1000, 2, 5000) < 2 * blk
    assert 3 * blk <= lib.grf_poly_kernel_block_workspace_bytes(1000, 3, 5000) < 4 * blk
    assert lib.grf_poly_kernel_block_workspace_bytes(1000, 8, 256) == lib.grf_poly_kernel_block_workspace_bytes(1000, 3, 257)
    assert 3 * 1000 * 65 * 8 <= lib.grf_poly_kernel_block_workspace_bytes(1000, 3, 65) < 3 * blk
    # the ticket and one partial per (block, column); the intermediates from n_f = 3 on, Psi never
    assert 256 + 250 * 65 * 8 <= lib.grf_poly_kernel_diag_workspace_bytes(1000, 2, 65) < 1000 * 65 * 8
    assert lib.grf_poly_kernel_diag_workspace_bytes(1000, 3, 65) >= 2 * 1000 * 65 * 8
    # Psi, two Krylov blocks and the transposed cotangent (not for the diagonal)
    assert lib.grf_poly_kernel_grad_workspace_bytes(1000, 300, 65, 0) >= 3 * 1000 * 256 * 8 + 300 * 65 * 8
    assert lib.grf_poly_kernel_grad_workspace_bytes(1000, 65, 0, 1) >= 3 * 1000 * 65 * 8
    assert lib.grf_poly_kernel_grad_workspace_bytes(1000, 65, 0, 1) < 4 * 1000 * 65 * 8 + 4096


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    d = ctypes.c_void_p(8)  # (never dereferenced: every call below is refused or returns before any device work)
    EINVAL, EUNSUP, OK = _lib.GRF_EINVAL, _lib.GRF_EUNSUPPORTED, 0

    bneed = lib.grf_poly_kernel_block_workspace_bytes(10, 4, 3)

    def block(n=10, g=d, gt=d, f=d, n_f=4, x1=d, n1=5, x2=d, n2=3, K=d, ldk=3, ws=d, ws_bytes=bneed):
        return lib.grf_poly_kernel_block_f64(n, g, d, d, gt, d, d, f, n_f, x1, n1, x2, n2, K, ldk, ws, ws_bytes, None)

    assert block(n=0) == EINVAL and block(g=None) == EINVAL and block(gt=None) == EINVAL and block(f=None) == EINVAL
    assert block(n_f=0) == EINVAL and block(n1=-1) == EINVAL and block(n2=-1) == EINVAL
    assert block(x1=None) == EINVAL and block(x2=None) == EINVAL and block(K=None) == EINVAL and block(ldk=2) == EINVAL
    assert block(n=1 << 31) == EUNSUP and block(n1=1 << 31) == EUNSUP
    assert block(ws=None) == EINVAL and block(ws_bytes=bneed - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()
    assert block(n1=0, K=None, ws=None) == OK and block(n2=0, ldk=0, K=None, ws=None) == OK   # (nothing touched)

    dneed = lib.grf_poly_kernel_diag_workspace_bytes(10, 4, 3)

    def diag(n=10, gt=d, f=d, n_f=4, x=d, n_x=3, out=d, ws=d, ws_bytes=dneed):
        return lib.grf_poly_kernel_diag_f64(n, gt, d, d, f, n_f, x, n_x, out, ws, ws_bytes, None)

    assert diag(n=0) == EINVAL and diag(gt=None) == EINVAL and diag(f=None) == EINVAL and diag(n_f=0) == EINVAL
    assert diag(x=None) == EINVAL and diag(out=None) == EINVAL and diag(n_x=-1) == EINVAL
    assert diag(n=1 << 31) == EUNSUP
    assert diag(ws=None) == EINVAL and diag(ws_bytes=dneed - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()
    assert diag(n_x=0, out=None, ws=None) == OK

    gneed = lib.grf_poly_kernel_grad_workspace_bytes(10, 5, 3, 0)

    def grad(n=10, gt=d, f=d, n_f=4, x1=d, n1=5, inv1=d, x2=d, n2=3, inv2=d, g=d, ldg=3, dg=0, out=d, ws=d,
             ws_bytes=gneed):
        return lib.grf_poly_kernel_grad_f64(n, gt, d, d, f, n_f, x1, n1, inv1, x2, n2, inv2, g, ldg, dg, out, ws,
                                            ws_bytes, None)

    assert grad(n=0) == EINVAL and grad(gt=None) == EINVAL and grad(f=None) == EINVAL and grad(n_f=0) == EINVAL
    assert grad(out=None) == EINVAL and grad(x1=None) == EINVAL and grad(g=None) == EINVAL
    assert grad(inv1=None) == EINVAL and grad(x2=None) == EINVAL and grad(inv2=None) == EINVAL and grad(ldg=2) == EINVAL
    assert grad(n=1 << 31) == EUNSUP
    assert grad(ws=None) == EINVAL and grad(ws_bytes=gneed - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()
    assert grad(dg=1, inv1=None, x2=None, inv2=None, ws=None) == EINVAL   # (the diagonal form needs no maps)
    assert b"workspace" in lib.grf_last_error()
