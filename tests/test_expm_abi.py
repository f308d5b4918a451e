"""CPU: the exact diffusion kernel's entry points (grf_gemm_nt_f64, grf_expm_sym_f64 and their helpers) are an
additive part of ABI 9 -- declared in the header with the reference lines they serve and their order rules,
listed in the binding, exported by the built library -- and their arguments are checked before anything
touches a device."""
import ctypes
import os
import re

import expm_reference as R

import abi_contract

NEW = ["grf_gemm_nt_f64_workspace_bytes", "grf_gemm_nt_f64", "grf_expm_squarings", "grf_expm_sym_f64_workspace_bytes",
       "grf_expm_sym_f64"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grf.h")


def test_header_declares_the_entry_points_with_their_reference_lines_and_the_order_rules():
    with open(HEADER) as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\b(size_t|int32_t)\s+" + name + r"\s*\(", text), name
    section = text[text.index("the exact diffusion kernel exp(-beta L) on the fp64 matrix cores"):]
    for cite in ("graph_kernels/diffusion_kernel.py:6-12", "gpflow_kernels/diffusion_kernel_exact.py:6-46"):
        assert cite in section, cite
    assert section.count("Order rule") >= 2 and "17 + s products" in section and "v_mfma_f64_16x16x4_f64" in section
    assert re.search(r"#define\s+GRF_ABI_VERSION\s+9\b", text)


def test_symbols_are_bound_and_exported_and_the_abi_is_still_9():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_the_kernel_is_in_the_build():
    with open(os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd", "csrc", "Makefile")) as fh:
        assert "grf_expm.hip" in fh.read()
    from grf_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        assert b"gemm_nt_f64_kernel" in fh.read()


def test_workspace_sizes_are_positive_and_monotone():
    from grf_amd import _lib
    lib = _lib.load()
    sizes = [1, 2, 3, 127, 128, 129, 300, 1100, 2708, 8192]
    e = [lib.grf_expm_sym_f64_workspace_bytes(n) for n in sizes]
    g = [lib.grf_gemm_nt_f64_workspace_bytes(n, n) for n in sizes]
    assert all(x > 0 for x in e + g)
    assert e == sorted(e) and g == sorted(g)
    for n, x in zip(sizes, e):
        assert x >= 3 * n * n * 8  # X and the two ping-pong buffers
    # the ticket and one fp64 partial per 128 x 128 tile
    assert lib.grf_gemm_nt_f64_workspace_bytes(129, 300) >= 256 + 2 * 3 * 8
    assert lib.grf_gemm_nt_f64_workspace_bytes(300, 129) == lib.grf_gemm_nt_f64_workspace_bytes(129, 300)


def test_squarings_agree_with_the_restatement():
    from grf_amd import _lib
    lib = _lib.load()
    for rho in (0.0, 1e-300, 0.2, 1.0, 1.0000000001, 1.5, 2.0, 3.0, 4.0, 4.1, 800.0, 1024.0, 239200.0, 2.0 ** 60):
        assert lib.grf_expm_squarings(rho) == R.squarings(rho), rho
    assert lib.grf_expm_squarings(float("inf")) == -1 == lib.grf_expm_squarings(float("nan"))


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    EINVAL, EUNSUP = _lib.GRF_EINVAL, _lib.GRF_EUNSUPPORTED
    a, b, c, w = (ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20),
                  ctypes.c_void_p(4 << 20))  # (never dereferenced: every call below is refused)
    need = lib.grf_gemm_nt_f64_workspace_bytes(10, 12)

    def gemm(n1=10, n2=12, nk=7, A=a, lda=7, a_rows=10, ra=None, B=b, ldb=7, b_rows=12, rb=None, Z=None, ldz=12,
             C=c, ldc=12, sym=0, W=None, ldw=12, out=None, ws=None, ws_bytes=0):
        return lib.grf_gemm_nt_f64(n1, n2, nk, 1.0, A, lda, a_rows, ra, B, ldb, b_rows, rb, 1.0, Z, ldz, 0.0, C, ldc,
                                   sym, W, ldw, out, ws, ws_bytes, None)

    assert gemm(n1=-1) == EINVAL and gemm(nk=-1) == EINVAL and gemm(n1=1 << 31) == EUNSUP
    assert gemm(n1=0) == 0 and gemm(n2=0) == 0  # (touches nothing)
    assert gemm(A=None) == EINVAL and gemm(B=None) == EINVAL and gemm(lda=6) == EINVAL and gemm(ldb=6) == EINVAL
    assert gemm(a_rows=9) == EINVAL and gemm(ra=w, a_rows=0) == EINVAL
    assert gemm(C=None) == EINVAL and gemm(ldc=11) == EINVAL and gemm(Z=w, ldz=11) == EINVAL
    assert gemm(sym=1) == EINVAL                                      # n1 != n2
    assert gemm(n2=10, b_rows=10, ldc=10, sym=1, ra=w) == EINVAL      # maps in the symmetric mode
    assert gemm(n2=10, b_rows=10, ldc=10, sym=1, W=w, ldw=10, out=w, ws=w, ws_bytes=need) == EINVAL
    assert b"symmetric" in lib.grf_last_error()
    assert gemm(C=a) == EINVAL and gemm(C=ctypes.c_void_p((1 << 20) + 8)) == EINVAL  # C overlaps A
    assert gemm(C=ctypes.c_void_p((2 << 20) - 8)) == EINVAL                          # C's end overlaps B's start
    assert b"overlaps" in lib.grf_last_error()
    assert gemm(Z=ctypes.c_void_p((3 << 20) + 8)) == EINVAL and gemm(Z=c, ldz=13) == EINVAL  # a partial alias
    assert gemm(W=w, out=None, ws=w, ws_bytes=need) == EINVAL and gemm(W=w, ldw=11, out=w, ws=w, ws_bytes=need) == EINVAL
    assert gemm(W=w, out=w, ws=None, ws_bytes=need) == EINVAL and gemm(W=w, out=w, ws=w, ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()

    eneed = lib.grf_expm_sym_f64_workspace_bytes(10)

    def expm(n=10, L=a, ldl=10, beta=2.0, rho=4.0, E=b, lde=10, ws=c, ws_bytes=eneed):
        return lib.grf_expm_sym_f64(n, L, ldl, beta, rho, E, lde, ws, ws_bytes, None)

    assert expm(n=0) == EINVAL and expm(L=None) == EINVAL and expm(E=None) == EINVAL
    assert expm(ldl=9) == EINVAL and expm(lde=9) == EINVAL and expm(n=1 << 31, ldl=1 << 31, lde=1 << 31) == EUNSUP
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert expm(beta=bad) == EINVAL, bad
    assert expm(rho=float("inf")) == EINVAL and expm(rho=float("nan")) == EINVAL and expm(rho=2.0 ** 80) == EINVAL
    assert expm(ws=None) == EINVAL and expm(ws_bytes=eneed - 1) == EINVAL
    assert b"workspace" in lib.grf_last_error()
    assert expm(E=a) == EINVAL and expm(E=c) == EINVAL and expm(L=c) == EINVAL
    assert b"overlap" in lib.grf_last_error()
