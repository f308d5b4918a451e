"""CPU: the diagonally preconditioned solves' entry points (purely additive to ABI 9): declared in the binding,
exported by the built library, and checked for their arguments before anything touches a device."""
import ctypes

import abi_contract

NEW = ["grf_gram_jacobi_f64", "grf_pcg_workspace_bytes", "grf_pcg_gram_solve_f64", "grf_pcg_gram_solve_lanczos_f64",
       "grf_pcg_poly_workspace_bytes", "grf_pcg_poly_solve_f64", "grf_pcg_poly_solve_lanczos_f64"]


def test_new_symbols_are_bound_and_exported():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_workspaces_hold_the_second_partial_sums():
    from grf_amd import _lib
    lib = _lib.load()
    for n_sys, n_cols, s in ((1, 1, 1), (600, 2708, 64), (100000, 100000, 256)):
        plain = lib.grf_cg_workspace_bytes(n_sys, n_cols, s)
        assert lib.grf_pcg_workspace_bytes(n_sys, n_cols, s) >= plain + 256 * s * 8 - 256
        plain = lib.grf_cg_poly_workspace_bytes(n_sys, n_cols, s)
        assert lib.grf_pcg_poly_workspace_bytes(n_sys, n_cols, s) >= plain + 256 * s * 8 - 256


# the four workspace sizes at (n_sys, n_cols | n, n_rhs), GRF_SPMM_TILE_BYTES unset: literals read from the build of the
# commit before the layouts were folded into one base layout (the engine sizes its buffers by these functions, so
# any moved or resized buffer shows here)
PINNED_WORKSPACES = {
    "grf_cg_workspace_bytes": (3840, 2749696, 1046936832),
    "grf_pcg_workspace_bytes": (5888, 2880768, 1047461120),
    "grf_cg_poly_workspace_bytes": (4352, 5522688, 1434136832),
    "grf_pcg_poly_workspace_bytes": (6400, 5653760, 1434661120),
}


def test_workspace_sizes_are_pinned():
    import os
    from grf_amd import _lib
    assert "GRF_SPMM_TILE_BYTES" not in os.environ, \
        "GRF_SPMM_TILE_BYTES is set: the sizes are pinned for the default tile budget (8 MiB); unset it"
    lib = _lib.load()
    shapes = ((1, 1, 1), (600, 2708, 64), (100000, 100000, 256))
    for name, sizes in PINNED_WORKSPACES.items():
        assert tuple(getattr(lib, name)(*a) for a in shapes) == sizes, name


def test_messages_name_the_entry_that_was_called():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    d = ctypes.c_void_p(8)  # (never dereferenced: a bad stride is refused before anything is read)
    tail = (0.1, d, 3, 4, 1.0, 5, d, 4, d, 1 << 40, None, None)   # ld_rhs = 3 < n_rhs = 4
    gram = (4, d, d, d, None, 8, d, d, d) + tail
    poly = (4, 8, d, d, d, d, d, d, d, 2, d, d) + tail
    for fn, args, family in ((lib.grf_cg_gram_solve_f64, gram + (None,), b"grf_cg_gram_solve"),
                             (lib.grf_pcg_gram_solve_f64, gram + (d, None), b"grf_pcg_gram_solve"),
                             (lib.grf_cg_poly_solve_f64, poly + (None,), b"grf_cg_poly_solve"),
                             (lib.grf_pcg_poly_solve_f64, poly + (d, None), b"grf_pcg_poly_solve")):
        assert fn(*args) == _lib.GRF_EINVAL
        err = lib.grf_last_error()
        assert b"strides" in err and err.startswith(family), err


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    d = ctypes.c_void_p(8)  # (never dereferenced: every call below is refused by its argument checks)
    big = 1 << 40

    def gram(lanczos=False, n_sys=4, n_rhs=4, ld_rhs=4, ldx=4, max_iter=5, ws=d, ws_bytes=big, dinv=d, coef=d,
             ld_coef=4, rhs=d):
        head = (n_sys, d, d, d, None, 8, d, d, d, 0.1, rhs, ld_rhs, n_rhs, 1.0, max_iter, d, ldx, ws, ws_bytes, None,
                None)
        if lanczos:
            return lib.grf_pcg_gram_solve_lanczos_f64(*head, coef, ld_coef, dinv, None)
        return lib.grf_pcg_gram_solve_f64(*head, dinv, None)

    def poly(lanczos=False, n_sys=4, n_rhs=4, ld_rhs=4, ldx=4, max_iter=5, ws=d, ws_bytes=big, dinv=d, coef=d,
             ld_coef=4, inv=d):
        head = (n_sys, 8, d, d, d, d, d, d, d, 2, d, inv, 0.1, d, ld_rhs, n_rhs, 1.0, max_iter, d, ldx, ws, ws_bytes,
                None, None)
        if lanczos:
            return lib.grf_pcg_poly_solve_lanczos_f64(*head, coef, ld_coef, dinv, None)
        return lib.grf_pcg_poly_solve_f64(*head, dinv, None)

    for fn in (gram, poly):
        for lz in (False, True):
            assert fn(lz, dinv=None) == _lib.GRF_EINVAL
            assert b"pcg" in lib.grf_last_error()
            assert fn(lz, n_rhs=0, ld_rhs=0, ldx=0, ld_coef=0) == _lib.GRF_EUNSUPPORTED
            assert fn(lz, n_rhs=257, ld_rhs=257, ldx=257, ld_coef=257) == _lib.GRF_EUNSUPPORTED
            assert b"n_rhs" in lib.grf_last_error()
            assert fn(lz, ld_rhs=3) == _lib.GRF_EINVAL
            assert fn(lz, ldx=3) == _lib.GRF_EINVAL
            assert fn(lz, max_iter=-1) == _lib.GRF_EINVAL
            assert b"strides" in lib.grf_last_error()
            assert fn(lz, ws_bytes=8) == _lib.GRF_EINVAL
            assert b"workspace" in lib.grf_last_error()
            assert fn(lz, ws=None) == _lib.GRF_EINVAL
            assert fn(lz, n_sys=0) == _lib.GRF_EINVAL
        assert fn(True, coef=None) == _lib.GRF_EINVAL
        assert fn(True, ld_coef=3) == _lib.GRF_EINVAL
        assert b"coefficient" in lib.grf_last_error()
    assert gram(rhs=None) == _lib.GRF_EINVAL
    assert poly(inv=None) == _lib.GRF_EINVAL
    # the plain workspace is too short for the preconditioned solve (the second partial sums)
    assert gram(n_rhs=256, ld_rhs=256, ldx=256, ws_bytes=lib.grf_cg_workspace_bytes(4, 8, 256)) == _lib.GRF_EINVAL
    assert poly(n_rhs=256, ld_rhs=256, ldx=256, ws_bytes=lib.grf_cg_poly_workspace_bytes(4, 8, 256)) == _lib.GRF_EINVAL

    # the Jacobi kernel's checks
    assert lib.grf_gram_jacobi_f64(4, None, d, d, None, 0.1, d, None) == _lib.GRF_EINVAL
    assert lib.grf_gram_jacobi_f64(4, d, d, d, None, 0.1, None, None) == _lib.GRF_EINVAL
    assert lib.grf_gram_jacobi_f64(-1, d, d, d, None, 0.1, d, None) == _lib.GRF_EINVAL
    assert lib.grf_gram_jacobi_f64(4, d, d, d, None, -0.1, d, None) == _lib.GRF_EINVAL
    assert b"grf_gram_jacobi_f64" in lib.grf_last_error()
    assert lib.grf_gram_jacobi_f64(0, d, d, d, None, 0.1, None, None) == _lib.GRF_OK   # nothing to do, nothing touched
