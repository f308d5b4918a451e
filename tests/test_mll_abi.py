"""CPU: ABI 9 adds the marginal likelihood's two entry points (and the contraction's workspace
companion): declared in the binding, exported by the built library, and checked for their arguments
before anything touches a device."""
import ctypes

import abi_contract

NEW = ["grf_cg_gram_solve_lanczos_f64", "grf_steps_frob_f64", "grf_steps_frob_workspace_bytes"]


def test_new_symbols_are_bound_and_exported():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_steps_frob_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    assert lib.grf_steps_frob_workspace_bytes(1, 1) >= 256 + 8
    assert lib.grf_steps_frob_workspace_bytes(1 << 20, 64) >= 256 + 64 * 8
    one = (ctypes.c_void_p * 1)(8)
    p = one  # (a host array: the harness sends its bytes, not this process's address)
    d = ctypes.c_void_p(8)  # (never dereferenced: every call below is refused by its argument checks)

    def call(n_sel=4, L=1, ld=4, ldw=4, n_rhs=4, out=d, ws=d, ws_bytes=1 << 20):
        return lib.grf_steps_frob_f64(n_sel, L, p, p, p, None, d, d, ld, d, d, ldw, d, n_rhs, out, ws, ws_bytes, None)

    assert call(n_rhs=257, ld=257, ldw=257) == _lib.GRF_EUNSUPPORTED
    assert call(L=65) == _lib.GRF_EUNSUPPORTED
    assert call(n_rhs=0) == _lib.GRF_EINVAL
    assert call(ld=3) == _lib.GRF_EINVAL
    assert call(ldw=3) == _lib.GRF_EINVAL
    assert call(out=None) == _lib.GRF_EINVAL
    assert call(ws_bytes=8) == _lib.GRF_EINVAL
    assert b"workspace" in lib.grf_last_error()
    assert call(n_sel=-1) == _lib.GRF_EINVAL
