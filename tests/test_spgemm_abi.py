"""CPU: the SpGEMM's three entry points are an additive part of ABI 9 -- declared in the header, listed in
the binding, exported by the built library -- their GRF_SPGEMM_* constants agree between the header and the
binding, and their arguments are checked before anything touches a device."""
import ctypes
import os
import re

import abi_contract

NEW = ["grf_spgemm_workspace_bytes", "grf_spgemm_csr_count", "grf_spgemm_csr_fill"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grf.h")


def _header() -> str:
    with open(HEADER) as fh:
        return fh.read()


def test_header_declares_the_entry_points_with_their_reference_lines():
    text = _header()
    for name in NEW:
        assert re.search(r"\b(size_t|int32_t)\s+" + name + r"\s*\(", text), name
    assert "general_kernel_pofm.py:7-42" in text
    assert re.search(r"#define\s+GRF_ABI_VERSION\s+9\b", text)


def test_symbols_are_bound_and_exported_and_the_abi_is_still_9():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_constants_agree_between_header_and_binding():
    from grf_amd import _lib
    macros = dict(re.findall(r"#define\s+GRF_SPGEMM_(\w+)\s+(\d+)", _header()))
    assert set(macros) == {"SORT_PRODUCTS", "ACC_SLOTS", "BIG_MIN_WAVES", "BIG_MAX_WAVES"}
    for name, value in macros.items():
        assert getattr(_lib, "SPGEMM_" + name) == int(value), name
    bound = {k for k in dir(_lib) if k.startswith("SPGEMM_")}
    assert bound == {"SPGEMM_" + k for k in macros}


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    d = ctypes.c_void_p(8)  # (never dereferenced: every call below is refused by its argument checks)
    need = lib.grf_spgemm_workspace_bytes(5, 7, 1000)
    # counters + the row queue + at least one wave's bitmap (n_cols bits) and ranks (an int32 per 64 columns)
    assert need >= 256 + 5 * 4 + 1000 // 8 + 1000 // 16
    assert lib.grf_spgemm_workspace_bytes(5, 7, 1 << 20) > need
    assert lib.grf_spgemm_workspace_bytes(5, 70, 1000) == need  # (n_mid does not enter)

    def count(n_rows=5, n_mid=7, n_cols=1000, a_ptr=d, cnt=d, ws=d, ws_bytes=need):
        return lib.grf_spgemm_csr_count(n_rows, n_mid, n_cols, a_ptr, d, d, d, cnt, ws, ws_bytes, None)

    def fill(n_rows=5, n_mid=7, n_cols=1000, c_ptr=d, c_idx=d, c_val=d, ws=d, ws_bytes=need):
        return lib.grf_spgemm_csr_fill(n_rows, n_mid, n_cols, d, d, d, d, d, d, c_ptr, c_idx, c_val, None, ws,
                                       ws_bytes, None)

    for call in (count, fill):
        assert call(n_rows=-1) == _lib.GRF_EINVAL
        assert call(n_cols=1 << 31) == _lib.GRF_EUNSUPPORTED
        assert call(n_mid=1 << 31) == _lib.GRF_EUNSUPPORTED
        assert call(ws=None) == _lib.GRF_EINVAL
        assert call(ws_bytes=need - 1) == _lib.GRF_EINVAL
        assert b"workspace" in lib.grf_last_error()
    assert count(a_ptr=None) == _lib.GRF_EINVAL
    assert count(cnt=None) == _lib.GRF_EINVAL
    assert fill(c_ptr=None) == _lib.GRF_EINVAL
    assert fill(c_idx=None) == _lib.GRF_EINVAL
    assert fill(c_val=None) == _lib.GRF_EINVAL
