"""CPU: the exact posterior's entry points (grf_posterior_rhs_f64, grf_posterior_reduce_f64 and its workspace
size) are an additive part of ABI 9 -- declared in the header with the reference lines they serve and their order
rules, listed in the binding, exported by the built library -- and their arguments are checked before anything
touches a device."""
import ctypes
import os
import re

import abi_contract

NEW = ["grf_posterior_rhs_f64", "grf_posterior_reduce_workspace_bytes", "grf_posterior_reduce_f64"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grf.h")


def test_header_declares_the_entry_points_with_their_reference_lines_and_the_order_rules():
    with open(HEADER) as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\b(size_t|int32_t)\s+" + name + r"\s*\(", text), name
    section = text[text.index("the exact posterior mean and variance (predict_f)"):]
    for cite in ("wind_experiment.py:396-398", "run_scaling_experiment.py:621", "run_scaling_experiment.py:729",
                 "wind_experiment.py:319-324"):
        assert cite in section, cite
    assert section.count("Order rule") >= 2 and "never clamped" in section
    assert re.search(r"#define\s+GRF_ABI_VERSION\s+9\b", text)


def test_symbols_are_bound_and_exported_and_the_abi_is_still_9():
    from grf_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION


def test_the_kernels_are_in_the_build():
    with open(os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd", "csrc", "Makefile")) as fh:
        assert "grf_posterior.hip" in fh.read()
    from grf_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        blob = fh.read()
    assert b"posterior_reduce_kernel" in blob and b"posterior_rhs_kernel" in blob


def test_workspace_size_is_positive_and_monotone():
    from grf_amd import _lib
    lib = _lib.load()
    ns = [0, 1, 63, 64, 65, 257, 1025, 70001, 1 << 20, (1 << 31) - 1]
    Ss = [1, 2, 5, 63, 64, 65, 128, 129, 256]
    for S in Ss:
        w = [lib.grf_posterior_reduce_workspace_bytes(n, S) for n in ns]
        assert all(x >= 256 + 2 * S * 8 for x in w) and w == sorted(w), S
        assert w[-1] >= 256 + 256 * 2 * S * 8                    # one partial pair per (row block, column)
    for n in ns:
        w = [lib.grf_posterior_reduce_workspace_bytes(n, S) for S in Ss]
        assert w == sorted(w), n
    assert lib.grf_posterior_reduce_workspace_bytes(-5, 0) > 0 and lib.grf_posterior_reduce_workspace_bytes(10, 1000) > 0


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    lib = abi_contract.device_less_lib()  # (made-up pointers: never in a process that sees a GPU)
    EINVAL, EUNSUP = _lib.GRF_EINVAL, _lib.GRF_EUNSUPPORTED
    P = lambda k: ctypes.c_void_p(k << 24)  # noqa: E731  (never dereferenced: every call below is refused or empty)
    b, x, al, pr, va, me, ws = (P(k) for k in range(1, 8))
    need = lib.grf_posterior_reduce_workspace_bytes(100, 7)

    def red(n=100, S=7, B=b, ldb=7, X=x, ldx=9, alpha=al, prior=pr, var=va, mean=me, w=ws, wb=need):
        return lib.grf_posterior_reduce_f64(n, S, B, ldb, X, ldx, alpha, prior, 0.0, var, mean, w, wb, None)

    assert red(n=-1) == EINVAL and red(S=-1) == EINVAL
    assert red(S=257, ldb=300, ldx=300) == EUNSUP and red(n=1 << 31) == EUNSUP
    assert red(S=0) == 0 and red(n=0, S=0) == 0                                      # (touches nothing)
    assert red(B=None) == EINVAL and red(X=None) == EINVAL and red(prior=None) == EINVAL and red(var=None) == EINVAL
    assert red(alpha=None) == EINVAL and red(mean=None) == EINVAL                    # nullable together only
    assert b"together" in lib.grf_last_error()
    assert red(ldb=6) == EINVAL and red(ldx=6) == EINVAL
    assert b"pitch" in lib.grf_last_error()
    assert red(w=None) == EINVAL and red(wb=need - 1) == EINVAL and red(wb=0) == EINVAL
    assert b"workspace" in lib.grf_last_error()
    at = lambda base, off: ctypes.c_void_p(base.value + off)  # noqa: E731
    assert red(var=b) == EINVAL and red(var=at(b, (99 * 7 + 6) * 8)) == EINVAL       # B's first and last entry
    assert red(mean=at(x, (99 * 9 + 6) * 8)) == EINVAL and red(var=at(x, -6 * 8)) == EINVAL
    assert red(var=at(al, 99 * 8)) == EINVAL and red(mean=pr) == EINVAL and red(var=at(pr, 6 * 8)) == EINVAL
    assert red(var=at(ws, need - 8)) == EINVAL and red(mean=ws) == EINVAL
    assert red(mean=at(va, 6 * 8)) == EINVAL and red(mean=va) == EINVAL
    assert b"overlaps" in lib.grf_last_error()

    ptr, idx, val, nodes, E, prior = (P(k) for k in range(8, 14))

    def rhs(n_rows=50, p=ptr, i=idx, v=val, n_cols=40, nd=nodes, S=7, e=E, lde=8, pri=prior):
        return lib.grf_posterior_rhs_f64(n_rows, p, i, v, n_cols, nd, S, e, lde, pri, None)

    assert rhs(n_rows=-1) == EINVAL and rhs(n_cols=-1) == EINVAL and rhs(S=-1) == EINVAL
    assert rhs(S=257, lde=300) == EUNSUP and rhs(n_rows=1 << 31) == EUNSUP and rhs(n_cols=1 << 31) == EUNSUP
    assert rhs(S=0) == 0                                                             # (touches nothing)
    assert rhs(p=None) == EINVAL and rhs(nd=None) == EINVAL and rhs(pri=None) == EINVAL and rhs(e=None) == EINVAL
    assert rhs(lde=6) == EINVAL
    assert b"lde" in lib.grf_last_error()
    assert rhs(pri=E) == EINVAL and rhs(pri=at(E, (39 * 8 + 6) * 8)) == EINVAL and rhs(e=at(prior, -8)) == EINVAL
    assert rhs(pri=at(nodes, 24)) == EINVAL and rhs(e=at(nodes, -8)) == EINVAL and rhs(e=at(ptr, 50 * 8)) == EINVAL
    assert b"overlaps" in lib.grf_last_error()
