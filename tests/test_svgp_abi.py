"""CPU: the SVGP classification's entry points (grf_robustmax_ve_f64, grf_robustmax_predict_f64, grf_rows_sqsum_f64)
live in a header of their own, include/grf_svgp.h -- declared there with the notebook and GPflow lines they serve and
each kernel's order rule, bound by the binding through a mapping of their own, exported by the built library --
while include/grf.h, its ABI revision, ``SIGNATURES``, ``exported_symbols()`` and ``exported_symbols_dense_solve()``
name exactly what they named before; and their arguments are checked before anything touches a device.

The refusals are exercised with made-up pointers that are never dereferenced, under tests/abi_contract.py's one
rule: never in a process that can see a GPU.  Where this process sees one, the same function runs in a child
started without visible devices (this file, ``--refusals``)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NEW = ["grf_robustmax_ve_f64", "grf_robustmax_predict_f64", "grf_rows_sqsum_f64"]
HEADER = os.path.join(ROOT, "include", "grf_svgp.h")
GRF_H = os.path.join(ROOT, "include", "grf.h")
DENSE_SOLVE_H = os.path.join(ROOT, "include", "grf_dense_solve.h")


def test_header_declares_the_entry_points_with_their_citations_and_order_rules():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r'#include\s+"grf.h"', text)
    assert "GRF_ABI_VERSION" in text and not re.search(r"#define\s+GRF_ABI_VERSION", text)
    for name in NEW:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", text), name
    flat = re.sub(r"\s*\n \*\s*", " ", text)  # (comment lines joined)
    for cite in ("experiments/dense/cora/classification_multiple_{GRF,GRF_small,diff,diff_small}.ipynb",
                 "gpflow.likelihoods.MultiClass(num_classes=7)", "gpflow.models.SVGP(", "whiten=True",
                 "likelihoods/multiclass.py", "RobustMax.prob_is_largest", "MultiClass._variational_expectations",
                 "_predict_non_logged_density", "MultiClass._predict_mean_and_var",
                 "numpy.polynomial.hermite.hermgauss"):
        assert cite in flat, cite
    assert "Order rule" in text
    for phrase in ("ascending c", "pairwise tree", "no floating-point atomics", "two calls give the same bits",
                   "full product divided by C_ic", "ascending j", "never read or written",
                   "A label outside [0, P) gives NaN", "gets gradient 0"):
        assert phrase in flat, phrase
    assert re.search(r"#define\s+GRF_SVGP_MAX_CLASSES\s+64\b", text)
    assert re.search(r"#define\s+GRF_SVGP_MAX_GH\s+64\b", text)


def test_the_older_headers_are_untouched_by_the_new_names_and_grf_h_still_defines_abi_9():
    with open(GRF_H) as fh:
        text = fh.read()
    assert re.search(r"#define\s+GRF_ABI_VERSION\s+9\b", text)
    with open(DENSE_SOLVE_H) as fh:
        text += fh.read()
    for name in NEW:
        assert name not in text, name


def test_symbols_are_bound_and_exported_through_the_new_mapping_only():
    from grf_amd import _lib
    lib = _lib.load()
    assert _lib.exported_symbols_svgp() == sorted(NEW) == sorted(_lib.SVGP_SIGNATURES)
    for name in NEW:
        assert name not in _lib.SIGNATURES and name not in _lib.exported_symbols(), name
        assert name not in _lib.exported_symbols_dense_solve(), name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SVGP_SIGNATURES[name][1] and fn.restype is _lib.SVGP_SIGNATURES[name][0], name
    assert lib.grf_version() == 9 == _lib.ABI_VERSION
    assert (_lib.SVGP_MAX_CLASSES, _lib.SVGP_MAX_GH) == (64, 64)


def test_the_kernels_are_in_the_build():
    with open(os.path.join(PKG, "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert "grf_svgp.hip" in mk and "grf_svgp.h" in mk and "-ffp-contract=off" in mk
    from grf_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        data = fh.read()
    for kernel in (b"robustmax_ve_kernel", b"robustmax_predict_kernel", b"rows_sqsum_kernel"):
        assert kernel in data, kernel


def _p(k: int, off: int = 0) -> int:
    """Made-up device pointer number k (16 MiB apart, never dereferenced)."""
    return (k << 24) + off


def _refusals() -> None:
    """Every refusal of include/grf_svgp.h, with made-up pointers: only where no device is visible."""
    from grf_amd import _lib
    lib = _lib.load()
    assert int(lib.grf_device_count()) == 0, "made-up pointers are never handed to an entry point beside a GPU"
    EINVAL, EUNSUP = _lib.GRF_EINVAL, _lib.GRF_EUNSUPPORTED
    mu, var, y, gx, gw, ve, dmu, dvar, ps = (_p(k) for k in range(1, 10))
    err = lib.grf_last_error

    def call_ve(n=10, P=7, mu=mu, ldmu=8, var=var, ldvar=9, y=y, gx=gx, gw=gw, n_gh=20, eps=1e-3, ve=ve, dmu=dmu,
                lddmu=7, dvar=dvar, lddvar=10):
        return lib.grf_robustmax_ve_f64(n, P, mu, ldmu, var, ldvar, y, gx, gw, n_gh, eps, ve, dmu, lddmu, dvar,
                                        lddvar, None)

    def call_predict(n=10, P=7, mu=mu, ldmu=8, var=var, ldvar=9, gx=gx, gw=gw, n_gh=20, eps=1e-3, ps=ps, ldps=7):
        return lib.grf_robustmax_predict_f64(n, P, mu, ldmu, var, ldvar, gx, gw, n_gh, eps, ps, ldps, None)

    for call, who in ((call_ve, b"grf_robustmax_ve_f64"), (call_predict, b"grf_robustmax_predict_f64")):
        assert call(n=0) == 0 and call(n=0, mu=None, var=None, gx=None, gw=None) == 0      # (touches nothing)
        assert call(n=-1) == EINVAL and b"negative" in err() and who in err()
        assert call(n=1 << 31) == EUNSUP
        for P in (1, 0, -3, 65):
            assert call(P=P, ldmu=80, ldvar=80) == EINVAL and b"outside [2, 64]" in err(), P
        for n_gh in (0, -1, 65):
            assert call(n_gh=n_gh) == EINVAL and b"outside [1, 64]" in err(), n_gh
        for eps in (0.0, 1.0, -0.5, float("nan")):
            assert call(eps=eps) == EINVAL and b"epsilon" in err(), eps
        for missing in ("mu", "var", "gx", "gw"):
            assert call(**{missing: None}) == EINVAL and b"missing" in err(), missing
        assert call(ldmu=6) == EINVAL and call(ldvar=6) == EINVAL and b"below P" in err()
        for huge in ((1 << 63) - 1, 1 << 62, (1 << 61) // 9 + 7):
            assert call(ldmu=huge) == EINVAL and call(ldvar=huge) == EINVAL, huge
        assert b"address space" in err()
    # the fused entry's own arguments
    assert call_ve(y=None) == EINVAL and call_ve(ve=None) == EINVAL and b"missing" in err()
    assert call_ve(dmu=None) == EINVAL and call_ve(dvar=None) == EINVAL and b"go together" in err()
    assert call_ve(lddmu=6) == EINVAL and call_ve(lddvar=6) == EINVAL and b"below P" in err()
    for huge in ((1 << 63) - 1, 1 << 62):
        assert call_ve(lddmu=huge) == EINVAL and call_ve(lddvar=huge) == EINVAL and b"address space" in err()
    span_mu = (9 * 8 + 7) * 8
    assert call_ve(ve=mu) == EINVAL and call_ve(dmu=mu + span_mu - 8) == EINVAL and call_ve(dvar=var) == EINVAL
    assert call_ve(ve=y + 36) == EINVAL and call_ve(dmu=gx + 8) == EINVAL and call_ve(dvar=gw + 152) == EINVAL
    assert b"overlap the inputs" in err()
    assert call_ve(dmu=ve + 72) == EINVAL and call_ve(dvar=dmu) == EINVAL and b"one another" in err()
    # the predictive entry's
    assert call_predict(ps=None) == EINVAL and b"missing" in err()
    assert call_predict(ldps=6) == EINVAL and b"below P" in err()
    assert call_predict(ldps=1 << 62) == EINVAL and b"address space" in err()
    assert call_predict(ps=mu + 16) == EINVAL and call_predict(ps=var) == EINVAL and call_predict(ps=gw) == EINVAL
    assert b"overlap" in err()

    T, base, out = _p(11), _p(12), _p(13)

    def sqsum(n=10, groups=3, length=17, T=T, ldt=52, base=base, out=out, ldout=4):
        return lib.grf_rows_sqsum_f64(n, groups, length, T, ldt, base, out, ldout, None)

    assert sqsum(n=0) == 0 and sqsum(groups=0) == 0 and sqsum(n=0, T=None, out=None) == 0  # (touches nothing)
    assert sqsum(n=-1) == EINVAL and sqsum(groups=-1) == EINVAL and sqsum(length=-1) == EINVAL
    assert b"negative" in err()
    assert sqsum(n=1 << 31) == EUNSUP and sqsum(groups=1 << 20, length=1 << 20) == EUNSUP
    assert sqsum(T=None) == EINVAL and sqsum(out=None) == EINVAL and b"missing" in err()
    assert sqsum(ldt=50) == EINVAL and sqsum(ldout=2) == EINVAL and b"below" in err()
    for huge in ((1 << 63) - 1, 1 << 62):
        assert sqsum(ldt=huge) == EINVAL and sqsum(ldout=huge) == EINVAL and b"address space" in err()
    assert sqsum(out=T + 8) == EINVAL and sqsum(out=base + 72) == EINVAL and b"overlap" in err()
    assert sqsum(n=1 << 27, groups=1, length=1, T=_p(100), ldt=1, base=None, out=_p(300), ldout=1) == EUNSUP and b"work-items" in err()


def test_argument_checks_need_no_device():
    from grf_amd import _lib
    if int(_lib.load().grf_device_count()) == 0:
        _refusals()
        return
    env = dict(os.environ, ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--refusals"], env=env, capture_output=True,
                          text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr


if __name__ == "__main__":
    if sys.argv[1:] == ["--refusals"]:
        _refusals()
        sys.exit(0)
    sys.exit(2)
