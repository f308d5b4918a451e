"""GPU: the dense fp64 NT product on the matrix cores (grf_gemm_nt_f64 of csrc/grf_expm.hip), the exact diffusion
kernel built on it (grf_expm_sym_f64) and their surfaces (GRFEngine.gemm_nt_f64 / diffusion_expm,
api.diffusion_kernel_exact, gpflow_kernels.diffusion_kernel_exact.GraphDiffusionKernel, tools/grf_error.py
--truth expm) against tests/expm_reference.py.

Entry 1, called directly into NaN-filled buffers with padded pitches:
* bitwise on integer-valued inputs (every sum below 2^53) in the general, symmetric and contraction modes, with
  alpha, gamma Z, delta, Z aliasing C, and row maps that repeat, are unsorted, or name a single row; sizes 1, 3,
  15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257 (the tile is 128 x 128) in n1 != n2 pairs, nk in 0, 1, 3, 4, 5,
  15, 16, 17, 31, 32, 33, 300 (the k-tile is 16 deep, the ring two k-tiles);
* on real inputs within (nk + 4) 2^-53 sum_k |a||b| of float64 numpy plus one rounding per addend operation (the
  bound of nk fused multiply-adds in any order); the contraction within (D + 4) 2^-53 sum |w||a||b| with the
  kernel's own depth D = nk + 64 + 6 + 3 + tiles;
* the symmetric mode with A != B (two commuting polynomials of one symmetric integer matrix): C bitwise symmetric
  and bitwise the general mode's upper triangle; run-to-run bits; the ticket zero after every call; the
  GRF_EINVAL cases write nothing.

Entry 2 and the surfaces: every case of expm_reference against the eigendecomposition truth within the 10x bound
the CPU test asserts for the restatement, E bitwise symmetric, run-to-run bits, n in 1, 2, 129 and 1100, s = 0 and
s >= 10; the kernel class against the reference's fixture, its gradients, its cache; the error tool.
"""
import json
import math
import os
import sys

import numpy as np
import pytest

import expm_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TILE, KT = 128, 16
SIZES = [1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257]
NKS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 300]
PAIRS = list(zip(SIZES, SIZES[5:] + SIZES[:5]))  # every size as n1 and as n2, n1 != n2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _tiles(n1, n2):
    return -(-n1 // TILE) * -(-n2 // TILE)


def _padded(a, pad, tail=64):
    """A NaN-filled device buffer holding `a` at pitch cols + pad; (buffer, pitch)."""
    import torch
    rows, cols = a.shape
    ld = cols + pad
    host = np.full(rows * ld + tail, np.nan)
    host[:rows * ld].reshape(rows, ld)[:, :cols] = a
    return torch.from_numpy(host).cuda(), ld


def _view(buf, rows, cols, ld):
    return buf.cpu().numpy()[:rows * ld].reshape(rows, ld)[:, :cols].copy()


def _untouched(buf, rows, cols, ld):
    out = buf.cpu().numpy()
    body = out[:rows * ld].reshape(rows, ld)
    return bool(np.isnan(body[:, cols:]).all() and np.isnan(out[rows * ld:]).all())


def _dev_i32(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _raw(eng, A, B, *, ra=None, rb=None, alpha=1.0, gamma=1.0, Z=None, alias=False, delta=0.0, symmetric=False,
         W=None, pads=(3, 5, 1), expect=0):
    """grf_gemm_nt_f64 itself.  Returns C (or the contraction's value) after checking that nothing outside
    [n1 x n2] of C, nothing past any buffer and nothing of the inputs' padding was written, and that the ticket
    is zero again."""
    import torch
    from grf_amd.engine import _p
    nk = A.shape[1]
    n1 = A.shape[0] if ra is None else len(ra)
    n2 = B.shape[0] if rb is None else len(rb)
    ab, lda = _padded(A, pads[0])
    bb, ldb = _padded(B, pads[1])
    dra, drb = _dev_i32(ra), _dev_i32(rb)
    ldc = n2 + pads[2]
    cb = torch.full((n1 * ldc + 64,), float("nan"), dtype=torch.float64, device="cuda")
    zb, ldz = None, 0
    if Z is not None and alias:
        cb, ldc = _padded(Z, pads[2])
        zb, ldz = cb, ldc
    elif Z is not None:
        zb, ldz = _padded(Z, 2)
    wb, ldw, ob, ws, need = None, 0, None, None, 0
    if W is not None:
        wb, ldw = _padded(W, 4)
        need = eng.lib.grf_gemm_nt_f64_workspace_bytes(n1, n2)
        ws = torch.full((need // 8 + 64,), float("nan"), dtype=torch.float64, device="cuda")
        ob = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    rc = eng.lib.grf_gemm_nt_f64(n1, n2, nk, alpha, _p(ab), lda, A.shape[0], _p(dra), _p(bb), ldb, B.shape[0], _p(drb),
                                 gamma, _p(zb), ldz, delta, None if W is not None else _p(cb), ldc, int(symmetric),
                                 _p(wb), ldw, _p(ob), _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    assert rc == expect, eng.lib.grf_last_error()
    assert _untouched(ab, A.shape[0], nk, lda) and _untouched(bb, B.shape[0], nk, ldb), "an operand was written"
    if W is not None:
        assert np.isnan(cb.cpu().numpy()).all(), "the contraction wrote C"
        assert np.isnan(ws[need // 8:].cpu().numpy()).all(), "wrote past the workspace"
        assert int(ws[:1].view(torch.int32)[0].item()) == 0, "the ticket is not zero after the call"
        o = ob.cpu().numpy()
        assert np.isnan(o[1:]).all()
        return o[0]
    if rc != 0:
        return cb.cpu().numpy()
    assert _untouched(cb, n1, n2, ldc), "wrote outside [n1 x n2] of C"
    return _view(cb, n1, n2, ldc)


def _ints(rng, shape, lim=9):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _expected(A, B, ra, rb, alpha, gamma, Z, delta):
    Ar = A if ra is None else A[ra]
    Br = B if rb is None else B[rb]
    C = alpha * (Ar @ Br.T)
    if Z is not None:
        C = C + gamma * Z
    return C + delta * np.eye(*C.shape)


@pytest.mark.parametrize("n1,n2", PAIRS)
def test_general_and_contraction_are_exact_on_integers(eng, n1, n2):
    rng = np.random.default_rng(n1 * 1000 + n2)
    for q, nk in enumerate(NKS):
        A, B = _ints(rng, (n1, nk)), _ints(rng, (n2, nk))
        Z = _ints(rng, (n1, n2)) if q % 2 else None
        alpha, gamma, delta = (1.0, 1.0, 0.0) if q % 3 == 0 else (-3.0, 2.0, 5.0)
        want = _expected(A, B, None, None, alpha, gamma, Z, delta)
        got = _raw(eng, A, B, alpha=alpha, gamma=gamma, Z=Z, alias=(q % 4 == 1), delta=delta, pads=(q % 3, 5 - q % 4, 1))
        assert _same_bits(got + 0.0, want + 0.0), (n1, n2, nk)
        Wt = _ints(rng, (n1, n2), 3)
        out = _raw(eng, A, B, alpha=alpha, gamma=gamma, Z=Z, delta=delta, W=Wt)
        assert out == float((Wt * want).sum()), (n1, n2, nk)


def _commuting(n, rng):
    """Two different commuting polynomials of one symmetric integer matrix: A = S + 2 I, B = S^2 - 3 S + I."""
    S = np.triu(rng.integers(-1, 2, (n, n)), 0).astype(np.float64)
    S = S + np.triu(S, 1).T
    return S + 2 * np.eye(n), S @ S - 3 * S + np.eye(n)


@pytest.mark.parametrize("n", SIZES + [130, 300])
def test_symmetric_mode_is_bitwise_symmetric_and_equals_the_general_upper_triangle(eng, n):
    rng = np.random.default_rng(n)
    A, B = _commuting(n, rng)
    assert n == 1 or not np.array_equal(A, B)
    Z = _ints(rng, (n, n))
    Z = np.triu(Z) + np.triu(Z, 1).T
    for use_z in (False, True):
        kw = dict(alpha=2.0, gamma=-1.0, Z=Z if use_z else None, delta=7.0)
        want = _expected(A, B, None, None, 2.0, -1.0, Z if use_z else None, 7.0)
        assert np.array_equal(want, want.T)
        sym = _raw(eng, A, B, symmetric=True, alias=use_z, **kw)
        gen = _raw(eng, A, B, **kw)
        assert _same_bits(sym, sym.T)
        assert _same_bits(np.triu(sym), np.triu(gen)) and _same_bits(sym + 0.0, want + 0.0)
        assert _same_bits(sym, _raw(eng, A, B, symmetric=True, alias=use_z, **kw))  # run to run


def test_symmetric_mode_on_real_commuting_inputs_is_bitwise_symmetric(eng):
    rng = np.random.default_rng(5)
    n = 257
    S = rng.standard_normal((n, n))
    S = S + S.T
    A, B = S + 0.3 * np.eye(n), S @ S - 0.5 * S  # (B symmetric in exact arithmetic; rounded, nearly so)
    B = np.triu(B) + np.triu(B, 1).T
    sym, gen = _raw(eng, A, B, symmetric=True), _raw(eng, A, B)
    assert _same_bits(sym, sym.T) and _same_bits(np.triu(sym), np.triu(gen))
    assert not _same_bits(gen, gen.T)  # (the general mode's two triangles are different sums)


@pytest.mark.parametrize("name", ["repeated", "unsorted", "single"])
def test_row_maps_are_just_rows(eng, name):
    rng = np.random.default_rng(17)
    na, nb, nk = 140, 70, 37
    A, B = _ints(rng, (na, nk)), _ints(rng, (nb, nk))
    if name == "repeated":
        ra, rb = np.array([5, 5, 5, 139, 0, 5, 139] * 21), np.array([3, 3, 69, 3] * 40)
    elif name == "unsorted":
        ra, rb = rng.permutation(na)[:131], rng.permutation(nb)
    else:
        ra, rb = np.array([77]), np.array([12])
    for maps in ((ra, rb), (ra, None), (None, rb)):
        want = _expected(A, B, maps[0], maps[1], 1.0, 1.0, None, 0.0)
        got = _raw(eng, A, B, ra=maps[0], rb=maps[1])
        assert _same_bits(got + 0.0, want + 0.0)
        Wt = _ints(rng, want.shape, 3)
        assert _raw(eng, A, B, ra=maps[0], rb=maps[1], W=Wt) == float((Wt * want).sum())
        assert _same_bits(got, _raw(eng, A, B, ra=maps[0], rb=maps[1]))  # run to run


@pytest.mark.parametrize("n1,n2,nk", [(257, 129, 300), (129, 257, 17), (65, 300, 33), (128, 128, 1), (17, 3, 5)])
def test_real_inputs_within_the_derived_bounds(eng, n1, n2, nk):
    """nk fused multiply-adds in any order are within nk 2^-53 sum |a||b| of the exact sum (4 more for the
    epilogue's scale and numpy's own roundings); each addend operation (gamma Z: a product and a sum; delta: a
    sum) rounds a value no larger than the sum of the absolute values of all terms once.  Largest error / bound
    ratios observed are printed."""
    rng = np.random.default_rng(n1 + n2 + nk)
    A, B = rng.standard_normal((n1, nk)), rng.standard_normal((n2, nk))
    Z, Wt = rng.standard_normal((n1, n2)), rng.standard_normal((n1, n2))
    alpha, gamma, delta = 0.7, -1.3, 0.9
    P = abs(alpha) * (np.abs(A) @ np.abs(B).T)
    eye = np.eye(n1, n2)
    for use_z in (False, True):
        Zq = Z if use_z else None
        want = _expected(A, B, None, None, alpha, gamma, Zq, delta)
        total = P + (abs(gamma) * np.abs(Z) if use_z else 0.0) + abs(delta) * eye
        bound = (nk + 4) * U * P + ((2 if use_z else 0) + eye) * U * total
        got = _raw(eng, A, B, alpha=alpha, gamma=gamma, Z=Zq, delta=delta)
        ratio = float((np.abs(got - want) / bound).max())
        print(f"gemm {n1}x{n2}x{nk} z={use_z}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0
        D = nk + 64 + 6 + 3 + _tiles(n1, n2)
        cbound = (D + 4) * U * float((np.abs(Wt) * total).sum())
        out = _raw(eng, A, B, alpha=alpha, gamma=gamma, Z=Zq, delta=delta, W=Wt)
        cratio = abs(out - float((Wt * want).sum())) / cbound
        print(f"contraction {n1}x{n2}x{nk} z={use_z}: error / bound = {cratio:.3f}")
        assert cratio <= 1.0
        assert out == _raw(eng, A, B, alpha=alpha, gamma=gamma, Z=Zq, delta=delta, W=Wt)  # run to run


def test_invalid_calls_write_nothing_and_empty_calls_touch_nothing(eng):
    import torch
    from grf_amd import _lib
    from grf_amd.engine import _p
    rng = np.random.default_rng(3)
    A, B = _ints(rng, (20, 9)), _ints(rng, (20, 9))
    # symmetric mode with a row map; ld below n
    got = _raw(eng, A, B, ra=np.arange(20), symmetric=True, expect=_lib.GRF_EINVAL)
    assert np.isnan(got).all()
    buf = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
    a, b, c = buf[:1024], buf[1024:2048], buf[2048:]

    def call(n1=20, n2=20, nk=9, A=a, lda=9, B=b, ldb=9, C=c, ldc=20, Z=None, ldz=20):
        rc = eng.lib.grf_gemm_nt_f64(n1, n2, nk, 1.0, _p(A), lda, n1, None, _p(B), ldb, n2, None, 1.0, _p(Z), ldz, 0.0,
                                     _p(C), ldc, 0, None, 0, None, None, 0, eng.stream)
        torch.cuda.synchronize()
        return rc

    assert call(ldc=19) == _lib.GRF_EINVAL and call(lda=8) == _lib.GRF_EINVAL and call(Z=b, ldz=19) == _lib.GRF_EINVAL
    assert call(C=buf[100:]) == _lib.GRF_EINVAL        # C inside A
    assert call(C=buf[1024 - 8:]) == _lib.GRF_EINVAL   # C's rows run into B
    assert call(Z=buf[2048 + 1:]) == _lib.GRF_EINVAL   # Z overlaps C without being C
    assert call(n1=0) == 0 and call(n2=0) == 0
    assert np.isnan(buf.cpu().numpy()).all()
    # nk == 0: gamma Z + delta I, A and B unused
    Z = _ints(rng, (20, 13))
    zb, ldz = _padded(Z, 2)
    cb = torch.full((20 * 14 + 8,), float("nan"), dtype=torch.float64, device="cuda")
    rc = eng.lib.grf_gemm_nt_f64(20, 13, 0, 9.0, None, 0, 0, None, None, 0, 0, None, -2.0, _p(zb), ldz, 3.0, _p(cb), 14, 0,
                                 None, 0, None, None, 0, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0 and _untouched(cb, 20, 13, 14)
    assert np.array_equal(_view(cb, 20, 13, 14), -2.0 * Z + 3.0 * np.eye(20, 13))


def test_engine_gemm_on_views_and_the_memory_guard(eng, monkeypatch):
    import torch
    rng = np.random.default_rng(9)
    big = torch.from_numpy(_ints(rng, (150, 90))).cuda()
    A, B = big[:131, 3:70], big[20:150, 10:77]  # (row pitch 90, offsets that are not 16-byte aligned)
    ra = torch.tensor([4, 4, 130, 0], device="cuda")
    want = A.cpu().numpy()[[4, 4, 130, 0]] @ B.cpu().numpy().T
    got = eng.gemm_nt_f64(A, B, ra=ra)
    assert np.array_equal(got.cpu().numpy(), want)
    Wt = torch.from_numpy(_ints(rng, want.shape, 3)).cuda()
    assert float(eng.gemm_nt_f64(A, B, ra=ra, W=Wt)[0]) == float((Wt.cpu().numpy() * want).sum())
    Zt = torch.from_numpy(_ints(rng, want.shape)).cuda()
    z0 = Zt.cpu().numpy().copy()
    out = eng.gemm_nt_f64(A, B, ra=ra, alpha=2.0, gamma=-1.0, Z=Zt, delta=1.0, out=Zt)
    assert out is Zt and np.array_equal(Zt.cpu().numpy(), 2.0 * want - z0 + np.eye(*want.shape))
    with pytest.raises(ValueError, match="row indices"):
        eng.gemm_nt_f64(A, B, ra=torch.tensor([131], device="cuda"))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (12345, 1 << 40))
    with pytest.raises(ValueError, match=r"n = 131 .* 12345 bytes of free device memory"):
        eng.gemm_nt_f64(A, B)
    with pytest.raises(ValueError, match=r"n = 300 .* 12345 bytes of free device memory"):
        eng.diffusion_expm(torch.zeros((300, 300), dtype=torch.float64, device="cuda"), 1.0, 2.0)


# ------------------------------------------------------------------------------------------ entry 2
def _expm(eng, L, beta, rho):
    import torch
    E = eng.diffusion_expm(torch.from_numpy(np.ascontiguousarray(L)).cuda(), beta, rho)
    return E.cpu().numpy()


@pytest.mark.parametrize("key,g,normalize,beta", list(R.cases()))
def test_expm_cases_against_the_truth(eng, key, g, normalize, beta):
    W, L, rho, T = R.case_data(g, normalize, beta)
    E = _expm(eng, L, beta, rho)
    err = float(np.abs(E - T).max())
    print(f"{key}: s = {R.squarings(rho)}, |E - truth| = {err:.2e} (restatement {R.MEASURED[key]:.2e})")
    assert np.array_equal(E, E.T), "E is not bitwise symmetric"
    assert _same_bits(E, _expm(eng, L, beta, rho)), "two calls differ"
    assert err <= 10 * R.MEASURED[key]


def test_expm_case_list_reaches_s_zero_and_s_ten(eng):
    s = [eng.expm_squarings(R.case_data(g, nz, b)[2]) for _, g, nz, b in R.cases()]
    assert s == [R.squarings(R.case_data(g, nz, b)[2]) for _, g, nz, b in R.cases()]
    assert min(s) == 0 and max(s) >= 10


def _path_laplacian(n):
    W = np.zeros((n, n))
    i = np.arange(n - 1)
    W[i, i + 1] = W[i + 1, i] = 1.0
    return W, R.laplacian(W, True)


@pytest.mark.parametrize("n", [1, 2, 129, 1100])
def test_expm_small_sizes_and_many_tiles(eng, n):
    """Normalised path graphs at beta = 2 (s = 2, 19 products).  Every factor is symmetric with spectrum in
    [-1, e], so a row's 2-norm is at most 3 and, by Cauchy-Schwarz, sum_k |a_ik||b_jk| <= 9: a product's entry is
    within 9 (n + 4) 2^-53 of exact; an error matrix with such entries has 2-norm at most n times that, and the
    Horner steps (||X|| / k <= 1) and squarings (each at most doubles an error) carry it on: at most
    2^s (17 + s) 9 n (n + 4) 2^-53 in any entry.  The eigendecomposition truth is good to ~n 2^-53 ||beta L||."""
    W, L = (np.zeros((1, 1)), np.array([[0.7]])) if n == 1 else _path_laplacian(n)
    beta, rho = 2.0, 4.0
    E = _expm(eng, L, beta, rho)
    err = float(np.abs(E - R.expm_truth(L, beta)).max())
    bound = 2 ** 2 * 19 * 9 * n * (n + 4) * U
    print(f"n = {n}: |E - truth| = {err:.2e}, bound {bound:.2e}")
    assert np.array_equal(E, E.T) and err <= bound
    assert _same_bits(E, _expm(eng, L, beta, rho))
    if n == 1:
        # 19 products on a scalar: each one rounding, the two squarings doubling the relative error twice
        assert abs(E[0, 0] - math.exp(-1.4)) <= 2 ** 2 * 19 * U * math.exp(-1.4)


def test_expm_refuses_bad_scalars(eng):
    import torch
    L = torch.eye(4, dtype=torch.float64, device="cuda")
    for beta, rho in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, float("inf")),
                      (1.0, float("nan"))):
        with pytest.raises(ValueError):
            eng.diffusion_expm(L, beta, rho)


# ----------------------------------------------------------------------------------------- surfaces
def test_api_against_the_reference_fixture(golden):
    from grf_amd import api
    d = golden("expm")
    for name in ("toy", "isolated"):
        for beta in d["betas"]:
            K = api.diffusion_kernel_exact(d[name + "_adj"], float(beta))
            # the bound of tests/test_expm_reference.py::test_restatement_against_the_reference_fixture
            assert K.dtype == np.float64 and np.abs(K - d[f"{name}_K_{beta:g}"]).max() <= 1e-13, (name, beta)
            assert np.array_equal(K, K.T)
    W = d["isolated_adj"]
    Kc = api.diffusion_kernel_exact(W, 0.5, normalize_laplacian=False)
    assert np.abs(Kc - R.expm_truth(R.laplacian(W, False), 0.5)).max() <= 1e-13


def test_kernel_class_against_the_fixture_and_its_cache(golden):
    import torch
    from efficient_graph_gp.gpflow_kernels.diffusion_kernel_exact import GraphDiffusionKernel
    d = golden("expm")
    W, sigma = d["isolated_adj"], 1.7
    k = GraphDiffusionKernel(W, beta=0.5, sigma_f=sigma)
    assert isinstance(k, torch.nn.Module) and {n for n, _ in k.named_parameters()} == {"raw_beta", "raw_sigma_f"}
    ref = sigma ** 2 * d["isolated_K_0.5"]
    x1, x2 = np.array([[3], [7], [3], [39]]), np.array([0, 7, 7, 12, 1])
    K = k.K(x1, x2)
    assert isinstance(K, np.ndarray) and K.shape == (4, 5)
    assert np.abs(K - ref[np.ix_(x1.ravel(), x2)]).max() <= sigma ** 2 * 2e-13
    assert np.abs(k.K_diag(x1) - np.diag(ref)[x1.ravel()]).max() <= sigma ** 2 * 2e-13
    assert np.array_equal(k(x1), k.K(x1)) and np.array_equal(k(x1, full_cov=False), k.K_diag(x1))
    assert np.abs(k.diffusion_kernel() - ref).max() <= sigma ** 2 * 2e-13
    assert k.expm_count == 1  # one E for all of the above
    k.K_torch(x1, x2)
    assert k.expm_count == 1
    # a step on beta rebuilds E; invalidate() does too
    opt = torch.optim.SGD(k.parameters(), lr=0.1)
    k.K_torch(x1).sum().backward()
    opt.step()
    k.K(x1)
    assert k.expm_count == 2
    k.K(x1)
    assert k.expm_count == 2
    k.invalidate()
    k.K(x1)
    assert k.expm_count == 3
    with pytest.raises(IndexError):
        k.K(np.array([40]))
    with pytest.raises(ValueError):
        GraphDiffusionKernel(W, beta=-1.0)
    d2 = GraphDiffusionKernel(W)
    assert abs(float(d2.beta) - 2.0) < 1e-12 and abs(float(d2.sigma_f) - 1.0) < 1e-12


@pytest.mark.parametrize("key,g,normalize,beta", [c for c in R.grad_cases() if c[1] in ("er", "star")])
def test_kernel_gradients(key, g, normalize, beta):
    """K_torch(x1, x2).backward() with x1 != x2 and repeated indices.  d/dbeta against the restatement's analytic
    formula on the device's own E within the contraction bound (D + 4) 2^-53 sigma_f^2 sum |G||L||E|,
    D = n + 64 + 6 + 3 + tiles (two more roundings for the sigma_f^2 scale); d/dsigma_f (a torch sum of n1 n2 terms)
    within (n1 n2 + 4) 2^-53 of its scale; both end to end against the restatement within the bound the CPU test
    asserts against central differences."""
    import torch
    from efficient_graph_gp.gpflow_kernels.diffusion_kernel_exact import GraphDiffusionKernel, _ExactKernelFunction
    W, L, rho, _ = R.case_data(g, normalize, beta)
    x1, x2, G = R.grad_inputs()
    k = GraphDiffusionKernel(W, beta=beta, sigma_f=R.GRAD_SIGMA, normalize_laplacian=normalize)
    assert abs(beta * k.radius - rho) <= 1e-12 * rho
    assert np.array_equal(k.laplacian, L) or np.abs(k.laplacian - L).max() <= 4 * U
    bt = torch.tensor(beta, dtype=torch.float64, device="cuda", requires_grad=True)
    sg = torch.tensor(R.GRAD_SIGMA, dtype=torch.float64, device="cuda", requires_grad=True)
    i1, i2 = k._index_pair(x1, x2)
    K = _ExactKernelFunction.apply(bt, sg, k, i1, i2)
    (K * torch.from_numpy(G).cuda()).sum().backward()
    E = k.expm(beta).cpu().numpy()
    Kref = (R.GRAD_SIGMA ** 2 * E)[np.ix_(x1, x2)]
    assert (np.abs(K.detach().cpu().numpy() - Kref) <= 4 * U * np.abs(Kref)).all()
    Ld = k.laplacian
    d_beta, d_sigma, scale_beta, scale_sigma = R.kernel_grads(Ld, E, R.GRAD_SIGMA, x1, x2, G)
    D = L.shape[0] + 64 + 6 + 3 + _tiles(x1.size, x2.size)
    e_beta, e_sigma = abs(float(bt.grad) - d_beta) / scale_beta, abs(float(sg.grad) - d_sigma) / scale_sigma
    print(f"{key}: own-E errors / scale: beta {e_beta:.2e} (bound {(D + 6) * U:.2e}), sigma {e_sigma:.2e}")
    assert e_beta <= (D + 6) * U and e_sigma <= (x1.size * x2.size + 4) * U
    Er = R.expm_restated(L, beta, rho)
    r_beta, r_sigma, rs_beta, rs_sigma = R.kernel_grads(L, Er, R.GRAD_SIGMA, x1, x2, G)
    f_beta, f_sigma = abs(float(bt.grad) - r_beta) / rs_beta, abs(float(sg.grad) - r_sigma) / rs_sigma
    print(f"{key}: end to end against the restatement: beta {f_beta:.2e}, sigma {f_sigma:.2e}; "
          f"bounds {R.MEASURED_GRAD[key]}")
    assert f_beta <= 10 * R.MEASURED_GRAD[key][0] and f_sigma <= 10 * R.MEASURED_GRAD[key][1]
    # through the module's own parameters: the softplus chain rule
    k.zero_grad()
    (k.K_torch(x1, x2) * torch.from_numpy(G).cuda()).sum().backward()
    assert abs(float(k.raw_beta.grad) - float(bt.grad) * float(torch.sigmoid(k.raw_beta))) <= 1e-12 * abs(float(bt.grad))
    assert k.raw_sigma_f.grad is not None


def test_package_level_names_stay_stubs():
    import efficient_graph_gp.gpflow_kernels as GK
    import efficient_graph_gp.gpflow_kernels.diffusion_kernel_exact as mod
    with pytest.raises(NotImplementedError):
        GK.GraphDiffusionKernel(np.zeros((2, 2)))
    assert mod.GraphDiffusionKernel is not GK.GraphDiffusionKernel


def test_error_tool_splits_truncation_and_monte_carlo_error(monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("grf_error_tool", os.path.join(ROOT, "tools", "grf_error.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["grf_error.py", "--graph", "ring:200", "--truth", "expm", "--walks", "16,256",
                                      "--seeds", "2", "--length", "6"])
    tool.main()
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["truth"] == "expm" and res["n"] == 200 and res["expm_products"] == 17 + 1
    rows = res["rows"]
    # the series of exp(-L / 2) cut after L^5 on a spectrum in [0, 2]: a small but visible truncation error
    assert 1e-8 < res["truncation"] < 1e-2
    for r in rows:
        assert abs(r["total"] - r["monte_carlo"]) <= r["truncation"] * 1.0000001  # the triangle inequality
    assert rows[1]["monte_carlo"] < rows[0]["monte_carlo"]
