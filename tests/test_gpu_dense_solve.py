"""GPU: grf_potrf_f64 and grf_trsm_f64 (include/grf_dense_solve.h) called directly at edge shapes.

Matrices A = Phi Phi^T + 0.1 I with Phi a random 5 %-dense n x 3n matrix; n in {1, 2, nb - 1, nb, nb + 1, 2 nb + 1,
300} (nb = 128); lda, ldf, ldb larger than n with the padding and the strict upper triangle of A filled with NaN,
so a read outside the contract shows; nrhs in {1, 3, 64, 65, 130}.

Assertions (u = 2^-53, gamma_k = k u / (1 - k u); evaluated on the host in np.longdouble, as comparisons):
  * |A - L L^T| <= gamma_{n+1} |L| |L^T| on the lower triangle (Higham, Accuracy and Stability, Thm 10.3);
  * |b - T x| <= gamma_n |T| |x| for T = L and T = L^T (Thm 8.5);
  * F's upper triangle is the bitwise mirror of its lower; logdet equals the ascending host sum of 2 log F_ii (the
    header's statement restated in fp64: the terms RN(2 log F_ii) added in ascending i) to n u relative;
  * a second call gives the same bits, and so does a call on a workspace reused after another n;
  * A and the padding of F and B are unchanged;
  * a matrix that is not positive definite gives info = k + 1, a NaN logdet and GRF_OK, and the next call on a good
    matrix with the same workspace is correct.
"""
import ctypes

import numpy as np
import pytest

import gpr_reference as R

pytestmark = pytest.mark.gpu

NB = 128
SIZES = [1, 2, NB - 1, NB, NB + 1, 2 * NB + 1, 300]
NRHS = [1, 3, 64, 65, 130]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def dev():
    import torch
    from grf_amd import _lib
    from grf_amd.engine import GRFEngine
    eng = GRFEngine("cuda:0")
    assert _lib.DENSE_SOLVE_NB == NB
    return eng, eng.lib, torch


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def _padded_a(torch, A, pad=3):
    """A's lower triangle and diagonal inside an n x (n + pad) NaN-filled device buffer."""
    n = A.shape[0]
    host = np.full((n, n + pad), np.nan)
    low = np.tril_indices(n)
    host[low] = A[low]
    return torch.from_numpy(host).cuda()


def _potrf(dev, Ad, n, ws=None, pad=5):
    eng, lib, torch = dev
    Fd = torch.full((n, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    logdet = torch.full((1,), 123.0, dtype=torch.float64, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    if ws is None:
        ws = torch.empty(int(lib.grf_potrf_f64_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    rc = lib.grf_potrf_f64(n, _p(Ad), Ad.stride(0), _p(Fd), Fd.stride(0), _p(logdet), _p(info), _p(ws), ws.numel(),
                           eng.stream)
    torch.cuda.synchronize()
    return rc, Fd, logdet, info


def _trsm(dev, Fd, n, Bd, transposed, ws=None):
    eng, lib, torch = dev
    nrhs = Bd.shape[0]
    if ws is None:
        ws = torch.empty(int(lib.grf_trsm_f64_workspace_bytes(n, nrhs)), dtype=torch.uint8, device="cuda")
    rc = lib.grf_trsm_f64(n, nrhs, _p(Fd), Fd.stride(0), int(transposed), _p(Bd), Bd.stride(0), _p(ws), ws.numel(),
                          eng.stream)
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def factored(dev):
    """n -> (A, device A, F (padded, device), host F[:, :n], logdet, info), computed once per size."""
    torch = dev[2]
    out = {}
    for n in SIZES:
        A = R.spd_matrix(n, seed=1000 + n)
        Ad = _padded_a(torch, A)
        a_bits = _bits(Ad).copy()
        rc, Fd, logdet, info = _potrf(dev, Ad, n)
        assert rc == 0
        assert np.array_equal(_bits(Ad), a_bits), "A was modified"
        out[n] = (A, Ad, Fd, Fd.cpu().numpy()[:, :n].copy(), float(logdet.item()), int(info.item()))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_factorisation(dev, factored, n):
    A, Ad, Fd, F, logdet, info = factored[n]
    assert info == 0
    assert np.all(np.isnan(Fd.cpu().numpy()[:, n:])), "F's padding was written"
    assert np.array_equal(F.view(np.int64), F.T.copy().view(np.int64)), "upper triangle is not the bitwise mirror"
    excess = R.factor_residual_excess(A, F)
    print(f"n={n}: max(|A - LL^T| - gamma_(n+1) |L||L^T|) = {float(excess):.3e}")
    assert excess <= 0
    ref = R.LD(R.logdet_ascending(F))
    print(f"n={n}: logdet {logdet!r}, host {float(ref)!r}, |diff| / (n u |ref|) = "
          f"{float(abs(R.LD(logdet) - ref) / (n * R.U * abs(ref))):.3f}")
    assert abs(R.LD(logdet) - ref) <= n * R.U * abs(ref)
    # a second call returns the same bits
    rc, Fd2, logdet2, info2 = _potrf(dev, Ad, n)
    assert rc == 0 and int(info2.item()) == 0
    assert np.array_equal(_bits(Fd2)[:, :n], F.view(np.int64)) and _bits(logdet2)[0] == np.float64(logdet).view(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_solves(dev, factored, n):
    torch = dev[2]
    A, Ad, Fd, F, _, _ = factored[n]
    L = np.tril(F)
    for nrhs in NRHS:
        B = np.random.default_rng(7 * n + nrhs).standard_normal((nrhs, n))
        host = np.full((nrhs, n + 7), np.nan)
        host[:, :n] = B
        for transposed, T in ((0, L), (1, L.T)):
            Bd = torch.from_numpy(host).cuda()
            assert _trsm(dev, Fd, n, Bd, transposed) == 0
            X = Bd.cpu().numpy()
            assert np.all(np.isnan(X[:, n:])), "B's padding was written"
            excess = R.solve_residual_excess(T, X[:, :n], B)
            print(f"n={n} nrhs={nrhs} transposed={transposed}: max(|b - Tx| - gamma_n |T||x|) = {float(excess):.3e}")
            assert excess <= 0
            Bd2 = torch.from_numpy(host).cuda()
            assert _trsm(dev, Fd, n, Bd2, transposed) == 0
            assert np.array_equal(_bits(Bd2)[:, :n], X[:, :n].view(np.int64)), "second call differs"
    assert np.array_equal(_bits(Fd)[:, :n], F.view(np.int64)), "F was modified"


def test_reused_workspaces_after_another_size(dev, factored):
    eng, lib, torch = dev
    ws = torch.empty(int(lib.grf_potrf_f64_workspace_bytes(300)), dtype=torch.uint8, device="cuda")
    tws = torch.empty(int(lib.grf_trsm_f64_workspace_bytes(300, 130)), dtype=torch.uint8, device="cuda")
    rhs = {}
    for n in (300, 130, 300):
        if n in factored:
            A, Ad, _, F, logdet, _ = factored[n]
        else:
            A = R.spd_matrix(n, seed=1000 + n)
            Ad = _padded_a(torch, A)
            _, Ff, ld, _ = _potrf(dev, Ad, n)
            F, logdet = Ff.cpu().numpy()[:, :n].copy(), float(ld.item())
        rc, Fd, ld, info = _potrf(dev, Ad, n, ws=ws)
        assert rc == 0 and int(info.item()) == 0
        assert np.array_equal(_bits(Fd)[:, :n], F.view(np.int64)), n
        assert _bits(ld)[0] == np.float64(logdet).view(np.int64), n
        B = np.random.default_rng(n).standard_normal((130, n))
        for transposed in (0, 1):
            fresh, reused = torch.from_numpy(B).cuda(), torch.from_numpy(B).cuda()
            assert _trsm(dev, Fd, n, fresh, transposed) == 0 and _trsm(dev, Fd, n, reused, transposed, ws=tws) == 0
            assert np.array_equal(_bits(fresh), _bits(reused)), (n, transposed)
            rhs.setdefault((n, transposed), []).append(_bits(reused))
    for (n, transposed), got in rhs.items():
        assert all(np.array_equal(got[0], g) for g in got), (n, transposed)


@pytest.mark.parametrize("k", [5, NB, 2 * NB])
def test_not_positive_definite(dev, k):
    eng, lib, torch = dev
    n = 2 * NB + 1
    r = np.random.default_rng(k)
    # an exact factor: small integers, so A = L0 L0^T and every step of its factorisation are exact in fp64
    L0 = np.tril(r.integers(-1, 2, (n, n)).astype(np.float64), -1) + np.diag(r.integers(1, 4, n).astype(np.float64))
    A = L0 @ L0.T
    good = _padded_a(torch, A)
    Abad = A.copy()
    Abad[k, k] -= L0[k, k] ** 2 + 1.0
    ws = torch.empty(int(lib.grf_potrf_f64_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    rc, Fd, logdet, info = _potrf(dev, _padded_a(torch, Abad), n, ws=ws)
    assert rc == 0
    assert int(info.item()) == k + 1
    assert np.isnan(float(logdet.item()))
    F = Fd.cpu().numpy()[:, :n]
    assert np.array_equal(np.tril(F)[:k, :k], L0[:k, :k]), "the part before the failing pivot is the exact factor"
    # the next call on a good matrix with the same workspace is correct (here: exact)
    rc, Fd, logdet, info = _potrf(dev, good, n, ws=ws)
    assert rc == 0 and int(info.item()) == 0
    F = Fd.cpu().numpy()[:, :n]
    assert np.array_equal(np.tril(F), L0)
    ref = R.LD(R.logdet_ascending(F))
    assert abs(R.LD(float(logdet.item())) - ref) <= n * R.U * abs(ref)


def test_engine_methods(dev, factored):
    eng, lib, torch = dev
    A, _, _, F, logdet, _ = factored[300]
    Fe, ld, info = eng.cholesky(torch.from_numpy(A).cuda())
    assert int(info.item()) == 0
    assert np.array_equal(_bits(Fe), F.view(np.int64)) and _bits(ld)[0] == np.float64(logdet).view(np.int64)
    B = np.random.default_rng(0).standard_normal((3, 300))
    Bd = torch.from_numpy(B).cuda()
    X = eng.cholesky_solve(Fe, Bd).cpu().numpy()
    assert np.array_equal(Bd.cpu().numpy(), B), "B is not modified unless inplace"
    kappa = np.linalg.cond(A)
    Xt = np.linalg.solve(A, B.T).T
    assert np.abs(X - Xt).max() <= 300 * float(R.U) * kappa * np.abs(Xt).max()
    half = eng.cholesky_solve(Fe, Bd, transposed=False)
    assert R.solve_residual_excess(np.tril(F), half.cpu().numpy(), B) <= 0
    with pytest.raises(ValueError):
        eng.cholesky_solve(Fe, torch.zeros(300, 3, dtype=torch.float64, device="cuda"))
