"""GPU: the diagonally preconditioned solves -- grf_gram_jacobi_f64, grf_pcg_gram_solve(_lanczos)_f64 and
grf_pcg_poly_solve(_lanczos)_f64 through GRFEngine.gram_jacobi / cg_solve / cg_solve_poly, then
marginal_log_likelihood, posterior_moments, pathwise_predict and SparseGraphGP with preconditioner="jacobi" --
against the numpy restatement (tests/pcg_reference.py), the unpreconditioned solves and the dense truth.

Tolerances
  * Jacobi kernel: exact against the same entry-order sum (the squares of fp32 values are exact in fp64, so every
    addition rounds once either way); two calls give the same bits.
  * precond = ones: every output bit-identical to the plain solve (every product with 1 is exact).
  * iterates: fp64 against the restatement for max_iter in {1, 2, 3, 5} to 1e-10 relative, coefficients to 1e-10,
    equal counts -- the bound tests/test_gpu_cg.py holds the plain solve to while the trajectory is still
    determined by its inputs.
  * marginal likelihood (identity probes, tolerance 1e-12, max_iter 48): GPU error against the dense truth <= 10 x
    the restatement's own error on that case (the rule of tests/test_gpu_mll.py).
  * predict_f at tolerance 1e-10: GPU error against the dense truth <= 10 x the error of the restatement of the same
    preconditioned solves (pcg_reference.moments: linear_cg's stall floor differs under a preconditioner), never below
    1e-12 of the largest prior (the rule of tests/test_gpu_posterior.py); at the default tolerance
    truth - 1e-12 prior <= var <= prior (1 + 1e-12).

Measured on an MI355X (this file's own printed figures, `pytest -m gpu -s tests/test_gpu_pcg.py`): iterates against the
restatement 1.2e-16 .. 1.1e-15 on Phi and 1.6e-16 .. 6.5e-16 on the operator; Cora 56 plain / 21 Jacobi / 21 restatement;
the marginal likelihood's and predict_f's errors against the dense truth equal the restatement's own to three digits
(e.g. steps n = 200, s2 = 0.05: value 3.6e-11, d/df 8.3e-6, d/ds2 5.6e-11; predict_f on Phi: mean 1.1e-6, var 5.4e-9,
cov 8.7e-7); at the default tolerance (var - truth) / prior lies in [1.0e-7, 7.7e-5] on Phi (12 iterations, plain 35)
and [7.3e-15, 5.7e-11] on the operator (11, plain 11).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import mll_reference as R
import pcg_reference as P
import poly_reference as PR
import posterior_reference as PO

pytestmark = pytest.mark.gpu

N, F = 300, [1.0, -0.5, 0.25, -0.125]


def _graph(n, deg, seed):
    r = np.random.default_rng(seed)
    m = int(n * deg / 2)
    u, v = r.integers(0, n, m), r.integers(0, n, m)
    keep = u != v
    A = sp.coo_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(n, n)).tocsr()
    A = (A + A.T).tocsr()
    A.data[:] = 1.0
    return A


def _phi_scipy(phi):
    M = phi.to_scipy().astype(np.float64)
    M.data = phi.val32[:phi.nnz].cpu().numpy().astype(np.float64)
    return M


def _upload(M, eng):
    """DeviceCSR.from_scipy plus the fp32 values the solvers read (M's values are fp32-representable)."""
    import torch
    from grf_amd.engine import DeviceCSR
    dev = DeviceCSR.from_scipy(M, eng.device)
    dev.val32 = dev.val.to(torch.float32)
    return dev


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(b)))


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


@pytest.fixture(scope="module")
def big(eng):
    """The walk's Phi on 1000 nodes (16 walks, p_halt 0.2, L = 4) on the device and as scipy (fp32 values widened)."""
    G = eng.laplacian(_graph(1000, 8, 5))
    phi = eng.compact(eng.walk_phi(G, 16, 0.2, 4, F, seed=3))
    return phi, _phi_scipy(phi)


@pytest.fixture(scope="module")
def world(eng):
    """N = 300: the walk's step matrices and Phi(F) (as tests/test_gpu_mll.py), the walk operator and its dense
    p(G)."""
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.engine import WalkPolynomial
    from grf_amd.features import StepMatrices
    A = _graph(N, 6, 11)
    pre = GraphPreprocessor(A, walks_per_node=8, p_halt=0.2, max_walk_length=4, random_walk_seed=3, use_tqdm=False)
    ops = pre.preprocess_graph()
    mats = [sp.csr_matrix(M.astype(np.float32).astype(np.float64)) for M in pre.step_matrices_scipy]
    steps = StepMatrices(ops, eng)
    f = torch.tensor(F, dtype=torch.float32)
    phi = steps.phi(f)
    G = eng.laplacian(A)
    Gs = G.to_scipy()
    op = WalkPolynomial(G, 4, engine=eng)
    Gd = Gs.toarray()
    return dict(eng=eng, ops=ops, mats=mats, steps=steps, f=f, phi=phi, P=_phi_scipy(phi), op=op, G=Gs,
                Pop=PR.dense_poly(Gs, F, 4), Gpow=[np.linalg.matrix_power(Gd, l) for l in range(4)])


# ------------------------------------------------------------------------------------ 1. the Jacobi kernel
def _rows_matrix():
    """A 40 x 260 Phi with rows of 0, 1, 63, 64, 65 and 200 entries among ordinary ones (fp32 values)."""
    r = np.random.default_rng(8)
    n_rows, n_cols = 40, 260
    lens = list(r.integers(2, 30, n_rows))
    lens[:6] = [0, 1, 63, 64, 65, 200]
    rows = []
    for ln in lens:
        row = np.zeros(n_cols)
        row[np.sort(r.permutation(n_cols)[:ln])] = (r.standard_normal(ln) * 10.0 ** r.integers(-3, 4, ln)).astype(np.float32)
        rows.append(row)
    M = sp.csr_matrix(np.array(rows))
    assert list(np.diff(M.indptr)) == lens
    return M


def test_jacobi_kernel_is_the_entry_order_sum(eng):
    import torch
    from grf_amd.engine import _p
    M = _rows_matrix()
    dev = _upload(M, eng)
    r = np.random.default_rng(1)
    maps = [None, np.array([0]), np.array([5]), np.array([3, 0, 3, 5, 5, 1, 0, 39, 2, 4]), r.integers(0, 40, 131)]
    for rows in maps:
        for noise in (0.0, 0.3, 1e-2):
            want = P.jacobi_dinv(M, noise, rows)
            n_sel = len(want)
            rt = None if rows is None else torch.from_numpy(rows)
            got = eng.gram_jacobi(dev, rt, noise)
            assert got.dtype == torch.float64 and got.shape == (n_sel,)
            assert np.array_equal(got.cpu().numpy(), want), (rows, noise)
            assert torch.equal(got, eng.gram_jacobi(dev, rt, noise))
    assert eng.gram_jacobi(dev, torch.tensor([0]), 0.0).item() == 1.0        # an empty row, no noise: 1
    assert eng.gram_jacobi(dev, torch.tensor([0]), 0.25).item() == 4.0
    # the entry point itself: nothing past the n_sel results is written
    rows = torch.tensor([5, 0, 5], dtype=torch.int32, device="cuda")
    out = torch.full((3 + 8,), float("nan"), dtype=torch.float64, device="cuda")
    rc = eng.lib.grf_gram_jacobi_f64(3, _p(dev.ptr), _p(dev.idx), _p(dev.val32), _p(rows), 0.5, _p(out), eng.stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isnan(out[3:]).all()
    assert np.array_equal(out[:3].cpu().numpy(), P.jacobi_dinv(M, 0.5, [5, 0, 5]))


def test_jacobi_kernel_on_the_walks_phi(eng, big):
    import torch
    phi, Ps = big
    rows = np.sort(np.random.default_rng(0).permutation(1000)[:601])
    got = eng.gram_jacobi(phi, torch.from_numpy(rows), 0.01).cpu().numpy()
    assert np.array_equal(got, P.jacobi_dinv(Ps, 0.01, rows))


# ------------------------------------------------------------------------------------ 2. precond = ones
def _system(Ps, n_sys, S, seed, noise):
    r = np.random.default_rng(seed)
    tr = np.sort(r.permutation(Ps.shape[0])[:n_sys])
    B = r.standard_normal((n_sys, S))
    Pt = Ps[tr]
    return tr, B, (lambda v: Pt @ (Pt.T @ v) + noise * v)


@pytest.mark.parametrize("n_sys,S", [(1, 1), (5, 65), (600, 64), (257, 256)])
def test_unit_diagonal_is_the_plain_solve(eng, big, n_sys, S):
    import torch
    phi, Ps = big
    noise = 0.1
    tr, B, _ = _system(Ps, n_sys, S, 7 * n_sys + S, noise)
    Bd, rows = torch.from_numpy(B).cuda(), torch.from_numpy(tr)
    one = torch.ones(n_sys, dtype=torch.float64, device="cuda")
    for kw in (dict(max_iter=3), dict(tolerance=1e-2, max_iter=400)):
        X0, it0, res0, c0 = eng.cg_solve(phi, Bd, noise, rows, return_residuals=True, return_lanczos=True, **kw)
        X1, it1, res1, c1 = eng.cg_solve(phi, Bd, noise, rows, return_residuals=True, return_lanczos=True,
                                         precond=one, **kw)
        assert it0 == it1 and torch.equal(X0, X1) and np.array_equal(res0, res1) and torch.equal(c0, c1)
        X2, it2, res2 = eng.cg_solve(phi, Bd, noise, rows, return_residuals=True, precond=one, **kw)
        assert it2 == it0 and torch.equal(X2, X0) and np.array_equal(res2, res0)
        if "tolerance" in kw and n_sys > 5:
            assert 11 <= it0 < 400 and res0.mean() < 1e-2
    with pytest.raises(ValueError):
        eng.cg_solve(phi, Bd.float(), noise, rows, max_iter=3, precond=one)
    with pytest.raises(ValueError):
        eng.cg_solve(phi, Bd, noise, rows, max_iter=3, precond=one[:-1] if n_sys > 1 else torch.ones(2).double().cuda())
    with pytest.raises(ValueError):
        eng.cg_solve(phi, Bd, noise, rows, max_iter=3, precond=one.float())


# ------------------------------------------------------------------------------------ 3. iterates
@pytest.mark.parametrize("S", [1, 64, 65, 256])
def test_iterates_vs_restatement(eng, big, S):
    import torch
    phi, Ps = big
    n_sys = 601                                                       # a row subset, not a multiple of 4
    for noise in (1e-2, 1.0):
        tr, B, mm = _system(Ps, n_sys, S, S, noise)
        Bd, rows = torch.from_numpy(B).cuda(), torch.from_numpy(tr)
        dinv = eng.gram_jacobi(phi, rows, noise)
        dn = P.jacobi_dinv(Ps, noise, tr)
        assert np.array_equal(dinv.cpu().numpy(), dn)
        for mi in (1, 2, 3, 5):
            X, it, res, coef = eng.cg_solve(phi, Bd, noise, rows, max_iter=mi, return_residuals=True,
                                            return_lanczos=True, precond=dinv)
            Xo, ito, al, be, reso = P.pcg_lanczos(mm, B, dn, max_iter=mi)
            assert it == ito == mi
            rel = np.linalg.norm(X.cpu().numpy() - Xo) / np.linalg.norm(Xo)
            print(f"S={S} noise={noise} max_iter={mi}: rel {rel:.2e}")
            assert rel <= 1e-10, (noise, mi, rel)
            c = coef.cpu().numpy()
            assert c.shape == (2 * mi, S)
            for i in range(mi):
                assert np.abs(c[i] - al[i]).max() <= 1e-10 * np.abs(al[i]).max(), (mi, i)
                assert np.abs(c[mi + i] - be[i]).max() <= 1e-10 * np.abs(be[i]).max(), (mi, i)
            assert np.abs(res - reso).max() <= 1e-10 * np.abs(reso).max()
        X2, it2, res2, coef2 = eng.cg_solve(phi, Bd, noise, rows, max_iter=5, return_residuals=True,
                                            return_lanczos=True, precond=dinv)
        assert torch.equal(X, X2) and np.array_equal(res, res2) and torch.equal(coef, coef2)   # deterministic
        X3, it3 = eng.cg_solve(phi, Bd, noise, rows, max_iter=5, precond=dinv)
        assert it3 == 5 and torch.equal(X3, X)                        # the entry point without coefficients


def test_zero_columns_and_limits(eng, big):
    import torch
    phi, Ps = big
    noise = 0.1
    tr, B, mm = _system(Ps, 601, 9, 3, noise)
    B[:, 4] = 0.0
    rows = torch.from_numpy(tr)
    dinv = eng.gram_jacobi(phi, rows, noise)
    Bd = torch.from_numpy(B).cuda()
    X, it, res, coef = eng.cg_solve(phi, Bd, noise, rows, tolerance=1e-2, return_residuals=True, return_lanczos=True,
                                    precond=dinv)
    assert it >= 11 and not X[:, 4].cpu().numpy().any() and res[4] == 0.0
    assert not coef[:, 4].cpu().numpy().any()                         # the zero column never moves
    X, it = eng.cg_solve(phi, Bd, noise, rows, max_iter=0, precond=dinv)
    assert it == 0 and not X.cpu().numpy().any()
    X, it, res = eng.cg_solve(phi, torch.zeros_like(Bd), noise, rows, return_residuals=True, precond=dinv)
    assert it == 0 and not X.cpu().numpy().any() and not res.any()


# ------------------------------------------------------------------------------------ 4. the golden Cora Phi
def test_full_run_on_cora(eng, golden):
    """All 2708 rows, noise 0.01, tolerance 1e-2, 8 Gaussian columns from default_rng(0) (the columns of
    tests/test_pcg_reference.py: restatement 60 plain, 21 Jacobi)."""
    import torch
    Ps = P.cora_phi(golden)
    n = Ps.shape[0]
    phi = _upload(Ps, eng)
    noise, tol = 0.01, 1e-2
    B = np.random.default_rng(0).standard_normal((n, 8))
    Bd = torch.from_numpy(B).cuda()
    mm = R._khat_matmul(Ps, noise)
    dinv = eng.gram_jacobi(phi, None, noise)
    dn = P.jacobi_dinv(Ps, noise)
    assert np.array_equal(dinv.cpu().numpy(), dn)
    Xj, itj, resj = eng.cg_solve(phi, Bd, noise, tolerance=tol, return_residuals=True, precond=dinv)
    Xp, itp, resp = eng.cg_solve(phi, Bd, noise, tolerance=tol, return_residuals=True)
    _, ito, _, _, _ = P.pcg_lanczos(mm, B, dn, tolerance=tol)
    print(f"cora: gpu plain {itp}, gpu jacobi {itj}, restatement jacobi {ito}")
    assert resj.mean() < tol and resp.mean() < tol
    assert abs(itj - ito) <= 1                                        # rounding-sensitive at the threshold
    assert 2 * itj <= itp
    # both stopped with ||K^ x - b|| ~ tol ||b|| per column: they agree within the stopping tolerance, measured
    # where the rule measures it (the residual of one solution under the operator, against the other's)
    Xj, Xp = Xj.cpu().numpy(), Xp.cpu().numpy()
    nb = np.linalg.norm(B, axis=0)
    rj, rp = np.linalg.norm(mm(Xj) - B, axis=0) / nb, np.linalg.norm(mm(Xp) - B, axis=0) / nb
    assert rj.mean() < 2 * tol and rp.mean() < 2 * tol
    assert (np.linalg.norm(mm(Xj - Xp), axis=0) / nb).mean() <= 2 * tol


# ------------------------------------------------------------------------------------ 5. the operator
def _ring(n):
    i = np.arange(n)
    A = sp.coo_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n)).tocsr()
    return A


@pytest.mark.parametrize("graph", ["ring", "er"])
def test_poly_variant(eng, graph):
    import torch
    from grf_amd.engine import WalkPolynomial
    n = 64 if graph == "ring" else 300
    A = _ring(n) if graph == "ring" else _graph(n, 6, 21)
    G = eng.laplacian(A)
    op = WalkPolynomial(G, 4, engine=eng)
    Pd = PR.dense_poly(G.to_scipy(), F, 4)
    f = torch.tensor(F, dtype=torch.float64)
    r = np.random.default_rng(n)
    n_sys = 41 if graph == "ring" else 201
    tr = np.sort(r.permutation(n)[:n_sys])
    Pt = Pd[tr]
    rows = torch.from_numpy(tr)
    for noise, S in ((1e-2, 65), (1.0, 7)):
        mm = lambda v: Pt @ (Pt.T @ v) + noise * v
        B = r.standard_normal((n_sys, S))
        Bd = torch.from_numpy(B).cuda()
        dn = 1.0 / (np.sum(Pt * Pt, axis=1) + noise) * r.uniform(0.5, 2.0, n_sys)   # an explicit diagonal
        dinv = torch.from_numpy(dn).cuda()
        for mi in (1, 2, 3, 5):
            X, it, res, coef = eng.cg_solve_poly(op, f, Bd, noise, rows, max_iter=mi, return_residuals=True,
                                                 return_lanczos=True, precond=dinv)
            Xo, ito, al, be, reso = P.pcg_lanczos(mm, B, dn, max_iter=mi)
            assert it == ito == mi
            rel = np.linalg.norm(X.cpu().numpy() - Xo) / np.linalg.norm(Xo)
            print(f"{graph} noise={noise} max_iter={mi}: rel {rel:.2e}")
            assert rel <= 1e-10
            c = coef.cpu().numpy()
            for i in range(mi):
                assert np.abs(c[i] - al[i]).max() <= 1e-10 * np.abs(al[i]).max()
                assert np.abs(c[mi + i] - be[i]).max() <= 1e-10 * np.abs(be[i]).max()
        X2, _ = eng.cg_solve_poly(op, f, Bd, noise, rows, max_iter=5, precond=dinv)
        assert torch.equal(X2, X)
        # ones: the plain operator solve, bit for bit
        one = torch.ones(n_sys, dtype=torch.float64, device="cuda")
        for kw in (dict(max_iter=3), dict(tolerance=1e-2, max_iter=200)):
            a = eng.cg_solve_poly(op, f, Bd, noise, rows, return_residuals=True, return_lanczos=True, **kw)
            b = eng.cg_solve_poly(op, f, Bd, noise, rows, return_residuals=True, return_lanczos=True, precond=one, **kw)
            assert a[1] == b[1] and torch.equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and torch.equal(a[3], b[3])
        # the Jacobi diagonal of the operator
        dj = eng.poly_jacobi(op, f, rows, noise).cpu().numpy()
        want = 1.0 / (np.sum(Pt * Pt, axis=1) + noise)
        assert np.abs(dj - want).max() <= 1e-12 * want.max()


# ------------------------------------------------------------------------------------ 6. marginal likelihood
def _train(n_train, seed):
    r = np.random.default_rng(seed)
    return np.sort(r.permutation(N)[:n_train]), r.standard_normal(n_train)


_mll_cases = {}


def _mll_case(world, path, n_train, noise):
    """Restatement (Jacobi) and dense truth with identity probes: computed once per case, left unchanged."""
    key = (path, n_train, noise)
    if key not in _mll_cases:
        tr, y = _train(n_train, 7 + n_train)
        if path == "steps":
            Pt, Ms = world["P"][tr], [M[tr] for M in world["mats"]]
        else:
            Pt, Ms = sp.csr_matrix(world["Pop"][tr]), [sp.csr_matrix(M[tr]) for M in world["Gpow"]]
        G = R.identity_probes(n_train)
        est = P.estimate(Pt, Ms, y, noise, G, tolerance=1e-12, max_iter=48)
        tru = R.dense_truth(Pt, Ms, y, noise)
        tol = {q: 10.0 * _rel(est[q], tru[q]) for q in ("value", "grad_f", "grad_noise")}
        _mll_cases[key] = dict(tr=tr, y=y, G=G, est=est, tru=tru, tol=tol)
    return _mll_cases[key]


@pytest.mark.parametrize("noise", [0.05, 1.0])
@pytest.mark.parametrize("n_train", [64, 200])
@pytest.mark.parametrize("path", ["steps", "operator"])
def test_mll_jacobi_exactness(world, path, n_train, noise):
    import torch
    c = _mll_case(world, path, n_train, noise)
    steps, f = (world["steps"], world["f"]) if path == "steps" else (world["op"], torch.tensor(F, dtype=torch.float64))
    value, g_f, g_noise, iters = world["eng"].marginal_log_likelihood(
        steps, f, torch.from_numpy(c["tr"]), torch.from_numpy(c["y"]), noise, torch.from_numpy(c["G"]).cuda(), 1e-12,
        48, preconditioner="jacobi")
    got = dict(value=value, grad_f=g_f.cpu().numpy(), grad_noise=g_noise)
    assert iters == c["est"]["iters"] == 48
    for q in ("value", "grad_f", "grad_noise"):
        print(f"jacobi mll {path} n={n_train} s2={noise} {q}: gpu vs truth {_rel(got[q], c['tru'][q]):.3e}  "
              f"restatement vs truth {_rel(c['est'][q], c['tru'][q]):.3e}  tolerance {c['tol'][q]:.3e}")
    for q in ("value", "grad_f", "grad_noise"):
        assert _rel(got[q], c["tru"][q]) <= c["tol"][q], q


class _NoiseParam:
    def __init__(self, value):
        import torch
        self.noise = torch.tensor([value], dtype=torch.float64, requires_grad=True)


@pytest.mark.parametrize("path", ["steps", "operator"])
def test_model_backward_fills_the_engines_gradients(world, path):
    import torch
    from efficient_graph_gp_sparse.models import SparseGraphGP
    n_train, noise = 64, 0.3
    tr, y = _train(n_train, 21)
    x_train = torch.tensor(tr, dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(y, dtype=torch.float32, device="cuda")
    lik = _NoiseParam(noise)
    gp = SparseGraphGP(x_train, y_train, lik, world["ops"] if path == "steps" else world["op"], 4).cuda()
    with torch.no_grad():
        gp.covar_module.raw_modulator_vector.copy_(torch.tensor(F))
    Z = torch.randn(n_train, 7, generator=torch.Generator().manual_seed(5))
    mll = gp.marginal_log_likelihood(probes=Z, tolerance=1e-8, max_iter=60, per_datum=False, preconditioner="jacobi")
    mll.backward()
    iters = gp.last_cg_iterations
    fvec = gp.covar_module.modulator_vector.detach()
    steps = world["steps"] if path == "steps" else world["op"]
    value, g_f, g_noise, it = world["eng"].marginal_log_likelihood(
        steps, fvec, torch.from_numpy(tr), y_train, noise, Z, 1e-8, 60, preconditioner="jacobi")
    assert it == iters >= 11 and mll.item() == value
    assert lik.noise.grad.item() == g_noise
    gf = gp.covar_module.raw_modulator_vector.grad
    assert gf is not None and gf.abs().max() > 0
    assert torch.equal(gf, g_f.to(gf.device, gf.dtype).reshape(gf.shape))   # (the modulator is the raw parameter)
    with pytest.raises(ValueError):
        gp.marginal_log_likelihood(probes=Z, preconditioner="cholesky")
    with pytest.raises(ValueError):
        world["eng"].marginal_log_likelihood(steps, fvec, torch.from_numpy(tr), y_train, noise, Z,
                                             preconditioner="pivoted")


# ------------------------------------------------------------------------------------ 7. predict_f / predict_y / nlpd
NOISE = 0.1


def _nodes(n_train, n_test, seed):
    r = np.random.default_rng(seed)
    train = np.sort(r.permutation(N)[:n_train])
    test = r.integers(0, N, n_test)
    test[0], test[7], test[-1] = train[0], test[6], test[1]
    return train, test, r.standard_normal(n_train)


class _Lik:
    noise = NOISE


def _model(world, path, n_train, seed):
    import torch
    from efficient_graph_gp_sparse.models import SparseGraphGP
    train, test, y = _nodes(n_train, 65, seed)
    x_train = torch.tensor(train, dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(y, dtype=torch.float32, device="cuda")
    x_test = torch.tensor(test, dtype=torch.float32, device="cuda").unsqueeze(1)
    gp = SparseGraphGP(x_train, y_train, _Lik(), world["ops"] if path == "csr" else world["op"], 4).cuda()
    with torch.no_grad():
        gp.covar_module.raw_modulator_vector.copy_(torch.tensor(F))
    return gp, train, test, y_train.cpu().numpy().astype(np.float64), x_test


@pytest.mark.parametrize("path", ["csr", "operator"])
def test_model_moments_with_jacobi(world, path):
    import torch
    gp, train, test, y, x_test = _model(world, path, 200, 77)
    Pm = world["P"] if path == "csr" else world["Pop"]
    tru = PO.dense_truth(Pm, train, test, y, NOISE)
    est = P.moments(Pm, train, test, y, NOISE, tolerance=1e-10, max_iter=200, full_cov=True)   # (Jacobi, as the GPU)
    err = PO.errors(est, tru, True)
    tol = {q: max(10.0 * e, 1e-12) for q, e in err.items()}
    mean, var = gp.predict_f(x_test, tolerance=1e-10, max_iter=200, preconditioner="jacobi")
    assert gp.last_cg_iterations >= 11
    mean_c, cov = gp.predict_f(x_test, full_cov=True, tolerance=1e-10, max_iter=200, preconditioner="jacobi")
    assert torch.equal(cov, cov.t()) and torch.equal(mean_c, mean)
    got = dict(mean=mean.cpu().numpy(), var=var.cpu().numpy(), cov=cov.cpu().numpy())
    e = PO.errors(got, tru, True)
    for q in e:
        print(f"jacobi predict_f {path} {q}: gpu vs truth {e[q]:.3e}  restatement vs truth {err[q]:.3e}  "
              f"tolerance {tol[q]:.3e}")
    for q in e:
        assert e[q] <= tol[q], q
    assert got["var"][7] == got["var"][6] and got["mean"][7] == got["mean"][6]
    # the default tolerance: between the truth and the prior, up to rounding
    mean_d, var_d = gp.predict_f(x_test, preconditioner="jacobi")
    it_j = gp.last_cg_iterations
    gp.predict_f(x_test)
    it_p = gp.last_cg_iterations
    v = var_d.cpu().numpy()
    slack = (v - tru["var"]) / tru["prior"]
    print(f"{path}: default tolerance, iterations jacobi {it_j} plain {it_p}; (var - truth) / prior in "
          f"[{slack.min():.3e}, {slack.max():.3e}]")
    assert np.all(v >= tru["var"] - 1e-12 * tru["prior"]) and np.all(v <= tru["prior"] * (1.0 + 1e-12))
    mean_y, var_y = gp.predict_y(x_test, preconditioner="jacobi")
    assert torch.equal(mean_y, mean_d) and torch.equal(var_y, var_d + NOISE)
    mean_cy, cov_y = gp.predict_y(x_test, full_cov=True, preconditioner="jacobi")
    assert torch.equal(cov_y, cov_y.t()) and torch.equal(mean_cy, mean_d)
    y_test = torch.from_numpy(np.random.default_rng(4).standard_normal(65)).cuda()
    got_n = gp.nlpd(x_test, y_test, preconditioner="jacobi")
    want = PO.nlpd(y_test.cpu().numpy(), mean_y.cpu().numpy(), np.sqrt(var_y.cpu().numpy()))
    assert abs(got_n.item() - want) <= 1e-13 * abs(want)
    for fn in (gp.predict_f, gp.predict_y):
        with pytest.raises(ValueError):
            fn(x_test, preconditioner="ilu")
    with pytest.raises(ValueError):
        gp.nlpd(x_test, y_test, preconditioner=1)


# ------------------------------------------------------------------------------------ 8. predict
@pytest.mark.parametrize("path", ["csr", "operator"])
def test_pathwise_predict_with_jacobi(world, path):
    import torch
    eng = world["eng"]
    gp, train, test, y, x_test = _model(world, path, 200, 31)
    Pm = world["P"].toarray() if path == "csr" else world["Pop"]
    r = np.random.default_rng(2)
    S = 9
    e1, e2 = r.standard_normal((S, N)), np.sqrt(NOISE) * r.standard_normal((S, 200))
    phi, f = (world["phi"], None) if path == "csr" else (world["op"], torch.tensor(F, dtype=torch.float64))
    out, it = eng.pathwise_predict(phi, torch.from_numpy(train), torch.from_numpy(test), torch.from_numpy(y), NOISE,
                                   torch.from_numpy(e1), torch.from_numpy(e2), max_iter=3, f=f,
                                   preconditioner="jacobi")
    Pt, Pe = Pm[train], Pm[test]
    b = y[None, :] - (e1 @ Pt.T + e2)
    dn = 1.0 / (np.sum(Pt * Pt, axis=1) + NOISE)
    V, ito, _, _, _ = P.pcg_lanczos(lambda v: Pt @ (Pt.T @ v) + NOISE * v, b.T, dn, max_iter=3)
    want = e1 @ Pe.T + (Pe @ (Pt.T @ V)).T
    assert it == ito == 3
    rel = np.linalg.norm(out.cpu().numpy() - want) / np.linalg.norm(want)
    print(f"{path}: pathwise predict, 3 iterations: rel {rel:.2e}")
    assert rel <= 1e-10
    # the model: seeded draws, fewer iterations than the plain solve at one tolerance; fp32 refused
    torch.manual_seed(9)
    a = gp.predict(x_test, n_samples=16, tolerance=1e-2, preconditioner="jacobi")
    it_j = gp.last_cg_iterations
    torch.manual_seed(9)
    b2 = gp.predict(x_test, n_samples=16, tolerance=1e-2, preconditioner="jacobi")
    assert torch.equal(a, b2) and a.dtype == torch.float32 and a.shape == (16, 65)
    torch.manual_seed(9)
    gp.predict(x_test, n_samples=16, tolerance=1e-2)
    print(f"{path}: predict at tolerance 1e-2: jacobi {it_j} iterations, plain {gp.last_cg_iterations}")
    with pytest.raises(ValueError):
        gp.predict(x_test, cg_dtype=torch.float32, preconditioner="jacobi")
    with pytest.raises(ValueError):
        gp.predict(x_test, preconditioner="none")
    with pytest.raises(ValueError):
        eng.pathwise_predict(phi, torch.from_numpy(train), torch.from_numpy(test), torch.from_numpy(y), NOISE,
                             torch.from_numpy(e1), torch.from_numpy(e2), dtype=torch.float32, f=f,
                             preconditioner="jacobi")
