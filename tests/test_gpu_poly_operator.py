"""GPU: the exact walk-power kernel as a matrix-free operator (csrc/grf_poly.hip, the polynomial matvec of
csrc/grf_cg.hip) against tests/poly_reference.py.

* grf_poly_apply_f64: the restatement's bits on integer-valued inputs (every sum|terms| below 2^53), its bound
  2 D 2^-53 sum|terms| per step on real ones; directed weighted G with rows of 0, 1, 63, 64, 65 and 200 entries,
  row-sparse inputs through an unsorted node selection, row maps of length 1 and N, padded pitches over NaN.
* poly_gram_matvec against the dense K^ and against gram_matvec on exact_steps of a ring.
* the CG entry points against oracle/cg.py's linear_cg on the dense K^ (cond <= 5), 1e-10.
* grf_poly_grad_f64: bits on integers, bound on reals, the ticket zero afterwards.
* the marginal likelihood with identity probes against tests/mll_reference.py's dense truth, held to 10 x the
  restatement's own error, on a graph whose exact step matrices do not fit (exact_steps raises).
* SparseGraphGP on the operator.

Exactness ratios measured on an MI355X (test_mll_exactness's printed figures, relative error of the GPU
against the dense truth over the CPU restatement's): 1.00 in all twelve rows; the figures are in that test's docstring.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import mll_reference as R
import poly_reference as PR
from oracle import cg as OCG

pytestmark = pytest.mark.gpu

S_ALL = [1, 2, 3, 11, 12, 47, 48, 64, 65, 130, 256]


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _csr(eng, G):
    from grf_amd.engine import DeviceCSR
    return DeviceCSR.from_scipy(sp.csr_matrix(G), eng.device)


def _op(eng, G, L):
    from grf_amd.engine import WalkPolynomial
    return WalkPolynomial(_csr(eng, G), L, engine=eng)


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _padded(a, pad, tail=64):
    """(device buffer, pitch): `a` laid out with `pad` extra NaN columns per row and NaN after its end."""
    import torch
    rows, S = a.shape
    ld = S + pad
    buf = torch.full((rows * ld + tail,), float("nan"), dtype=torch.float64, device="cuda")
    buf[:rows * ld].view(rows, ld)[:, :S] = _dev(a)
    return buf, ld


def _apply_raw(eng, A, f, n_f, X, in_idx, out_idx, pad):
    """grf_poly_apply_f64 itself on padded buffers; returns Y (n_out x S) after checking that nothing outside
    it was written."""
    import torch
    from grf_amd.engine import _p
    n, S = A.n_rows, X.shape[1]
    inv = None
    if in_idx is not None:
        inv_h = np.full(n, -1, np.int32)
        inv_h[np.asarray(in_idx)] = np.arange(len(in_idx), dtype=np.int32)
        inv = _dev(inv_h)
    rmap = None if out_idx is None else _dev(np.asarray(out_idx, np.int32))
    n_out = n if out_idx is None else len(out_idx)
    xb, ldx = _padded(X, pad)
    ldy = S + pad
    yb = torch.full((n_out * ldy + 64,), float("nan"), dtype=torch.float64, device="cuda")
    need = eng.lib.grf_poly_workspace_bytes(n, n_f, S)
    ws = torch.full((need // 8 + 64,), float("nan"), dtype=torch.float64, device="cuda")
    ft = _dev(np.asarray(f, np.float64))
    rc = eng.lib.grf_poly_apply_f64(n, _p(A.ptr), _p(A.idx), _p(A.val), _p(ft), n_f, _p(inv), _p(rmap), n_out, _p(xb),
                                    ldx, S, _p(yb), ldy, _p(ws), need, eng.stream)
    assert rc == 0, eng.lib.grf_last_error()
    out = yb.cpu().numpy()
    body = out[:n_out * ldy].reshape(n_out, ldy)
    assert np.isnan(body[:, S:]).all() and np.isnan(out[n_out * ldy:]).all(), "wrote outside [rows x S] of Y"
    assert np.isnan(ws[need // 8:].cpu().numpy()).all(), "wrote past the workspace"
    assert np.isnan(xb.cpu().numpy()[X.shape[0] * ldx:]).all()
    return body[:, :S].copy()


def _configs(n, seed):
    """(in_idx, out_idx): a row-sparse input through an unsorted selection with a row map of length N; a dense
    input with a row map of length 1; no maps."""
    r = np.random.default_rng(seed)
    T = r.permutation(n)[:max(1, (2 * n) // 3)]
    return [(T, r.permutation(n)), (None, r.permutation(n)[:1]), (None, None)]


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
@pytest.mark.parametrize("n_f", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_poly_apply(eng, n, n_f, integer):
    G = PR.directed_graph(n, 100 * n + n_f, integer)
    if n == 300:
        assert sorted(set(np.diff(G.indptr))) == [0, 1, 3, 63, 64, 65, 200]
        assert abs(G - G.T).max() > 0
    A = _csr(eng, G)
    f = PR.modulator(n_f, n, integer)
    for si, S in enumerate(S_ALL):
        for ci, (in_idx, out_idx) in enumerate(_configs(n, S)):
            X = PR.block(n if in_idx is None else len(in_idx), S, 7 * S + ci, integer)
            want, bound = PR.horner(G, f, n_f, X, in_idx=in_idx, out_idx=out_idx)
            got = _apply_raw(eng, A, f, n_f, X, in_idx, out_idx, pad=(si + ci) % 3)
            if integer:
                assert PR.abs_chain_max(G, f, n_f, X, in_idx) < 2.0 ** 53
                assert np.array_equal(got, want), (S, ci)
            else:
                assert np.all(np.abs(got - want) <= bound), (S, ci, float(np.max(np.abs(got - want) - bound)))
            if S in (3, 65) and ci == 0:
                again = _apply_raw(eng, A, f, n_f, X, in_idx, out_idx, pad=1)
                assert np.array_equal(again.view(np.uint64), got.view(np.uint64)), "two calls differ"


def test_engine_poly_apply_transpose_and_modulator_cut(eng):
    n, L = 300, 5
    G = PR.directed_graph(n, 9, integer=True)
    op = _op(eng, G, L)
    assert op.L == L and op.shape == (n, n) and op.Gt is not op.G
    f = PR.modulator(10, 3, integer=True)          # longer than L: cut to L
    X = PR.block(n, 12, 1, integer=True)
    got = eng.poly_apply(op, _dev(f), _dev(X)).cpu().numpy()
    assert np.array_equal(got, PR.horner(G, f[:L], L, X)[0])
    assert np.array_equal(got, eng.poly_apply(op, _dev(f[:L]), _dev(X)).cpu().numpy())
    Gt = sp.csr_matrix(G.T)
    Gt.sort_indices()
    gt = eng.poly_apply(op, _dev(f), _dev(X), transpose=True).cpu().numpy()
    assert np.array_equal(gt, PR.horner(Gt, f, L, X)[0]) and not np.array_equal(gt, got)
    sym = _op(eng, G + G.T, 3)
    assert sym.Gt is sym.G
    import torch
    with pytest.raises(ValueError):
        eng.poly_apply(op, _dev(f), _dev(X[:5]), in_rows=torch.tensor([1, 2, 2, 3, 4]))
    with pytest.raises(NotImplementedError):
        eng.poly_apply(op, _dev(f), _dev(PR.block(n, 257, 0, True)))


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_poly_gram_matvec_vs_dense(eng, integer):
    n, L, S, noise = 300, 4, 65, 0.25
    G = PR.directed_graph(n, 21, integer, long_rows=(0, 1, 63, 64, 65), weights=(-1.0, 1.0))
    f = PR.modulator(L, 4, integer)
    r = np.random.default_rng(8)
    T = r.permutation(n)[:200]
    V = PR.block(200, S, 2, integer)
    op = _op(eng, G, L)
    got = eng.poly_gram_matvec(op, _dev(f), _dev(V), rows=_dev(T), cols=_dev(T), noise=noise).cpu().numpy()
    Gt = sp.csr_matrix(G.T)
    Gt.sort_indices()
    W, eW = PR.horner(Gt, f, L, V, in_idx=T)
    Y, eY = PR.horner(G, f, L, W, out_idx=T, Xerr=eW)
    want = Y + noise * V
    Pt = PR.dense_poly(G, f, L)[T]
    dense = Pt @ (Pt.T @ V) + noise * V
    if integer:
        assert np.array_equal(got, want) and np.array_equal(got, dense)
    else:
        eps = 2.0 ** -53
        assert np.all(np.abs(got - want) <= eY + 2 * eps * np.abs(want))
        # the dense product's own rounding: a sum of n terms in each of its two matmuls
        mag = np.abs(Pt) @ (np.abs(Pt).T @ np.abs(V)) + noise * np.abs(V)
        assert np.all(np.abs(got - dense) <= eY + 2 * (n + 2) * eps * mag)


def test_poly_gram_matvec_vs_exact_steps_on_a_ring(eng):
    """The same K from the step matrices' path: Phi = sum_l f_l M_l on exact_steps, whose values (and Phi's)
    are rounded to fp32 -- n_f 2^-23 sum|terms| covers one fp32 rounding of the step values and one of Phi in
    each of the product's two factors."""
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.features import StepMatrices
    n, L, S = 400, 5, 12
    i = np.arange(n)
    A = sp.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))
    pre = GraphPreprocessor(A, max_walk_length=L, exact=True)
    steps = StepMatrices(pre.preprocess_graph(), engine=eng)
    op = pre.walk_operator()
    assert op.L == L and op.shape == (n, n)
    f = torch.tensor([1.0, -0.7, 0.3, -0.11, 0.03], dtype=torch.float64)
    r = np.random.default_rng(3)
    T = torch.from_numpy(r.permutation(n)[:150])
    V = _dev(r.standard_normal((150, S)))
    got = eng.poly_gram_matvec(op, f, V, rows=T, cols=T, noise=0.1).cpu().numpy()
    phi = steps.phi(f)
    ref = eng.gram_matvec(phi, V, rows=T, cols=T, noise=0.1).cpu().numpy()
    Pa = np.abs(PR.dense_poly(abs(op.G.to_scipy()), np.abs(f.numpy()), L))[T.numpy()]
    mag = Pa @ (Pa.T @ np.abs(V.cpu().numpy())) + 0.1 * np.abs(V.cpu().numpy())
    assert np.all(np.abs(got - ref) <= L * 2.0 ** -23 * mag)


# ----------------------------------------------------------------------------------------------- CG
_systems = {}


def _system(n_sys):
    if n_sys not in _systems:
        G, f, T, noise = PR.well_conditioned_system(300, n_sys, n_sys)
        _systems[n_sys] = (G, f, T, noise, PR.dense_khat(G, f, len(f), T, noise))
    return _systems[n_sys]


@pytest.mark.parametrize("S", [1, 3, 65, 256])
@pytest.mark.parametrize("n_sys", [1, 2, 5, 64, 257])
def test_cg_poly_vs_linear_cg(eng, n_sys, S):
    """x and the Lanczos coefficients against linear_cg on the dense K^ (cond <= 5, asserted by the generator)
    within 1e-10.  In exact arithmetic CG ends after n_sys iterations: beta of iteration n_sys - 1 and every
    coefficient after it are quotients of rounding residues without relative accuracy (all below 1e-20 here),
    so those rows are compared absolutely against 1e-10 instead of relative to their own size."""
    G, f, T, noise, K = _system(n_sys)
    op = _op(eng, G, len(f))
    r = np.random.default_rng(10 * n_sys + S)
    B = r.standard_normal((n_sys, S))
    if S >= 3:
        B[:, 1] = 0.0  # a zero right-hand side
    for max_iter in (1, 2, 3, 4):
        want, it_ref, ral, rbe = R.cg_lanczos(lambda v: K @ v, B, max_iter=max_iter)
        w2, it2 = OCG.linear_cg(lambda v: K @ v, B, max_iter=max_iter)
        assert it2 == it_ref and np.array_equal(w2, want)
        x, it, res, coef = eng.cg_solve_poly(op, _dev(f), _dev(B), noise, _dev(T), max_iter=max_iter,
                                             return_residuals=True, return_lanczos=True)
        x0, it0, res0 = eng.cg_solve_poly(op, _dev(f), _dev(B), noise, _dev(T), max_iter=max_iter,
                                          return_residuals=True)
        assert it == it0 == it_ref
        assert np.array_equal(x.cpu().numpy(), x0.cpu().numpy()) and np.array_equal(res, res0)
        x = x.cpu().numpy()
        assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max(), (max_iter, np.abs(x - want).max())
        if S >= 3:
            assert not x[:, 1].any()
        coef = coef.cpu().numpy()
        for k in range(it):
            for name, got, ref, residue in (("alpha", coef[k], ral[k], k >= n_sys),
                                            ("beta", coef[max_iter + k], rbe[k], k >= n_sys - 1)):
                scale = 1.0 if residue else np.abs(ref).max()
                assert np.abs(got - ref).max() <= 1e-10 * scale, (name, k, max_iter)


# ----------------------------------------------------------------------------------------- gradient
def _grad_raw(eng, op, f, n_f, T, A, B, wt):
    import torch
    from grf_amd.engine import _p
    n, S = op.shape[0], A.shape[1]
    inv_h = np.full(n, -1, np.int32)
    inv_h[T] = np.arange(len(T), dtype=np.int32)
    need = eng.lib.grf_poly_grad_workspace_bytes(n, S)
    ws = torch.full((need // 8 + 64,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((n_f + 8,), float("nan"), dtype=torch.float64, device="cuda")
    ab, ld = _padded(A, 1)
    bb, _ = _padded(B, 1)
    Gt = op.Gt
    # (named, so that the device copies live until the call has run)
    ft, inv, wd = _dev(np.asarray(f, np.float64)), _dev(inv_h), _dev(np.asarray(wt, np.float64))
    rc = eng.lib.grf_poly_grad_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, len(T), _p(inv), _p(ab),
                                   _p(bb), ld, _p(wd), S, _p(out), _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    assert int(ws[:1].view(torch.int32)[0].item()) == 0, "the ticket is not zero afterwards"
    assert np.isnan(ws[need // 8:].cpu().numpy()).all() and np.isnan(out[n_f:].cpu().numpy()).all()
    return out[:n_f].cpu().numpy()


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
@pytest.mark.parametrize("n_f", [1, 2, 8])
@pytest.mark.parametrize("n_sel", [1, 3, 257])
def test_poly_grad(eng, n_sel, n_f, integer):
    n = 300
    if integer:  # (weights +-1 and two entries per row keep sum|terms| of the products U W below 2^53)
        G = PR.directed_graph(n, 31 + n_f, True, long_rows=(0, 1, 65), degree=2, weights=(-1.0, 1.0))
    else:
        G = PR.directed_graph(n, 31 + n_f, False)
    op = _op(eng, G, n_f)
    f = PR.modulator(n_f, 5, integer)
    T = np.random.default_rng(n_sel).permutation(n)[:n_sel]
    for S in (1, 65, 256):
        A, B = PR.block(n_sel, S, 1 + S, integer), PR.block(n_sel, S, 2 + S, integer)
        wt = PR.block(1, S, 3, integer)[0] if integer else np.random.default_rng(S).standard_normal(S)
        want, bound, mag = PR.krylov_grad(G, f, n_f, T, A, B, wt)
        got = _grad_raw(eng, op, f, n_f, T, A, B, wt)
        if integer:
            assert mag < 2.0 ** 53
            assert np.array_equal(got, want), S
        else:
            assert np.all(np.abs(got - want) <= bound), (S, got - want, bound)
        assert np.array_equal(_grad_raw(eng, op, f, n_f, T, A, B, wt).view(np.uint64), got.view(np.uint64))
        if S == 65:
            via = eng.poly_grad(op, _dev(f), _dev(T), _dev(A), _dev(B), _dev(wt)).cpu().numpy()
            assert np.array_equal(via.view(np.uint64), got.view(np.uint64))


# ------------------------------------------------------------------------------- marginal likelihood
@pytest.fixture(scope="module")
def er_world(eng):
    """An Erdos-Renyi graph of mean degree 10, N = 2000, L = 8: its exact step matrices fill in."""
    n, L = 2000, 8
    r = np.random.default_rng(2024)
    U = sp.random(n, n, density=10.0 / n / 2, random_state=r, format="csr")
    A = ((U + U.T) > 0).astype(np.float64).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    G = eng.laplacian(A)
    from grf_amd.engine import WalkPolynomial
    op = WalkPolynomial(G, L, engine=eng)
    f = np.array([(-1.0) ** l / float(np.prod(np.arange(1, l + 1))) for l in range(L)])  # exp(-G), beta = 1
    Gd = G.to_scipy().toarray()
    powers = [np.eye(n)]
    for _ in range(1, L):
        powers.append(powers[-1] @ Gd)
    P = sum(fl * M for fl, M in zip(f, powers))
    return dict(n=n, L=L, G=G, op=op, f=f, powers=powers, P=P)


def test_exact_steps_do_not_fit(eng, er_world):
    """What the operator is for: G^2 of this graph already has ~110 entries per row (220 000), so a budget of
    100 000 entries -- room for G itself, 11 per row -- is exceeded at the second power."""
    assert er_world["G"].nnz < 100_000
    with pytest.raises(ValueError, match="max_nnz"):
        eng.exact_steps(er_world["G"], er_world["L"], max_nnz=100_000)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(b)))


@pytest.mark.parametrize("noise", [0.05, 1.0])
@pytest.mark.parametrize("n_train", [64, 128])
def test_mll_exactness(eng, er_world, n_train, noise):
    """Identity probes Z = sqrt(n) I, tolerance 1e-12, max_iter 48: value, d/df and d/ds2 against the dense
    truth built from dense p(G)[T] and G^l[T]; the GPU is held to 10 x the CPU restatement's own error
    against that truth (the rule of tests/test_gpu_mll.py).

    Measured on an MI355X (this test's printed figures, `pytest -m gpu -s`), relative error against the dense
    truth, GPU / CPU restatement:
      n = 64,  s2 = 0.05: value 1.4e-11 / 1.4e-11, d/df 7.4e-07 / 7.4e-07, d/ds2 2.3e-10 / 2.3e-10
      n = 64,  s2 = 1.0:  value 3.9e-12 / 3.9e-12, d/df 3.0e-06 / 3.0e-06, d/ds2 4.1e-10 / 4.1e-10
      n = 128, s2 = 0.05: value 9.5e-11 / 9.5e-11, d/df 4.1e-07 / 4.1e-07, d/ds2 1.7e-09 / 1.7e-09
      n = 128, s2 = 1.0:  value 1.3e-12 / 1.3e-12, d/df 3.5e-07 / 3.5e-07, d/ds2 9.5e-11 / 9.5e-11
    The ratio is 1.00 to the three digits printed in every row (48 iterations on both sides): on these
    well-conditioned exact kernels the two follow the same CG trajectory, and what is left is linear_cg's own
    distance from the truth.
    """
    import torch
    w = er_world
    r = np.random.default_rng(7 + n_train)
    tr = r.permutation(w["n"])[:n_train]
    y = r.standard_normal(n_train)
    Pt = w["P"][tr]
    Ms = [M[tr] for M in w["powers"]]
    Z = R.identity_probes(n_train)
    est = R.estimate(Pt, Ms, y, noise, Z, tolerance=1e-12, max_iter=48)
    tru = R.dense_truth(Pt, Ms, y, noise)
    value, g_f, g_noise, iters = eng.marginal_log_likelihood(
        w["op"], torch.from_numpy(w["f"]), torch.from_numpy(tr), torch.from_numpy(y), noise, _dev(Z), 1e-12, 48)
    got = dict(value=value, grad_f=g_f.cpu().numpy(), grad_noise=g_noise)
    assert got["grad_f"].shape == (w["L"],)
    for q in ("value", "grad_f", "grad_noise"):
        print(f"exactness n={n_train} s2={noise} {q}: gpu vs truth {_rel(got[q], tru[q]):.3e}  "
              f"restatement vs truth {_rel(est[q], tru[q]):.3e}  iterations {iters} / {est['iters']}")
    for q in ("value", "grad_f", "grad_noise"):
        assert _rel(got[q], tru[q]) <= 10.0 * _rel(est[q], tru[q]), q


# ---------------------------------------------------------------------------------- SparseGraphGP
def test_sparse_graph_gp_on_the_operator(eng):
    import torch
    from efficient_graph_gp_sparse.models import SparseGraphGP
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    n, L = 600, 4
    U = sp.random(n, n, density=6.0 / n / 2, random_state=np.random.default_rng(21), format="csr")
    A = ((U + U.T) > 0).astype(np.float64).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    pre = GraphPreprocessor(A, max_walk_length=L)
    op = pre.walk_operator()

    class Lik:
        noise = torch.tensor([0.05], dtype=torch.float64, requires_grad=True)

    r = np.random.default_rng(0)
    perm = r.permutation(n)
    x_train = torch.tensor(perm[:400], dtype=torch.float32, device="cuda").unsqueeze(1)
    y_train = torch.tensor(r.standard_normal(400), dtype=torch.float32, device="cuda")
    x_test = torch.tensor(perm[400:500], dtype=torch.float32, device="cuda").unsqueeze(1)
    gp = SparseGraphGP(x_train, y_train, Lik(), op, L).cuda()
    assert gp.num_nodes == n
    torch.manual_seed(123)
    out = gp.predict(x_test, n_samples=32, max_iter=3)
    assert out.shape == (32, 100) and out.dtype == torch.float32 and gp.last_cg_iterations == 3
    torch.manual_seed(123)
    e1 = torch.randn(32, n, device="cuda")
    e2 = torch.sqrt(torch.tensor(0.05, device="cuda")) * torch.randn(32, 400, device="cuda")
    f = gp.covar_module.modulator_vector.detach().cpu().numpy().astype(np.float64)
    Phi = sp.csr_matrix(PR.dense_poly(op.G.to_scipy(), f, L))
    want, it = OCG.pathwise_predict(Phi, perm[:400], perm[400:500], y_train.cpu().numpy(), 0.05, e1.cpu().numpy(),
                                    e2.cpu().numpy(), max_iter=3)
    # the model returns float32 like the reference (1e-5, as test_gpu_cg's mirror test); the engine's fp64
    # samples meet the oracle to 1e-10 at 3 iterations (test_pathwise_predict_vs_oracle's figure)
    rel = np.linalg.norm(out.cpu().numpy() - want) / np.linalg.norm(want)
    assert it == 3 and rel <= 1e-5, rel
    out64, it64 = eng.pathwise_predict(op, torch.from_numpy(perm[:400]), torch.from_numpy(perm[400:500]), y_train,
                                       0.05, e1, e2, max_iter=3, f=torch.from_numpy(f))
    rel64 = np.linalg.norm(out64.cpu().numpy() - want) / np.linalg.norm(want)
    assert it64 == 3 and out64.dtype == torch.float64 and rel64 <= 1e-10, rel64

    Z = torch.randn(400, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    mll = gp.marginal_log_likelihood(probes=Z, tolerance=1e-6)
    mll.backward()
    gf, gn = gp.covar_module.raw_modulator_vector.grad, Lik.noise.grad
    assert gf is not None and gf.shape == (L,) and bool(torch.isfinite(gf).all()) and bool(gf.abs().sum() > 0)
    assert gn is not None and bool(torch.isfinite(gn).all()) and float(gn.abs().sum()) > 0
    idx = x_train.flatten().long()
    for call in (lambda: gp.covar_module.forward(idx, idx), lambda: gp.covar_module.forward(None, None, diag=True),
                 gp.covar_module._get_feature_matrix):
        with pytest.raises(NotImplementedError, match="predict"):
            call()
