"""GPU: K blocks, diagonals and modulator gradients from the walk operator (grf_poly_kernel_block_f64 /
_diag_f64 / _grad_f64 of csrc/grf_poly.hip, GRFEngine.poly_kernel_*, grf_kernel on a WalkPolynomial,
SparseWalkOperatorKernel) against tests/poly_block_reference.py.

* every column of a block is bit-identical to ``poly_gram_matvec`` on its unit vector: one, two and three
  column blocks (the last one column wide), repeated and unsorted indices, ``None`` for all nodes, rows of 0, 1,
  63, 64, 65 and 200 entries, symmetric and directed G, padded pitches over NaN;
* the restatement's bits on integer-valued inputs (every sum|terms| below 2^53) for block, diagonal and both
  gradients; its bounds on real ones (the chains' 2 D 2^-53 sum|terms| per step carried through both chains, the
  column reductions' with D = poly_block_reference.reduction_depth);
* the diagonal against the block's diagonal, run-to-run bits, tickets zero after every call;
* grf_kernel on the operator against grf_kernel on the exact step matrices of a ring and a grid (3e-5 |Phi||Phi|^T);
* autograd, exact symmetry of K(x, x), no host synchronisation, the memory guard, SparseWalkOperatorKernel.

Observed error / bound ratios on real inputs (test_real_inputs_within_the_restatements_bounds prints them; the
largest over its cases, measured on an MI355X): see that test's docstring.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import poly_block_reference as BR
import poly_reference as PR

pytestmark = pytest.mark.gpu

N2_ALL = [1, 63, 64, 65, 255, 256, 257, 513]
N1_ALL = [1, 5, 257]


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _op(eng, G, L):
    from grf_amd.engine import DeviceCSR, WalkPolynomial
    return WalkPolynomial(DeviceCSR.from_scipy(sp.csr_matrix(G), eng.device), L, engine=eng)


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _nan(numel):
    import torch
    return torch.full((numel,), float("nan"), dtype=torch.float64, device="cuda")


def _ticket_is_zero(ws):
    import torch
    return int(ws[:1].view(torch.int32)[0].item()) == 0


def _block_raw(eng, op, f, n_f, x1, x2, pad):
    """grf_poly_kernel_block_f64 itself into a NaN buffer of pitch n2 + pad; K after checking that nothing
    outside [n1 x n2] and nothing past the buffer or the workspace was written."""
    import torch
    from grf_amd.engine import _p
    n, n1, n2 = op.shape[0], len(x1), len(x2)
    ldk = n2 + pad
    kb = _nan(n1 * ldk + 64)
    need = eng.lib.grf_poly_kernel_block_workspace_bytes(n, n_f, n2)
    ws = _nan(need // 8 + 64)
    ft, d1, d2 = _dev(np.asarray(f, np.float64)), _dev(np.asarray(x1, np.int32)), _dev(np.asarray(x2, np.int32))
    G, Gt = op.G, op.Gt
    rc = eng.lib.grf_poly_kernel_block_f64(n, _p(G.ptr), _p(G.idx), _p(G.val), _p(Gt.ptr), _p(Gt.idx), _p(Gt.val),
                                           _p(ft), n_f, _p(d1), n1, _p(d2), n2, _p(kb), ldk, _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    out = kb.cpu().numpy()
    body = out[:n1 * ldk].reshape(n1, ldk)
    assert np.isnan(body[:, n2:]).all() and np.isnan(out[n1 * ldk:]).all(), "wrote outside [n1 x n2] of K"
    assert np.isnan(ws[need // 8:].cpu().numpy()).all(), "wrote past the workspace"
    return body[:, :n2].copy()


def _diag_raw(eng, op, f, n_f, x):
    import torch
    from grf_amd.engine import _p
    n, n_x = op.shape[0], len(x)
    need = eng.lib.grf_poly_kernel_diag_workspace_bytes(n, n_f, n_x)
    ws, out = _nan(need // 8 + 64), _nan(n_x + 8)
    ft, dx = _dev(np.asarray(f, np.float64)), _dev(np.asarray(x, np.int32))
    Gt = op.Gt
    rc = eng.lib.grf_poly_kernel_diag_f64(n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, _p(dx), n_x, _p(out),
                                          _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    assert _ticket_is_zero(ws), "the ticket is not zero afterwards"
    assert np.isnan(ws[need // 8:].cpu().numpy()).all() and np.isnan(out[n_x:].cpu().numpy()).all()
    return out[:n_x].cpu().numpy()


def _grad_raw(eng, op, f, n_f, g, x1, x2=None, diag=False, pad=1):
    """grf_poly_kernel_grad_f64 itself (x1, x2 without repeats: the maps are then one-to-one)."""
    import torch
    from grf_amd.engine import _p
    n, n1 = op.shape[0], len(x1)
    n2 = n1 if diag else len(x2)
    need = eng.lib.grf_poly_kernel_grad_workspace_bytes(n, n1, n2, int(diag))
    ws, out = _nan(need // 8 + 64), _nan(n_f + 8)
    ft, d1 = _dev(np.asarray(f, np.float64)), _dev(np.asarray(x1, np.int32))
    Gt = op.Gt
    head = (n, _p(Gt.ptr), _p(Gt.idx), _p(Gt.val), _p(ft), n_f, _p(d1), n1)
    if diag:
        gd = _dev(np.asarray(g, np.float64))
        rc = eng.lib.grf_poly_kernel_grad_f64(*head, None, None, n1, None, _p(gd), 1, 1, _p(out), _p(ws), need,
                                              eng.stream)
    else:
        inv = []
        for x in (x1, x2):
            h = np.full(n, -1, np.int32)
            h[np.asarray(x)] = np.arange(len(x), dtype=np.int32)
            inv.append(_dev(h))
        d2 = _dev(np.asarray(x2, np.int32))
        ldg = n2 + pad
        gb = _nan(n1 * ldg + 64)
        gb[:n1 * ldg].view(n1, ldg)[:, :n2] = _dev(np.asarray(g, np.float64))
        rc = eng.lib.grf_poly_kernel_grad_f64(*head, _p(inv[0]), _p(d2), n2, _p(inv[1]), _p(gb), ldg, 0, _p(out),
                                              _p(ws), need, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.grf_last_error()
    assert _ticket_is_zero(ws), "the ticket is not zero afterwards"
    assert np.isnan(ws[need // 8:].cpu().numpy()).all() and np.isnan(out[n_f:].cpu().numpy()).all()
    return out[:n_f].cpu().numpy()


def _unit_matvec_columns(eng, op, f, x1, x2):
    """K[x1, x2] column by column from poly_gram_matvec on unit vectors: the distinct nodes of x2 in chunks of
    256 columns (the operator's limit), a column of the block being the column of its node."""
    import torch
    xu, pos = np.unique(np.asarray(x2), return_inverse=True)
    cols = []
    for c0 in range(0, xu.size, 256):
        chunk = xu[c0:c0 + 256]
        eye = torch.eye(chunk.size, dtype=torch.float64, device="cuda")
        cols.append(eng.poly_gram_matvec(op, f, eye, rows=_dev(np.asarray(x1)), cols=_dev(chunk)))
    return torch.cat(cols, dim=1).cpu().numpy()[:, pos]


def _graph(n, n_f, integer=False):
    """Directed, with rows of 0, 1, 63, 64, 65 and 200 entries at n = 300; symmetric at n = 130."""
    G = PR.directed_graph(n, 100 * n + n_f, integer)
    if n == 130:
        G = sp.csr_matrix(G + G.T)
        G.sort_indices()
        assert abs(G - G.T).max() == 0
    elif n > 1:
        assert abs(G - G.T).max() > 0
    if n == 300:
        assert sorted(set(np.diff(G.indptr))) == [0, 1, 3, 63, 64, 65, 200]
    return G


@pytest.mark.parametrize("n_f", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 64, 65, 130, 300])
def test_block_columns_are_bit_identical_to_the_unit_matvec(eng, n, n_f):
    G = _graph(n, n_f)
    op = _op(eng, G, n_f)
    assert (op.Gt is op.G) == (n == 130 or n == 1)
    f = PR.modulator(n_f, n, integer=False)
    fd = _dev(f)
    for i2, n2 in enumerate(N2_ALL):
        x2 = BR.index_list(n, n2, n2)
        for i1, n1 in enumerate(N1_ALL):
            x1 = BR.index_list(n, n1, 7 * n1 + n2)
            got = _block_raw(eng, op, f, n_f, x1, x2, pad=(i1 + i2) % 3)
            want = _unit_matvec_columns(eng, op, fd, x1, x2)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n1, n2)
            if n_f == 1:
                assert np.array_equal(got, (f[0] * f[0]) * (x1[:, None] == x2[None, :]))
            if (n1, n2) in ((5, 65), (257, 257)):
                via = eng.poly_kernel_block(op, fd, _dev(x1), _dev(x2)).cpu().numpy()
                again = _block_raw(eng, op, f, n_f, x1, x2, pad=1)
                assert np.array_equal(via.view(np.uint64), got.view(np.uint64))
                assert np.array_equal(again.view(np.uint64), got.view(np.uint64)), "two calls differ"
    # None: all nodes, on either side
    x = BR.index_list(n, 5, 3)
    full = eng.poly_kernel_block(op, fd).cpu().numpy()
    assert full.shape == (n, n)
    assert np.array_equal(full, _block_raw(eng, op, f, n_f, np.arange(n), np.arange(n), pad=0))
    assert np.array_equal(eng.poly_kernel_block(op, fd, _dev(x), None).cpu().numpy(), full[x])
    assert np.array_equal(eng.poly_kernel_block(op, fd, None, _dev(x)).cpu().numpy(), full[:, x])
    # an empty side touches nothing
    assert tuple(eng.poly_kernel_block(op, fd, _dev(x[:0]), _dev(x)).shape) == (0, 5)
    assert tuple(eng.poly_kernel_block(op, fd, _dev(x), _dev(x[:0])).shape) == (5, 0)
    assert eng.poly_kernel_diag(op, fd, _dev(x[:0])).numel() == 0


def _integer_case(n_f):
    # (weights +-1 and two entries per row keep every sum|terms| of both chains and of the products below 2^53)
    n = 300
    G = PR.directed_graph(n, 31 + n_f, True, long_rows=(0, 1, 65), degree=2, weights=(-1.0, 1.0))
    return n, G, PR.modulator(n_f, 5, integer=True)


@pytest.mark.parametrize("n_f", [1, 2, 3, 8])
def test_integer_inputs_give_the_restatements_bits(eng, n_f):
    n, G, f = _integer_case(n_f)
    op = _op(eng, G, n_f)
    fa, Ga = np.abs(f), abs(G)
    for n1, n2 in ((5, 65), (257, 513), (1, 256)):
        x1, x2 = BR.index_list(n, n1, n1), BR.index_list(n, n2, n2 + 1)
        assert BR.kernel_block(Ga, fa, n_f, x1, x2)[0].max() < 2.0 ** 53
        want, _ = BR.kernel_block(G, f, n_f, x1, x2)
        assert np.array_equal(_block_raw(eng, op, f, n_f, x1, x2, pad=2), want), (n1, n2)
        assert np.array_equal(want, BR.dense_block(G, f, n_f, x1, x2))
        dwant, _ = BR.kernel_diag(G, f, n_f, x2)
        dgot = _diag_raw(eng, op, f, n_f, x2)
        assert np.array_equal(dgot, dwant), n2
        assert np.array_equal(dgot, np.diag(_block_raw(eng, op, f, n_f, x2, x2, pad=0)))   # the block's diagonal
        if n_f == 1:
            assert np.array_equal(dgot, np.full(n2, f[0] * f[0]))
        # the gradients: the C entry point on distinct nodes, the engine on the repeated ones
        r = np.random.default_rng(n1 + n2)
        u1, u2 = r.permutation(n)[:n1], r.permutation(n)[:min(n2, n)]
        g = PR.block(n1, len(u2), n1, integer=True)
        gwant, _, mag = BR.kernel_grad(G, f, n_f, g, u1, u2)
        assert mag < 2.0 ** 53
        ggot = _grad_raw(eng, op, f, n_f, g, u1, u2)
        assert np.array_equal(ggot, gwant), (n1, n2)
        assert np.array_equal(_grad_raw(eng, op, f, n_f, g, u1, u2, pad=0).view(np.uint64), ggot.view(np.uint64))
        g = PR.block(n1, n2, n2, integer=True)
        gwant, _, mag = BR.kernel_grad(G, f, n_f, g, x1, x2)
        assert mag < 2.0 ** 53
        assert np.array_equal(eng.poly_kernel_grad(op, _dev(f), _dev(g), _dev(x1), _dev(x2)).cpu().numpy(), gwant)
        gd = PR.block(1, n2, 3, integer=True)[0]
        dgwant, _, mag = BR.kernel_diag_grad(G, f, n_f, gd, x2)
        assert mag < 2.0 ** 53
        dggot = _grad_raw(eng, op, f, n_f, gd, x2, diag=True)
        assert np.array_equal(dggot, dgwant), n2
        assert np.array_equal(_grad_raw(eng, op, f, n_f, gd, x2, diag=True).view(np.uint64), dggot.view(np.uint64))
        via = eng.poly_kernel_grad(op, _dev(f), _dev(gd), _dev(x2), diag=True).cpu().numpy()
        assert np.array_equal(via.view(np.uint64), dggot.view(np.uint64))


@pytest.mark.parametrize("n_f", [1, 2, 3, 8])
def test_real_inputs_within_the_restatements_bounds(eng, n_f, capsys):
    """Largest observed |device - restatement| / bound over the cases of this test on an MI355X (printed below;
    a ratio of 0 means equal bits):

        n_f   block   diagonal   block gradient   diagonal gradient
        1     0       0          0.0032           0.0015
        2     0.11    0.0091     0.0060           0.0056
        3     0.10    0.043      0.0047           0.0054
        8     0.11    0.11       0.0096           0.0032
    """
    n = 300
    G = _graph(n, n_f)
    f = PR.modulator(n_f, 6, integer=False)
    op = _op(eng, G, n_f)
    ratios = dict(block=0.0, diag=0.0, grad=0.0, dgrad=0.0)

    def ratio(key, got, want, bound):
        err = np.abs(np.asarray(got) - np.asarray(want))
        assert np.all(err <= bound), (key, float(np.max(err - bound)))
        nz = np.asarray(bound) > 0
        if np.any(nz):
            ratios[key] = max(ratios[key], float(np.max(err[nz] / np.asarray(bound)[nz])))

    for n1, n2 in ((5, 65), (257, 513), (1, 256)):
        x1, x2 = BR.index_list(n, n1, n1), BR.index_list(n, n2, n2 + 1)
        want, bound = BR.kernel_block(G, f, n_f, x1, x2)
        ratio("block", _block_raw(eng, op, f, n_f, x1, x2, pad=1), want, bound)
        dwant, dbound = BR.kernel_diag(G, f, n_f, x2)
        dgot = _diag_raw(eng, op, f, n_f, x2)
        ratio("diag", dgot, dwant, dbound)
        assert np.array_equal(_diag_raw(eng, op, f, n_f, x2).view(np.uint64), dgot.view(np.uint64))
        assert np.array_equal(eng.poly_kernel_diag(op, _dev(f), _dev(x2)).cpu().numpy().view(np.uint64),
                              dgot.view(np.uint64))
        # the diagonal against the block's own diagonal: each within its bound of the same numbers
        kd, kbound = BR.kernel_block(G, f, n_f, x2, x2)
        bd = np.diag(_block_raw(eng, op, f, n_f, x2, x2, pad=0))
        assert np.all(np.abs(dgot - bd) <= dbound + np.diag(kbound) + np.abs(dwant - np.diag(kd)))
        r = np.random.default_rng(n1 + n2)
        g = r.standard_normal((n1, n2))
        gwant, gbound, _ = BR.kernel_grad(G, f, n_f, g, x1, x2)
        ratio("grad", eng.poly_kernel_grad(op, _dev(f), _dev(g), _dev(x1), _dev(x2)).cpu().numpy(), gwant, gbound)
        u1, u2 = r.permutation(n)[:n1], r.permutation(n)[:min(n2, n)]
        gu = r.standard_normal((n1, len(u2)))
        gwant, gbound, _ = BR.kernel_grad(G, f, n_f, gu, u1, u2)
        ggot = _grad_raw(eng, op, f, n_f, gu, u1, u2)
        ratio("grad", ggot, gwant, gbound)
        assert np.array_equal(_grad_raw(eng, op, f, n_f, gu, u1, u2).view(np.uint64), ggot.view(np.uint64))
        gd = r.standard_normal(n2)
        dgwant, dgbound, _ = BR.kernel_diag_grad(G, f, n_f, gd, x2)
        ratio("dgrad", _grad_raw(eng, op, f, n_f, gd, x2, diag=True), dgwant, dgbound)
    with capsys.disabled():
        print(f"\n[poly block ratios] n_f={n_f} " + " ".join(f"{k}={v:.2g}" for k, v in ratios.items()))


def _ring(n):
    i = np.arange(n)
    return sp.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))


def _grid(h, w):
    idx = np.arange(h * w).reshape(h, w)
    a = np.r_[idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    b = np.r_[idx[:, 1:].ravel(), idx[1:, :].ravel()]
    A = sp.csr_matrix((np.ones(2 * a.size), (np.r_[a, b], np.r_[b, a])), shape=(h * w, h * w))
    A.sort_indices()
    return A


@pytest.mark.parametrize("graph", ["ring", "grid"])
def test_operator_kernel_agrees_with_the_exact_step_matrices(eng, graph):
    """DESIGN.md section 11 against section 12: where exact=True stays sparse, grf_kernel on the operator and on
    the exact step matrices give the same K within the project's K tolerance 3e-5 (|Phi||Phi|^T)_ij (the Phi
    path's fp32 values), and the same modulator gradients within 3e-5 of their sum|terms|."""
    import torch
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    from grf_amd.features import StepMatrices, grf_kernel
    A = _ring(400) if graph == "ring" else _grid(17, 23)
    n, L = A.shape[0], 5
    pre = GraphPreprocessor(A, max_walk_length=L, exact=True)
    steps = StepMatrices(pre.preprocess_graph(), engine=eng)
    op = pre.walk_operator()
    fv = np.array([1.0, -0.7, 0.3, -0.11, 0.03])
    r = np.random.default_rng(5)
    x1, x2 = torch.from_numpy(r.permutation(n)[:70]).cuda(), torch.from_numpy(r.permutation(n)[:90]).cuda()
    W = torch.from_numpy(r.standard_normal((70, 90))).cuda()
    wd = torch.from_numpy(r.standard_normal(90)).cuda()
    Gd = op.G.to_scipy().toarray()
    Pa = np.abs(PR.dense_poly(op.G.to_scipy(), fv, L))      # |Phi|
    i1, i2 = x1.cpu().numpy(), x2.cpu().numpy()
    out = {}
    for name, s in (("operator", op), ("steps", steps)):
        f = torch.tensor(fv, dtype=torch.float64, device="cuda", requires_grad=True)
        K = grf_kernel(f, s, x1, x2)
        (K * W).sum().backward()
        gK, f.grad = f.grad.clone(), None
        d = grf_kernel(f, s, x2, x2, diag=True)
        (d * wd).sum().backward()
        out[name] = [t.detach().cpu().numpy() for t in (K, gK, d, f.grad)]
    K, gK, d, gd = out["operator"]
    Ks, gKs, ds, gds = out["steps"]
    assert np.all(np.abs(K - Ks) <= 3e-5 * (Pa[i1] @ Pa[i2].T))
    assert np.all(np.abs(d - ds) <= 3e-5 * np.sum(Pa[i2] * Pa[i2], axis=1))
    Wa, wa = np.abs(W.cpu().numpy()), np.abs(wd.cpu().numpy())
    for l in range(L):
        Ml = np.abs(np.linalg.matrix_power(Gd, l))
        terms = float(np.sum(Wa * (Ml[i1] @ Pa[i2].T + Pa[i1] @ Ml[i2].T)))
        assert abs(gK[l] - gKs[l]) <= 3e-5 * terms, l
        dterms = 2.0 * float(np.sum(wa * np.sum(Ml[i2] * Pa[i2], axis=1)))
        assert abs(gd[l] - gds[l]) <= 3e-5 * dterms, l


def test_autograd_matches_the_restated_gradients_and_kxx_is_symmetric(eng):
    import torch
    from grf_amd.features import grf_kernel
    n, L = 300, 5
    G = _graph(n, L)
    op = _op(eng, G, L)
    fv = PR.modulator(7, 2, integer=False)          # longer than L: cut to L, zero gradient past it
    xv = BR.index_list(n, 70, 9)
    x = _dev(xv)
    f = torch.tensor(fv, dtype=torch.float64, device="cuda", requires_grad=True)
    K = grf_kernel(f, op, x, x)
    assert K.dtype == torch.float64 and torch.equal(K, K.t())
    want, bound = BR.kernel_block(G, fv, L, xv, xv)
    assert np.all(np.abs(K.detach().cpu().numpy() - want) <= 0.5 * (bound + bound.T))
    K.sum().backward()
    gwant, gbound, _ = BR.kernel_grad(G, fv, L, np.ones((70, 70)), xv, xv)
    got = f.grad.cpu().numpy()
    assert np.all(np.abs(got[:L] - gwant) <= gbound) and not got[L:].any()
    f.grad = None
    d = grf_kernel(f, op, x, x, diag=True)
    dwant, dbound = BR.kernel_diag(G, fv, L, xv)
    assert np.all(np.abs(d.detach().cpu().numpy() - dwant) <= dbound)
    d.sum().backward()
    dgwant, dgbound, _ = BR.kernel_diag_grad(G, fv, L, np.ones(70), xv)
    got = f.grad.cpu().numpy()
    assert np.all(np.abs(got[:L] - dgwant) <= dgbound) and not got[L:].any()
    # equal values in two different tensors: still exactly symmetric; K(all, all) too; f's dtype and device kept
    K2 = grf_kernel(f, op, x, x.clone())
    assert torch.equal(K2, K2.t()) and torch.equal(K2, K.detach())
    Kall = grf_kernel(f, op)
    assert tuple(Kall.shape) == (n, n) and torch.equal(Kall, Kall.t())
    f32 = torch.tensor(fv, dtype=torch.float32, requires_grad=True)    # a parameter left on the CPU
    K32 = grf_kernel(f32, op, x, x[:7])
    assert K32.dtype == torch.float32 and K32.is_cuda
    K32.sum().backward()
    assert f32.grad is not None and f32.grad.dtype == torch.float32 and not f32.grad.is_cuda
    with pytest.raises(ValueError, match="same tensor"):
        grf_kernel(f, op, x, x[:70].clone(), diag=True)


def test_operator_kernel_forward_backward_issue_no_host_sync(eng):
    """As test_sparse_kernel_forward_backward_issue_no_host_sync on the Phi path: K[x1, x2], K(x, x), the diagonal
    and the modulator gradient of the operator run under torch.cuda.set_sync_debug_mode("error")."""
    import torch
    from grf_amd.features import grf_kernel
    n, L = 300, 4
    op = _op(eng, _graph(n, L), L)
    f = torch.tensor(PR.modulator(L, 1, integer=False), dtype=torch.float64, device="cuda", requires_grad=True)
    x1 = torch.tensor([0, 3, 5, 17, 39, 3], device="cuda")
    x2 = torch.tensor([1, 3, 20], device="cuda")
    W = torch.randn(6, 3, device="cuda", dtype=torch.float64)
    ref_K = grf_kernel(f, op, x1, x2).detach().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        K = grf_kernel(f, op, x1, x2)
        Ks = grf_kernel(f, op, x1, x1)
        Kd = grf_kernel(f, op, x1, x1, diag=True)
        loss = (K * W).sum() + Ks.sum() + Kd.sum()
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(K.detach(), ref_K)
    assert torch.equal(Ks.detach(), Ks.detach().t())
    assert f.grad is not None and bool(torch.isfinite(f.grad).all()) and bool(f.grad.abs().sum() > 0)


def test_memory_guard_raises_before_allocating(eng):
    import torch
    n = 400_000     # K(all, all) would take 1.28 TB
    op = _op(eng, _ring(n), 3)
    f = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=r"400000 x 400000.*free device memory"):
        eng.poly_kernel_block(op, f)
    with pytest.raises(ValueError, match=r"400000 x 400000.*free device memory"):
        eng.poly_kernel_grad(op, f, torch.zeros(1, dtype=torch.float64, device="cuda").expand(n, n), None, None)
    assert torch.cuda.max_memory_allocated() - before < 64 << 20
    assert tuple(eng.poly_kernel_diag(op, f, torch.tensor([5, 5, 0], device="cuda")).shape) == (3,)


def test_sparse_walk_operator_kernel_forward(eng):
    import torch
    from efficient_graph_gp_sparse.gptorch_kernels_sparse import SparseGRFKernel, SparseWalkOperatorKernel
    from efficient_graph_gp_sparse.preprocessor import GraphPreprocessor
    r = np.random.default_rng(77)
    n, L = 300, 4
    U = sp.random(n, n, density=0.02, random_state=r, format="csr")
    A = ((U + U.T) > 0).astype(np.float64).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    op = GraphPreprocessor(A, max_walk_length=L).walk_operator()
    torch.manual_seed(0)
    kern = SparseWalkOperatorKernel(L, op).cuda()
    kern.raw_modulator_vector.data = kern.raw_modulator_vector.data.double()
    fv = kern.modulator_vector.detach().cpu().numpy()
    G = op.G.to_scipy()
    x1v, x2v = BR.index_list(n, 40, 1), BR.index_list(n, 300, 2)
    x1, x2 = _dev(x1v), _dev(x2v)
    K = kern.forward(x1, x2)
    want, bound = BR.kernel_block(G, fv, L, x1v, x2v)
    assert K.dtype == torch.float64 and np.all(np.abs(K.detach().cpu().numpy() - want) <= bound)
    d = kern.forward(x2, x2, diag=True)
    dwant, dbound = BR.kernel_diag(G, fv, L, x2v)
    assert np.all(np.abs(d.detach().cpu().numpy() - dwant) <= dbound)
    (K.sum() + d.sum()).backward()
    gwant = BR.kernel_grad(G, fv, L, np.ones((40, 300)), x1v, x2v)
    dgwant = BR.kernel_diag_grad(G, fv, L, np.ones(300), x2v)
    got = kern.raw_modulator_vector.grad.cpu().numpy()
    assert np.all(np.abs(got - (gwant[0] + dgwant[0])) <= gwant[1] + dgwant[1] + 2.0 ** -52 * np.abs(got))
    with pytest.raises(NotImplementedError, match="SparseWalkOperatorKernel"):
        kern._get_feature_matrix()
    plain = SparseGRFKernel(L, op).cuda()
    for call in (lambda: plain.forward(x1, x2), lambda: plain.forward(x2, x2, diag=True)):
        with pytest.raises(NotImplementedError, match="SparseWalkOperatorKernel"):
            call()
    with pytest.raises(TypeError):
        SparseWalkOperatorKernel(L, [])
