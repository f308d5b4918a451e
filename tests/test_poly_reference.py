"""CPU: pins tests/poly_reference.py, the restatement the GPU tests of the walk polynomial operator compare
against -- Horner against exact rational arithmetic on integer cases and against numpy's matrix powers on
real ones (within its own bound), the gradient contraction against the dense formula and against central
differences of a^T K^(f) b on a non-symmetric G."""
from fractions import Fraction

import numpy as np
import pytest

import poly_reference as PR


def _fraction_poly_apply(G, f, X):
    """p(G) X in exact rationals, from the definition sum_l f_l G^l X."""
    Gd = G.toarray()
    n, S = X.shape
    Gf = [[Fraction(int(v)) for v in row] for row in Gd]
    cur = [[Fraction(int(v)) for v in row] for row in X]
    out = [[Fraction(0)] * S for _ in range(n)]
    for l, fl in enumerate(f):
        if l:
            cur = [[sum(Gf[i][k] * cur[k][c] for k in range(n) if Gf[i][k]) for c in range(S)] for i in range(n)]
        for i in range(n):
            for c in range(S):
                out[i][c] += Fraction(int(fl)) * cur[i][c]
    return out


@pytest.mark.parametrize("n_f", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 5, 12])
def test_horner_is_exact_on_integers(n, n_f):
    G = PR.directed_graph(n, 10 * n + n_f, integer=True)
    f = PR.modulator(n_f, n, integer=True)
    X = PR.block(n, 3, n_f, integer=True)
    assert PR.abs_chain_max(G, f, n_f, X) < 2.0 ** 53
    Y, bound = PR.horner(G, f, n_f, X)
    want = _fraction_poly_apply(G, f, X)
    assert all(Fraction(float(Y[i, c])) == want[i][c] for i in range(n) for c in range(3))
    # (the bound is never zero on nonzero terms, and an integer result needs none)
    assert np.all(bound >= 0.0)


def test_modulator_is_cut_to_L():
    G = PR.directed_graph(9, 3, integer=True)
    f = PR.modulator(6, 1, integer=True)
    X = PR.block(9, 2, 0, integer=True)
    assert np.array_equal(PR.horner(G, f, 4, X)[0], PR.horner(G, f[:4], 4, X)[0])
    assert np.array_equal(PR.dense_poly(G, f, 4), PR.dense_poly(G, f[:4], 9))


@pytest.mark.parametrize("n_f", [1, 2, 5, 8])
def test_horner_meets_matrix_power_within_its_bound(n_f):
    n = 300
    G = PR.directed_graph(n, 40 + n_f, integer=False)
    assert sorted(set(np.diff(G.indptr))) == [0, 1, 3, 63, 64, 65, 200]
    f = PR.modulator(n_f, 7, integer=False)
    r = np.random.default_rng(5)
    T = r.permutation(n)[:70]
    out = r.permutation(n)[:40]
    X = PR.block(70, 11, 3, integer=False)
    P = PR.block(40, 11, 4, integer=False)
    Y, bound = PR.horner(G, f, n_f, X, in_idx=T, out_idx=out, P=P, noise=0.3)
    want = (PR.dense_poly(G, f, n_f) @ PR.scatter_rows(X, T, n))[out] + 0.3 * P
    assert np.all(np.abs(Y - want) <= bound + 1e-300)
    # the bound is a rounding bound, not slack: relative to the result's scale it stays near 2^-53 x row length
    assert bound.max() <= 1e-11 * max(np.abs(want).max(), 1.0)


def test_gradient_matches_dense_formula_and_central_differences():
    n, L = 60, 5
    G = PR.directed_graph(n, 77, integer=False, long_rows=())
    assert abs(G - G.T).max() > 0.05  # (directed: a mix-up of G and G^T would show)
    f = PR.modulator(L, 9, integer=False)
    r = np.random.default_rng(11)
    T = r.permutation(n)[:25]
    A, B = PR.block(25, 4, 1, integer=False), PR.block(25, 4, 2, integer=False)
    wt = r.standard_normal(4)
    got, bound, _ = PR.krylov_grad(G, f, L, T, A, B, wt)
    want = PR.dense_grad(G, f, L, T, A, B, wt)
    assert np.all(np.abs(got - want) <= bound + 1e-12 * np.abs(want).max())

    def quad(fv):
        K = PR.dense_khat(G, fv, L, T, 0.0)
        return float(np.sum(wt * np.sum(A * (K @ B), axis=0)))

    h = 1e-5
    for l in range(L):
        e = np.zeros(L)
        e[l] = h
        cd = (quad(f + e) - quad(f - e)) / (2 * h)
        assert abs(cd - got[l]) <= 1e-8 * max(abs(got[l]), np.abs(got).max()), l


def test_integer_gradient_is_exact():
    n, L = 12, 3
    G = PR.directed_graph(n, 5, integer=True)
    f = PR.modulator(L, 2, integer=True)
    T = np.array([7, 2, 9, 0])
    A, B = PR.block(4, 3, 5, integer=True), PR.block(4, 3, 6, integer=True)
    wt = np.array([1.0, -2.0, 1.0])
    got, _, mag = PR.krylov_grad(G, f, L, T, A, B, wt)
    assert mag < 2.0 ** 53
    assert np.array_equal(got, PR.dense_grad(G, f, L, T, A, B, wt))


def test_well_conditioned_generator_asserts_its_condition():
    G, f, T, noise = PR.well_conditioned_system(300, 257, 1)
    assert np.linalg.cond(PR.dense_khat(G, f, len(f), T, noise)) <= 5.0
    assert len(set(T.tolist())) == 257 and not np.array_equal(T, np.sort(T))
