"""CPU pins of tests/dense_gram_reference.py (no GPU): the bf16 rounding against torch.bfloat16, the three-plane
split against Fractions, the plane layout on a hand-written example, the plan restatements at the shapes of
tests/test_gpu_dense_gram_kernels.py with the expected numbers written out, the conditions every input of that file
claims (2^24, coverage, live planes, exactness), and the real_case bounds on a plain numpy emulation of either chain."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import dense_gram_reference as D


def _bf16_torch(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


# --------------------------------------------------------------------------------------------------- bf16_rne
def test_bf16_rne_matches_torch_bfloat16():
    r = np.random.default_rng(0)
    rand = np.ldexp(r.integers(1 << 23, 1 << 24, 20000).astype(np.float64), r.integers(-83, 36, 20000))
    rand = (rand * r.choice([-1.0, 1.0], 20000)).astype(np.float32)
    # exact ties: the odd multiples of half a bf16 ulp, whose neighbours are an even and an odd bf16 (both ways)
    hi = r.integers(0x0080, 0x7F00, 4000).astype(np.uint32)               # normal bf16 bit patterns, either parity
    ties = ((hi << 16) | 0x8000).view(np.float32)
    ties = np.concatenate([ties, -ties])
    tu = ties.view(np.uint32)
    near = np.concatenate([(tu + 1).view(np.float32), (tu - 1).view(np.float32)])  # one fp32 ulp either side
    for name, x in (("random", rand), ("ties", ties), ("near ties", near), ("edges", D.edge_values())):
        assert _same(D.bf16_rne(x), _bf16_torch(x)), name
    up, down = (tu >> 16) & 1 == 1, (tu >> 16) & 1 == 0
    assert up.any() and down.any()
    got = D.bf16_rne(ties).view(np.uint32)
    assert np.all(got[down] == (tu[down] & 0xFFFF0000)) and np.all(got[up] == (tu[up] & 0xFFFF0000) + 0x10000)
    assert np.all((D.bf16_rne(rand).view(np.uint32) & 0xFFFF) == 0)


# ----------------------------------------------------------------------------------------------------- split3
def _is_bf16(x):
    """x (a Fraction) has at most 8 significant bits and a normal bf16 exponent."""
    if x == 0:
        return True
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 7)
    return q.denominator == 1 and -126 <= e <= 127


def test_split3_exact_sum_and_plane_sizes():
    r = np.random.default_rng(1)
    rand = np.ldexp(r.integers(1 << 23, 1 << 24, 3000).astype(np.float64), r.integers(-83, 36, 3000))
    x = np.concatenate([(rand * r.choice([-1.0, 1.0], 3000)).astype(np.float32), D.edge_values()])
    assert np.float32(2.0 ** 60) in x and np.float32(2.0 ** -60) in x and np.float32(-2.0 ** 60) in x
    a0, a1, a2 = D.split3(x)
    neg = pos = 0
    for a, p0, p1, p2 in zip(x, a0, a1, a2):
        fa, f0, f1, f2 = (Fraction(float(v)) for v in (a, p0, p1, p2))
        assert f0 + f1 + f2 == fa, a
        assert _is_bf16(f0) and _is_bf16(f1) and _is_bf16(f2), a
        assert abs(f1) <= abs(fa) / 2 ** 8 and abs(f2) <= abs(fa) / 2 ** 16, a
        neg += f0 * f1 < 0 or f1 * f2 < 0
        pos += f1 != 0 and f2 != 0
    assert neg > 100 and pos > 1000            # sign changes between planes and live last planes are covered


def test_planes_ref_layout_by_hand():
    """2 x 17: k-tile 0 holds columns 0..15, k-tile 1 column 16 and fifteen zero columns."""
    A = np.zeros((2, 32), np.float32)
    A[0, :17] = np.arange(1, 18)                      # small integers: bf16 exactly, planes 1 and 2 zero
    A[1, 0] = 1.0 + 2.0 ** -9 + 2.0 ** -18            # planes 1, 2^-9, 2^-18
    A[1, 16] = -(1.0 + 2.0 ** -9 + 2.0 ** -18) * 4
    A[:, 17:] = 7.0                                   # (past k_dim: must not appear)
    P = D.planes_ref(A, 17)
    assert P.shape == (2, 192) and P.dtype == np.uint8
    h = P.view(np.uint16).reshape(2, 2, 3, 16)        # [row][k-tile][plane][k]
    bits = lambda v: int(np.array([v], np.float32).view(np.uint32)[0] >> 16)
    assert [int(v) for v in h[0, 0, 0]] == [bits(float(i)) for i in range(1, 17)]
    assert int(h[0, 1, 0, 0]) == bits(17.0) and not h[0, 1, 0, 1:].any() and not h[0, :, 1:].any()
    assert (int(h[1, 0, 0, 0]), int(h[1, 0, 1, 0]), int(h[1, 0, 2, 0])) == (bits(1.0), bits(2.0 ** -9), bits(2.0 ** -18))
    assert (int(h[1, 1, 0, 0]), int(h[1, 1, 1, 0]), int(h[1, 1, 2, 0])) == (bits(-4.0), bits(-2.0 ** -7), bits(-2.0 ** -16))
    assert not h[1, :, :, 1:].any()
    # the byte offsets themselves: row 1, k-tile 1, plane 2, k = 0 is bytes 96 + 64 .. 96 + 65 (little endian)
    assert P[1, 96 + 64] == bits(-2.0 ** -16) & 0xFF and P[1, 96 + 65] == bits(-2.0 ** -16) >> 8
    assert P[0, 2 * 3] == bits(4.0) & 0xFF and P[0, 2 * 3 + 1] == bits(4.0) >> 8


# ------------------------------------------------------------------------------------------------------ plans
def test_plan_restatements_at_the_gpu_shapes():
    p = D.dense_plan(129, 80)
    assert (p["tiles"], p["n_whole"], p["n_split"], p["k_split"]) == (3, 0, 3, 32)
    for n in D.NS_SLICES:
        for k, pieces in D.PIECES.items():
            p = D.dense_plan(n, k)
            assert (p["n_whole"], p["n_split"]) == (0, pieces) and D.path_of("ws", n, k, 0) == "slices", (n, k)
            assert p["k_split"] * (pieces - 1) < p["kpad"] <= p["k_split"] * pieces          # no empty piece
    assert D.dense_plan(129, 17)["k_split"] == 16 and D.dense_plan(129, 65)["k_split"] == 32
    for n in D.NS_WHOLE:
        assert D.dense_plan(n, 16)["n_split"] == 1 and D.path_of("split", n, 16, 0) == "whole"
        for k in D.KS_WHOLE:
            assert D.path_of("upper", n, k, workspace=False) == "whole"
    assert D.dense_plan(257, 33)["tiles"] == 6 and D.dense_plan(400, 33)["tiles"] == 10
    # stream-K over the 128-tiles
    assert D.dense_plan(2817, 33)["tiles"] == 276
    q = D.sk_plan(2817, 33)
    assert (q["kt"], q["total"], q["units"], q["grid"]) == (3, 828, 2, 414)
    assert D.sk_cut_items(0, q["kt"], q["units"], q["total"]) == 276
    q = D.sk_plan(2817, 80)
    assert (q["kt"], q["total"], q["units"], q["grid"]) == (5, 1380, 3, 460)
    assert D.sk_cut_items(0, q["kt"], q["units"], q["total"]) == 276
    q = D.sk_plan(2817, 20)
    assert (q["kt"], q["total"], q["units"], q["grid"]) == (2, 552, 2, 276)
    assert D.sk_cut_items(0, q["kt"], q["units"], q["total"]) == 0              # the uncut control
    assert D.path_of("ws", 2817, 33, 0) == "streamk" and D.path_of("split", 2817, 33, 0) == "streamk"
    assert D.path_of("ws", 2817, 0, 0) == "whole" and D.path_of("planes", 2817, 33, 0) == "whole"
    # the tail split (live only in the planes tile kernel: ws / split stream from 256 tiles on)
    p = D.dense_plan(3969, 33)
    assert (p["tiles"], p["n_whole"], p["n_split"], p["k_split"]) == (528, 0, 3, 16)
    p = D.dense_plan(5633, 33)
    assert (p["tiles"], p["n_whole"], p["split_tiles"], p["n_split"], p["k_split"]) == (1035, 512, 523, 3, 16)
    assert D.path_of("planes", 3969, 33, 0) == "tail" and D.path_of("planes", 5633, 33, 0) == "tail"
    assert D.path_of("split", 5633, 33, 0) == "streamk"
    # wide items
    w = D.sk_plan_wide(5633, 33)
    assert (w["items"], w["dp_rounds"], w["units"], w["grid"], w["xcd_slots"]) == (529, 1, 4, 256, 1)
    assert w["total"] - w["dp_rounds"] * w["grid"] * w["kt"] == 273 * 3         # 1 round + 273 items streamed
    w = D.sk_plan_wide(5633, 33, xcd=False)
    assert (w["dp_rounds"], w["units"], w["grid"], w["xcd_slots"]) == (0, 7, 227, 0)
    items = {1: 1, 129: 2, 257: 4, 385: 6}
    for n in D.NS_WIDE:
        for k in D.KS_WIDE:
            w = D.sk_plan_wide(n, k)
            assert (w["items"], w["dp_rounds"], w["xcd_slots"]) == (items[n], 0, 0)
            assert w["units"] == 1 and w["grid"] == items[n] * D.cdiv(k, 16)    # every k-tile its own slot
            assert D.path_of("split", n, k, 1) == "wide" and D.path_of("planes", n, k, 1) == "wide"
    assert not D.wide_items(63) and D.wide_items(64) and not D.wide_items(64, 0) and D.wide_items(1, 1)


# --------------------------------------------------------------------------- the conditions of the GPU cases
SMALL = D.gpu_shapes(large=False)
LARGE = [s for s in D.gpu_shapes() if s not in SMALL]


def _check_int(n, k):
    A, K = D.int_case(n, k, 0, D.lda_of(n, k))
    M = A[:, :k].astype(np.int64)
    assert np.array_equal(M.astype(np.float32), A[:, :k]) and not A[:, k:].any()
    assert int((np.abs(M) @ np.abs(M).T).max()) < 2 ** 24
    assert D.planes_abs_gram_max(A) < 2 ** 24           # ... and so are the sums of the plane products
    rows = np.arange(n) if n <= 400 else np.random.default_rng(n).integers(0, n, 64)
    assert K.dtype == np.int64 and np.array_equal(K[rows], M[rows] @ M.T)      # (integer arithmetic throughout)
    assert D.coverage_ok(A, k)
    big = np.abs(M) > 255
    assert big.any() and np.all(M[big] % 2 != 0) and np.abs(M).max() <= 511 and np.all(np.abs(M[~big]) <= 15)
    _, a1, a2 = D.split3(A)
    assert np.array_equal(a1 != 0, np.abs(A) > 255) and not a2.any()
    return A


@pytest.mark.parametrize("n,k", SMALL, ids=lambda v: str(v))
def test_int_and_probe_case_conditions(n, k):
    _check_int(n, k)
    c = D.probe_case(n, k, 0, D.lda_of(n, k))
    _check_probe(c, n, k)


@pytest.mark.parametrize("n,k", LARGE, ids=lambda v: str(v))
def test_int_case_conditions_large(n, k):
    _check_int(n, k)
    if (n, k) == (D.N_SK, 33):
        _check_probe(D.probe_case(n, k, 0, D.lda_of(n, k)), n, k)


def _check_probe(c, n, k):
    A = c.A
    P, W = A[~c.is_w, :k], A[c.is_w, :k]
    m, e = np.frexp(np.abs(P))
    assert np.all(m == 0.5) and e.min() >= -2 and e.max() <= 4            # +-2^e, e in [-3, 3]
    assert np.all((W != 0).sum(axis=1) == 1) and np.all(W[np.arange(len(W)), c.col[c.is_w]] != 0)
    w = W[np.arange(len(W)), c.col[c.is_w]]
    _, w1, w2 = D.split3(w)
    assert np.all(w1 != 0) and np.all(w2 != 0) and np.all((np.abs(w) >= 2.0 ** -20) & (np.abs(w) < 2.0 ** 21))
    assert D.coverage_ok(A, k, rows=~c.is_w)
    # P x P: exact on a 2^-6 grid below 2^13, so exact in fp32 in any order
    pp = np.abs(P.astype(np.float64)) @ np.abs(P.astype(np.float64)).T
    assert pp.max() < 2 ** 13 and np.array_equal(pp * 64, np.rint(pp * 64))
    ref32 = c.ref.astype(np.float32)
    exact = ~c.same
    assert np.array_equal(ref32[exact].astype(np.float64), c.ref[exact])        # the claimed-exact entries are fp32
    if n > 1:
        assert c.same.sum() >= c.is_w.sum() and np.all(np.diag(c.same) == c.is_w)
    # a sample of entries of every kind, in Fractions
    r = np.random.default_rng(n * 100 + k)
    for _ in range(60):
        i, j = int(r.integers(0, n)), int(r.integers(0, n))
        s = sum(D.frac(A[i, q]) * D.frac(A[j, q]) for q in range(k))
        assert Fraction(float(c.ref[i, j])) == s, (i, j)
        if not c.same[i, j]:
            assert Fraction(float(ref32[i, j])) == s, (i, j)
            if c.is_w[i] and c.is_w[j]:
                assert s == 0 and not np.signbit(ref32[i, j])


# ------------------------------------------------------------------------------ the bounds on the emulations
@pytest.mark.parametrize("n,k", [(129, 33), (129, 80), (200, 17)])
def test_real_case_bounds_hold_for_the_emulated_chains(n, k):
    A, ref, T, S = D.real_case(n, k, 0, D.lda_of(n, k))
    nz = A[:, :k] != 0
    assert 0.1 < nz.mean() < 0.3 and (A[::2] < 0).any() and not (A[1::2] < 0).any()
    mag = np.abs(A[:, :k][nz])
    assert mag.max() / mag.min() > 1e3 and (T == 0).any() and T.max() >= 4
    worst = {}
    for split, K in ((False, D.emulate_fp32(A, k)), (True, D.emulate_split(A, k))):
        bound = D.real_bound(T, S, split)
        err = np.abs(K.astype(np.float64) - ref)
        assert np.all(err <= bound), (split, float((err - bound).max()))
        assert np.all(K[T == 0] == 0)                                   # no live term: the bound is 0
        worst[split] = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"n = {n} k = {k}: worst err / bound of the emulations: fp32 {worst[False]:.3f} split {worst[True]:.3f}")
    # the split's six products lose what the bound says they may: its emulation differs from the fp32 chain's
    assert not np.array_equal(D.emulate_fp32(A, k), D.emulate_split(A, k))
