"""Numpy restatements for the dense Gram kernels (csrc/grf_gram_dense.hip): the bf16 three-plane split, the plane
layout, the host plans, and the builders of inputs on which K = A A^T is known to the bit.

No torch and no GPU here; tests/test_dense_gram_reference.py pins this file on the CPU (Fractions, torch.bfloat16)
and tests/test_gpu_dense_gram_kernels.py holds the kernels to it.

The split.  ``split3`` is the sequence of plane0 / next_plane2: a0 = bf16(a), r = a - a0, a1 = bf16(r),
a2 = r - a1, every step in fp32, conversions round to nearest even.  Stated domain: finite values with
2^-60 <= |a| <= 2^60, or 0.  There a0 + a1 + a2 == a exactly and every plane is a bf16.  OUTSIDE the domain and
not restated here: values so small that a plane falls into the bf16 subnormal range (the conversion instruction's
treatment of subnormals is not pinned), and values whose a0 rounds to infinity.  No case leaves the domain.

The plans.  ``dense_plan``, ``sk_plan``, ``sk_plan_wide`` and ``wide_items`` restate the host code of
grf_gram_dense.hip and its constants (256 CUs, 512 slots of two workgroups per CU, at most 1024 split tiles, tiles
of 128, k-tiles of 16).  They are used ONLY to assert that a test case lands on the path its name claims, never as
an oracle for K.  A change of those constants in the library must change them here.

The inputs.
  * ``int_case``: integer entries with max(|A| |A|^T) < 2^24 (asserted on the CPU for every case used): every
    partial sum in every order and decomposition is an exactly representable integer, so K is the int64 A A^T bit
    for bit on every path.  The planes of an integer are integers, and the same holds for their products.
  * ``probe_case``: exact entries that need plane 2; see its docstring for which entries are exact and for the
    derivation of the 2^-22 |w w'| bound on the rest.
  * ``real_case``: Phi-like data judged against float64 within ``real_bound``.

``real_bound``.  T = the number of k at which both factors are nonzero (a zero term adds exactly), S = sum |a b|.
  fp32 paths: (T + 4) 2^-24 S.  One FMA per nonzero term, each rounding once (2^-24 relative to a partial sum that
    is at most S in magnitude; the second-order terms T^2 2^-48 are far below the slack), and at most three slab
    additions where a tile is cut into at most four pieces: + 4.
  split paths: (T + 4) 2^-23 S + 2^-22 S.  The dropped products a1 b2 + a2 b1 + a2 b2 are at most (2^-23 + 2^-32)
    |a b| per term; c1 holds at most 2^-7 S (|a0 b1| + |a1 b0| <= 2 * 2^-8 |a b| and the rest below) so its
    roundings are 2^-7 of a chain's; the final c0 + c1 rounds once (2^-24): together below 2^-22 S.  The chain
    term (T + 4) 2^-23 S ASSUMES that one v_mfma_f32_32x32x16_bf16 accumulate errs by at most one ulp of the
    result (2^-23) rather than half an ulp; how the instruction rounds its 16-term sum has not been measured.  A
    k-tile is one accumulate per product, so the count T of terms is itself generous.
The CPU test shows that a plain numpy emulation of either chain meets these bounds before they are asked of a kernel.
"""
from fractions import Fraction

import numpy as np

TILE, BK, PLANE_BYTES = 128, 16, 96
CUS, SLOTS, MAX_SPLIT_TILES, TICKET_BYTES = 256, 512, 1024, 4096


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the split
def bf16_rne(x):
    """fp32 -> the nearest bf16 (returned as fp32), ties to even, by integer arithmetic on the bits."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(a):
    """(a0, a1, a2) of fp32 a, the sequence of plane0 / next_plane2 (all fp32 arithmetic)."""
    a = np.ascontiguousarray(a, np.float32)
    a0 = bf16_rne(a)
    r = (a - a0).astype(np.float32)
    a1 = bf16_rne(r)
    a2 = (r - a1).astype(np.float32)
    return a0, a1, a2


def bf16_bits(x):
    """The uint16 image of values that are bf16 exactly."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert np.all((u & 0xFFFF) == 0), "not a bf16"
    return (u >> 16).astype(np.uint16)


def planes_ref(A, k_dim):
    """uint8 [n, 96 ceil(k_dim / 16)]: row r, k-tile t at 96 t: plane 0 of k = 16 t .. 16 t + 15 (bf16, k order),
    plane 1, plane 2; columns from k_dim to the k-tile's end are zeros."""
    A = np.asarray(A, np.float32)
    n, kt = A.shape[0], cdiv(k_dim, BK)
    X = np.zeros((n, kt * BK), np.float32)
    X[:, :k_dim] = A[:, :k_dim]
    out = np.zeros((n, kt, 3, BK), np.uint16)
    for p, plane in enumerate(split3(X)):
        out[:, :, p, :] = bf16_bits(plane).reshape(n, kt, BK)
    return out.reshape(n, kt * 3 * BK).view(np.uint8).reshape(n, kt * PLANE_BYTES)


def edge_values():
    """fp32 values at the edges of split3: bf16 ties in plane 0 and plane 1 (both ways, and one fp32 ulp either
    side), remainders of either sign, both ends of the domain, zeros."""
    f = np.float32
    base = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,                    # ties of plane 0: down to 1, up to 1 + 2^-6
            1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
            1.0 + 3 * 2.0 ** -8 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -8 - 2.0 ** -23,
            1.0 + 2.0 ** -7 + 2.0 ** -16, 1.0 + 2.0 ** -7 + 3 * 2.0 ** -16,    # ties of plane 1
            1.0 + 2.0 ** -7 + 2.0 ** -16 + 2.0 ** -23, 1.0 + 2.0 ** -7 + 3 * 2.0 ** -16 - 2.0 ** -23,
            1.0 + 2.0 ** -7 - 2.0 ** -20, 1.0 + 2.0 ** -7 + 2.0 ** -9 - 2.0 ** -21,  # a1 < 0 < a0; a2 < 0 < a1
            2.0 - 2.0 ** -23, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24,                     # a0 rounds up to a power of 2
            255.0, 257.0, 511.0, 65537.0, 16777215.0, 1.0, 0.0]
    vals = []
    for s in (1.0, -1.0):
        for e in (0, -60, 59, 17, -31):
            vals += [s * b * 2.0 ** e for b in base if (e > -60 or b >= 1.0 or b == 0.0) and (e < 59 or b < 2.0)]
    vals += [2.0 ** 60, -2.0 ** 60, 2.0 ** -60, -2.0 ** -60, 2.0 ** 60 * (1 - 2.0 ** -24), 2.0 ** -60 * (1 + 2.0 ** -23)]
    v = np.array(vals, np.float64).astype(f)
    assert np.all((v == 0) | ((np.abs(v) >= f(2.0 ** -60)) & (np.abs(v) <= f(2.0 ** 60))))
    return v


def edge_matrix(n, k, seed):
    """[n, k] of edge_values in a seeded order, random full-mantissa values of the domain between them."""
    r = np.random.default_rng(seed)
    e = edge_values()
    m = np.ldexp(r.integers(1 << 23, 1 << 24, (n, k)).astype(np.float64), r.integers(-83, 36, (n, k)))
    m *= r.choice([-1.0, 1.0], (n, k))
    pick = r.random((n, k)) < 0.6
    m[pick] = e[r.integers(0, len(e), int(pick.sum()))]
    if n * k >= len(e):
        m.reshape(-1)[r.permutation(n * k)[:len(e)]] = e     # every edge value at least once
    return m.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the plans
def dense_plan(n, k_dim):
    nt = cdiv(n, TILE)
    tiles, kpad = nt * (nt + 1) // 2, cdiv(k_dim, BK) * BK
    split, tail = 1, 0
    if tiles < SLOTS:
        split, tail = max(1, min(4, SLOTS // max(tiles, 1))), tiles
    elif tiles % SLOTS:
        split, tail = 3, min(tiles, SLOTS + tiles % SLOTS)
    tail = min(tail, MAX_SPLIT_TILES)
    ktiles = kpad // BK
    split = max(1, min(split, ktiles))
    if split == 1:
        tail = 0
    n_whole, k_split, n_split = tiles - tail, cdiv(ktiles, split) * BK, split
    if tail > 0:
        n_split = cdiv(kpad, k_split)
    if n_split <= 1:
        n_split, n_whole = 1, tiles
    return dict(nt=nt, tiles=tiles, kpad=kpad, n_whole=n_whole, n_split=n_split, k_split=k_split,
                split_tiles=tiles - n_whole)


def sk_plan(n, k_dim):
    nt, kt = cdiv(n, TILE), cdiv(k_dim, BK)
    total = nt * (nt + 1) // 2 * kt
    units = max(1, cdiv(total, min(SLOTS, max(total, 1))))
    return dict(kt=kt, total=total, units=units, grid=cdiv(total, units))


def sk_plan_wide(n, k_dim, xcd=True):
    nt = cdiv(n, TILE)
    np_ = (nt + 1) // 2
    items, kt = np_ * (nt + 1) - np_ * np_, cdiv(k_dim, BK)
    total, dp_rounds, xcd_slots = items * kt, 0, 0
    if xcd and items >= 2 * CUS:
        grid, dp_rounds, xcd_slots = CUS, items // CUS, 1
        rest = items - dp_rounds * grid
        if 0 < rest < grid // 4:
            dp_rounds -= 1
        units = max(1, cdiv(total - dp_rounds * grid * kt, grid))
    else:
        units = max(1, cdiv(total, min(CUS, max(total, 1))))
        grid = cdiv(total, units)
    return dict(items=items, kt=kt, total=total, dp_rounds=dp_rounds, units=units, grid=grid, xcd_slots=xcd_slots)


def wide_items(nt, wide_env=-1):
    return wide_env == 1 or (wide_env != 0 and nt >= 64)


def sk_cut_items(total_base, kt, units, total):
    """Number of items of kt units, laid end to end from unit total_base on, that a slot boundary cuts."""
    cut = 0
    for tb in range(total_base, total, kt):
        cut += (tb - total_base) // units != (tb + kt - 1 - total_base) // units
    return cut


def path_of(entry, n, k_dim, wide_env=-1, workspace=True):
    """The kernel family an entry point takes: 'whole', 'slices', 'tail', 'streamk', 'wide' (host dispatch restated)."""
    p = dense_plan(n, k_dim)
    if entry in ("split", "planes") and workspace and wide_items(p["nt"], wide_env) and p["kpad"] > 0:
        return "wide"
    if entry in ("ws", "split") and workspace and p["tiles"] >= CUS and p["kpad"] > 0:
        return "streamk"
    if not workspace or p["n_split"] == 1:
        return "whole"
    return "slices" if p["n_whole"] == 0 and p["tiles"] < SLOTS else "tail"


# ------------------------------------------------------------------------------------------------ the inputs
def pad_lda(M, lda):
    n, k = M.shape
    assert lda % 16 == 0 and lda >= cdiv(k, BK) * BK
    A = np.zeros((n, lda), np.float32)
    A[:, :k] = M
    return A


def int_case(n, k, seed, lda=None):
    """(A [n, lda] fp32, K [n, n] int64 = A A^T).  Every entry a nonzero integer: |a| <= 15 for most, about 3 % odd
    with 256 < |a| <= 511 (nine significant bits: a0 is even, a1 = +-1, so the (0,1), (1,0) and (1,1) products are
    live).  Mixed signs."""
    r = np.random.default_rng([n, k, seed, 1])
    M = r.integers(1, 16, (n, k)) * r.choice([-1, 1], (n, k))
    big = r.random((n, k)) < 0.03
    big[r.integers(0, n), r.integers(0, k)] = True
    M[big] = (2 * r.integers(128, 256, int(big.sum())) + 1) * r.choice([-1, 1], int(big.sum()))
    d = M.astype(np.float64)                   # (the float64 product of integers below 2^24 is the int64 one)
    return pad_lda(M.astype(np.float32), lda or cdiv(k, BK) * BK), np.rint(d @ d.T).astype(np.int64)


class Probe:
    """A [n, lda]; is_w [n]; col [n] (the W rows' column); ref [n, n] float64 = A A^T exact; same [n, n] bool: the
    W x W' entries that share a column (the diagonal included)."""


def probe_case(n, k, seed, lda=None):
    """Even rows P: every column +-2^e, e in [-3, 3]: bf16 exactly, P x P sums exact on a 2^-6 grid below 2^13.
    Odd rows W: one nonzero at column r mod k, a full 24-bit mantissa with a1 != 0 and a2 != 0 times 2^s, s in
    [-20, 20].  Exact and held bitwise on every path: all P x P; W x P and P x W (one term w * +-2^e: the MFMA adds
    w0 p into c0 and w1 p, w2 p into c1, whose sum (w - w0) p is an fp32 value, then c0 + c1 = w p); W x W' with
    different columns (+0).  W x W' sharing a column: on the fp32 path one FMA from 0, fl(w w'), bitwise.  On the
    split paths within 2^-22 |w w'|: the dropped products w1 w2' + w2 w1' + w2 w2' are at most (2^-23 + 2^-32)
    |w w'|; c1 is a chain of five products of magnitude at most 2^-7 |w w'| in all, so its at most five roundings
    give 5 * 2^-24 * 2^-7 |w w'| < 2^-28 |w w'|; c0 = w0 w0' is exact (16 bits); the final c0 + c1 rounds once,
    2^-24 |w w'| (1 + 2^-6).  Sum: below (2^-23 + 2^-24 + 2^-27) |w w'| < 2^-22 |w w'|."""
    r = np.random.default_rng([n, k, seed, 2])
    M = np.zeros((n, k), np.float64)
    M[0::2] = np.ldexp(r.choice([-1.0, 1.0], (cdiv(n, 2), k)), r.integers(-3, 4, (cdiv(n, 2), k)))
    c = Probe()
    c.is_w = np.arange(n) % 2 == 1
    c.col = np.arange(n) % k
    for i in range(1, n, 2):
        while True:
            w = np.float32(np.ldexp(float(r.integers(1 << 23, 1 << 24)), int(r.integers(-43, -2))) * r.choice([-1.0, 1.0]))
            _, w1, w2 = split3(np.array([w]))
            if w1[0] != 0 and w2[0] != 0:
                break
        M[i, c.col[i]] = w
    c.A = pad_lda(M.astype(np.float32), lda or cdiv(k, BK) * BK)
    assert np.array_equal(c.A[:, :k].astype(np.float64), M)
    c.ref = M @ M.T + 0.0
    c.same = np.outer(c.is_w, c.is_w) & (c.col[:, None] == c.col[None, :])
    return c


def real_case(n, k, seed, lda=None):
    """(A, ref float64 A A^T, T, S): about 20 % nonzero over four decades, signs in alternate rows (the data of
    tests/test_gpu_parity.py test_gram_dense_split_vs_fp64_and_fp32)."""
    r = np.random.default_rng([n, k, seed, 3])
    v = (r.random((n, k)) * 10.0 ** r.uniform(-3, 1, (n, k))) * (r.random((n, k)) < 0.2)
    v[::2] *= np.sign(r.standard_normal((cdiv(n, 2), k)))
    A = pad_lda(v.astype(np.float32), lda or cdiv(k, BK) * BK)
    return (A,) + real_judges(A)


def real_judges(A):
    d = A.astype(np.float64)
    nz = (d != 0).astype(np.float64)
    return d @ d.T, nz @ nz.T, np.abs(d) @ np.abs(d).T


def real_bound(T, S, split):
    if split:
        return (T + 4) * 2.0 ** -23 * S + 2.0 ** -22 * S
    return (T + 4) * 2.0 ** -24 * S


# ------------------------------------------------------------------------------------------- conditions, emulation
def planes_abs_gram_max(A):
    """max of (|a0| + |a1| + |a2|) (|a0| + |a1| + |a2|)^T: bounds every partial sum of every plane product."""
    q = sum(np.abs(p).astype(np.float64) for p in split3(A))
    return float((q @ q.T).max())


def coverage_ok(A, k_dim, rows=None):
    """For every k-tile t and every 32 x 32 block of K on or above the diagonal, the partial Gram of k-tile t alone
    (over ``rows`` only, default all: the P rows of a probe case) has a nonzero entry in that block."""
    n = A.shape[0]
    d = A.astype(np.float64)
    if rows is not None:
        d = d * np.asarray(rows, np.float64)[:, None]
    nb = cdiv(n, 32)
    for t in range(cdiv(k_dim, BK)):
        Z = d[:, BK * t:BK * (t + 1)]
        hit = np.zeros((nb * 32, nb * 32), bool)
        hit[:n, :n] = (Z @ Z.T) != 0
        blocks = hit.reshape(nb, 32, nb, 32).any(axis=(1, 3))
        if not np.all(blocks[np.triu_indices(nb)]):
            return False
    return True


def emulate_fp32(A, k_dim):
    """K by a float32 chain in k order: one rounding per term (the product exact in float64)."""
    d = A[:, :k_dim].astype(np.float64)
    acc = np.zeros((A.shape[0], A.shape[0]), np.float32)
    for k in range(k_dim):
        acc = (acc.astype(np.float64) + np.outer(d[:, k], d[:, k])).astype(np.float32)
    return acc


def emulate_split(A, k_dim):
    """K by the six plane products on two accumulators, one float32 rounding per term: per k-tile c0 takes a0 b0,
    then c1 takes (0,1) (1,0) (0,2) (1,1) (2,0) in that order; c0 + c1 at the end."""
    P = [p[:, :k_dim].astype(np.float64) for p in split3(A)]
    n = A.shape[0]
    c0, c1 = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
    for t in range(cdiv(k_dim, BK)):
        ks = range(BK * t, min(BK * (t + 1), k_dim))
        for k in ks:
            c0 = (c0.astype(np.float64) + np.outer(P[0][:, k], P[0][:, k])).astype(np.float32)
        for p, q in ((0, 1), (1, 0), (0, 2), (1, 1), (2, 0)):
            for k in ks:
                c1 = (c1.astype(np.float64) + np.outer(P[p][:, k], P[q][:, k])).astype(np.float32)
    return c0 + c1


def frac(x):
    return Fraction(float(x))


# ---------------------------------------------------------------------------------- the cases of the GPU file
NS_WHOLE, KS_WHOLE = (1, 63, 64, 65, 127, 128, 129, 257), (1, 15, 16, 17, 33)
NS_SLICES, KS_SLICES = (129, 257, 400), (17, 33, 65, 80)
PIECES = {17: 2, 33: 3, 65: 3, 80: 3}           # k-slices per tile at NS_SLICES ("no empty piece": 80 = 3 x 32)
N_SK, KS_SK, K_SK_UNCUT = 2817, (33, 80), 20
NS_TAIL, K_TAIL = (3969, 5633), 33
NS_WIDE, KS_WIDE = (1, 129, 257, 385), (16, 17, 33, 80)
N_XCD, K_XCD = 5633, 33


def gpu_shapes(large=True):
    """Every (n, k) the GPU file runs int_case at (and probe_case where n <= 400 or (n, k) = (N_SK, 33))."""
    s = {(n, k) for n in NS_WHOLE for k in KS_WHOLE} | {(n, k) for n in NS_SLICES for k in KS_SLICES}
    s |= {(n, k) for n in NS_WIDE for k in KS_WIDE}
    if large:
        s |= {(N_SK, k) for k in KS_SK + (K_SK_UNCUT,)} | {(n, K_TAIL) for n in NS_TAIL} | {(N_XCD, K_XCD)}
    return sorted(s)


def lda_of(n, k):
    """The leading dimension a case uses: kpad for odd n, the engine's multiple of 64 for even n."""
    return cdiv(k, BK) * BK if n % 2 else cdiv(max(k, 1), 64) * 64
