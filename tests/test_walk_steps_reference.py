"""CPU: pins tests/walk_steps_reference.py (the restatements test_gpu_walk_steps_kernels.py holds the HIP
kernels to) against the C oracle where the oracle can represent the case, and shows that the cases can
fail: the summation orders show in the bits, every fused-kernel plan is reached, every planted row occurs.
"""
import numpy as np
import pytest

import walk_steps_reference as R
from oracle import oracle as O


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _oracle_case(kind, n=12, L=5, m=9, seed=3):
    """Slots the oracle can hold: node ids < n = n_src."""
    rng = np.random.default_rng(seed)
    node = rng.integers(0, n, size=(n, L, m)).astype(np.int32)
    node[rng.random(size=node.shape) < 0.3] = -1
    node[1] = -1
    node[2] = 4
    load = R.loads(rng, node.shape, kind, m)
    node[3, 0, :] = -1
    node[3, 0, 0] = node[3, 0, 1] = 7      # an (a, -a) run: a kept explicit zero
    load[3, 0, 0], load[3, 0, 1] = 1.75, -1.75
    return node, load


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("norm", [R.NORM_DIV, R.NORM_MUL_RECIP])
def test_steps_and_phi_equal_the_oracle(kind, norm):
    node, load = _oracle_case(kind)
    n, L, m = node.shape
    rows = R.steps_ref(node, load, norm)
    mats = O.reduce_steps(node, load, norm)
    zero_kept = False
    for l in range(L):
        M = mats[l]
        for s in range(n):
            a, b = M.indptr[s], M.indptr[s + 1]
            assert np.array_equal(M.indices[a:b], rows[s][l][0]), (s, l)
            assert np.array_equal(_bits(M.data[a:b]), _bits(rows[s][l][1])), (s, l)
            zero_kept |= bool(np.any(rows[s][l][1] == 0.0))
    assert zero_kept
    for name, f, n_f in R.modulators(L, kind):
        cnt, idx, v64, v32 = R.phi_ref(rows, f, n_f, cap=n)
        ref = O.phi_sparse(mats, [] if f is None else list(f))
        assert np.array_equal(np.diff(ref.indptr), cnt), name
        assert np.array_equal(ref.indices, np.concatenate(idx)), name
        assert np.array_equal(_bits(ref.data), _bits(np.concatenate(v64))), name
        assert all(np.array_equal(a.view(np.uint32), b.astype(np.float32).view(np.uint32)) for a, b in zip(v32, v64))
        # the cap cuts the row and clamps the count
        c2, i2, w2, _ = R.phi_ref(rows, f, n_f, cap=2)
        assert np.array_equal(c2, np.minimum(cnt, 2))
        assert all(np.array_equal(i2[s], idx[s][:2]) and np.array_equal(_bits(w2[s]), _bits(v64[s][:2]))
                   for s in range(n))


@pytest.mark.parametrize("rng", [O.RNG_PCG64, O.RNG_PHILOX])
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_det_walk_equals_the_oracle(rng, rule):
    for name, ptr, idx, val in R.det_graphs():
        for L in (1, 2, 3, 4, 7):
            for m in (1, 3):
                node, load = R.det_walk_ref(ptr, idx, val, m, 0.0, L, rule)
                # (the oracle reads no entry of an empty graph; it still wants non-empty arrays)
                ix = idx if idx.size else np.zeros(1, np.int32)
                vl = val if val.size else np.zeros(1, np.float64)
                on, ol = O.walk_slots(ptr, ix, vl, m, 0.0, L, rng=rng, load_rule=rule, seed=5)
                assert np.array_equal(on, node), (name, L, m)
                live = node >= 0
                assert np.array_equal(_bits(ol[live]), _bits(load[live])), (name, L, m)
                if name == "huge5" and rule == 0 and L >= 3:
                    assert np.isinf(load[live]).any()
                if name.startswith(("empty", "path")):
                    assert (node[-1, 1:] == -1).all()      # a zero-degree source records one visit


def test_int_cases_stay_integers():
    """The "int" loads: every load a multiple of m, so every walk-order sum, every NORM_DIV step value and
    every Phi partial sum with the integer modulators is an integer below 2^53 -- any order gives the same
    bits.  (Under NORM_MUL_RECIP the step values are acc * RN(1 / m): one rounding each, not integers.)"""
    for (m, L), _ in R.FUSED_SHAPES:
        node, load, _ = R.fused_case(m, L, "int")
        assert np.all(load == np.rint(load)) and np.all(np.rint(load / m) * m == load)
        assert np.abs(load).sum() < 2.0 ** 53
        rows = R.steps_ref(node, load, R.NORM_DIV)
        for name, f, n_f in R.modulators(L, "int"):
            if f is None:
                continue
            assert np.all(f == np.rint(f))
            mag = sum(float(np.abs(per[l][1]).sum()) * abs(float(f[l])) for per in rows for l in range(min(n_f, L)))
            assert mag < 2.0 ** 53
        assert all(np.all(v == np.rint(v)) for per in rows for _, v in per)


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_orders_show_in_the_bits():
    """Reversed walk order, reversed step order and a -0.0 start each change bits of the "real" cases, so a
    kernel that sums in another order, or from another zero, fails the bitwise comparison."""
    walk_shapes = step_shapes = 0
    for (m, L), _ in R.FUSED_SHAPES:
        node, load, _ = R.fused_case(m, L, "real")
        rows = R.steps_ref(node, load, R.NORM_DIV)
        flat = [v for per in rows for _, v in per]
        if m >= 3:
            rev = R.steps_ref(node, load, R.NORM_DIV, reverse=True)
            assert _differs(flat, [v for per in rev for _, v in per]), (m, L)
            walk_shapes += 1
        # a walk-order sum that starts from -0.0 keeps the sign of a run of -0.0 loads: the step row's
        # explicit zero changes sign
        neg = R.steps_ref(node, load, R.NORM_DIV, start=-0.0)
        assert _differs(flat, [v for per in neg for _, v in per]), (m, L)
        if L >= 3:
            f = R.modulators(L, "real")[0][1]
            a = R.phi_ref(rows, f, L, cap=m * L)
            b = R.phi_ref(rows, f, L, cap=m * L, reverse=True)
            assert np.array_equal(a[0], b[0]) and _differs(a[2], b[2]), (m, L)
            step_shapes += 1
            # The step-order sum of a Phi entry cannot show its starting zero: -0.0 + t and 0.0 + t are the
            # same bits for every t != 0, they differ only for t = -0.0, and a sum that is +-0 is dropped
            # from Phi either way.  (The start shows in the step rows, above.)
            c = R.phi_ref(rows, f, L, cap=m * L, start=-0.0)
            assert np.array_equal(a[0], c[0]) and not _differs(a[2], c[2])
    assert walk_shapes >= 12 and step_shapes >= 9


def test_fused_shapes_cover_every_plan():
    got = []
    for (m, L), pair in R.FUSED_SHAPES:
        assert m * L <= 4096
        P, T, kper = R.fused_plan(m, L)
        assert (kper, T) == pair and P == kper * T and P >= m * L
        got.append(pair)
    assert sorted(got) == sorted(R.FUSED_PAIRS) and len(set(got)) == 13
    full = [(m, L) for (m, L), _ in R.FUSED_SHAPES if m * L == R.fused_plan(m, L)[0]]
    half = [(m, L) for (m, L), _ in R.FUSED_SHAPES if m * L == R.fused_plan(m, L)[0] // 2 + 1]
    assert len(full) >= 3 and len(half) >= 2


@pytest.mark.parametrize("shape", [s for s, _ in R.FUSED_SHAPES])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_planted_rows_occur(shape, kind):
    m, L = shape
    P, T, kper = R.fused_plan(m, L)
    node, load, planted = R.fused_case(m, L, kind)
    assert node.shape == (6, L, m) and node.dtype == np.int32
    assert (node[0] == -1).all()
    assert (node[1] == R.TOP - 1).all()
    assert len(set(node[2].ravel().tolist())) == m * L and {0, 1, R.TOP - 1, R.TOP} <= set(node[2].ravel().tolist())
    for s, fill in ((3, False), (4, True)):
        keys = R.sorted_keys(node[s], m, L)
        starts = {}
        i = 0
        while i < len(keys):
            j = i
            while j + 1 < len(keys) and keys[j + 1][:2] == keys[i][:2]:
                j += 1
            starts.setdefault(j - i + 1, set()).add(i % kper)
            last = (i, j)
            i = j + 1
        for length in (kper - 1, kper, kper + 1, 2 * kper + 3):
            if 1 <= length <= m:
                assert {0, kper - 1} <= starts.get(length, set()), (s, length, starts)
        assert last[1] == len(keys) - 1 and last[1] > last[0]       # a run ends at the last real key
        assert keys[-1][0] == R.TOP
        assert R.crosses_block(keys, kper)
        if fill:
            assert len(keys) == m * L                                # no empty slot: m L = P rows are full
        else:
            assert len(keys) < m * L
    assert R.crosses_block(R.sorted_keys(node[1], m, L), kper) or m <= kper
    # a kept explicit zero, a dropped zero, the (1, -1, 0, ...) cancellation and a truncated row
    rows = R.steps_ref(node, load, R.NORM_DIV)
    if "cancel_node" in planted:
        i0, v0 = rows[5][0]
        at = int(np.flatnonzero(i0 == planted["cancel_node"])[0])
        assert v0[at] == 0.0
        full = R.phi_ref(rows, R.modulators(L, kind)[0][1], L, cap=m * L)
        assert planted["cancel_node"] not in full[1][5].tolist()
    if "negzero_node" in planted:
        i0, v0 = rows[5][0]
        z = v0[int(np.flatnonzero(i0 == planted["negzero_node"])[0])]
        assert z == 0.0 and not np.signbit(z)
    if "pm_node" in planted:
        pm = R.phi_ref(rows, R.modulators(L, kind)[2][1], L, cap=m * L)
        assert planted["pm_node"] not in pm[1][5].tolist()
        full = R.phi_ref(rows, R.modulators(L, kind)[0][1], L, cap=m * L)
        assert planted["pm_node"] in full[1][5].tolist() or kind == "int"
    full = R.phi_ref(rows, R.modulators(L, kind)[0][1], L, cap=m * L)
    cut = R.phi_ref(rows, R.modulators(L, kind)[0][1], L, cap=max(1, int(full[0].max()) - 1))
    assert (cut[0] < full[0]).any() and cut[0].max() == max(1, int(full[0].max()) - 1)


def test_divisor_case_sweeps_every_exponent():
    for m in (1, 3, 7, 100):
        node, load, L = R.divisor_case(m)
        assert m * L <= 4096 and L <= 64 and node.shape == load.shape == (node.shape[0], L, m)
        assert all(len(set(node[s].ravel().tolist())) == m * L for s in range(node.shape[0]))   # single-walk runs
        ex = (load.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)
        assert set(ex.ravel().tolist()) == set(range(2048))
        assert np.isinf(load).sum() == 2 and (load == 0).sum() == 4 and np.signbit(load).any()
        sub = (ex == 0) & (load != 0)
        assert sub.sum() >= 8


def test_slots_case_rows():
    for m in (1, 2, 63, 257):
        node, load = R.slots_case(m, 3, 5, "real")
        assert (node[1] == -1).all() and (node[2] == R.TOP).all()
        assert all(len(set(node[3, l].tolist())) == m for l in range(3))
        assert (node[4] >= 0).all() and node.max() == R.TOP
        if m >= 2:
            i0, v0 = R.steps_ref(node, load, R.NORM_DIV)[0][0]
            assert v0[int(np.flatnonzero(i0 == 3)[0])] == 0.0


def test_aug_header_restatement():
    assert R.aug_header(1, 0) == (1, 1, 1) and R.aug_header(2, 0) == (1, 1, 1)
    assert R.aug_header(5, 5) == (1, 3, 3) and R.aug_header(5, 5, allow16=False) == (0, 3, 3)
    assert R.aug_header(2 ** 31 - 1, 2 ** 32 - 1) == (0, 31, 32)
