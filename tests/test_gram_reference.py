"""CPU pins of tests/gram_reference.py (no GPU): the restated fixed-point contract against scalar Fractions,
the guarantee of the shift rule, the derived distance to the exact Gram, the host-built transposes decoded back
to Phi, the tile enumeration, and the edges every case claims."""
from fractions import Fraction

import numpy as np
import pytest

import gram_reference as G


# -------------------------------------------------------------------------------------------- scalar restatements
def _rne_f32(x):
    """float32 nearest to the exact Fraction x, ties to even (normal range)."""
    if x == 0:
        return 0.0
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f & 1):
        f += 1
    return s * float(f) * 2.0 ** (e - 23)


def _fx_scalar(a, sh):
    a = int(a)
    lo = a & 0xffffffff
    lo = lo - (1 << 32) if lo >= 1 << 31 else lo              # the low word, signed
    hi = (a - lo) >> 32                                       # a = hi 2^32 + lo exactly
    hi_f, lo_f = _rne_f32(Fraction(hi)), _rne_f32(Fraction(lo))
    return np.float32(_rne_f32(Fraction(hi_f) * 2 ** 32 + Fraction(lo_f))) * np.float32(2.0) ** np.float32(-sh)


CRAFTED = [0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, -(2 ** 32), -(2 ** 32) - 1,
           (1 << 56) + (1 << 32) - 1, -((1 << 56) + (1 << 32) - 1), (3 << 32) + 0xffffff80, (1 << 61) + 0x80000001,
           2 ** 62 - 1, -(2 ** 62) + 1, (0x1000001 << 32) + 0xffffffff, -((0x1000001 << 32) + 0xffffffff),
           (0x1000003 << 32) | 0x80000000, 0x80000080, 0xffffff80, 0x7fffffff, 0x80000000, -0x80000000, -0x80000001,
           -2, -604900739, (0x1000001 << 32) + 0x80000000, -((0x1000001 << 32) + 0x7fffffc0)]


def test_fx_to_float_matches_fractions_and_is_no_plain_cast():
    rng = np.random.default_rng(0)
    a = np.array(CRAFTED + rng.integers(-2 ** 62 + 1, 2 ** 62, 1500, dtype=np.int64).tolist()
                 + (rng.integers(-2 ** 62, 2 ** 62, 1500, dtype=np.int64) >> rng.integers(0, 40, 1500)).tolist(),
                 np.int64)
    got = G.fx_to_float_ref(a, 0)
    ref = np.array([_fx_scalar(x, 0) for x in a], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    cast = np.array([_rne_f32(Fraction(int(x))) for x in a], np.float32)
    differs = int((got != cast).sum())
    print(f"fx_to_float: {len(a)} inputs, {differs} differ from the correctly rounded conversion")
    assert differs >= 1
    for sh in (-29, 7, 49, 110):
        g = G.fx_to_float_ref(a[:200], sh)
        r = np.array([_fx_scalar(x, 0) for x in a[:200]], np.float64) * 2.0 ** -sh
        assert np.array_equal(g.astype(np.float64), r)


def test_round_terms_ties_to_even_against_fractions():
    t = G.tie_case()
    v = t.P.data[1:]
    q = G.round_terms(np.float32(1.0), v, t.tie_shift)
    assert np.array_equal(q, t.tie_expect)
    for h, qq in zip(t.edges["halves"], q):
        x = Fraction(float(h))
        assert x.denominator == 2 and abs(Fraction(int(qq)) - x) == Fraction(1, 2) and qq % 2 == 0
    rng = np.random.default_rng(1)
    a, b = G._values(rng, 3000), G._values(rng, 3000)
    sh = rng.integers(20, 40, 3000)
    q = G.round_terms(a, b, sh)
    for i in range(0, 3000, 7):
        x = Fraction(float(a[i])) * Fraction(float(b[i])) * Fraction(2) ** int(sh[i])
        f = x.numerator // x.denominator
        r = x - f
        ref = f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f & 1) else 0)
        assert int(q[i]) == ref


# ---------------------------------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def cases():
    return G.geometry_cases() + [G.tie_case(), G.hub_case(), G.probe_case(4096), G.probe_case(8192)]


def _rows(c):
    return np.arange(c.row_begin, c.row_end)


def test_shift_rule_guarantee_and_distance_to_exact_gram(cases):
    """max |q| < 2^51 and max sum |q| < 2^62 (the rule's own guarantee), and K within
    c_ij 2^(-sh_i - 1) + 1.5 * 2^-23 |K_ij| of the exact Gram (half a unit per rounded term, 1.5 ulp of
    fx_to_float)."""
    for c in cases:
        sh = c.shifts[0]
        rows = _rows(c)[:40]
        K, mq, ms, _ = G.gram_fx_ref(c.P, sh, rows=rows)
        print(f"{c.name}: shifts {sh.min()}..{sh.max()} log2 max|q| {np.log2(max(mq, 1)):.3f} "
              f"log2 max sum|q| {np.log2(max(ms, 1)):.3f}")
        assert mq < 2 ** 51 and ms < 2 ** 62, c.name
        assert np.all(np.isfinite(K))
        A = c.P.astype(np.float64)
        S = c.P.copy().astype(np.float64)
        S.data[:] = 1.0
        exact = (A[rows] @ A.T).toarray()                    # fp64: error << the bound below for these sizes
        cnt = (S[rows] @ S.T).toarray()
        absum = (abs(A[rows]) @ abs(A).T).toarray()
        bound = cnt * np.exp2(-sh[rows].astype(np.float64) - 1)[:, None] + 1.5 * 2.0 ** -23 * np.abs(exact) \
            + (cnt + 2) * 2.0 ** -53 * absum                  # (the fp64 reference's own rounding: gamma_c)
        assert np.all(np.abs(K.astype(np.float64) - exact) <= bound), c.name


def test_hub_and_scaled_shifts(cases):
    by = {c.name: c for c in cases}
    sh, dec, _ = by["hub4100"].shifts
    assert sh[0] == 49 and dec.all()
    assert by["n130_up40"].shifts[0].max() < 0
    assert by["n130_down40"].shifts[0].min() > 100
    for name in ("n130_up40", "n130_down40"):
        K = G.gram_fx_ref(by[name].P, by[name].shifts[0])[0]
        nz = K[K != 0]
        assert np.all(np.abs(nz) >= np.finfo(np.float32).tiny) and np.all(np.isfinite(K))
    t = by["ties"]
    K = G.gram_fx_ref(t.P, np.full(t.n, t.tie_shift, np.int32), rows=[0])[0]
    assert np.array_equal(K[0, 1:].astype(np.float64) * 1024, t.tie_expect.astype(np.float64))
    mixed = by["n130_W64"].P.data
    assert (mixed < 0).any() and (mixed > 0).any()
    z = mixed[mixed == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    e = np.frexp(np.abs(mixed[mixed != 0]))[1]
    assert e.min() <= -10 and e.max() >= 3


def test_sensitivity_to_shifts_and_to_fp64_rounding(cases):
    c = [c for c in cases if c.name == "n400_W192"][0]
    sh = c.shifts[0]
    K = G.gram_fx_ref(c.P, sh)[0]
    K3 = G.gram_fx_ref(c.P, sh - 30)[0]
    A = c.P.astype(np.float64)
    Kc = (A @ A.T).toarray().astype(np.float32)
    print(f"differs from the rounded fp64 Gram: {(K != Kc).mean():.3f}; shifts - 30 change {(K3 != K).mean():.3f}")
    assert (K3 != K).any()


@pytest.mark.parametrize("layout", ["line", "packed", "slot"])
def test_transposes_decode_back_to_phi(cases, layout):
    build = {"line": G.transpose_line_ref, "packed": G.transpose_packed_ref, "slot": G.transpose_slot_ref}[layout]
    unit = {"line": G.REC_LINE, "packed": G.REC_PACKED, "slot": G.REC_SLOT}[layout]
    for c in cases[:8] + cases[-2:-1]:
        for split in ((False, True) if layout != "slot" else (False,)):
            for seed in (None, 5):
                kw = {"split": split} if layout != "slot" else {}
                desc, rec, t_split = build(c.P, c.W, seed=seed, **kw)
                nb = -(-c.n // c.W)
                got = G.decode_transpose(desc, rec, unit, nb, c.P.shape[1], c.W)
                C = c.P.tocsc()
                n_ent = 0
                for k in range(c.P.shape[1]):
                    j = C.indices[C.indptr[k]:C.indptr[k + 1]]
                    v = C.data[C.indptr[k]:C.indptr[k + 1]].view(np.uint32)
                    for J in np.unique(j // c.W):
                        m = j // c.W == J
                        want = sorted(zip((j[m] - J * c.W).tolist(), v[m].tolist()))
                        ent = got.pop(int(J) * c.P.shape[1] + k)
                        if len(want) & 1:
                            assert ent[-1] == (0, 0), "pad record"
                            ent = ent[:-1]
                        assert sorted(ent) == want
                        n_ent += len(want)
                        if split:
                            sub = np.array([e[0] for e in ent]) * G.K_SUB // c.W
                            assert np.all(np.diff(sub) >= 0)
                            b = int(J) * c.P.shape[1] + k
                            assert np.array_equal(t_split[b], np.searchsorted(np.sort(sub), np.arange(G.K_SUB)))
                assert not got and n_ent == c.P.nnz, (c.name, layout)
                if layout == "line":   # every bucket on a line, the tails 0xFF
                    assert np.all(rec[-G.TAIL_BYTES:] == 0xFF)


def test_split_has_odd_offsets(cases):
    c = [c for c in cases if c.name == "n130_W64"][0]
    s = G.split_ref(c.P, c.W)
    assert (s & 1).any() and (s == 0).all(axis=1).any()


def test_tiles_enumerate_every_tile_once():
    for rows, W, sym in ((130, 64, True), (130, 64, False), (64, 64, True), (1, 64, True), (2600, 64, True),
                         (400, 192, True)):
        nb = -(-rows // W)
        t = G.tiles_ref(rows, W, nb, sym)
        assert len(set(t)) == len(t)
        want = {(J, r) for J in range(nb) for r in range(rows) if (not sym or r // W <= J)}
        assert set(t) == want
        assert t == sorted(t)
        a = [G.part_tiles_ref(len(t), p, p + 1, 3) for p in range(3)]
        assert a[0][0] == 0 and a[-1][1] == len(t) and all(a[i][1] == a[i + 1][0] for i in range(2))
    assert G.written_cols_ref((1, 64 + 17), 64, 130, True, True) == (64 + 16, 128)
    assert G.written_cols_ref((1, 64 + 17), 64, 130, True, False) == (64, 128)
    assert G.written_cols_ref((2, 64 + 17), 64, 130, True, True) == (128, 130)
    assert G.written_cols_ref((0, 63), 64, 130, True, True) == (56, 64)


def test_row_cuts_ref_small():
    P = G.csr(3, 4, [([0, 1, 2, 3], [1, 1, 1, 1]), ([], []), ([1, 2], [1, 1])])
    cuts = G.row_cuts_ref(P, np.array([8, 0, 0, 8], np.int32)).reshape(3, 8)
    assert cuts[0].tolist() == [0, 1, 1, 1, 1, 4, 4, 4]     # exclusive prefixes 0 8 8 8 of 16
    assert cuts[1].tolist() == [0] * 8
    assert cuts[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]     # all-zero weights: every cut found at offset 0


# --------------------------------------------------------------------------------------- the edges a case claims
def _edges(c, layout_desc, waves, batch, balance, rows):
    nb = -(-c.n // c.W)
    agg = {"totals": set(), "chunks": set(), "tails": set(), "pos": set()}
    for r in rows:
        for J in range(nb):
            for bl in G.wave_streams(c.P, r, J, layout_desc, c.P.shape[1], waves, batch, balance):
                e = G.stream_edges(bl)
                for k in agg:
                    agg[k] |= e[k]
    return agg


def test_probe_cases_hold_their_edges(cases):
    by = {c.name: c for c in cases}
    c4, c8 = by["probe_W4096"], by["probe_W8192"]
    nnz4 = set(G.row_lengths(c4.P)[:c4.row_end].tolist())
    assert set(G.NNZ_4WAVE) <= nnz4
    nnz8 = set(G.row_lengths(c8.P)[:c8.row_end].tolist())
    assert set(G.NNZ_8WAVE) <= nnz8
    d4 = G.transpose_packed_ref(c4.P, 4096)[0]
    e4 = _edges(c4, d4, 4, 128, True, range(c4.row_end))
    print("probe_W4096 totals", sorted(e4["totals"]), "tails", sorted(e4["tails"]), "pos", sorted(e4["pos"]))
    assert set(G.STREAM_T) <= e4["totals"]
    assert e4["chunks"] == {256, 512, 1024} and e4["tails"] >= set(range(1, 8))
    assert e4["pos"] >= {"last_of_chunk", "first_of_next_chunk", "crosses_markerless_chunk", "empty_between", "lane63",
                         "second_half"}
    d8 = G.transpose_packed_ref(c8.P, 8192)[0]
    e8 = _edges(c8, d8, 8, 64, True, range(c8.row_end))
    print("probe_W8192 totals", sorted(e8["totals"]), "tails", sorted(e8["tails"]), "pos", sorted(e8["pos"]))
    assert set(G.STREAM_T) <= e8["totals"] and e8["chunks"] == {256, 512, 1024}
    assert e8["pos"] >= {"last_of_chunk", "first_of_next_chunk", "crosses_markerless_chunk", "empty_between", "lane63"}
    # full windows: a chunk of exactly 512 / 1024 positions has no tail group at all
    assert 512 in e4["totals"] and 1024 in e4["totals"]


def test_geometry_cases_hold_their_edges(cases):
    by = {c.name: c for c in cases}
    assert {by[f"n{n}_W64"].n for n in (1, 5, 63, 64, 65, 130)} == {1, 5, 63, 64, 65, 130}
    assert any((c.n % c.W) % 4 for c in cases) and any(c.n % 2 for c in cases)
    for name in ("n63_W64", "n130_W64", "n400_W192"):
        assert (G.row_lengths(by[name].P) == 0).any(), name
    b = G.bands41_case()
    assert -(-b.n // b.W) == 41


def test_dense128_case_exceeds_the_lds_caps():
    """dense128_W128 holds what it is there for: every 16-row binning workgroup of band 0 above the 8192 entries kept in
    LDS, every 128-column region of band 0 above the 48 KiB image cap in the line and packed layouts and in the slot
    layout's overflow pairs, bands 1..4 far below both, and every row's shift decided."""
    c = G.dense128_case()
    n, W, cr = c.n, c.W, 128
    per_wg = np.add.reduceat(G.row_lengths(c.P), np.arange(0, n, 16))
    assert np.all(per_wg[:W // 16] == 10240) and per_wg[W // 16:].max() <= 48
    nb = -(-n // W)
    for build, unit in ((G.transpose_line_ref, G.REC_LINE), (G.transpose_packed_ref, G.REC_PACKED)):
        first = build(c.P, W)[0][0::2].astype(np.int64)                  # first unit of every bucket, then the total
        img = (first[cr::cr][:nb * (n // cr)] - first[0:nb * n:cr]) * unit
        assert np.all(img[:n // cr] == 98304) and img[n // cr:].max() < 48 * 1024, (unit, img)
    pairs = G.transpose_slot_ref(c.P, W)[0][1:2 * nb * n:2].astype(np.int64)
    ovf = (np.maximum(pairs - 2, 0) * 12).reshape(nb * (n // cr), cr).sum(axis=1)
    assert np.all(ovf[:n // cr] == 95232) and ovf[n // cr:].max() == 0
    assert c.shifts[1].all()
