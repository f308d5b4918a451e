"""Numpy restatements of the sparse Gram kernels (csrc/grf_gram.hip) and the builders of their edge cases.

No torch and no GPU here.  include/grf.h promises that every K entry is the fp32 rounding of an exact int64
fixed-point sum, whatever the order of the adds, so K is a pure function of (Phi, row shifts) and can be
restated to the bit:

  * per term   q = rint(Phi[i, k] * Phi[j, k] * 2^sh_i)   -- the product of two fp32 values scaled by a power of
    two is exact in fp64, and the kernel's fma with the magic number 1.5 * 2^52 rounds it once, ties to even;
  * per entry  the int64 sum of the q over k (two's complement, any order);
  * write-out  ``fx_to_float``: a = hi 2^32 + lo with lo the low word as a SIGNED int32, float32(hi), float32(lo),
    ONE fma hi * 2^32 + lo (the exact integer sum of the two rounded words, rounded once), then ldexp by -sh:
    at most 1.5 ulp from the exact sum, NOT its correct rounding.

The transposes are built on the host in the three bucket layouts of include/grf.h; every byte the layout
contract calls unused is 0xFF, so a kernel that reads one puts a NaN or garbage into K.  Nothing in this file
is measured on the device; tests/test_gram_reference.py pins it against Fractions on the CPU.
"""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

REC_LINE, REC_PACKED, REC_SLOT = 128, 12, 32
K_SUB = 8          # sub-bands of the split
CHUNK = 1024       # stream positions of one bucket-id chunk


# ------------------------------------------------------------------------------------------------- CSR helper
def csr(n_rows, n_cols, rows):
    """CSR (float32 values kept bit for bit, explicit zeros kept) from ``rows``: per row (columns, values)."""
    ptr = np.zeros(n_rows + 1, np.int64)
    idx, val = [], []
    for r, (c, v) in enumerate(rows):
        c = np.asarray(c, np.int32)
        v = np.asarray(v, np.float32)
        assert c.shape == v.shape and (len(c) == 0 or (np.all(np.diff(c) > 0) and c[0] >= 0 and c[-1] < n_cols))
        idx.append(c)
        val.append(v)
        ptr[r + 1] = ptr[r] + len(c)
    M = sp.csr_matrix((np.concatenate(val) if val else np.zeros(0, np.float32),
                       np.concatenate(idx) if idx else np.zeros(0, np.int32), ptr), shape=(n_rows, n_cols))
    assert M.data.dtype == np.float32
    return M


def row_lengths(P):
    return np.diff(P.indptr).astype(np.int64)


# --------------------------------------------------------------------------------------------- the shift rule
def _ilogb1(x):
    """ilogb(x) + 1 of an exact positive Fraction / float (0 for 0): x < 2^e."""
    x = Fraction(x)
    if x <= 0:
        return 0
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    return e + 1


def _is_pow2(v):
    m, _ = np.frexp(np.abs(v[v != 0]).astype(np.float64))
    return bool(np.all(m == 0.5))


def rowshift_ref(P):
    """(sh int32 [n_rows], decided bool [n_rows], mx): tr_rowshift_kernel's rule with the row sums exact.
    mx = max |Phi|, T = rowmax * mx, B = rowsum * mx * (1 + 1e-12), sh = min(51 - eT, 62 - eB) with
    e = ilogb + 1 (0 for 0).  The device sums |v| in fp64 in lane order, so a row is ``decided`` only when its
    exact B is not within 1e-9 (relative) of a power of two -- or when every value of Phi is a power of two,
    where each device step is exact."""
    P = P.tocsr()
    a = np.abs(P.data.astype(np.float64))
    mx = float(a.max()) if len(a) else 0.0
    pow2 = _is_pow2(P.data)
    n = P.shape[0]
    sh = np.zeros(n, np.int32)
    decided = np.ones(n, bool)
    one_eps = Fraction(1.0 + 1e-12)
    for r in range(n):
        v = a[P.indptr[r]:P.indptr[r + 1]]
        if len(v) == 0 or mx == 0.0:
            sh[r] = min(51, 62)
            continue
        s = sum(Fraction(float(x)) for x in v)
        T = Fraction(float(v.max())) * Fraction(mx)          # exact in fp64: two fp32 factors
        if pow2:
            B = Fraction(float(s) * mx * (1.0 + 1e-12))       # the device's own steps, each exact or one rounding
        else:
            B = s * Fraction(mx) * one_eps
        eT, eB = _ilogb1(T), _ilogb1(B)
        sh[r] = min(51 - eT, 62 - eB)
        if not pow2 and B > 0:
            lo = Fraction(2) ** (eB - 1)                      # lo <= B < 2 lo
            decided[r] = (B / lo - 1 > Fraction(1, 10 ** 9)) and (1 - B / (2 * lo) > Fraction(1, 10 ** 9))
    return sh, decided, np.float32(mx)


# ------------------------------------------------------------------------------------------------ fx_to_float
def _bit_length_u64(m):
    m = m.astype(np.uint64)
    n = np.zeros(m.shape, np.int64)
    for b in (32, 16, 8, 4, 2, 1):
        big = (m >> np.uint64(b)) != 0
        n = np.where(big, n + b, n)
        m = np.where(big, m >> np.uint64(b), m)
    return n + (m != 0)


def _round_u64_to_f32(mag):
    """float32 nearest (ties to even) to each uint64, as float64 values (exactly representable)."""
    mag = mag.astype(np.uint64)
    nb = _bit_length_u64(mag)
    s = np.maximum(nb - 24, 0).astype(np.uint64)
    q = mag >> s
    rem = mag - (q << s)
    half = np.where(s > 0, np.uint64(1) << (np.maximum(s, np.uint64(1)) - np.uint64(1)), np.uint64(0))
    up = (s > 0) & ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1)))
    q = q + up.astype(np.uint64)
    return np.ldexp(q.astype(np.float64), s.astype(np.int64))    # q <= 2^24: exact


def fx_to_float_ref(acc, sh):
    """The kernel's fx_to_float on an int64 array (|a| < 2^62, the shift rule's guarantee) with shift(s) sh ->
    float32: the low word as a SIGNED int32 lo and hi = (a >> 32) + (lo < 0), so a = hi 2^32 + lo exactly;
    float32(hi), float32(lo), ONE fma hi * 2^32 + lo (the exact integer sum of the two rounded words, rounded
    once), ldexp by -sh.  An exact zero sum is +0."""
    a = np.asarray(acc, np.int64)
    assert np.all(np.abs(a) < 2 ** 62)
    lo = (a & 0xffffffff).astype(np.uint32).view(np.int32)
    hi = ((a >> 32) + (lo < 0)).astype(np.int32)
    hi_f, lo_f = hi.astype(np.float32), lo.astype(np.float32)                      # rounded to nearest even
    s = hi_f.astype(np.float64).astype(np.int64) * (1 << 32) + lo_f.astype(np.float64).astype(np.int64)
    f = _round_u64_to_f32(np.abs(s).astype(np.uint64))
    f = np.where(s < 0, -f, f).astype(np.float32)
    return np.ldexp(f, -np.asarray(sh, np.int64)).astype(np.float32)


def round_terms(a, v, sh):
    """q = rint(a * v * 2^sh) as int64 (a, v fp32 values; ties to even as the magic-number fma)."""
    x = np.ldexp(np.asarray(a, np.float64) * np.asarray(v, np.float64), np.asarray(sh, np.int64))
    return np.rint(x).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the Gram
def gram_fx_ref(P, sh, rows=None, t_rows_block=None, k_slice=None):
    """K[rows, :] = Phi[rows] PhiB^T in the kernel's fixed point with the given shifts (sh indexed by Phi's
    row).  t_rows_block: PhiB (CSR with Phi's columns; default Phi itself).  k_slice = (k_begin, k_end).
    Returns (K float32 [len(rows) x t_rows], max |q|, max sum |q|, the int64 sums)."""
    P = P.tocsr()
    B = (P if t_rows_block is None else t_rows_block.tocsr())
    C = B.tocsc()                                                # (explicit zeros and the fp32 bits are kept)
    t_rows = B.shape[0]
    rows = np.arange(P.shape[0]) if rows is None else np.asarray(rows)
    k0, k1 = (0, P.shape[1]) if k_slice is None else k_slice
    K = np.zeros((len(rows), t_rows), np.float32)
    S = np.zeros((len(rows), t_rows), np.int64)
    mq = ms = 0
    clen = np.diff(C.indptr)
    for o, i in enumerate(rows):
        ks = P.indices[P.indptr[i]:P.indptr[i + 1]]
        av = P.data[P.indptr[i]:P.indptr[i + 1]]
        keep = (ks >= k0) & (ks < k1)
        ks, av = ks[keep], av[keep]
        if len(ks):
            ln = clen[ks]
            starts = C.indptr[ks]
            e = np.repeat(starts - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(int(ln.sum()))
            q = round_terms(np.repeat(av, ln), C.data[e], int(sh[i]))
            j = C.indices[e]
            np.add.at(S[o], j, q)
            ab = np.zeros(t_rows, np.int64)
            np.add.at(ab, j, np.abs(q))
            mq = max(mq, int(np.abs(q).max(initial=0)))
            ms = max(ms, int(ab.max(initial=0)))
        K[o] = fx_to_float_ref(S[o], int(sh[i]))
    return K, mq, ms, S


def sym_ref(P, sh):
    """Whole K of the symmetric entry points: the upper triangle from row i's shift, mirrored down."""
    K = gram_fx_ref(P, sh)[0]
    iu = np.triu_indices(K.shape[0], 1)
    K[iu[1], iu[0]] = K[iu]
    return K


def add_ref(K_fx, prior):
    """The add path's write-out: float32(K_fx) + prior in fp32 (one rounding)."""
    return (K_fx.astype(np.float32) + prior.astype(np.float32)).astype(np.float32)


def mirror_ref(K):
    K = K.copy()
    iu = np.triu_indices(K.shape[0], 1)
    K[iu[1], iu[0]] = K[iu]
    return K


# --------------------------------------------------------------------------------------------- the transposes
def _buckets(PB, W, split, seed):
    """Per non-empty bucket b = band * n_cols + k: (local rows, values) in storage order, and t_split.
    seed permutes the entries inside each bucket (inside each sub-band with a split); None keeps row order."""
    PB = PB.tocsr()
    t_rows, n_cols = PB.shape
    nb = -(-t_rows // W)
    C = PB.tocsc()
    C.sort_indices()
    rng = np.random.default_rng(seed) if seed is not None else None
    out = {}
    t_split = np.zeros((nb * n_cols, K_SUB), np.uint16) if split else None
    for k in np.flatnonzero(np.diff(C.indptr)):
        j = C.indices[C.indptr[k]:C.indptr[k + 1]].astype(np.int64)
        v = C.data[C.indptr[k]:C.indptr[k + 1]]
        band = j // W
        for J in np.unique(band):
            m = band == J
            jl, vl = j[m] - J * W, v[m]
            b = int(J) * n_cols + int(k)
            if split:
                sub = (jl * K_SUB) // W
                t_split[b] = np.searchsorted(sub, np.arange(K_SUB), side="left")
                if rng is not None:
                    order = np.lexsort((rng.random(len(jl)), sub))       # a random order inside each sub-band
                    jl, vl = jl[order], vl[order]
            elif rng is not None:
                order = rng.permutation(len(jl))
                jl, vl = jl[order], vl[order]
            out[b] = (jl, vl)
    return out, nb, t_split


def _pair_bytes(jl, vl):
    """The 12-byte record pairs of one bucket (an odd bucket ends with the pad record (0, +0.0))."""
    c = len(jl)
    p = (c + 1) // 2
    cols = np.zeros(2 * p, np.uint32)
    vals = np.zeros(2 * p, np.float32)
    cols[:c] = 8 * jl
    vals[:c] = vl
    assert cols.max(initial=0) < 65536
    rec = np.zeros((p, 3), np.uint32)
    rec[:, 0] = cols[0::2] | (cols[1::2] << 16)
    rec[:, 1] = vals[0::2].view(np.uint32)
    rec[:, 2] = vals[1::2].view(np.uint32)
    return rec.view(np.uint8).reshape(-1)


TAIL_BYTES = 128


def _transpose_units(PB, W, unit, split, seed):
    bk, nb, t_split = _buckets(PB, W, split, seed)
    n_cols = PB.shape[1]
    nbk = nb * n_cols
    pairs = np.zeros(nbk, np.int64)
    for b, (jl, _) in bk.items():
        pairs[b] = (len(jl) + 1) // 2
    units = -(-(12 * pairs) // unit)
    first = np.concatenate([[0], np.cumsum(units)])
    total = int(first[-1])
    desc = np.zeros(2 * (nbk + 1), np.uint32)
    desc[0:2 * nbk:2] = first[:-1]
    desc[1:2 * nbk:2] = pairs
    desc[2 * nbk] = total & 0xffffffff
    desc[2 * nbk + 1] = total >> 32
    rec = np.full(total * unit + TAIL_BYTES, 0xFF, np.uint8)
    for b, (jl, vl) in bk.items():
        pb = _pair_bytes(jl, vl)
        o = int(first[b]) * unit
        rec[o:o + len(pb)] = pb
    return desc, rec, t_split


def transpose_line_ref(PB, W, seed=None, split=False):
    """GRF_REC_LINE: (t_desc uint32 [2 (nbk + 1)], t_rec uint8, t_split uint16 [nbk x 8] or None).  A non-empty
    bucket starts on a 128-byte line; the line tail behind its pairs and TAIL_BYTES behind the total are 0xFF."""
    return _transpose_units(PB, W, REC_LINE, split, seed)


def transpose_packed_ref(PB, W, seed=None, split=False):
    """GRF_REC_PACKED: buckets pair after pair (unit = one pair); an empty bucket takes no unit."""
    return _transpose_units(PB, W, REC_PACKED, split, seed)


def transpose_slot_ref(PB, W, seed=None):
    """GRF_REC_SLOT: slot b = {u32 pairs, u32 first overflow pair, two inline pairs (zeroed payload)}, the other
    pairs packed from byte 32 nbk on.  t_desc holds {b, pairs} (the Gram tiles do not read it; the row cuts do)."""
    bk, nb, _ = _buckets(PB, W, False, seed)
    n_cols = PB.shape[1]
    nbk = nb * n_cols
    pairs = np.zeros(nbk, np.int64)
    for b, (jl, _) in bk.items():
        pairs[b] = (len(jl) + 1) // 2
    ovf = np.maximum(pairs - 2, 0)
    first = np.concatenate([[0], np.cumsum(ovf)])
    total_ovf = int(first[-1])
    rec = np.full(32 * nbk + 12 * total_ovf + TAIL_BYTES, 0xFF, np.uint8)
    slots = np.zeros((nbk, 8), np.uint32)
    slots[:, 0] = pairs
    slots[:, 1] = first[:-1]
    rec[:32 * nbk] = slots.view(np.uint8).reshape(-1)
    for b, (jl, vl) in bk.items():
        pb = _pair_bytes(jl, vl)
        inl = min(len(pb), 24)
        rec[32 * b + 8:32 * b + 8 + inl] = pb[:inl]
        if len(pb) > 24:
            o = 32 * nbk + 12 * int(first[b])
            rec[o:o + len(pb) - 24] = pb[24:]
    desc = np.zeros(2 * (nbk + 1), np.uint32)
    desc[0:2 * nbk:2] = np.arange(nbk)
    desc[1:2 * nbk:2] = pairs
    units = -(-(32 * nbk + 12 * total_ovf) // 32)
    desc[2 * nbk] = units
    return desc, rec, None


def split_ref(PB, W):
    """t_split alone: uint16 [nbk x 8], the entries of bucket b before each sub-band of W / 8 rows."""
    return _buckets(PB, W, True, None)[2]


def decode_transpose(desc, rec, unit, n_bands, n_cols, W):
    """(band, k) -> list of (local row, value bits) per bucket, pad records dropped; for all three layouts."""
    nbk = n_bands * n_cols
    out = {}
    for b in np.flatnonzero(desc[1:2 * nbk:2]):
        p = int(desc[2 * b + 1])
        if unit == REC_SLOT:
            hdr = rec[32 * b:32 * b + 8].view(np.uint32)
            assert hdr[0] == p
            raw = rec[32 * b + 8:32 * b + 8 + 12 * min(p, 2)]
            if p > 2:
                o = 32 * nbk + 12 * int(hdr[1])
                raw = np.concatenate([raw, rec[o:o + 12 * (p - 2)]])
        else:
            o = int(desc[2 * b]) * unit
            raw = rec[o:o + 12 * p]
        w = np.ascontiguousarray(raw).view(np.uint32).reshape(p, 3)
        cols = np.stack([w[:, 0] & 0xffff, w[:, 0] >> 16], 1).reshape(-1)
        vals = np.stack([w[:, 1], w[:, 2]], 1).reshape(-1)
        assert np.all(cols % 8 == 0)
        ent = list(zip((cols // 8).tolist(), vals.tolist()))
        out[int(b)] = ent
    return out


# ------------------------------------------------------------------------------------- tiles and the small kernels
def tiles_ref(rows, W, nb, sym):
    """The band-major tile sequence [(J, r)]: band J holds the local rows 0 .. count(J) - 1."""
    return [(J, r) for J in range(nb) for r in range(min((J + 1) * W, rows) if sym else rows)]


def part_tiles_ref(total, pb, pe, n_parts):
    return total * pb // n_parts, total * pe // n_parts


def written_cols_ref(tile, W, t_rows, sym, split):
    """The columns [c0, c1) of K row r that tile (J, r) writes: its band, from the row's sub-band on for a
    diagonal tile (r >= J W in symmetric mode) when a split is given."""
    J, r = tile
    j0 = J * W
    wlen = min(W, t_rows - j0)
    dsub = ((r - J * W) * K_SUB) // W if (split and sym and r >= J * W) else 0
    return j0 + dsub * (W // K_SUB), j0 + wlen


def col_pairs_ref(desc, n_bands, n_cols):
    pairs = desc[1:2 * n_bands * n_cols:2].astype(np.int64).reshape(n_bands, n_cols)
    return np.minimum(pairs.sum(0), 0x7fffffff).astype(np.int32)


def row_cuts_ref(P, col_w):
    """cuts[8 r + s] = the first offset in row r whose exclusive prefix of column weights times 8 is at least
    s * total (s = 0: 0; not found: the row length)."""
    P = P.tocsr()
    n = P.shape[0]
    cuts = np.zeros((n, 8), np.int32)
    for r in range(n):
        w = col_w[P.indices[P.indptr[r]:P.indptr[r + 1]]].astype(np.int64)
        excl = np.concatenate([[0], np.cumsum(w)[:-1]]) if len(w) else np.zeros(0, np.int64)
        tot = int(w.sum())
        for s in range(1, 8):
            hit = np.flatnonzero(excl * 8 >= s * tot)
            cuts[r, s] = hit[0] if len(hit) else len(w)
    return cuts.reshape(-1)


def hub_panel_ref(P, hub_pos, ldp, fill=0.0):
    P = P.tocsr()
    out = np.full((P.shape[0], ldp), fill, np.float32)
    for r in range(P.shape[0]):
        for e in range(P.indptr[r], P.indptr[r + 1]):
            q = hub_pos[P.indices[e]]
            if q >= 0:
                out[r, q] = P.data[e]
    return out


def drop_columns_ref(desc, n_bands, n_cols, cols):
    d = desc.copy()
    for J in range(n_bands):
        for k in cols:
            d[2 * (J * n_cols + int(k)) + 1] = 0
    return d


def densify_ref(P, lda):
    P = P.tocsr()
    out = np.zeros((P.shape[0], lda), np.float32)
    for r in range(P.shape[0]):
        s = slice(P.indptr[r], P.indptr[r + 1])
        out[r, P.indices[s]] = P.data[s]
    return out


def densify_padded_ref(cnt, idx, val, cap, lda):
    out = np.zeros((len(cnt), lda), np.float32)
    for r in range(len(cnt)):
        out[r, idx[r * cap:r * cap + cnt[r]]] = val[r * cap:r * cap + cnt[r]]
    return out


def to_padded(P, cap, rng=None):
    """Padded rows (cnt, idx, val) of a CSR; the slots behind a row's entries hold garbage (column -1, NaN)."""
    P = P.tocsr()
    n = P.shape[0]
    cnt = row_lengths(P).astype(np.int32)
    assert cnt.max(initial=0) <= cap
    idx = np.full(n * cap, -1, np.int32)
    val = np.full(n * cap, np.nan, np.float32)
    for r in range(n):
        idx[r * cap:r * cap + cnt[r]] = P.indices[P.indptr[r]:P.indptr[r + 1]]
        val[r * cap:r * cap + cnt[r]] = P.data[P.indptr[r]:P.indptr[r + 1]]
    return cnt, idx, val


# ------------------------------------------------------------------------------------------------ the streams
def wave_streams(P, row, J, desc, n_cols, waves, batch, balance, n_inline=None):
    """The pair streams the kernel builds for tile (J, row): per wave a list of batches, each the list of the
    pair counts of its nonzeros' buckets in band J (line / packed layouts; n_inline = 2 models the slot layout's
    two virtual buckets per nonzero).  balance: equal contiguous shares in batches of ``batch``; else
    round-robin batches."""
    P = P.tocsr()
    ks = P.indices[P.indptr[row]:P.indptr[row + 1]]
    cnt = desc[1::2][J * n_cols + ks].astype(np.int64)
    nnz = len(ks)
    out = []
    for w in range(waves):
        bl = []
        if balance:
            share = -(-nnz // waves)
            s0, s1 = min(w * share, nnz), min((w + 1) * share, nnz)
            for g in range(s0, s1, batch):
                bl.append(cnt[g:min(g + batch, s1)])
        else:
            for g in range(w * batch, nnz, batch * waves):
                bl.append(cnt[g:min(g + batch, nnz)])
        if n_inline is not None:
            bl = [np.stack([np.minimum(c, n_inline), c - np.minimum(c, n_inline)], 1).reshape(-1) for c in bl]
        out.append(bl)
    return out


def stream_edges(batches):
    """The edges one wave's batches reach: totals, chunk sizes, tail-group window counts, and the bucket
    positions (a bucket starting on a chunk's last / first position, an empty bucket between non-empty ones, a
    bucket that runs through a chunk with no marker of its own, a non-empty bucket at lane 63 / in the second half)."""
    e = {"totals": set(), "chunks": set(), "tails": set(), "pos": set()}
    for c in batches:
        total = int(c.sum())
        e["totals"].add(total)
        if total == 0:
            continue
        chunk = 256 if total <= 256 else 512 if total <= 512 else CHUNK
        e["chunks"].add(chunk)
        for c0 in range(0, total, chunk):
            cend = min(total, c0 + chunk)
            left = (cend - c0) % 512
            if left:
                e["tails"].add(-(-left // 64))
        starts = np.concatenate([[0], np.cumsum(c)[:-1]])
        ne = np.flatnonzero(c > 0)
        for i in ne:
            if chunk == CHUNK and starts[i] > 0 and starts[i] % CHUNK == CHUNK - 1:
                e["pos"].add("last_of_chunk")
            if chunk == CHUNK and starts[i] > 0 and starts[i] % CHUNK == 0:
                e["pos"].add("first_of_next_chunk")
            if i == 63:
                e["pos"].add("lane63")
            if i >= 64:
                e["pos"].add("second_half")
        if chunk == CHUNK:
            marked = set((starts[ne] // CHUNK).tolist())
            if any(cc not in marked for cc in range(1, -(-total // CHUNK))):
                e["pos"].add("crosses_markerless_chunk")      # the ids of that chunk come from the carry alone
        if len(ne) >= 2 and np.any(np.diff(ne) > 1):
            e["pos"].add("empty_between")
    return e


# --------------------------------------------------------------------------------------------- value generators
def _values(rng, size):
    """fp32 values: mixed signs, magnitudes 2^-12 .. 2^3 (a random 24-bit significand each)."""
    m = rng.uniform(1.0, 2.0, size) * np.exp2(rng.integers(-12, 3, size))
    return (m * rng.choice([-1.0, 1.0], size)).astype(np.float32)


class Case:
    """One Phi with its band width, the probe rows [row_begin, row_end) to compute, and the edges it claims."""

    def __init__(self, name, P, W, row_begin=0, row_end=None, edges=None, PB=None):
        self.name, self.P, self.W = name, P, W
        self.row_begin, self.row_end = row_begin, P.shape[0] if row_end is None else row_end
        self.edges = edges or {}
        self.PB = PB
        self._sh = None

    @property
    def n(self):
        return self.P.shape[0]

    @property
    def shifts(self):
        if self._sh is None:
            self._sh = rowshift_ref(self.P)
        return self._sh


STREAM_T = (1, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512, 513, 1023, 1024,
            1025, 1536, 2048, 2049)
NNZ_4WAVE = (0, 1, 3, 4, 5, 511, 512, 513, 1025)
NNZ_RR = (127, 128, 129, 512, 513)
NNZ_8WAVE = (63, 64, 65, 512, 513)


def probe_case(W, seed=0, waves=None):
    """Probe rows at band width W (4096: 4 waves, 8192: 8 waves), n = 2 W.  Band 1 holds the prescribed
    columns: column k has exactly c_k entries there; the probe rows sit at the start of band 0 and reference
    chosen columns, so the tile (band 1, probe row) gives every wave an exact stream.

      * single-bucket probes: ``waves`` nonzeros per row, one per wave, on columns of 2 T or 2 T - 1 entries
        for every T of STREAM_T that fits a band (2 T <= W);
      * two-bucket probes (``waves * 2`` nonzeros, a share of 2): pair counts (1023, 5) -- the second bucket
        starts on the last position of chunk 0 --, (1024, 5) -- on the first position of chunk 1 --, and
        (2048, 1) -- T = 2049, whose first bucket crosses a chunk with no marker;
      * row-length probes on light columns (0 .. 3 entries in band 1, so empty buckets lie between non-empty
        ones), one row per count of NNZ_4WAVE / NNZ_8WAVE."""
    rng = np.random.default_rng(seed)
    waves = waves or (8 if W > 4096 else 4)
    n = 2 * W
    col_cnt = np.zeros(n, np.int64)
    probes = []            # (edge name, columns)
    k = 0
    heavy = []
    for T in STREAM_T:
        for c in (2 * T, 2 * T - 1):
            if c <= W:
                heavy.append((T, c, k))
                col_cnt[k] = c
                k += 1
    while len(heavy) % waves:
        col_cnt[k] = 3
        heavy.append((2, 3, k))
        k += 1
    for g in range(0, len(heavy), waves):
        grp = heavy[g:g + waves]
        probes.append(("T=" + ",".join(f"{t}{'o' if c & 1 else 'e'}" for t, c, _ in grp), [kk for _, _, kk in grp]))
    # two-bucket shares: every wave gets (first, second)
    for first, second, tag in ((1023, 5, "last_of_chunk"), (1024, 5, "first_of_next_chunk"),
                               (2048, 1, "T=2049 crosses_markerless_chunk")):
        if 2 * first > W:
            continue
        cols = []
        for _ in range(waves):
            col_cnt[k], col_cnt[k + 1] = 2 * first, 2 * second - 1
            cols += [k, k + 1]
            k += 2
        probes.append((tag, cols))
    light0 = k
    col_cnt[light0:] = rng.integers(0, 4, n - light0)
    col_cnt[light0 + 1::7] = 0       # empty buckets between non-empty ones
    nnzs = NNZ_8WAVE if waves == 8 else NNZ_4WAVE
    for c in nnzs:
        cols = np.sort(rng.choice(np.arange(light0, n), c, replace=False)) if c else np.zeros(0, np.int64)
        probes.append((f"nnz={c}", cols.tolist()))
    n_probe = len(probes)
    assert n_probe <= W
    rows = [([], [])] * n
    rows = list(rows)
    for p, (_, cols) in enumerate(probes):
        rows[p] = (np.asarray(cols, np.int32), _values(rng, len(cols)))
    # band 1: column k in c_k distinct rows
    by_row = [[] for _ in range(W)]
    for kk in np.flatnonzero(col_cnt):
        for j in rng.choice(W, int(col_cnt[kk]), replace=False):
            by_row[j].append(kk)
    for j in range(W):
        c = np.asarray(sorted(by_row[j]), np.int32)
        rows[W + j] = (c, _values(rng, len(c)))
    P = csr(n, n, rows)
    edges = {"probes": [name for name, _ in probes], "waves": waves, "col_cnt": col_cnt}
    return Case(f"probe_W{W}", P, W, 0, n_probe, edges)


def random_case(name, n, W, density, seed, scale=0.0, empty_rows=(), zeros=True, n_cols=None):
    """A random Phi (mixed signs, magnitudes over 2^-12 .. 2^3, explicit +0.0 and -0.0 entries, empty rows),
    scaled by 2^scale."""
    rng = np.random.default_rng(seed)
    n_cols = n if n_cols is None else n_cols
    rows = []
    for r in range(n):
        if r in empty_rows:
            rows.append(([], []))
            continue
        c = np.flatnonzero(rng.random(n_cols) < density).astype(np.int32)
        v = _values(rng, len(c))
        if zeros and len(v) >= 2:
            v[0] = np.float32(0.0)
            v[-1] = np.float32(-0.0)
        rows.append((c, np.ldexp(v, int(scale)).astype(np.float32)))
    return Case(name, csr(n, n_cols, rows), W)


def hub_case(seed=3):
    """Row 0 holds 4100 equal entries (all ones): the sum bound 62 - eB binds and the shift is 49; T = 1 is a power
    of two.  The other rows are sparse +-1 / +-1/2 (powers of two: every row is decided).  n = 4160 at W = 4096."""
    rng = np.random.default_rng(seed)
    n = 4160
    rows = [(np.arange(4100, dtype=np.int32), np.ones(4100, np.float32))]
    for r in range(1, n):
        c = np.sort(rng.choice(n, 3, replace=False)).astype(np.int32)
        rows.append((c, (rng.choice([-1.0, 1.0], 3) * np.exp2(rng.integers(-1, 1, 3))).astype(np.float32)))
    return Case("hub4100", csr(n, n, rows), 4096, 0, 6, {"hub_row": 0})


def tie_case():
    """Crafted ties with explicit shift 10 on row 0 (a = 1): v = (m + 1/2) 2^-10 gives a * v * 2^sh half-integer
    with an even and an odd lower neighbour in both signs: 2.5 -> 2, 3.5 -> 4, -2.5 -> -2, -3.5 -> -4, 0.5 -> 0,
    -0.5 -> -0, 1.5 -> 2.  Row j > 0 holds v_j in column 0; row 0 holds 1 in column 0."""
    halves = np.array([2.5, 3.5, -2.5, -3.5, 0.5, -0.5, 1.5, -1.5, 1048576.5, -1048577.5], np.float64)
    n = len(halves) + 1
    rows = [([0], [1.0])] + [([0], [np.float32(h * 2.0 ** -10)]) for h in halves]
    c = Case("ties", csr(n, n, rows), 64, 0, 1, {"halves": halves})
    c.tie_shift = 10
    c.tie_expect = np.rint(halves).astype(np.int64)
    return c


def geometry_cases():
    """n in {1, 5, 63, 64, 65, 130} at W = 64 (ragged last band, wlen % 4 != 0, odd ldk = n), W = 192, the two
    power-of-two scalings, and ~41 bands for the symmetric tile location."""
    out = [random_case(f"n{n}_W64", n, 64, min(1.0, 6.0 / n + 0.05), 100 + n, empty_rows=(2,) if n > 5 else ())
           for n in (1, 5, 63, 64, 65, 130)]
    out.append(random_case("n400_W192", 400, 192, 0.04, 7, empty_rows=(0, 191, 399)))
    out.append(random_case("n130_up40", 130, 64, 0.1, 8, scale=40))
    out.append(random_case("n130_down40", 130, 64, 0.1, 9, scale=-40))
    return out


def bands41_case():
    return random_case("n2600_W64", 2600, 64, 0.004, 11, empty_rows=(5, 2599))


def dense128_case(seed=13):
    """n = 640 at W = 128 with band 0 dense: rows 0..127 hold all 640 columns, every other row 3 random ones.
    Each 16-row binning workgroup of band 0 holds 10240 entries (above the 8192 it can keep in LDS) and each of
    band 0's five 128-column regions has a 98304-byte line / packed image and 95232 bytes of slot overflow pairs
    (above the 48 KiB image cap), so the device transposes take their oversized-region paths there while bands
    1..4 stay on the LDS paths in the same launch."""
    rng = np.random.default_rng(seed)
    n = 640
    rows = [(np.arange(n, dtype=np.int32), _values(rng, n)) for _ in range(128)]
    for _ in range(128, n):
        rows.append((np.sort(rng.choice(n, 3, replace=False)).astype(np.int32), _values(rng, 3)))
    return Case("dense128_W128", csr(n, n, rows), 128)
