"""GPU: the dense Gram kernels (csrc/grf_gram_dense.hip) called directly through the C ABI and held to
tests/dense_gram_reference.py (pinned on the CPU by tests/test_dense_gram_reference.py).

Every value assertion is bitwise, or against a bound that the reference file derives and that the CPU test shows
a plain emulation meets; nothing measured is asserted.
  * ``int_case``: integer A with max(|A| |A|^T) < 2^24, so K is the int64 A A^T bit for bit on every path: fp32 MFMA
    and bf16 split, whole tiles, per-tile k-slices with slabs, the tail split, stream-K, wide items with and
    without the XCD rounds, fp32 staged or planes written once, full and upper_only write-out.
  * ``probe_case``: entries that need plane 2, exact where one term or exactly summable terms make them so, within
    2^-22 |w w'| where the split drops products.
  * ``real_case``: against float64 within ``real_bound``; the worst err / bound per path is printed.
The coverage condition of the inputs (CPU test) makes a skipped tile, 32 x 32 block, k-tile or slab change an
asserted entry.  Each case first asserts, with the host restatement of the plans, that it runs the path its name
claims.  The test owns every buffer: A zero-padded to lda (kpad for odd n, a multiple of 64 for even n), K
NaN-filled with a PAD tail, the workspace zero-filled and sized by the library.  After every call the tickets are
zero, K's padding columns and tail are still NaN, K is bitwise symmetric, and a second call gives the same bits.

Found by this file (fixed in the same change): with k_dim = 0 and 256 tiles or more (n >= 2817) grf_gram_dense_ws
and grf_gram_dense_split took the stream-K branch with an empty grid and returned a launch error instead of the
zero K they return below 256 tiles (``test_k_zero_from_256_tiles_on``).
Measured on an MI355X (information, not asserted; profiles/dense_gram_kernels_gpu_tests.log): 90 cases in under 5 s,
the slowest 0.25 s; worst err / bound of real_case 0.34-0.43 on the fp32 paths and 0.14-0.21 on the split paths.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import dense_gram_reference as D

pytestmark = pytest.mark.gpu

PAD = 11
NULL = ctypes.c_void_p(0)
FP32 = ("dense", "upper", "ws")                     # entry points on the fp32 MFMA
UPPER = ("upper", "split_upper")
NEEDS_WS = ("ws", "split", "planes")


@pytest.fixture(scope="module")
def eng():
    from grf_amd.engine import GRFEngine
    return GRFEngine("cuda:0")


def _t(a, eng):
    return torch.as_tensor(np.ascontiguousarray(a)).to(eng.device)


def _vp(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off)


def _i32(t):
    return t.view(torch.int32)


def _env(monkeypatch, wide=None, xcd=None):
    for name, v in (("GRF_DENSE_WIDE", wide), ("GRF_DENSE_XCD", xcd)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _workspace(eng, n, k):
    nbytes = max(int(eng.lib.grf_gram_dense_split_workspace_bytes(n, k)), int(eng.lib.grf_gram_dense_workspace_bytes(n, k)),
                 D.TICKET_BYTES)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=eng.device)
    assert ws.data_ptr() % 256 == 0
    return ws


def _planes(eng, A, n, k, lda, pad=0):
    """The planes of A written by grf_split_planes into a 0xA5-filled [n, ldp] buffer."""
    ldp = int(eng.lib.grf_planes_row_bytes(k)) + pad
    P = torch.full((max(n, 1) * max(ldp, 16) + PAD,), 0xA5, dtype=torch.uint8, device=eng.device)
    rc = eng.lib.grf_split_planes(n, k, _vp(A), lda, _vp(P), ldp, eng.stream)
    assert rc == 0, eng.lib.grf_last_error()
    return P, ldp


class Op:
    """One operand on the device: A [n, lda] (and its planes, made on first use)."""

    def __init__(self, eng, A, n, k):
        self.eng, self.n, self.k, self.lda = eng, n, k, A.shape[1]
        self.A = _t(A, eng)
        self._P = None

    def planes(self):
        if self._P is None:
            self._P = _planes(self.eng, self.A, self.n, self.k, self.lda)
        return self._P

    def ref64(self):
        """float64 A A^T on the device (exact for int_case and for probe_case's exact entries), -0 folded to +0."""
        d = self.A[:, :max(self.k, 1)].double() if self.k else torch.zeros((self.n, 1), dtype=torch.float64,
                                                                            device=self.A.device)
        return d @ d.T + 0.0


def _call(eng, entry, op, buf, ldk, off=0, ws=None, ws_bytes=None, planes=None):
    n, k, Kp = op.n, op.k, _vp(buf, 4 * off)
    wp = _vp(ws) if ws is not None else NULL
    wb = (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes
    lib, st = eng.lib, eng.stream
    if entry == "dense":
        return lib.grf_gram_dense(n, k, _vp(op.A), op.lda, Kp, ldk, st)
    if entry == "upper":
        return lib.grf_gram_dense_upper(n, k, _vp(op.A), op.lda, Kp, ldk, st)
    if entry == "split_upper":
        return lib.grf_gram_dense_split_upper(n, k, _vp(op.A), op.lda, Kp, ldk, st)
    if entry == "ws":
        return lib.grf_gram_dense_ws(n, k, _vp(op.A), op.lda, Kp, ldk, wp, wb, st)
    if entry == "split":
        return lib.grf_gram_dense_split(n, k, _vp(op.A), op.lda, Kp, ldk, wp, wb, st)
    assert entry == "planes"
    P, ldp = op.planes() if planes is None else planes
    return lib.grf_gram_dense_planes(n, k, _vp(P), ldp, Kp, ldk, wp, wb, st)


def _gram(eng, entry, op, ws=None, ldk=None, off=0, planes=None):
    """Two calls into two NaN-filled K buffers; the checks every call must pass; the [n, n] body (a device view)."""
    n = op.n
    ldk = -(-n // 4) * 4 + 4 if ldk is None else ldk
    bodies = []
    for _ in range(2):
        buf = torch.full((off + n * ldk + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        rc = _call(eng, entry, op, buf, ldk, off, ws, planes=planes)
        assert rc == 0, (entry, n, op.k, rc, eng.lib.grf_last_error())
        if ws is not None:
            assert not bool(ws[:D.TICKET_BYTES].any()), (entry, n, op.k, "tickets not back at zero")
        full = buf[off:off + n * ldk].view(n, ldk)
        assert bool(torch.isnan(full[:, n:]).all()) and bool(torch.isnan(buf[off + n * ldk:]).all()) \
            and bool(torch.isnan(buf[:off]).all()), (entry, n, op.k, "padding overwritten")
        bodies.append(full[:, :n])
    a, b = _i32(bodies[0]), _i32(bodies[1])
    assert torch.equal(a, b), (entry, n, op.k, "second call differs")
    if entry not in UPPER:
        assert torch.equal(a, a.T), (entry, n, op.k, "not bitwise symmetric")
    return bodies[0]


def _upper_views(K, ref):
    """upper_only: (K, ref) restricted to col >= row; the 128-tiles strictly below the diagonal must still be NaN."""
    n = K.shape[0]
    t = torch.arange(n, device=K.device) // D.TILE
    below = t[:, None] > t[None, :]
    assert bool(torch.isnan(K[below]).all()), "upper_only wrote a tile below the diagonal"
    r = torch.arange(n, device=K.device)
    iu = r[:, None] <= r[None, :]
    return K[iu], ref[iu]


def _mismatch(K, ref):
    bad = torch.nonzero(_i32(K.contiguous()) != _i32(ref.contiguous()))
    return int(bad.shape[0]), [(ix.tolist(), float(K[tuple(ix)]), float(ref[tuple(ix)])) for ix in bad[:5]]


_OPS = {}


def _op(eng, kind, n, k):
    """(Op, judge) of a case, made once for n <= 400."""
    key = (kind, n, k)
    if key in _OPS:
        return _OPS[key]
    lda = D.lda_of(n, k)
    if kind == "int":
        A, Kint = D.int_case(n, k, 0, lda)
        op = Op(eng, A, n, k)
        ref = op.ref64().float()
        if n <= 400:
            assert np.array_equal(ref.cpu().numpy().astype(np.int64), Kint)        # the int64 A A^T itself
        else:
            rows = np.random.default_rng(n).integers(0, n, 64)
            assert np.array_equal(ref[_t(rows, eng)].cpu().numpy().astype(np.int64), Kint[rows])
        out = (op, ref)
    elif kind == "probe":
        c = D.probe_case(n, k, 0, lda)
        op = Op(eng, c.A, n, k)
        ref64 = op.ref64()
        if n <= 400:
            assert np.array_equal(ref64.cpu().numpy(), c.ref)
        out = (op, (ref64, _t(c.same, eng)))
    else:
        A = D.real_case(n, k, 0, lda)[0]
        out = (Op(eng, A, n, k), None)
    if n <= 400:
        _OPS[key] = out
    return out


def _hold_int(eng, entry, n, k, ws, what, **kw):
    op, ref = _op(eng, "int", n, k)
    K = _gram(eng, entry, op, ws, **kw)
    if entry in UPPER:
        K, ref = _upper_views(K, ref)
    assert torch.equal(_i32(K), _i32(ref)), (what, "int", entry, n, k) + _mismatch(K, ref)


def _hold_probe(eng, entry, n, k, ws, what, **kw):
    op, (ref64, same) = _op(eng, "probe", n, k)
    K = _gram(eng, entry, op, ws, **kw)
    ref = ref64.float()                              # fl(w w') where one product is the whole entry
    if entry in FP32:                                # one FMA from 0: every entry bitwise
        if entry in UPPER:
            K, ref = _upper_views(K, ref)
        assert torch.equal(_i32(K), _i32(ref)), (what, "probe", entry, n, k) + _mismatch(K, ref)
        return
    if entry in UPPER:
        r = torch.arange(n, device=K.device)
        iu = r[:, None] <= r[None, :]
        _upper_views(K, ref)
        exact, loose = ~same & iu, same & iu
    else:
        exact, loose = ~same, same
    Ke, re_ = K[exact], ref[exact]
    assert torch.equal(_i32(Ke), _i32(re_)), (what, "probe", entry, n, k, int((_i32(Ke) != _i32(re_)).sum()))
    err = (K[loose].double() - ref64[loose]).abs()
    assert bool((err <= 2.0 ** -22 * ref64[loose].abs()).all()), (what, "probe W x W'", entry, n, k, float(err.max()))


def _hold_real(eng, entry, n, k, ws, what):
    op, _ = _op(eng, "real", n, k)
    K = _gram(eng, entry, op, ws)
    d = op.A.double()
    ref, T, S = d @ d.T, (d != 0).double() @ (d != 0).double().T, d.abs() @ d.abs().T
    bound = (T + 4) * 2.0 ** -24 * S if entry in FP32 else (T + 4) * 2.0 ** -23 * S + 2.0 ** -22 * S
    if n <= 400:                                     # the device judges are the reference file's
        r0, T0, S0 = D.real_judges(op.A.cpu().numpy())
        assert np.array_equal(T.cpu().numpy(), T0) and np.allclose(S.cpu().numpy(), S0, rtol=1e-13, atol=0)
        assert np.allclose(bound.cpu().numpy(), D.real_bound(T0, S0, entry not in FP32), rtol=1e-12, atol=0)
    err = (K.double() - ref).abs()
    if entry in UPPER:
        err, bound = _upper_views(err, bound)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"REAL {what:<28} {entry:<11} n = {n:5d} k = {k:3d}: worst err / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (what, "real", entry, n, k, ratio)


# -------------------------------------------------------------------------------------------------- whole tiles
@pytest.mark.parametrize("n", D.NS_WHOLE)
@pytest.mark.parametrize("entry", ["dense", "upper", "split_upper", "split"])
def test_whole_tiles_bitwise(eng, monkeypatch, entry, n):
    """Whole tiles, no workspace (grf_gram_dense_split: one k-tile, so its plan has nothing to cut).  upper_only
    also with ldk = n + 1 and K one float past an aligned address (ldk % 4 != 0, allowed for upper_only only)."""
    _env(monkeypatch, wide=0)
    ks = (16,) if entry == "split" else D.KS_WHOLE
    t0 = time.perf_counter()
    for k in ks:
        ws = _workspace(eng, n, k) if entry == "split" else None
        assert D.path_of(entry, n, k, 0, workspace=ws is not None) == "whole"
        for kw in ({},) + (({"ldk": n + 1, "off": 1},) if entry in UPPER else ()):
            _hold_int(eng, entry, n, k, ws, "whole", **kw)
            _hold_probe(eng, entry, n, k, ws, "whole", **kw)
    torch.cuda.synchronize()
    print(f"whole {entry} n = {n}: k in {ks}: {time.perf_counter() - t0:.3f} s")


# ------------------------------------------------------------------------------------- per-tile k-slices + slabs
@pytest.mark.parametrize("n", D.NS_SLICES)
@pytest.mark.parametrize("entry", ["ws", "split", "planes"])
def test_kslices_bitwise(eng, monkeypatch, entry, n):
    _env(monkeypatch, wide=0)
    t0 = time.perf_counter()
    for k, pieces in D.PIECES.items():
        p = D.dense_plan(n, k)
        assert D.path_of(entry, n, k, 0) == "slices" and (p["n_whole"], p["n_split"]) == (0, pieces)
        ws = _workspace(eng, n, k)
        _hold_int(eng, entry, n, k, ws, "slices")
        _hold_probe(eng, entry, n, k, ws, "slices")
    torch.cuda.synchronize()
    print(f"slices {entry} n = {n}: k in {tuple(D.PIECES)}: {time.perf_counter() - t0:.3f} s")


def test_ws_without_workspace_runs_unsplit(eng, monkeypatch):
    """grf_gram_dense_ws with NULL or a too small workspace: whole tiles, the same exact K."""
    _env(monkeypatch, wide=0)
    n, k = 129, 80
    op, ref = _op(eng, "int", n, k)
    for ws in (None, torch.zeros(D.TICKET_BYTES, dtype=torch.uint8, device=eng.device)):
        K = _gram(eng, "ws", op, ws)
        assert torch.equal(_i32(K), _i32(ref))


# ------------------------------------------------------------------------------------ stream-K over the 128-tiles
@pytest.mark.parametrize("k", D.KS_SK + (D.K_SK_UNCUT,))
@pytest.mark.parametrize("entry", ["ws", "split"])
def test_stream_k_bitwise(eng, monkeypatch, entry, k):
    """n = 2817 (276 tiles): k = 33 and 80 cut every tile across slots, k = 20 leaves every tile whole (control)."""
    _env(monkeypatch, wide=0)
    n = D.N_SK
    q = D.sk_plan(n, k)
    assert D.path_of(entry, n, k, 0) == "streamk"
    assert D.sk_cut_items(0, q["kt"], q["units"], q["total"]) == (0 if k == D.K_SK_UNCUT else 276)
    ws = _workspace(eng, n, k)
    t0 = time.perf_counter()
    _hold_int(eng, entry, n, k, ws, "stream-K")
    if k == 33:
        _hold_probe(eng, entry, n, k, ws, "stream-K")
    torch.cuda.synchronize()
    print(f"stream-K {entry} n = {n} k = {k}: grid {q['grid']} units {q['units']}: {time.perf_counter() - t0:.3f} s")


# ------------------------------------------------------------------------- the tail split (planes tile kernel only)
@pytest.mark.parametrize("n", D.NS_TAIL)
def test_tail_split_bitwise(eng, monkeypatch, n):
    _env(monkeypatch, wide=0)
    k = D.K_TAIL
    p = D.dense_plan(n, k)
    assert D.path_of("planes", n, k, 0) == "tail" and p["n_split"] == 3
    assert (p["n_whole"], p["split_tiles"]) == {3969: (0, 528), 5633: (512, 523)}[n]
    ws = _workspace(eng, n, k)
    t0 = time.perf_counter()
    _hold_int(eng, "planes", n, k, ws, "tail")
    torch.cuda.synchronize()
    print(f"tail planes n = {n} k = {k}: {p['n_whole']} whole + {p['split_tiles']} in 3: {time.perf_counter() - t0:.3f} s")


# ----------------------------------------------------------------------------------------------------- wide items
@pytest.mark.parametrize("n", D.NS_WIDE)
@pytest.mark.parametrize("entry", ["split", "planes"])
def test_wide_stream_k_bitwise(eng, monkeypatch, entry, n):
    """The 256 x 128 items forced at small n (odd tile-row counts: the second row block past n), stream-K only."""
    _env(monkeypatch, wide=1)
    t0 = time.perf_counter()
    for k in D.KS_WIDE:
        w = D.sk_plan_wide(n, k)
        assert D.path_of(entry, n, k, 1) == "wide" and w["dp_rounds"] == 0 and w["xcd_slots"] == 0
        ws = _workspace(eng, n, k)
        _hold_int(eng, entry, n, k, ws, "wide")
        _hold_probe(eng, entry, n, k, ws, "wide")
    torch.cuda.synchronize()
    print(f"wide {entry} n = {n}: k in {D.KS_WIDE}: {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("entry,xcd", [("split", 1), ("planes", 1), ("split", 0)])
def test_wide_xcd_rounds_bitwise(eng, monkeypatch, entry, xcd):
    """n = 5633 (529 items): one XCD-ordered round of whole items and 273 items streamed; GRF_DENSE_XCD=0 (once)
    streams all."""
    _env(monkeypatch, wide=1, xcd=None if xcd else 0)
    n, k = D.N_XCD, D.K_XCD
    w = D.sk_plan_wide(n, k, xcd=bool(xcd))
    assert (w["items"], w["dp_rounds"], w["xcd_slots"]) == ((529, 1, 1) if xcd else (529, 0, 0))
    ws = _workspace(eng, n, k)
    t0 = time.perf_counter()
    _hold_int(eng, entry, n, k, ws, "wide XCD")
    torch.cuda.synchronize()
    print(f"wide XCD={xcd} {entry} n = {n} k = {k}: grid {w['grid']} units {w['units']}: {time.perf_counter() - t0:.3f} s")


# ------------------------------------------------------------------------------ real data, once per distinct kernel
REAL = [("whole fp32", "dense", 129, 33, 0, None), ("whole fp32 upper (3 stages)", "upper", 129, 33, 0, None),
        ("whole split upper", "split_upper", 129, 33, 0, None), ("slices fp32", "ws", 129, 80, 0, None),
        ("slices split", "split", 129, 80, 0, None), ("slices planes", "planes", 129, 80, 0, None),
        ("stream-K fp32", "ws", D.N_SK, 80, 0, None), ("stream-K split", "split", D.N_SK, 80, 0, None),
        ("tail planes", "planes", 3969, 33, 0, None), ("wide split", "split", 129, 80, 1, None),
        ("wide planes", "planes", 129, 80, 1, None), ("wide XCD split", "split", D.N_XCD, 33, 1, None),
        ("wide XCD planes", "planes", D.N_XCD, 33, 1, None)]


@pytest.mark.parametrize("what,entry,n,k,wide,xcd", REAL, ids=[r[0].replace(" ", "_") for r in REAL])
def test_real_case_within_derived_bound(eng, monkeypatch, what, entry, n, k, wide, xcd):
    _env(monkeypatch, wide=wide, xcd=xcd)
    expect = {"whole": "whole", "slice": "slices", "strea": "streamk", "tail ": "tail", "wide ": "wide"}[what[:5]]
    ws = _workspace(eng, n, k) if entry in NEEDS_WS else None
    assert D.path_of(entry, n, k, wide, workspace=ws is not None) == expect
    _hold_real(eng, entry, n, k, ws, what)


# --------------------------------------------------------------------------------------------------------- planes
def _plane_inputs(n, k):
    lda = D.cdiv(k, 16) * 16 + (16 if n == 5 else 0)
    yield "int", D.int_case(n, k, 1, lda)[0]
    yield "probe", D.probe_case(n, k, 1, lda).A
    yield "real", D.real_case(n, k, 1, lda)[0]
    yield "edges", D.pad_lda(D.edge_matrix(n, k, n * 100 + k), lda)


@pytest.mark.parametrize("n", [1, 5, 129])
def test_split_planes_bytes(eng, n):
    """grf_split_planes against planes_ref byte for byte; bytes past the row's planes (ldp padded) untouched."""
    for k in (1, 16, 17, 33):
        for name, A in _plane_inputs(n, k):
            ref = D.planes_ref(A, k)
            for pad in (0, 32):
                P, ldp = _planes(eng, _t(A, eng), n, k, A.shape[1], pad)
                host = P.cpu().numpy()
                rows = host[:n * ldp].reshape(n, ldp)
                assert np.array_equal(rows[:, :ref.shape[1]], ref), (name, n, k, pad)
                assert np.all(rows[:, ref.shape[1]:] == 0xA5) and np.all(host[n * ldp:] == 0xA5), (name, n, k, pad)


@pytest.mark.parametrize("n_cols", [33, 7])
def test_densify_padded_planes_bytes(eng, n_cols):
    """Padded rows straight to planes: cnt of 0, 1 and cap; n_cols not a multiple of 16; slots past cnt ignored."""
    cap = 7 if n_cols == 7 else 8
    cnt = np.array([0, 1, cap, 3, cap, 0, 2], np.int32)
    r = np.random.default_rng(n_cols)
    e = D.edge_values()
    e = e[e != 0]
    idx = np.stack([r.permutation(n_cols)[:cap] for _ in cnt]).astype(np.int32)
    val = e[r.integers(0, len(e), (len(cnt), cap))].astype(np.float32)
    dense = np.zeros((len(cnt), n_cols), np.float32)
    for i, c in enumerate(cnt):
        dense[i, idx[i, :c]] = val[i, :c]
    ref = D.planes_ref(dense, n_cols)
    ldp = ref.shape[1] + 16
    P = torch.full((len(cnt) * ldp + PAD,), 0xA5, dtype=torch.uint8, device=eng.device)
    cnt_t, idx_t, val_t = _t(cnt, eng), _t(idx.reshape(-1), eng), _t(val.reshape(-1), eng)  # (named: alive at the launch)
    assert idx_t.numel() == val_t.numel() == len(cnt) * cap and int(cnt_t.max()) <= cap and int(idx_t.max()) < n_cols
    rc = eng.lib.grf_densify_padded_planes(len(cnt), cap, n_cols, _vp(cnt_t), _vp(idx_t), _vp(val_t), _vp(P), ldp,
                                           eng.stream)
    assert rc == 0, eng.lib.grf_last_error()
    host = P.cpu().numpy()
    rows = host[:len(cnt) * ldp].reshape(len(cnt), ldp)
    assert np.array_equal(rows[:, :ref.shape[1]], ref)
    assert np.all(rows[:, ref.shape[1]:] == 0xA5) and np.all(host[len(cnt) * ldp:] == 0xA5)


@pytest.mark.parametrize("wide", [0, 1])
def test_gram_planes_host_built_and_split_same_bits(eng, monkeypatch, wide):
    """grf_gram_dense_planes on planes_ref uploaded = on device-built planes = grf_gram_dense_split on A, path equal."""
    _env(monkeypatch, wide=wide)
    n, k = 129, 80
    assert D.path_of("planes", n, k, wide) == D.path_of("split", n, k, wide) == ("wide" if wide else "slices")
    ws = _workspace(eng, n, k)
    for kind in ("real", "probe", "int"):
        op = _op(eng, kind, n, k)[0]
        ref = D.planes_ref(op.A.cpu().numpy(), k)
        ldp = ref.shape[1] + 48
        host = np.full((n, ldp), 0x5A, np.uint8)
        host[:, :ref.shape[1]] = ref
        Kh = _gram(eng, "planes", op, ws, planes=(_t(host, eng), ldp))
        Kd = _gram(eng, "planes", op, ws)
        Ks = _gram(eng, "split", op, ws)
        assert torch.equal(_i32(Kh), _i32(Kd)) and torch.equal(_i32(Kd), _i32(Ks)), (kind, wide)


# ------------------------------------------------------------------------------------------ arguments, n = 0, k = 0
def _untouched(buf):
    return bool(torch.isnan(buf).all())


def test_argument_checks_return_einval_and_write_nothing(eng, monkeypatch):
    from grf_amd import _lib as C
    _env(monkeypatch, wide=0)
    n, k = 5, 17
    A = torch.zeros(n * 64 + 64, dtype=torch.float32, device=eng.device)
    need = int(eng.lib.grf_gram_dense_split_workspace_bytes(129, 33))
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=eng.device)
    assert ws.data_ptr() % 256 == 0 and need > D.TICKET_BYTES

    def fp32_args(entry, Aoff, lda, K, ldk, off=0):
        a = (n, k, _vp(A, Aoff), lda, _vp(K, 4 * off), ldk)
        fn = {"dense": eng.lib.grf_gram_dense, "upper": eng.lib.grf_gram_dense_upper,
              "split_upper": eng.lib.grf_gram_dense_split_upper, "ws": eng.lib.grf_gram_dense_ws,
              "split": eng.lib.grf_gram_dense_split}[entry]
        return fn(*a, _vp(ws), ws.numel(), eng.stream) if entry in NEEDS_WS else fn(*a, eng.stream)

    for entry in ("dense", "upper", "split_upper", "ws", "split"):
        for why, Aoff, lda, ldk, off in (("lda not a multiple of 16", 0, 40, 8, 0), ("lda < kpad", 0, 16, 8, 0),
                                         ("A misaligned", 4, 32, 8, 0), ("ldk % 4 != 0", 0, 32, 6, 0),
                                         ("K misaligned", 0, 32, 8, 1)):
            if entry in UPPER and why in ("ldk % 4 != 0", "K misaligned"):
                continue                                   # (allowed there: test_whole_tiles_bitwise)
            K = torch.full((n * 8 + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
            assert fp32_args(entry, Aoff, lda, K, ldk, off) == C.GRF_EINVAL, (entry, why)
            assert _untouched(K), (entry, why)
    # the workspace of the split and planes entries: too small, misaligned, NULL
    n2, k2 = 129, 33
    op = _op(eng, "int", n2, k2)[0]
    for entry in ("split", "planes"):
        op.planes()
        for why, wsv, nbytes in (("too small", ws, need - 1), ("misaligned", ws[128:], need), ("NULL", None, 0)):
            K = torch.full((n2 * 132 + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
            assert _call(eng, entry, op, K, 132, ws=wsv, ws_bytes=nbytes) == C.GRF_EINVAL, (entry, why)
            assert _untouched(K), (entry, why)
    K = torch.full((n2 * 133 + PAD,), float("nan"), dtype=torch.float32, device=eng.device)
    assert _call(eng, "planes", op, K, 133, ws=ws) == C.GRF_EINVAL and _untouched(K)      # ldk % 4 != 0
    assert not bool(ws[:D.TICKET_BYTES].any())


def test_n_zero_returns_ok_and_touches_nothing(eng):
    A = torch.zeros(64, dtype=torch.float32, device=eng.device)
    op = Op(eng, np.zeros((1, 16), np.float32), 0, 5)
    op.A = A
    P = torch.full((96 + PAD,), 0xA5, dtype=torch.uint8, device=eng.device)
    ws = _workspace(eng, 0, 5)
    for entry in ("dense", "upper", "split_upper", "ws", "split", "planes"):
        K = torch.full((PAD,), float("nan"), dtype=torch.float32, device=eng.device)
        assert _call(eng, entry, op, K, 4, ws=ws if entry in NEEDS_WS else None, planes=(P, 96)) == 0, entry
        assert _untouched(K) and not bool(ws.any()), entry
    assert eng.lib.grf_split_planes(0, 5, _vp(A), 16, _vp(P), 96, eng.stream) == 0 and bool((P == 0xA5).all())


def _hold_k_zero(eng, entry, n):
    op = Op(eng, np.zeros((n, 16), np.float32), n, 0)
    op._P = (torch.full((n * 96 + PAD,), 0xA5, dtype=torch.uint8, device=eng.device), 96)
    ws = _workspace(eng, n, 0) if entry in NEEDS_WS else None
    K = _gram(eng, entry, op, ws)
    if entry in UPPER:
        K = _upper_views(K, K)[0]
    assert not bool(_i32(K.contiguous()).any()), (entry, n, "K is not all +0")


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("n", [1, 129])
def test_k_zero_gives_zero_k(eng, monkeypatch, n, wide):
    _env(monkeypatch, wide=wide)
    for entry in ("dense", "upper", "split_upper", "ws", "split", "planes"):
        _hold_k_zero(eng, entry, n)


@pytest.mark.parametrize("entry", ["ws", "split", "planes"])
def test_k_zero_from_256_tiles_on(eng, monkeypatch, entry):
    """n = 2817 (276 tiles), k_dim = 0: the stream-K plan has no units and an empty grid; the parent returned
    GRF_EHIP from grf_gram_dense_ws and grf_gram_dense_split here.  A zero K, as below 256 tiles."""
    _env(monkeypatch, wide=0)
    assert D.dense_plan(D.N_SK, 0)["tiles"] >= D.CUS and D.sk_plan(D.N_SK, 0)["grid"] == 0
    _hold_k_zero(eng, entry, D.N_SK)
