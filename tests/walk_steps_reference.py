"""Plain numpy / Python restatements of the walk -> steps -> Phi pipeline and the cases its kernel tests use
(grf_walk.hip, grf_philox.h, grf_steps.hip).  No GPU, no torch: tests/test_walk_steps_reference.py pins
these against the C oracle where the oracle can represent the case, tests/test_gpu_walk_steps_kernels.py
holds the HIP kernels to them bit for bit.

Slots are ``node[n_src, L, m]`` (int32, -1 empty) and ``load[n_src, L, m]`` (fp64), as grf_walk writes them.
Step rows are ``rows[s][l] = (idx, val)`` with idx ascending; Phi rows ``(cnt, [idx_s], [v64_s], [v32_s])``.

Everything is IEEE fp64 taken operation by operation (Python floats and numpy scalars), in the orders the
kernels promise: loads added in walk order from 0.0, Phi terms added in step order from ``0.0 + first``.

Not restated: the Lemire rejection tail of the neighbour draw (probability < deg / 2^32 per step, out of
reach at testable degrees) -- the deterministic walks here draw no neighbour at all (out-degree <= 1).
"""
import numpy as np

NORM_DIV, NORM_MUL_RECIP = 0, 1
LOAD_CUMULATIVE, LOAD_NONCUMULATIVE, LOAD_ABLATION = 0, 1, 2
TOP = 2 ** 31 - 1  # the largest int32 node id


# ------------------------------------------------------------------------------------------ restatements
def steps_ref(node, load, norm, start=0.0, reverse=False):
    """rows[s][l] = (idx int64 ascending, val fp64): per (source, step) the loads of each node added in
    walk order starting from ``start`` (0.0), then acc / m (NORM_DIV) or acc * (1.0 / m) (NORM_MUL_RECIP).
    Explicit zeros are kept.  ``start`` / ``reverse`` exist for the sensitivity tests only."""
    node = np.asarray(node)
    load = np.asarray(load, np.float64)
    n_src, L, m = node.shape
    fm = np.float64(m)
    rows = []
    for s in range(n_src):
        per = []
        for l in range(L):
            acc = {}
            nd, ld = node[s, l].tolist(), load[s, l].tolist()
            order = range(m - 1, -1, -1) if reverse else range(m)
            for w in order:
                v = nd[w]
                if v >= 0:
                    acc[v] = acc.get(v, start) + ld[w]
            keys = sorted(acc)
            a = np.array([acc[k] for k in keys], np.float64)
            with np.errstate(all="ignore"):
                val = a / fm if norm == NORM_DIV else a * (np.float64(1.0) / fm)
            per.append((np.array(keys, np.int64), val))
        rows.append(per)
    return rows


def phi_ref(step_rows, f, n_f, cap, start=0.0, reverse=False):
    """(cnt int32 [n_src], idx list, v64 list, v32 list): per source and node ``f[l] * value`` added in step
    order from ``0.0 + first`` over the first min(n_f, L) steps; entries that are exactly zero dropped; nodes
    ascending; each row cut to ``cap`` entries with the count clamped.  v32 is v64 rounded once to fp32."""
    cnt, idxs, v64s, v32s = [], [], [], []
    for per in step_rows:
        Lf = min(int(n_f), len(per))
        acc = {}
        order = range(Lf - 1, -1, -1) if reverse else range(Lf)
        with np.errstate(all="ignore"):
            for l in order:
                fl = np.float64(f[l])
                idx, val = per[l]
                for k, v in zip(idx.tolist(), val):
                    t = fl * v
                    acc[k] = (acc[k] + t) if k in acc else (np.float64(start) + t)
        keys = [k for k in sorted(acc) if acc[k] != 0.0]  # (NaN != 0.0: kept, as the kernels keep it)
        keys = keys[:cap]
        v64 = np.array([acc[k] for k in keys], np.float64)
        with np.errstate(all="ignore"):
            v32 = v64.astype(np.float32)
        cnt.append(len(keys))
        idxs.append(np.array(keys, np.int64))
        v64s.append(v64)
        v32s.append(v32)
    return np.array(cnt, np.int32), idxs, v64s, v32s


def det_walk_ref(ptr, idx, val, m, p, L, rule, src_begin=0, src_end=None):
    """Slots of the walks on a graph where every visited node has out-degree <= 1 and p = 0: the visits
    follow the only edge; the load is ``load * ((deg * w) / (1 - p))`` (cumulative), that quotient
    (non-cumulative) or ``w`` (ablation); unreached slots are -1 (their loads 0.0, never compared)."""
    assert p == 0.0
    n = len(ptr) - 1
    src_end = n if src_end is None else src_end
    node = np.full((src_end - src_begin, L, m), -1, np.int32)
    load = np.zeros((src_end - src_begin, L, m), np.float64)
    keep = np.float64(1.0) - np.float64(p)
    with np.errstate(all="ignore"):
        for s in range(src_begin, src_end):
            cur, ld = s, np.float64(1.0)
            for l in range(L):
                node[s - src_begin, l, :] = cur
                load[s - src_begin, l, :] = ld
                deg = int(ptr[cur + 1] - ptr[cur])
                assert deg <= 1, "det_walk_ref: out-degree > 1"
                if l == L - 1 or deg == 0:
                    break
                w = np.float64(val[ptr[cur]])
                q = (np.float64(deg) * w) / keep
                ld = ld * q if rule == LOAD_CUMULATIVE else (q if rule == LOAD_NONCUMULATIVE else w)
                cur = int(idx[ptr[cur]])
    return node, load


def _next_pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def _ceil_log2(x):
    return max(0, int(x - 1).bit_length())


def fused_plan(m, L):
    """(P, T, kPer) of grf_phi_fused / grf_walk_phi: the host lines that size the sort and pick the threads
    per source (grf_steps.hip, "threads per source").  Used only to choose cases."""
    E = m * L
    P = max(64, _next_pow2(E))
    t_cap = min(256, max(64, ((m + 63) // 64) * 64))
    T = 256 if P >= 512 else (P // 2 if P >= 128 else 64)
    while T > t_cap and P // (T // 2) <= 16:
        T //= 2
    return P, T, P // T


def key_bits(m, L):
    """(wbits, lbits) of the fused kernel's (node, step, walk) keys."""
    return _ceil_log2(m), max(1, _ceil_log2(L))


# (m, L) -> the (kPer, T) it reaches: one shape per pair the host plan can reach.  E = m L equals P at
# (8, 8), (128, 2), (64, 4), (64, 8), (128, 8) and (4096, 1) (a full row leaves no sentinel key) and
# P / 2 + 1 at (13, 5) and (257, 1)
FUSED_SHAPES = [
    ((8, 8), (1, 64)),
    ((13, 5), (2, 64)),
    ((128, 2), (2, 128)),
    ((257, 1), (2, 256)),
    ((64, 4), (4, 64)),
    ((100, 5), (4, 128)),
    ((200, 5), (4, 256)),
    ((64, 8), (8, 64)),
    ((128, 8), (8, 128)),
    ((300, 5), (8, 256)),
    ((57, 17), (16, 64)),
    ((100, 20), (16, 128)),
    ((4096, 1), (16, 256)),
]
FUSED_PAIRS = [(1, 64), (2, 64), (2, 128), (2, 256), (4, 64), (4, 128), (4, 256), (8, 64), (8, 128), (8, 256),
               (16, 64), (16, 128), (16, 256)]


# ------------------------------------------------------------------------------------------------- loads
def loads(rng, shape, kind, m):
    """int: multiples of m in [-8 m, 8 m] (zeros included), so every sum of loads and, under NORM_DIV, every
    step value and Phi partial sum with the integer modulators is an integer below 2^53.
    real: magnitudes over ~30 binades, mixed signs (the summation order shows), a few -0.0."""
    if kind == "int":
        return (rng.integers(-8, 9, size=shape) * m).astype(np.float64)
    v = np.ldexp(rng.uniform(1.0, 2.0, size=shape), rng.integers(-15, 16, size=shape))
    v *= rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(size=shape) < 0.02] = -0.0
    return v


def modulators(L, kind, seed=0):
    """[(name, f or None, n_f)]: real-valued, with zeros, (1, -1, 0, ...), and the lengths 0, L - 1, L + 3."""
    rng = np.random.default_rng(1000 + seed + L)
    if kind == "int":
        base = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=L + 3)
    else:
        base = rng.standard_normal(L + 3) * np.ldexp(1.0, rng.integers(-4, 5, size=L + 3))
    zeros = base[:L].copy()
    zeros[::2] = 0.0
    if L == 1:
        zeros[0] = base[0]
    pm = np.zeros(L)
    pm[0] = 1.0
    if L > 1:
        pm[1] = -1.0
    out = [("full", base[:L].copy(), L), ("zeros", zeros, L), ("pm", pm, L), ("none", None, 0),
           ("long", base.copy(), L + 3)]
    if L > 1:
        out.append(("short", base[:L - 1].copy(), L - 1))
    return out


# ------------------------------------------------------------------------------------------------- cases
class _Row:
    """One source's slots built run by run in sorted key order (node, step, walk)."""

    def __init__(self, m, L, rng):
        self.m, self.L = m, L
        self.node = np.full((L, m), -1, np.int32)
        self.free = [list(rng.permutation(m)) for _ in range(L)]  # unused walks per step
        self.pos = 0        # sorted position of the next run
        self.cur = (-1, L)  # (node, step) of the last run
        self.runs = []      # (start, length, node, step)

    def room(self, l):
        return len(self.free[l])

    def next_slot(self, length, new_node=None):
        """The next (node, step) after the cursor with `length` free walks; None when the row is full."""
        nd, l = self.cur
        if new_node is not None:
            nd, l = new_node, -1
        for _ in range(2 * self.L + 2):
            l += 1
            if l >= self.L:
                if nd >= TOP:
                    return None
                nd, l = nd + 1, 0
            if self.room(l) >= length:
                return nd, l
        return None

    def add(self, length, new_node=None):
        at = self.next_slot(length, new_node)
        if at is None or length == 0:
            return False
        nd, l = at
        ws = sorted(self.free[l].pop() for _ in range(length))
        self.node[l, ws] = nd
        self.runs.append((self.pos, length, nd, l))
        self.pos += length
        self.cur = (nd, l)
        return True


def _runs_row(m, L, kper, rng, fill):
    """Runs of length kPer - 1, kPer, kPer + 1 and 2 kPer + 3 starting at sorted positions = 0 and
    = kPer - 1 (mod kPer), single visits between them; node ids 0, 1, ... and, last, 2^31 - 2 and 2^31 - 1.
    fill: every slot is then used (m L real keys; a full row when m L = P) and the last run, on node
    2^31 - 1, reaches the end of the keys.  Otherwise the last run (length >= 2) ends at the last real key
    and sentinels follow."""
    r = _Row(m, L, rng)
    for length in (kper - 1, kper, kper + 1, 2 * kper + 3):
        for at in (0, kper - 1):
            if length < 1 or length > m:
                continue
            while r.pos % kper != at % kper:
                if not r.add(1, new_node=r.cur[0] + 1 if rng.random() < 0.5 else None):
                    break
            r.add(length, new_node=r.cur[0] + 1 if rng.random() < 0.7 else None)
    if fill:
        # random runs on small ids, then node 2^31 - 2 and 2^31 - 1 take every walk left in every step
        # (two walks of every step are held back for node 2^31 - 1, so its last run is longer than one)
        held = [[r.free[l].pop() for _ in range(min(2, r.room(l)))] for l in range(L)]
        for _ in range(4 * kper):
            r.add(int(rng.integers(1, max(2, min(m, 2 * kper)))), new_node=None if rng.random() < 0.5 else r.cur[0] + 1)
        for l in range(L):
            k = r.room(l) // 2
            if k:
                r.cur = (TOP - 1, l - 1)
                r.add(k)
        for l in range(L):
            r.free[l] += held[l]
            if r.room(l):
                r.cur = (TOP, l - 1)
                r.add(r.room(l))
    else:
        r.cur = (TOP - 1, -1)
        r.add(1)
        r.cur = (TOP, -1)
        r.add(min(m, max(2, kper + 1)))
    return r.node


def fused_case(m, L, kind, seed=0):
    """(node, load, planted) with 6 sources (6 % 4 != 0):
      0 all empty; 1 every walk of every step on node 2^31 - 2 (runs of length m); 2 every slot a distinct
      node (0, 1, 2^31 - 2, 2^31 - 1 among them); 3 the planted runs, then sentinels; 4 the planted runs with
      every slot used; 5 a small pool of nodes (long runs, many steps per node) with empty slots, exact
      cancellations (a, -a alone in a run: a kept explicit zero in the step row, no Phi entry), equal step
      values at steps 0 and 1 of a node seen nowhere else (the modulator (1, -1, 0, ...) cancels them), a
      -0.0 load alone in its run and further -0.0 loads."""
    rng = np.random.default_rng(seed + 7919 * m + 104729 * L + (0 if kind == "int" else 1))
    kper = fused_plan(m, L)[2]
    E = m * L
    node = np.full((6, L, m), -1, np.int32)
    load = loads(rng, (6, L, m), kind, m)
    node[1] = TOP - 1
    ids = np.concatenate([[0, 1, TOP - 1, TOP], rng.choice(np.arange(2, 50 * E + 50), size=max(E - 4, 0), replace=False)])[:E]
    node[2] = rng.permutation(ids).reshape(L, m).astype(np.int32)
    node[3] = _runs_row(m, L, kper, rng, fill=False)
    node[4] = _runs_row(m, L, kper, rng, fill=True)
    pool = np.array([0, 1, 5, 6, 40, 41, 1000, TOP - 1, TOP], np.int64)[:max(2, min(9, m // 2 + 2))]
    node[5] = rng.choice(pool, size=(L, m)).astype(np.int32)
    node[5][rng.random(size=(L, m)) < 0.3] = -1
    planted = {}
    a = 3.0 * m if kind == "int" else 1.2345678901234567
    if m >= 2:  # node 77: walks 0 and 1 of step 0 carry a and -a, nothing else anywhere
        node[5][node[5] == 77] = -1
        node[5][0, 0] = node[5][0, 1] = 77
        load[5, 0, 0], load[5, 0, 1] = a, -a
        planted["cancel_node"] = 77
    if L >= 2 and m >= 3:  # node 99: one walk with load a at steps 0 and 1
        node[5][0, 2] = node[5][1, 2] = 99
        load[5, 0, 2] = load[5, 1, 2] = a
        planted["pm_node"] = 99
    if m >= 4:  # node 55: one walk with load -0.0 at step 0 -- the step row's explicit zero is 0.0 + -0.0 = +0.0
        node[5][0, 3] = 55
        load[5, 0, 3] = -0.0
        planted["negzero_node"] = 55
    return node, load, planted


def slots_case(m, L, n_src, kind, seed=0):
    """Slots for grf_steps at any m: source s is, by s % 5, 0 a pool of nodes around every id edge (0, 1,
    2^31 - 2, 2^31 - 1) with empty slots and an (a, -a) pair, 1 all empty, 2 one run of length m on node
    2^31 - 1, 3 all nodes distinct, 4 a pool of three nodes with no empty slot."""
    rng = np.random.default_rng(seed + 31 * m + 17 * L + n_src + (0 if kind == "int" else 5))
    node = np.full((n_src, L, m), -1, np.int32)
    load = loads(rng, (n_src, L, m), kind, m)
    pool = np.array([0, 1, 2, 7, 8, 65535, 65536, TOP - 1, TOP], np.int64)
    for s in range(n_src):
        t = s % 5
        if t == 0:
            node[s] = rng.choice(pool, size=(L, m)).astype(np.int32)
            node[s][rng.random(size=(L, m)) < 0.25] = -1
            if m >= 2:
                node[s][node[s] == 3] = -1
                node[s][0, 0] = node[s][0, m - 1] = 3
                load[s, 0, 0], load[s, 0, m - 1] = 2.5 * m, -2.5 * m
        elif t == 2:
            node[s] = TOP
        elif t == 3:
            for l in range(L):
                node[s, l] = (rng.permutation(m) * 131071 % (TOP - 5) + (l % 3)).astype(np.int32) if m > 4 else \
                    np.array([TOP, 0, TOP - 1, 1][:m], np.int32)
        elif t == 4:
            node[s] = rng.choice(pool[[0, 4, 8]], size=(L, m)).astype(np.int32)
    return node, load


def divisor_case(m):
    """(node, load, L): single-walk runs (every slot of a source its own node, so a step value is
    ``(0.0 + load) / m``) whose loads sweep every biased exponent 0..2046 with four mantissas and both signs,
    plus +-0, subnormals and +-inf: the fused kernel's Divisor on, at and off its fast window.  L <= 64 and
    m L <= 4096; the sources take the loads block by block."""
    rng = np.random.default_rng(97 + m)
    L = min(64, 4096 // m)
    E = m * L
    ex = np.repeat(np.arange(0, 2047, dtype=np.uint64), 4)
    man = np.tile(np.array([0, 1, 2 ** 52 - 1, 0], np.uint64), 2047)
    man[3::4] = rng.integers(0, 2 ** 52, size=2047, dtype=np.uint64)
    pos = ((ex << np.uint64(52)) | man).view(np.float64)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, 1e-310], np.float64)
    vals = np.concatenate([pos, -pos, special])
    n_src = -(-vals.size // E)
    load = np.zeros(n_src * E, np.float64)
    load[:vals.size] = vals
    load[vals.size:] = 1.0
    node = np.tile(np.arange(E, dtype=np.int32), n_src)
    return node.reshape(n_src, L, m), load.reshape(n_src, L, m), L


# ------------------------------------------------------------------------------- deterministic graphs
def det_graphs():
    """[(name, ptr int64, idx int32, val fp64)]: walk matrices whose nodes have out-degree <= 1 -- weighted
    directed cycles, paths into a sink, empty graphs, at n in {1, 2, 5}, and a cycle whose weights 1e200
    overflow the cumulative load to inf."""
    out = []
    for n in (1, 2, 5):
        w = np.array([0.75, -1.5, 3.0, 0.1, 7.0][:n])
        out.append((f"cycle{n}", np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32), w))
        ptr = np.minimum(np.arange(n + 1), n - 1).astype(np.int64)
        out.append((f"path{n}", ptr, np.arange(1, n, dtype=np.int32), w[:n - 1].copy()))
        out.append((f"empty{n}", np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)))
    out.append(("huge5", np.arange(6, dtype=np.int64), ((np.arange(5) + 1) % 5).astype(np.int32), np.full(5, 1e200)))
    return out


def aug_header(n, nnz, allow16=True):
    """{format, tb, rb} of grf_walk_aug's header as its comment derives them: tb, lb, rb the bits of the
    largest node id (>= 1), of a row length <= n and of a row start <= nnz (>= 1); format 1 (16-byte records)
    when allowed and tb + rb + lb <= 64."""
    tb = max(1, _ceil_log2(n))
    lb = _ceil_log2(n + 1)
    rb = max(1, _ceil_log2(nnz + 1))
    return (1 if allow16 and tb + rb + lb <= 64 else 0), tb, rb


# -------------------------------------------------------------------------------------------- helpers
def pack_steps(rows, m):
    """Step rows -> the padded arrays grf_phi reads: cnt[ns L], idx[ns L m], val[ns L m] (pad: -77 / NaN)."""
    ns, L = len(rows), len(rows[0])
    cnt = np.zeros(ns * L, np.int32)
    idx = np.full(ns * L * m, -77, np.int32)
    val = np.full(ns * L * m, np.nan, np.float64)
    for s in range(ns):
        for l in range(L):
            g = s * L + l
            k = len(rows[s][l][0])
            cnt[g] = k
            idx[g * m:g * m + k] = rows[s][l][0]
            val[g * m:g * m + k] = rows[s][l][1]
    return cnt, idx, val


def sorted_keys(node_row, m, L):
    """The fused kernel's sorted real keys of one source as (node, step, walk) tuples."""
    ks = [(int(node_row[l, w]), l, w) for l in range(L) for w in range(m) if node_row[l, w] >= 0]
    return sorted(ks)


def crosses_block(keys, kper):
    """True when a (node, step) run of the sorted keys continues past its first thread's block of kPer
    positions (the fused kernel's read-on loop runs)."""
    i = 0
    while i < len(keys):
        j = i
        while j + 1 < len(keys) and keys[j + 1][:2] == keys[i][:2]:
            j += 1
        if j // kper > i // kper:
            return True
        i = j + 1
    return False
