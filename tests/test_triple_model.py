"""CPU: tools/triple_model.py -- the record-triple grouping rule counted from block counts -- against a brute-force
grouping of the entries themselves, the model's totals against a per-bucket recount, and the transpose's slab
bound against its worst-case buckets.

The rule (include/grf.h, grf_rec_kind): a bucket's entries in block order (aligned 512-row blocks of the band); a
triple whose first entry lies in block e takes the following entries while they lie in block e or e + 1.  The
brute force below walks the entries one by one and knows nothing of block counts.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import triple_model as M  # noqa: E402


def brute_triples(rows):
    """The rule, entry by entry: rows of one bucket (band-local) -> list of triples (lists of rows)."""
    out = []
    for j in sorted(rows, key=lambda r: r // M.BLOCK_ROWS):  # (stable: any order inside a block)
        e = j // M.BLOCK_ROWS
        if out and len(out[-1]) < 3 and e - out[-1][0] // M.BLOCK_ROWS <= 1:
            out[-1].append(j)
        else:
            out.append([j])
    return out


def random_buckets(rng, n, W):
    """n buckets of band width W: sizes 0 .. ~40, some confined to few blocks, some spread thin."""
    buckets = []
    for i in range(n):
        c = int(rng.integers(0, 41)) if i % 5 else int(rng.integers(0, 6))
        kind = i % 4
        if kind == 0:
            pool = np.arange(W)
        elif kind == 1:   # one block
            b = int(rng.integers(0, M.n_blocks(W)))
            pool = np.arange(b * M.BLOCK_ROWS, min(W, (b + 1) * M.BLOCK_ROWS))
        elif kind == 2:   # even blocks only: every triple closes early
            pool = np.concatenate([np.arange(b * M.BLOCK_ROWS, min(W, (b + 1) * M.BLOCK_ROWS))
                                   for b in range(0, M.n_blocks(W), 2)])
        else:             # two far blocks
            pool = np.concatenate([np.arange(0, min(W, M.BLOCK_ROWS)), np.arange(max(0, W - M.BLOCK_ROWS), W)])
        buckets.append(rng.choice(pool, size=min(c, len(pool)), replace=False).tolist())
    return buckets


def counts_of(buckets, W):
    blk = np.zeros((len(buckets), M.n_blocks(W)), np.int64)
    for i, rows in enumerate(buckets):
        for j in rows:
            blk[i, j // M.BLOCK_ROWS] += 1
    return torch.from_numpy(blk)


def test_layout_matches_brute_force_grouping():
    rng = np.random.default_rng(5)
    for W in (4096, 1024, 256, 3520):
        buckets = random_buckets(rng, 300, W)
        blk = counts_of(buckets, W)
        T, take, own, rest = (x.numpy() for x in M.triple_layout(blk))
        for i, rows in enumerate(buckets):
            tri = brute_triples(rows)
            assert T[i] == len(tri), (W, i, rows)
            # every entry's slot from its block and its rank in the block = where the brute force put it
            want = {}
            for t, tr in enumerate(tri):
                for s, j in enumerate(tr):
                    want.setdefault(j // M.BLOCK_ROWS, []).append(3 * t + s)
            for e, slots in want.items():
                got = [own[i, e] + r if r < take[i, e] else rest[i, e] + (r - take[i, e]) for r in range(len(slots))]
                assert got == sorted(slots), (W, i, e)
            # offsets fit their 10 bits and a triple's first entry holds place 0
            for tr in tri:
                base = tr[0] // M.BLOCK_ROWS * M.BLOCK_ROWS
                assert all(0 <= j - base < 1024 for j in tr)


def test_bucket_costs_and_model_totals():
    rng = np.random.default_rng(9)
    W, n_rows, n_cols = 1024, 2048 + 70, 37
    dense = rng.random((n_rows, n_cols)) < 0.02
    dense[:, 3] = False                       # an empty column
    dense[5::97, 7] = True
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int64))
    idx = torch.from_numpy(np.nonzero(dense)[1].astype(np.int32))
    out = M.model(ptr, idx, n_rows, n_cols, W)
    nb = -(-n_rows // W)
    lines = {"pair": 0, "triple": 0}
    pos = {"pair": 0, "triple": 0}
    visits = 0
    for k in range(n_cols):
        seen = 0   # entries of column k in the bands <= b: the symmetric Gram's visits of bucket (b, k)
        for b in range(nb):
            rows = (np.nonzero(dense[b * W:(b + 1) * W, k])[0]).tolist()
            seen += len(rows)
            visits += seen
            pp, tp = (len(rows) + 1) // 2, len(brute_triples(rows))
            lines["pair"] += seen * -(-12 * pp // 128)
            pos["pair"] += seen * pp
            lines["triple"] += seen * -(-tp // 8)
            pos["triple"] += seen * tp
    assert out["bucket_visits"] == visits and out["nnz"] == int(dense.sum())
    for name in ("pair", "triple"):
        assert out[name]["lines"] == lines[name] and out[name]["positions"] == pos[name]


def test_poisson_buckets_reproduce_the_issue_table():
    """Poisson(17.8) buckets, rows uniform in a 4096 band (C4's mean bucket): 1.25 / 9.15 for pairs, 1.08 / 6.61
    for triples per non-empty bucket (+-0.01: 10^5 buckets)."""
    g = torch.Generator().manual_seed(0)
    c = torch.poisson(torch.full((100_000,), 17.8), generator=g).long()
    owner = torch.repeat_interleave(torch.arange(c.numel()), c)
    b = torch.randint(0, 8, (int(c.sum()),), generator=g)
    blk = torch.zeros(c.numel() * 8, dtype=torch.long).index_add_(0, owner * 8 + b, torch.ones_like(b)).view(-1, 8)
    cost = M.bucket_costs(blk)
    ne = float((c > 0).sum())
    for key, want in (("pair_lines", 1.25), ("pair_pos", 9.15), ("triple_lines", 1.08), ("triple_pos", 6.61)):
        assert abs(float(cost[key].sum()) / ne - want) < 0.01, key


def test_slab_bound_holds_for_the_worst_buckets():
    """A region's slab (lines) is sized from its entries E and buckets nb alone.  Worst case per entry: every entry
    alone in blocks 0, 2, 4, 6, so every triple closes with one entry; also buckets of 1 entry (a line each), full
    single-block buckets, and mixtures."""
    def lines_of(blk):
        return int(((M.triples(blk) + 7) // 8).sum())

    nb = 128
    worst = torch.tensor([[1, 0, 1, 0, 1, 0, 1, 0]]).repeat(nb, 1)
    assert int(M.triples(worst)[0]) == 4
    singles = torch.tensor([[0, 0, 0, 1, 0, 0, 0, 0]]).repeat(nb, 1)
    full = torch.tensor([[512, 0, 0, 0, 0, 0, 0, 0]]).repeat(nb, 1)
    spread = torch.tensor([[22, 0, 22, 0, 22, 0, 22, 0]]).repeat(nb, 1)   # 8 lines' worth, each block closing early
    rng = np.random.default_rng(1)
    mixed = torch.from_numpy(rng.integers(0, 30, (nb, 8)) * (rng.random((nb, 8)) < 0.4))
    empty_mostly = torch.zeros(nb, 8, dtype=torch.long)
    empty_mostly[::9, 0] = 25
    for blk in (worst, singles, full, spread, mixed, empty_mostly):
        E = int(blk.sum())
        assert lines_of(blk) <= M.triple_slab_bound(E, nb), (E, lines_of(blk))
    # per bucket: 3 T <= c + 8 (at most 4 early closes, 2 places each)
    for blk in (worst, spread, mixed):
        assert bool((3 * M.triples(blk) <= blk.sum(-1) + 8).all())


def test_pipeline_selects_the_format_per_graph(monkeypatch):
    """pipeline.rec_triples: triples for the symmetric whole K at W <= 4096 when Phi is not skewed and no hub columns
    are split off; GRF_REC_TRIPLES = 0 / 1 forces pairs / triples (never outside the symmetric mode or past W = 4096)."""
    sys.path.insert(0, os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd"))
    from grf_amd import pipeline as P
    f = np.ones(4)
    monkeypatch.delenv("GRF_REC_TRIPLES", raising=False)
    pl = P.plan_step(5000, 16, 4, 0.1, f)
    assert pl.mode == "sym" and P.rec_triples(pl)
    pl.skewed = True
    assert not P.rec_triples(pl)
    pl.skewed, pl.hubs = False, 96
    assert not P.rec_triples(pl)
    monkeypatch.setenv("GRF_REC_TRIPLES", "1")
    assert P.rec_triples(pl)
    wide = P.plan_step(5000, 16, 4, 0.1, f, band_width=8192)
    rows = P.plan_step(5000, 16, 4, 0.1, f, no_sym=True)
    assert not P.rec_triples(wide) and not P.rec_triples(rows)
    monkeypatch.setenv("GRF_REC_TRIPLES", "0")
    pl.hubs = 0
    assert not P.rec_triples(pl)
