"""Whole-K Gram bucket gathers: 12-byte record pairs (today) against 16-byte record triples, counted from a Phi
CSR and a band width -- no kernel runs, torch on the CPU or the GPU.

A bucket (band b, column k) holds the entries Phi[j, k] with j in band b.  Line buckets start on a 128-byte line.

* pairs: one stream position per two entries, 12 bytes each: ceil(c / 2) positions, ceil(12 positions / 128) lines.
* triples: {u32 cols, 3 x f32}, 16 bytes, 8 per line; cols = c0 | o1 << 12 | o2 << 22 with c0 the first entry's
  row in the band and o1 / o2 10-bit offsets from c0 & ~511.  A bucket's entries are laid out by aligned 512-row
  block of the band (any order inside a block) and cut greedily: a triple whose first entry is in block e takes
  the following entries while they lie in block e or e + 1.  So the triples of a bucket, and the slot of every
  entry, follow from the bucket's block counts alone (``triple_layout``): T positions, ceil(T / 8) lines.

Buckets are weighted with the visits of the symmetric whole-K Gram, as ``bench.gather_model`` weights them: bucket
(b, k) is read once by every entry of column k in the bands <= b.

usage: python tools/triple_model.py [--graph er|facebook|enron] [--band-width 4096] [--out FILE.json]
(er: the headline's C4 setup Phi, on the GPU; facebook / enron: tests/golden/snap.npz)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

BLOCK_ROWS = 512   # rows of one aligned block of a band (9 offset bits; two blocks = the 10-bit offsets' reach)
PAIR_BYTES, TRIPLE_BYTES, LINE_BYTES = 12, 16, 128


def n_blocks(band_width: int) -> int:
    return -(-int(band_width) // BLOCK_ROWS)


def block_counts(ptr: torch.Tensor, idx: torch.Tensor, n_rows: int, n_cols: int, band_width: int) -> torch.Tensor:
    """(bands, n_cols, blocks) int64: the entries of every bucket in each 512-row block of its band."""
    W, nblk = int(band_width), n_blocks(band_width)
    nb = max(1, -(-n_rows // W))
    ptr = ptr.long()
    nnz = int(ptr[n_rows])
    rows = torch.repeat_interleave(torch.arange(n_rows, device=ptr.device), ptr[1:n_rows + 1] - ptr[:n_rows])
    key = ((rows // W) * n_cols + idx[:nnz].long()) * nblk + (rows % W) // BLOCK_ROWS
    return torch.bincount(key, minlength=nb * n_cols * nblk).view(nb, n_cols, nblk)


def triple_layout(blk: torch.Tensor):
    """The grouping rule from block counts blk[..., B].  Returns (T, take, own, rest): T[...] the bucket's triples;
    take[..., e] the entries of block e that fill the triple left open by block e - 1, from slot own[..., e]
    (a slot is 3 * triple + place in the triple); rest[..., e] the first slot of block e's other entries, which
    start a new triple.  The entry of rank r in block e goes to slot own + r if r < take else rest + (r - take)."""
    shape = blk.shape[:-1]
    T = torch.zeros(shape, dtype=torch.long, device=blk.device)
    free = torch.zeros_like(T)  # free slots of the last triple, usable by the next block only
    takes, own, rest = [], [], []
    for e in range(blk.shape[-1]):
        c = blk[..., e].long()
        take = torch.minimum(free, c)
        takes.append(take)
        own.append(3 * T - free)
        rest.append(3 * T)
        c = c - take
        T = T + (c + 2) // 3
        free = torch.where(c > 0, (3 - c % 3) % 3, torch.zeros_like(c))
    return T, torch.stack(takes, -1), torch.stack(own, -1), torch.stack(rest, -1)


def triples(blk: torch.Tensor) -> torch.Tensor:
    return triple_layout(blk)[0]


def bucket_costs(blk: torch.Tensor) -> dict:
    """Per bucket: stream positions and 128-byte lines, for pairs and for triples."""
    c = blk.sum(-1)
    pp = (c + 1) // 2
    tp = triples(blk)
    return {"entries": c, "pair_pos": pp, "pair_lines": (PAIR_BYTES * pp + LINE_BYTES - 1) // LINE_BYTES,
            "triple_pos": tp, "triple_lines": (TRIPLE_BYTES * tp + LINE_BYTES - 1) // LINE_BYTES}


def triple_slab_bound(entries: int, buckets: int, n_blk: int = 8) -> int:
    """Lines that hold the triples of any `buckets` buckets with `entries` entries in all (the transpose's slab of
    a region, sized before its buckets are counted).  A triple closes early -- with fewer than 3 entries -- only
    when its bucket's entries run out of the blocks e, e + 1 it may span, so at most once per pair of blocks
    that starts a triple, ceil(n_blk / 2) times per bucket, each time wasting at most 2 slots:
    T_b <= (c_b + 2 ceil(n_blk / 2)) / 3, and lines_b = ceil(T_b / 8) <= (T_b + 7) / 8.  Summed over the buckets
    (the worst case, every entry alone in blocks 0, 2, 4, 6: T_b = c_b = 4 <= (4 + 8) / 3)."""
    early = (n_blk + 1) // 2
    return (entries + 2 * early * buckets) // 24 + buckets + 1


def model(ptr: torch.Tensor, idx: torch.Tensor, n_rows: int, n_cols: int, band_width: int, sym: bool = True) -> dict:
    """Lines and stream positions per bucket visit of the whole-K Gram tiles, pairs against triples."""
    blk = block_counts(ptr, idx, n_rows, n_cols, band_width)
    cost = bucket_costs(blk)
    ent = cost["entries"]
    visits = ent.cumsum(0) if sym else ent.sum(0, keepdim=True).expand_as(ent)
    v_all = int(visits.sum())
    v_non = int((visits * (ent > 0)).sum())
    out = {"band_width": int(band_width), "bands": int(blk.shape[0]), "n_rows": int(n_rows), "n_cols": int(n_cols),
           "nnz": int(ent.sum()), "bucket_visits": v_all, "nonempty_bucket_visits": v_non,
           "mean_entries_per_nonempty_bucket": float(ent.sum()) / max(1, int((ent > 0).sum()))}
    for name in ("pair", "triple"):
        lines, pos = int((visits * cost[name + "_lines"]).sum()), int((visits * cost[name + "_pos"]).sum())
        out[name] = {"lines": lines, "positions": pos, "lines_per_visit": lines / max(1, v_all),
                     "positions_per_visit": pos / max(1, v_all), "lines_per_nonempty_visit": lines / max(1, v_non),
                     "positions_per_nonempty_visit": pos / max(1, v_non),
                     "record_bytes": pos * (PAIR_BYTES if name == "pair" else TRIPLE_BYTES)}
    out["lines_change"] = out["triple"]["lines"] / max(1, out["pair"]["lines"]) - 1.0
    out["positions_change"] = out["triple"]["positions"] / max(1, out["pair"]["positions"]) - 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["er", "facebook", "enron"], default="er")
    ap.add_argument("--band-width", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "efficient-gaussian-process-on-graphs_amd")]
    import bench
    from grf_amd.dist import setup_phi
    from grf_amd.engine import DeviceCSR, GRFEngine

    eng = GRFEngine("cuda:0")
    bargs = argparse.Namespace(graph=args.graph, n=100_000, edges=1_000_000, avg_degree=10.0)
    A = bench.make_graph(bargs)
    m, L, p = 128, 8, 0.1
    phi = setup_phi(eng, DeviceCSR.from_scipy(A, eng.device), m, p, L, bench.diffusion_modulator(L, 1.0), seed=42)
    out = {"graph": args.graph, **model(phi.ptr, phi.idx, phi.n_rows, phi.n_cols, args.band_width)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
