"""Key-buckets probe: what does one sb_key_buckets call cost next to what an engine did before it to turn a numeric key
column into range-bucket ids (GROUP BY date_trunc, price bands, histograms, GROUP BY over a float column), and next to
the sibling walk sb_key_lookup on the same pages?

Per key type, page kind and number of bounds, timed on the context's stream with device events (median and min-max of
--steps runs after --warmup):
  A      sb_read_columns through a prepared batch, then torch.bucketize(right=True) over the bounds on the device: a
         bucket per row, -1 where the row is null
  B      Int64 only: one sb_key_lookup call through a prepared batch against a list of as many values (the bounds
         themselves; ids of two bytes): the same walk with an equality test where C keeps the lower bound, and unchanged
         by this call's arrival: the yardstick
  C      one sb_key_buckets call through a prepared batch (left-closed, ids of two bytes)
All three see the same pages.  The column has --rows rows of 1024 distinct keys (10 % nulls) in pages of --page-rows:
plain, Dict and RLE (runs of 64) pages of Int64 and of Float64 keys.  The bounds are 7 / 255 / 1023 of the keys, evenly
spread.  C's ids are compared with A's before anything is timed.  Prints one JSON line per case; --profile adds the
per-kernel split of B and C from sb_ctx_profile.

  python scripts/key_buckets_probe.py [--steps 20] [--warmup 3] [--rows 4000000] [--page-rows 65536] [--bounds 7,255,1023]
                                      [--only int64,float64] [--profile]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import sbo as S   # noqa: E402
from read_selected_probe import timed, unpack_bits   # noqa: E402

DISTINCT = 1024


def column(ktype, rows, runs):
    rng = np.random.default_rng(runs)
    pool = np.unique(rng.integers(-(1 << 40), 1 << 40, 2 * DISTINCT))[:DISTINCT]
    if ktype == "float64":
        pool = pool.astype(np.float64) / 1024.0   # (exact: 41 bits)
    else:
        pool = pool.astype(np.int64)
    v = np.repeat(pool[rng.integers(0, DISTINCT, rows // runs + 1)], runs)[:rows]
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    ptype = S.T_F64 if ktype == "float64" else S.T_I64
    return dict(ptype=ptype, nullable=True, rows=rows, values=np.ascontiguousarray(v), validity=validity, offsets=None), np.sort(pool)


def cases(rows, page_rows, only):
    for ktype in ("int64", "float64"):
        if only and ktype not in only:
            continue
        for name, runs, codec in (("plain", 1, S.NONE), ("dict", 1, S.DICT), ("rle", 64, S.RLE)):
            col, pool = column(ktype, rows, runs)
            yield ktype, name, col, pool, dict(max_page_size=page_rows, force_codec=codec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--page-rows", type=int, default=65536)
    ap.add_argument("--bounds", default="7,255,1023")
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the lookup and the buckets call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.key_buckets import KeyBucketsBatch
    from strawboat_amd.key_lookup import KeyLookupBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    rows = args.rows
    for ktype, name, col, pool, opt in cases(rows, args.page_rows, only):
        pages, metas = S.write_column(col["ptype"], col["nullable"], rows, col["values"], validity=col["validity"], offsets=col["offsets"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas)]
        rbatch = read.ReadBatch(ctx, cols)
        tdtype = torch.float64 if ktype == "float64" else torch.int64
        for n_bounds in [int(x) for x in args.bounds.split(",")]:
            bounds = np.ascontiguousarray(pool[(np.arange(n_bounds) * DISTINCT) // n_bounds + (DISTINCT // n_bounds) // 2])
            assert bounds.size == n_bounds and (bounds[1:] > bounds[:-1]).all()
            cbatch = KeyBucketsBatch(ctx, cols, [bounds], id_width=2)
            bbatch = KeyLookupBatch(ctx, cols, [bounds], None, None, 2) if ktype == "int64" else None
            bounds_dev = torch.from_numpy(bounds).to(ctx.torch_device)

            def run_a():
                a = rbatch.enqueue()[0]
                with torch.cuda.stream(ctx.torch_stream):
                    vals = a.values.view(tdtype)[:rows]
                    b = torch.bucketize(vals, bounds_dev, out_int32=True, right=True)   # (the number of bounds <= x)
                    return torch.where(unpack_bits(torch, a.validity, rows), b, torch.full_like(b, -1))

            rbatch.enqueue()
            ctx.synchronize()   # (a first read of these pages may be issued again by its launch hints: A is compared after it)
            want = run_a()
            got = cbatch.enqueue()[0]
            ctx.synchronize()
            mine = got.ids.view(torch.int16).to(torch.int32) & 0xFFFF
            mine = torch.where(mine == 0xFFFF, torch.full_like(mine, -1), mine)
            what = "%s %s, %d bounds" % (ktype, name, n_bounds)
            if not torch.equal(mine, want.to(torch.int32)):   # say which of the two the host disagrees with
                bad = torch.nonzero(mine != want.to(torch.int32)).flatten()
                r = int(bad[0])
                host = int(np.searchsorted(bounds, col["values"][r], side="right"))
                raise AssertionError("%s: %d ids differ, the first at row %d (value %r): C %d, A %d, numpy %d"
                                     % (what, bad.numel(), r, col["values"][r], int(mine[r]), int(want[r]), host))
            res = {"keys": ktype, "pages": name, "n_bounds": n_bounds, "rows": rows, "count": got.count, "matched": got.matched,
                   "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
            res["A_read_then_bucketize_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
            if bbatch is not None:
                res["B_key_lookup_ms"] = timed(torch, ctx, bbatch.enqueue, args.steps, args.warmup)
            res["C_key_buckets_ms"] = timed(torch, ctx, cbatch.enqueue, args.steps, args.warmup)
            res["A_over_C"] = round(res["A_read_then_bucketize_ms"]["median"] / res["C_key_buckets_ms"]["median"], 2)
            if bbatch is not None:
                res["C_over_B"] = round(res["C_key_buckets_ms"]["median"] / res["B_key_lookup_ms"]["median"], 3)
            if args.profile:
                for tag, batch in (("B", bbatch), ("C", cbatch)):
                    if batch is None:
                        continue
                    ctx.profile(True)
                    for _ in range(args.steps):
                        batch.enqueue()
                        ctx.synchronize()
                    res[tag + "_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
                    ctx.profile(False)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
