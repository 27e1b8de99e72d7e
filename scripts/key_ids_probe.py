"""Key-id probe: what does one sb_key_ids call cost next to what an engine did before it to GROUP BY a key column that
holds no dense small integers, or to SELECT DISTINCT it?

Per page kind, distinct count, selection and column count, timed with events on the context's stream (median and min-max
of --steps runs after --warmup):
  A      sb_read_columns through a prepared batch, then torch.unique(sorted=True, return_inverse=True) on the live rows
         (selected and not null), the inverse scattered back into an id per row (-1 elsewhere): keys and ids
  B      sb_read_selected through a prepared batch, then torch.unique on the valid values of its output: keys only, the
         DISTINCT use (B is given `selected` for free: a real caller learns it at a synchronize of its own)
  C      one sb_key_ids call through a prepared batch (max_keys 1024, ids of two bytes)
A and B run on code paths the new call does not touch; all three see the same pages and the same bitmap.  The pages are
None, RLE (runs of 64), Dict and LZ4 pages of a nullable Int64 column (10 % nulls), --rows rows in pages of --page-rows.
The selections are random (100 %, 10 %, 0.1 %) and clustered (10 % and 0.1 % as one stretch of rows).  C's keys and ids
are compared with A's before anything is timed.  Prints one JSON line per case; --profile adds the per-kernel split of C
from sb_ctx_profile.

  python scripts/key_ids_probe.py [--steps 10] [--warmup 2] [--rows 4000000] [--page-rows 65536] [--columns 4,16]
                                  [--distinct 16,256,1024] [--only none,rle,dict,lz4] [--profile]
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
from read_selected_probe import bitmap_bytes, timed, unpack_bits   # noqa: E402


def int_column(rows, uniq, runs):
    rng = np.random.default_rng(uniq)
    pool = rng.integers(-(1 << 40), 1 << 40, uniq)
    v = np.repeat(pool[rng.integers(0, uniq, rows // runs + 1)], runs)[:rows].astype(np.int64)
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    return dict(ptype=S.T_I64, nullable=True, rows=rows, values=v, validity=validity, offsets=None)


def cases(rows, page_rows, uniq):
    yield "none", int_column(rows, uniq, 1), dict(max_page_size=page_rows, force_codec=S.NONE)
    yield "rle", int_column(rows, uniq, 64), dict(max_page_size=page_rows, force_codec=S.RLE)
    yield "dict", int_column(rows, uniq, 1), dict(max_page_size=page_rows, force_codec=S.DICT)
    yield "lz4", int_column(rows, uniq, 1), dict(max_page_size=page_rows, force_codec=S.LZ4)


def selections(rows):
    rng = np.random.default_rng(3)
    yield "100%", np.ones(rows, bool)
    for p in (0.1, 0.001):
        yield "%g%% random" % (100 * p), rng.random(rows) < p
        m = np.zeros(rows, bool)
        at = int(rng.integers(0, rows - int(rows * p)))
        m[at:at + int(rows * p)] = True
        yield "%g%% clustered" % (100 * p), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--page-rows", type=int, default=65536)
    ap.add_argument("--columns", default="4,16")
    ap.add_argument("--distinct", default="16,256,1024")
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the key-id call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.key_ids import KeyIdsBatch
    from strawboat_amd.read_selected import ReadSelectedBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    rows = args.rows
    for uniq in [int(x) for x in args.distinct.split(",")]:
        for name, col, opt in cases(rows, args.page_rows, uniq):
            if only and name not in only:
                continue
            pages, metas = S.write_column(col["ptype"], col["nullable"], rows, col["values"], validity=col["validity"],
                                          options=S.make_options(**opt))
            dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
            for ncols in [int(x) for x in args.columns.split(",")]:
                cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(ncols)]
                rbatch = read.ReadBatch(ctx, cols)
                for sel_name, mask in selections(rows):
                    bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
                    mask_dev = torch.from_numpy(mask).to(ctx.torch_device)
                    selected = int(mask.sum())
                    sbatch = ReadSelectedBatch(ctx, cols, bitmap)
                    cbatch = KeyIdsBatch(ctx, cols, bitmap, 1024, 2)

                    def unique_of(arrs):
                        with torch.cuda.stream(ctx.torch_stream):
                            out = []
                            for a in arrs:
                                live = mask_dev & unpack_bits(torch, a.validity, rows)
                                keys, inv = torch.unique(a.values.view(torch.int64)[live], sorted=True, return_inverse=True)
                                ids = torch.full((rows,), -1, dtype=torch.int32, device=ctx.torch_device)
                                ids[live] = inv.to(torch.int32)
                                out.append((keys, ids))
                            return out

                    def run_a():
                        return unique_of(rbatch.enqueue())

                    def run_b():
                        arrs = sbatch.enqueue()
                        with torch.cuda.stream(ctx.torch_stream):
                            out = []
                            for a in arrs:
                                vals = a.values_buf[:selected * 8].view(torch.int64)
                                out.append(torch.unique(vals[unpack_bits(torch, a.validity_buf, selected)], sorted=True))
                            return out

                    arrs = rbatch.enqueue()
                    got = cbatch.enqueue()
                    # (the read's buffers are final at the synchronize: its interval may be issued a second time on a launch
                    # hint that missed)
                    ctx.synchronize()
                    ref = unique_of(arrs)
                    what = "%s, %d distinct, %s, %d columns" % (name, uniq, sel_name, ncols)
                    for g, (keys, ids) in zip(got, ref):
                        assert not g.overflow and np.array_equal(g.keys, keys.cpu().numpy()), "%s: the keys differ" % what
                        mine = g.ids.view(torch.int16).to(torch.int32) & 0xFFFF
                        mine = torch.where(mine == 0xFFFF, torch.full_like(mine, -1), mine)
                        assert torch.equal(mine, ids), "%s: the ids differ" % what
                    res = {"pages": name, "distinct": uniq, "selection": sel_name, "columns": ncols, "rows": rows, "selected": selected,
                           "n_keys": got[0].n_keys, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
                    res["A_read_then_unique_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
                    res["B_read_selected_then_unique_ms"] = timed(torch, ctx, run_b, args.steps, args.warmup)
                    res["C_key_ids_ms"] = timed(torch, ctx, cbatch.enqueue, args.steps, args.warmup)
                    res["A_over_C"] = round(res["A_read_then_unique_ms"]["median"] / res["C_key_ids_ms"]["median"], 2)
                    res["B_over_C"] = round(res["B_read_selected_then_unique_ms"]["median"] / res["C_key_ids_ms"]["median"], 2)
                    if args.profile:
                        ctx.profile(True)
                        for _ in range(args.steps):
                            cbatch.enqueue()
                            ctx.synchronize()
                        res["C_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
                        ctx.profile(False)
                    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
