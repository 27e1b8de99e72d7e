"""Top-k probe: what does sb_topk_columns cost next to what a caller holding a selection bitmap does today, and next to
the floor of one walk of the same pages?

Per shape, k and selection, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  T  sb_topk_columns through a prepared batch, LARGEST
  A  sb_read_selected through a prepared batch, then torch.topk over values[valid] of its output
     (A is given `selected` for free: a real caller learns it at a synchronize of its own before it can slice the output;
     and A has no row numbers: it could not fetch the winners' other columns)
  B  sb_aggregate_columns with `min` alone: one walk of the same pages that keeps one value, the floor of T
Shapes: C1 and C2 of workloads.py (1 M-row Int64 in one plain page; 1 M-row nullable Float64 in RLE pages), at k = 10 and
256 under random selections of 0.01 / 0.5 / 1.0.  --columns N puts N columns of the shape into one call; all of them share
one bitmap.  One adversarial shape: an Int64 column sorted ascending, asked for LARGEST with every row selected, so that
every step of every tile beats the bound and the buffer is pruned as often as it can be.
T's values are compared with A's before anything is timed (the winners' values, as a sorted multiset: A has no rows).
Prints one JSON line per shape, k and selection; --profile adds the per-kernel split of T from sb_ctx_profile.

  python scripts/topk_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only c1,c2,sorted] [--profile]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import workloads as W   # noqa: E402
from oracle import sbo as S   # noqa: E402
from read_selected_probe import bitmap_bytes, timed, unpack_bits   # noqa: E402

KS = (10, 256)
SELECTIVITIES = (0.01, 0.5, 1.0)


def shapes():
    c1 = W.c1_int64()
    c2 = W.c2_float64()
    asc = dict(ptype=S.T_I64, nullable=False, rows=1_000_000, values=np.arange(1_000_000, dtype=np.int64) * 3 - 7, validity=None, offsets=None)
    return [("c1_int64_none", c1, dict(force_codec=S.NONE), SELECTIVITIES),
            ("c2_float64_rle", c2, dict(max_page_size=W.PAGE, force_codec=S.RLE), SELECTIVITIES),
            ("sorted_int64_against_the_order", asc, dict(max_page_size=W.PAGE, force_codec=S.NONE), (1.0,))]


def torch_topk(torch, arr, dtype, selected, k):
    """what a caller does today with the selected rows of a column: the k largest values (no row numbers)"""
    vals = arr.values_buf[:selected * dtype.itemsize].view(dtype)
    if arr.validity_buf is not None:
        vals = vals[unpack_bits(torch, arr.validity_buf, selected)]
    if dtype.is_floating_point:
        vals = vals[~torch.isnan(vals)]
    return torch.topk(vals, min(k, vals.numel()), largest=True, sorted=True).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the top-k call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.aggregate import AggregateBatch
    from strawboat_amd.read_selected import ReadSelectedBatch
    from strawboat_amd.topk import TopKBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I64: torch.int64, S.T_F64: torch.float64}
    only = set(args.only.split(",")) if args.only else None
    for name, col, opt, ps in shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        dtype = dt[col["ptype"]]
        rng = np.random.default_rng(11)
        for p in ps:
            mask = rng.random(col["rows"]) < p if p < 1.0 else np.ones(col["rows"], bool)
            bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
            selected = int(mask.sum())
            sbatch = ReadSelectedBatch(ctx, cols, bitmap)
            abatch = AggregateBatch(ctx, cols, bitmap, ops=("min",))
            for k in KS:
                tbatch = TopKBatch(ctx, cols, k, True, bitmap)

                def run_a():
                    arrs = sbatch.enqueue()
                    with torch.cuda.stream(ctx.torch_stream):
                        return [torch_topk(torch, a, dtype, selected, k) for a in arrs]

                ref = run_a()
                got = tbatch.enqueue()
                ctx.synchronize()
                for r, g in zip(ref, got):
                    assert g.selected == selected and np.array_equal(g.values, r.cpu().numpy()), "%s k %d p %g: the winners differ" % (name, k, p)
                res = {"shape": name, "k": k, "selectivity": p, "columns": args.columns, "rows": col["rows"], "selected": selected,
                       "found": got[0].found, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
                res["T_topk_ms"] = timed(torch, ctx, tbatch.enqueue, args.steps, args.warmup)
                res["A_read_selected_then_torch_topk_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
                res["B_aggregate_min_ms"] = timed(torch, ctx, abatch.enqueue, args.steps, args.warmup)
                if args.profile:
                    ctx.profile(True)
                    for _ in range(args.steps):
                        tbatch.enqueue()
                        ctx.synchronize()
                    res["T_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
                    ctx.profile(False)
                print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
