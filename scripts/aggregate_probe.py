"""Aggregate probe: what does sb_aggregate_columns cost next to what a caller holding a selection bitmap does today?

Per shape and selection, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A  sb_read_selected through a prepared batch, then the torch reductions a caller writes today over its output: the
     validity bits of the selected rows unpacked, values[valid], and count / min / max / sum of those
     (A is given `selected` for free: a real caller learns it at a synchronize of its own before it can slice the output)
  B  sb_aggregate_columns through a prepared batch: count, min, max and sum
Shapes and selections are those of scripts/read_selected_probe.py: C1 (1 M-row Int64, one plain page), C2 (1 M-row
nullable Float64, RLE pages), a Dict Int32 column and an LZ4 Int64 column (the staged path); random bits at 0.001 / 0.01 /
0.1 / 0.5 / 1.0, and 0.01 clustered.  --columns N puts N columns of the shape into one call; all of them share one bitmap.
B's results are compared with A's before anything is timed (integers exactly, the float sum to 1e-9 of sum|x|).
Prints one JSON line per shape and selection.

  python scripts/aggregate_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only c1,c2] [--profile]
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
from read_selected_probe import bitmap_bytes, selections, shapes, timed, unpack_bits   # noqa: E402


def torch_reduce(torch, arr, dtype, selected):
    """what a caller does today with the selected rows of a column: (count, min, max, sum) as device scalars"""
    vals = arr.values_buf[:selected * dtype.itemsize].view(dtype)
    if arr.validity_buf is not None:
        vals = vals[unpack_bits(torch, arr.validity_buf, selected)]
    count = torch.tensor(vals.numel(), device=vals.device)
    if vals.numel() == 0:
        return count, None, None, None
    total = vals.sum(dtype=torch.float64) if dtype.is_floating_point else vals.sum(dtype=torch.int64)
    return count, vals.min(), vals.max(), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the aggregate call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.aggregate import AggregateBatch
    from strawboat_amd.read_selected import ReadSelectedBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I64: torch.int64, S.T_F64: torch.float64, S.T_I32: torch.int32}
    only = set(args.only.split(",")) if args.only else None
    for name, col, opt in shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        dtype = dt[col["ptype"]]
        for sel_name, mask in selections(col["rows"]):
            bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
            sbatch = ReadSelectedBatch(ctx, cols, bitmap)
            abatch = AggregateBatch(ctx, cols, bitmap)
            selected = int(mask.sum())

            def run_a():
                arrs = sbatch.enqueue()
                with torch.cuda.stream(ctx.torch_stream):
                    return [torch_reduce(torch, a, dtype, selected) for a in arrs]

            ref = run_a()
            got = abatch.enqueue()
            ctx.synchronize()
            for (rc, rmin, rmax, rsum), g in zip(ref, got):
                what = "%s %s" % (name, sel_name)
                assert g.selected == selected and g.count == int(rc), "%s: count differs" % what
                if rmin is None:
                    assert g.min is None and g.max is None, what
                    continue
                assert g.min == rmin.item() and g.max == rmax.item(), "%s: min / max differ" % what
                if dtype.is_floating_point:
                    assert abs(g.sum - rsum.item()) <= 1e-9 * max(abs(g.min), abs(g.max)) * g.count, "%s: sum differs" % what
                else:
                    assert g.sum % (1 << 64) == rsum.item() % (1 << 64), "%s: sum differs" % what
            res = {"shape": name, "selection": sel_name, "columns": args.columns, "rows": col["rows"], "selected": selected,
                   "count": got[0].count, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
            res["A_read_selected_then_torch_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
            res["A_read_selected_alone_ms"] = timed(torch, ctx, sbatch.enqueue, args.steps, args.warmup)
            res["B_aggregate_ms"] = timed(torch, ctx, abatch.enqueue, args.steps, args.warmup)
            if args.profile:
                ctx.profile(True)
                for _ in range(args.steps):
                    abatch.enqueue()
                    ctx.synchronize()
                res["B_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
                ctx.profile(False)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
