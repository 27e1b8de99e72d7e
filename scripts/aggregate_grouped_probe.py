"""Grouped aggregate probe: what does sb_aggregate_grouped cost next to what a caller holding a selection bitmap and a key
column does today, and next to the ungrouped sink?

Per shape, selection, number of groups and id pattern, timed with events on the context's stream (median and min-max of
--steps runs after --warmup):
  A      sb_read_selected through a prepared batch, the ids compacted by the same bitmap (and by the validity of the selected
         rows), then the torch scatter reductions a caller writes today: bincount, scatter_reduce amin / amax, index_add_
         (A is given `selected` for free, as in scripts/aggregate_probe.py)
  B      sb_aggregate_grouped through a prepared batch: selected, count, min, max and sum per group
  floor  sb_aggregate_columns through a prepared batch on the same columns: the ungrouped sink
Shapes and selections are those of scripts/read_selected_probe.py.  Ids are uint32, `random` (every lane of a wave another
group) or in `runs` of 4096 rows (a tile holds one or two groups).  --columns N puts N columns of the shape into one call;
all of them share one bitmap and one id array.  B's results are compared with A's before anything is timed (counts and
min / max exactly, integer sums modulo 2^64, the float sum to 1e-9 of count * max|x|).  Prints one JSON line per case.

  python scripts/aggregate_grouped_probe.py [--steps 20] [--warmup 3] [--columns 16] [--groups 4,256] [--ids random,runs]
                                            [--only c1,c2] [--sel "random 0.01,random 1"] [--profile]
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

RUN = 4096


def make_ids(kind, rows, n_groups):
    if kind == "random":
        return np.random.default_rng(5).integers(0, n_groups, rows).astype(np.uint32)
    return ((np.arange(rows) // RUN) % n_groups).astype(np.uint32)


def torch_grouped(torch, arr, dtype, selected, ids_sel, n_groups):
    """what a caller does today: (selected, count, min, max, sum) per group as device tensors; ids_sel: the ids of the
    selected rows"""
    vals = arr.values_buf[:selected * dtype.itemsize].view(dtype)
    ids = ids_sel
    sel_g = torch.bincount(ids, minlength=n_groups)
    if arr.validity_buf is not None:
        valid = unpack_bits(torch, arr.validity_buf, selected)
        vals, ids = vals[valid], ids[valid]
    count = torch.bincount(ids, minlength=n_groups)
    acc = torch.float64 if dtype.is_floating_point else torch.int64
    total = torch.zeros(n_groups, dtype=acc, device=vals.device).index_add_(0, ids, vals.to(acc))
    mn = torch.zeros(n_groups, dtype=dtype, device=vals.device).scatter_reduce(0, ids, vals, "amin", include_self=False)
    mx = torch.zeros(n_groups, dtype=dtype, device=vals.device).scatter_reduce(0, ids, vals, "amax", include_self=False)
    return sel_g, count, mn, mx, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--groups", default="4,256")
    ap.add_argument("--ids", default="random,runs")
    ap.add_argument("--only", default=None)
    ap.add_argument("--sel", default=None, help="comma-separated selection names (default: all)")
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the grouped call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.aggregate import AggregateBatch
    from strawboat_amd.aggregate_grouped import GroupedAggregateBatch
    from strawboat_amd.read_selected import ReadSelectedBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I64: torch.int64, S.T_F64: torch.float64, S.T_I32: torch.int32}
    only = set(args.only.split(",")) if args.only else None
    sels = set(s.strip() for s in args.sel.split(",")) if args.sel else None
    for name, col, opt in shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        dtype = dt[col["ptype"]]
        rows = col["rows"]
        for sel_name, mask in selections(rows):
            if sels and sel_name not in sels:
                continue
            bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
            sbatch = ReadSelectedBatch(ctx, cols, bitmap)
            fbatch = AggregateBatch(ctx, cols, bitmap)
            selected = int(mask.sum())
            floor = None
            for n_groups in [int(g) for g in args.groups.split(",")]:
                for kind in args.ids.split(","):
                    host_ids = make_ids(kind, rows, n_groups)
                    ids = torch.from_numpy(host_ids).to(ctx.torch_device)
                    ids64 = torch.from_numpy(host_ids.astype(np.int64)).to(ctx.torch_device)   # (A: what torch's scatters index with)
                    gbatch = GroupedAggregateBatch(ctx, cols, ids, n_groups, bitmap)

                    def run_a():
                        arrs = sbatch.enqueue()
                        with torch.cuda.stream(ctx.torch_stream):
                            ids_sel = ids64[unpack_bits(torch, bitmap, rows)]
                            return [torch_grouped(torch, a, dtype, selected, ids_sel, n_groups) for a in arrs]

                    ref = run_a()
                    got = gbatch.enqueue()
                    ctx.synchronize()
                    what = "%s %s %d groups %s" % (name, sel_name, n_groups, kind)
                    for (rsel, rcnt, rmin, rmax, rsum), g in zip(ref, got):
                        assert g.selected == selected and g.out_of_range == 0, what
                        assert [x.selected for x in g.groups] == rsel.tolist(), "%s: selected differs" % what
                        assert [x.count for x in g.groups] == rcnt.tolist(), "%s: count differs" % what
                        rmin, rmax, rsum = rmin.tolist(), rmax.tolist(), rsum.tolist()
                        for i, x in enumerate(g.groups):
                            if x.count == 0:
                                assert x.min is None and x.max is None, what
                                continue
                            assert x.min == rmin[i] and x.max == rmax[i], "%s: min / max differ" % what
                            if dtype.is_floating_point:
                                assert abs(x.sum - rsum[i]) <= 1e-9 * max(abs(x.min), abs(x.max)) * x.count, "%s: sum differs" % what
                            else:
                                assert x.sum % (1 << 64) == rsum[i] % (1 << 64), "%s: sum differs" % what
                    res = {"shape": name, "selection": sel_name, "columns": args.columns, "rows": rows, "selected": selected,
                           "n_groups": n_groups, "ids": kind, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
                    res["A_read_selected_then_torch_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
                    res["B_aggregate_grouped_ms"] = timed(torch, ctx, gbatch.enqueue, args.steps, args.warmup)
                    if floor is None:
                        floor = timed(torch, ctx, fbatch.enqueue, args.steps, args.warmup)
                    res["floor_aggregate_columns_ms"] = floor
                    if args.profile:
                        ctx.profile(True)
                        for _ in range(args.steps):
                            gbatch.enqueue()
                            ctx.synchronize()
                        res["B_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
                        ctx.profile(False)
                    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
