"""Weighted aggregate probe: what does sb_aggregate_weighted cost next to what a caller does without it, and next to the
plain grouped sum over the same pages?

Per shape, selection, number of groups and id pattern, timed with events on the context's stream.  The legs of a case are
run ALTERNATELY (A, W, F, A, W, F, ...), --steps rounds after --warmup; median and min-max per leg:
  A      sb_read_selected of y through a prepared batch, the ids and the weights compacted by the same bitmap (and by the
         validity of the selected rows), the multiply and index_add_ in torch, bincount for the counts: route "A" of
         scripts/aggregate_grouped_probe.py with the weight
  W      sb_aggregate_weighted through a prepared batch (count and sum)
  F      sb_aggregate_grouped_large with count and sum on the same columns through a prepared batch: the floor, sum(y) over
         the same walk without the weight
Shapes, selections and ids are those of scripts/aggregate_grouped_large_probe.py.  The weights are one float64 (or, with
--weights i64, int64) tensor of random values per shape, shared by the columns of a call.  W's results are compared with
A's before anything is timed: counts exactly, float sums to 1e-9 of count * max|y w|, int64 x int64 sums in their low 64
bits (A's int64 arithmetic wraps; W's sum is exact).  Prints one JSON line per case.

  python scripts/aggregate_weighted_probe.py [--steps 20] [--warmup 3] [--columns 1,16] [--groups 300,1024] [--ids random,runs]
                                             [--only c1,c2] [--sel "random 0.01,random 1"] [--weights f64] [--profile]
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
from aggregate_grouped_large_probe import timed_alternately   # noqa: E402
from aggregate_grouped_probe import make_ids   # noqa: E402
from read_selected_probe import bitmap_bytes, selections, shapes, unpack_bits   # noqa: E402


def torch_weighted(torch, arr, dtype, selected, ids_sel, w_sel, n_groups, acc):
    """what a caller does today: (selected, count, sum of products) per group as device tensors; ids_sel, w_sel: the ids and
    the weights of the selected rows"""
    vals = arr.values_buf[:selected * dtype.itemsize].view(dtype)
    ids, w = ids_sel, w_sel
    sel_g = torch.bincount(ids, minlength=n_groups)
    if arr.validity_buf is not None:
        valid = unpack_bits(torch, arr.validity_buf, selected)
        vals, ids, w = vals[valid], ids[valid], w[valid]
    count = torch.bincount(ids, minlength=n_groups)
    total = torch.zeros(n_groups, dtype=acc, device=vals.device).index_add_(0, ids, vals.to(acc) * w.to(acc))
    return sel_g, count, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", default="1,16")
    ap.add_argument("--groups", default="300,1024")
    ap.add_argument("--ids", default="random,runs")
    ap.add_argument("--only", default=None)
    ap.add_argument("--sel", default="random 0.01,random 1", help="comma-separated selection names")
    ap.add_argument("--weights", default="f64", help="f64 or i64")
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the weighted call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.aggregate_grouped_large import GroupedAggregateLargeBatch
    from strawboat_amd.aggregate_weighted import WeightedAggregateBatch
    from strawboat_amd.read_selected import ReadSelectedBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I64: torch.int64, S.T_F64: torch.float64, S.T_I32: torch.int32}
    only = set(args.only.split(",")) if args.only else None
    sels = set(s.strip() for s in args.sel.split(","))
    for name, col, opt in shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        dtype = dt[col["ptype"]]
        rows = col["rows"]
        rng = np.random.default_rng(11)
        if args.weights == "i64" and not dtype.is_floating_point:
            host_w = rng.integers(-1000, 1000, rows).astype(np.int64)
            acc = torch.int64
        else:
            host_w = (1.0 + rng.random(rows)) * rng.choice([-1.0, 1.0], rows)
            acc = torch.float64
        w = torch.from_numpy(host_w).to(ctx.torch_device)
        for n_cols in [int(c) for c in args.columns.split(",")]:
            cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(n_cols)]
            for sel_name, mask in selections(rows):
                if sel_name not in sels:
                    continue
                bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
                sbatch = ReadSelectedBatch(ctx, cols, bitmap)
                selected = int(mask.sum())
                for n_groups in [int(g) for g in args.groups.split(",")]:
                    for kind in args.ids.split(","):
                        host_ids = make_ids(kind, rows, n_groups)
                        ids = torch.from_numpy(host_ids.view(np.int32)).to(ctx.torch_device)
                        ids64 = torch.from_numpy(host_ids.astype(np.int64)).to(ctx.torch_device)   # (A: what torch's scatters index with)
                        wbatch = WeightedAggregateBatch(ctx, cols, [w] * n_cols, ids, n_groups, bitmap)
                        fbatch = GroupedAggregateLargeBatch(ctx, cols, ids, n_groups, bitmap, ops=("count", "sum"))

                        def run_a():
                            arrs = sbatch.enqueue()
                            with torch.cuda.stream(ctx.torch_stream):
                                bits = unpack_bits(torch, bitmap, rows)
                                ids_sel, w_sel = ids64[bits], w[bits]
                                return [torch_weighted(torch, a, dtype, selected, ids_sel, w_sel, n_groups, acc) for a in arrs]

                        what = "%s %s %d groups %s" % (name, sel_name, n_groups, kind)
                        got = wbatch.enqueue()
                        want = run_a()
                        ctx.synchronize()
                        scale = float(np.abs(host_w).max()) * float(np.abs(np.asarray(col["values"], np.float64)).max())
                        for c in range(n_cols):
                            sel_g, count, total = (t.cpu().numpy() for t in want[c])
                            assert got[c].selected == selected and got[c].out_of_range == 0, what
                            for g, grp in enumerate(got[c].groups):
                                assert (grp.selected, grp.count) == (int(sel_g[g]), int(count[g])), "%s group %d" % (what, g)
                                if acc == torch.float64:
                                    assert abs(grp.sum - float(total[g])) <= 1e-9 * scale * max(1, grp.count), "%s group %d: sum" % (what, g)
                                else:
                                    assert int(grp._c.sum_lo) == int(total[g]) & (2 ** 64 - 1), "%s group %d: sum" % (what, g)
                        res = {"shape": name, "selection": sel_name, "columns": n_cols, "rows": rows, "selected": selected,
                               "n_groups": n_groups, "ids": kind, "weights": "i64" if acc == torch.int64 else "f64", "page_bytes": int(pages.size),
                               "steps": args.steps, "warmup": args.warmup}
                        legs = {"A_read_selected_then_torch_ms": run_a, "W_aggregate_weighted_ms": wbatch.enqueue,
                                "F_aggregate_grouped_large_sum_ms": fbatch.enqueue}
                        res.update(timed_alternately(torch, ctx, legs, args.steps, args.warmup))
                        if args.profile:
                            ctx.profile(True)
                            for _ in range(args.steps):
                                wbatch.enqueue()
                                ctx.synchronize()
                            res["W_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
                            ctx.profile(False)
                        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
