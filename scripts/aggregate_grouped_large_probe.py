"""Large grouped aggregate probe: what does sb_aggregate_grouped_large cost next to what an engine with 257 .. 1024 groups
could do without it?

Per shape, selection, number of groups and id pattern, timed with events on the context's stream.  The legs of a case are
run ALTERNATELY (A, L, B4, A, L, B4, ...), --steps rounds after --warmup; median and min-max per leg:
  A      sb_read_selected through a prepared batch, the ids compacted by the same bitmap (and by the validity of the selected
         rows), then torch scatter reductions: bincount, scatter_reduce amin / amax, index_add_
  B4     ceil(n_groups / 256) sb_aggregate_grouped calls through prepared batches over the same pages, call j with the ids
         shifted by 256 j (torch, INSIDE the timed region: the ids 256 j .. 256 j + 255 become 0 .. 255, the rest wrap out
         of range).  What an engine can do with the 256-group call alone: the yardstick
  L      sb_aggregate_grouped_large through a prepared batch
With 256 groups the case times G, sb_aggregate_grouped itself, against L instead of B4 (reported, not gated).
Shapes are those of scripts/read_selected_probe.py (C1, C2, Dict, LZ4).  Ids are int32 (the unsigned bits), `random` or in
`runs` of 4096 rows.  L's results are compared with B4's (or G's) before anything is timed: counts and min / max exactly,
integer sums exactly, float sums to 1e-9 of count * max|x|.  Prints one JSON line per case.

  python scripts/aggregate_grouped_large_probe.py [--steps 20] [--warmup 3] [--columns 1,16] [--groups 256,300,1024]
                                                  [--ids random,runs] [--only c1,c2] [--sel "random 0.01,random 1"] [--profile]
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
from aggregate_grouped_probe import make_ids, torch_grouped   # noqa: E402
from read_selected_probe import bitmap_bytes, selections, shapes, unpack_bits   # noqa: E402


def timed_alternately(torch, ctx, legs, steps, warmup):
    """legs: {name: fn}.  One round runs every leg once, in order, each between two events and ended by a synchronize."""
    ms = {name: [] for name in legs}
    for it in range(warmup + steps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.torch_stream)
            fn()
            e1.record(ctx.torch_stream)
            ctx.synchronize()
            if it >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {name: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for name, v in ms.items()}


def same(a, b, floating, what):
    """two lists of Group: counts and min / max exactly, integer sums exactly, float sums closely"""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x.selected, x.count, x.nans, x.min_bytes, x.max_bytes) == (y.selected, y.count, y.nans, y.min_bytes, y.max_bytes), "%s group %d" % (what, i)
        if floating and x.count:
            assert abs(x.sum - y.sum) <= 1e-9 * max(abs(x.min), abs(x.max)) * x.count, "%s group %d: sum" % (what, i)
        else:
            assert x.sum == y.sum, "%s group %d: sum" % (what, i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", default="1,16")
    ap.add_argument("--groups", default="256,300,1024")
    ap.add_argument("--ids", default="random,runs")
    ap.add_argument("--only", default=None)
    ap.add_argument("--sel", default="random 0.01,random 1", help="comma-separated selection names")
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the large call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.aggregate_grouped import GroupedAggregateBatch
    from strawboat_amd.aggregate_grouped_large import GroupedAggregateLargeBatch
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
                        lbatch = GroupedAggregateLargeBatch(ctx, cols, ids, n_groups, bitmap)
                        calls = (n_groups + 255) // 256
                        shifted = [torch.empty_like(ids) for _ in range(calls)]
                        bbatches = [GroupedAggregateBatch(ctx, cols, shifted[j], min(256, n_groups - 256 * j), bitmap) for j in range(calls)]

                        def run_a():
                            arrs = sbatch.enqueue()
                            with torch.cuda.stream(ctx.torch_stream):
                                ids_sel = ids64[unpack_bits(torch, bitmap, rows)]
                                return [torch_grouped(torch, a, dtype, selected, ids_sel, n_groups) for a in arrs]

                        def run_b4():
                            out = []
                            for j in range(calls):
                                with torch.cuda.stream(ctx.torch_stream):
                                    torch.sub(ids, 256 * j, out=shifted[j])   # (int32 arithmetic: an id below 256 j wraps to >= 2^31)
                                out.append(bbatches[j].enqueue())
                            return out

                        what = "%s %s %d groups %s" % (name, sel_name, n_groups, kind)
                        got = lbatch.enqueue()
                        parts = run_b4()
                        ctx.synchronize()
                        for c in range(n_cols):
                            merged = [g for j in range(calls) for g in parts[j][c].groups]
                            assert got[c].selected == selected and got[c].out_of_range == 0, what
                            same(got[c].groups, merged, dtype.is_floating_point, what)
                        res = {"shape": name, "selection": sel_name, "columns": n_cols, "rows": rows, "selected": selected,
                               "n_groups": n_groups, "ids": kind, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup,
                               "B4_calls": calls}
                        legs = {"A_read_selected_then_torch_ms": run_a, "L_aggregate_grouped_large_ms": lbatch.enqueue}
                        if calls == 1:   # (256 groups: the old call itself, its ids as they are)
                            legs["G_aggregate_grouped_ms"] = bbatches[0].enqueue
                        else:
                            legs["B4_shifted_aggregate_grouped_ms"] = run_b4
                        res.update(timed_alternately(torch, ctx, legs, args.steps, args.warmup))
                        if args.profile:
                            ctx.profile(True)
                            for _ in range(args.steps):
                                lbatch.enqueue()
                                ctx.synchronize()
                            res["L_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
                            ctx.profile(False)
                        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
