"""Column-against-column probe: what does sb_filter_columns_cmp cost next to what an engine does today for `WHERE a < b`?

Per shape, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  B   sb_read_columns of BOTH columns, then a torch compare of the decoded values, AND with both validities, packed to one
      bit per row (the alternative an engine has today)
  C   sb_filter_columns_cmp of the left column's pages with the operand already on the device (decoded before the clock
      starts: the operand is a column the engine holds anyway, or an expression it computed)
  P   filter_pair: sb_read_columns of the right column into device buffers, then the comparison of the left pages
      against them, in one interval -- the read of `right` included
Shapes: Int32 dates (`l_commitdate < l_receiptdate`: right = left + 0 .. 60 days), Int64 and Float64, with the LEFT column in
None / RLE / Dict / LZ4 pages; the right column is always in plain pages.  --columns N puts N pairs into one call.
Every C and P bitmap is compared with B's before anything is timed.  Prints one JSON line per shape.

  python scripts/filter_cmp_probe.py [--steps 20] [--warmup 3] [--rows 1000000] [--columns 16] [--only int32,float64_rle]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import workloads as W   # noqa: E402
from oracle import sbo as S   # noqa: E402

CODECS = (("none", S.NONE), ("rle", S.RLE), ("dict", S.DICT), ("lz4", S.LZ4))


def pair(kind, rows, seed):
    """(left, right) column dicts: left in runs of 8 out of 1000 values (so that RLE and Dict pages are what a writer would
    pick), right = left plus a small delta that is 0 in a third of the rows; 10 % nulls on the left, 5 % on the right"""
    rng = np.random.default_rng(seed)
    base = np.repeat(rng.integers(0, 1000, rows // 8 + 1), 8)[:rows]
    delta = np.where(rng.random(rows) < 0.33, 0, rng.integers(-30, 60, rows))
    if kind == "int32":
        left, right, pt = (8000 + base).astype(np.int32), (8000 + base + delta).astype(np.int32), S.T_I32
    elif kind == "int64":
        left, right, pt = (base.astype(np.int64) << 20), ((base + delta).astype(np.int64) << 20), S.T_I64
    else:
        left, right, pt = base * 0.25, (base + delta) * 0.25, S.T_F64
    lv = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    rv = np.packbits(rng.random(rows) < 0.95, bitorder="little")
    return (dict(ptype=pt, nullable=True, rows=rows, values=np.ascontiguousarray(left), validity=lv, offsets=None),
            dict(ptype=pt, nullable=True, rows=rows, values=np.ascontiguousarray(right), validity=rv, offsets=None))


def write(col, **opt):
    return S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"], options=S.make_options(**opt))


def torch_compare(torch, a, b, dtype):
    """what a caller does today: compare the decoded values, AND with both validities, pack to bits"""
    m = a.values.view(dtype) < b.values.view(dtype)
    rows = m.numel()
    pad = (-rows) % 8
    if pad:
        m = torch.cat([m, torch.zeros(pad, dtype=torch.bool, device=m.device)])
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=m.device)
    bits = (m.view(-1, 8).to(torch.uint8) * w).sum(dim=1, dtype=torch.uint8)
    for arr in (a, b):
        if arr.validity is not None:
            bits = bits & arr.validity[:bits.numel()]
    return bits


def timed(torch, ctx, fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.torch_stream)
        fn()
        e1.record(ctx.torch_stream)
        ctx.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I32: torch.int32, S.T_I64: torch.int64, S.T_F64: torch.float64}
    only = set(args.only.split(",")) if args.only else None
    n = args.columns
    for kind in ("int32", "int64", "float64"):
        left, right = pair(kind, args.rows, 7)
        rpages, rmetas = write(right, max_page_size=W.PAGE, force_codec=S.NONE)
        rdev = torch.from_numpy(np.ascontiguousarray(rpages)).to(ctx.torch_device)
        rcols = [read.ColumnPages(right["ptype"], True, rdev, rmetas) for _ in range(n)]
        for cname, codec in CODECS:
            name = "%s_%s" % (kind, cname)
            if only and not any(name.startswith(o) for o in only):
                continue
            lpages, lmetas = write(left, max_page_size=W.PAGE, force_codec=codec)
            ldev = torch.from_numpy(np.ascontiguousarray(lpages)).to(ctx.torch_device)
            lcols = [read.ColumnPages(left["ptype"], True, ldev, lmetas) for _ in range(n)]
            both = read.ReadBatch(ctx, lcols + rcols)
            right_only = read.ReadBatch(ctx, rcols)
            for _ in range(2):   # (the reads settle their launch hints before torch kernels are put behind them: filter_probe.py)
                both.enqueue()
                ctx.synchronize()
                operands = right_only.enqueue()
                ctx.synchronize()
            cbatch = sb.FilterCmpBatch(ctx, lcols, "lt", operands)
            pbatch = sb.FilterCmpBatch(ctx, lcols, "lt", right_only.arrays)

            def run_b():
                arrs = both.enqueue()
                with torch.cuda.stream(ctx.torch_stream):
                    return [torch_compare(torch, arrs[i], arrs[n + i], dt[left["ptype"]]) for i in range(n)]

            def run_c():
                return cbatch.enqueue()

            def run_p():
                right_only.enqueue()
                return pbatch.enqueue()

            ref = run_b()
            ctx.synchronize()
            nb = (args.rows + 7) // 8
            for fn in (run_c, run_p):
                sels = fn()
                ctx.synchronize()
                for r, s in zip(ref, sels):
                    assert torch.equal(r[:nb], s.bitmap[:nb]), "%s: the call and the torch expression differ" % name
            res = {"shape": name, "columns": n, "rows": args.rows, "selected": sels[0].selected,
                   "left_page_bytes": int(lpages.size), "right_page_bytes": int(rpages.size), "steps": args.steps, "warmup": args.warmup}
            for key, fn in (("B_read_both_then_torch", run_b), ("C_cmp_operand_on_device", run_c), ("P_filter_pair", run_p)):
                res[key + "_ms"] = timed(torch, ctx, fn, args.steps, args.warmup)
            res["B_over_C"] = round(res["B_read_both_then_torch_ms"]["median"] / res["C_cmp_operand_on_device_ms"]["median"], 2)
            res["B_over_P"] = round(res["B_read_both_then_torch_ms"]["median"] / res["P_filter_pair_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
