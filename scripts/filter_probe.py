"""Filter probe: what does sb_filter_columns cost next to the two ways a caller gets a selection today?

Per shape, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A  sb_read_columns alone
  B  A, then a plain torch compare of the decoded values, AND with the validity, packed to one bit per row
     (what a caller without the filter call does)
  C  sb_filter_columns
Shapes: C1 (1 M-row Int64, one plain page), C1 as Float64, C2 (1 M-row nullable Float64, RLE pages), a Dict Int32 column
and an LZ4 Int64 column (the staged path).  --columns N puts N columns of the shape into one call.
Every C result is compared with B's before anything is timed.  Prints one JSON line per shape.
Binary shapes (sb_filter_columns_var, `s <= literal` on C3's zipf Utf8, 1 M rows): Dict pages of 64 Ki rows, the same
column as one long Dict page, Basic None and Basic LZ4 pages.  torch has no string compare, so they have no leg B: A alone
is a lower bound for any read-then-compare.  C's bitmap is checked against a host-side compare of A's output first.

  python scripts/filter_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only c1,c2]
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


def shapes():
    rng = np.random.default_rng(7)
    c1 = W.c1_int64()
    c1f = dict(c1, ptype=S.T_F64, values=rng.random(c1["rows"]) * 1000.0)
    c2 = W.c2_float64()
    d = dict(ptype=S.T_I32, nullable=False, rows=1_000_000, values=rng.integers(0, 1000, 1_000_000).astype(np.int32), validity=None, offsets=None)
    z = dict(ptype=S.T_I64, nullable=False, rows=1_000_000, values=np.repeat(rng.integers(0, 1 << 40, 125_000), 8).astype(np.int64),
             validity=None, offsets=None)
    return [("c1_int64_none", c1, dict(force_codec=S.NONE), int(np.median(c1["values"]))),
            ("c1_float64_none", c1f, dict(force_codec=S.NONE), 500.0),
            ("c2_float64_rle", c2, dict(max_page_size=W.PAGE, force_codec=S.RLE), 128.0),
            ("dict_int32", d, dict(max_page_size=W.PAGE, force_codec=S.DICT), 500),
            ("lz4_int64", z, dict(max_page_size=W.PAGE, force_codec=S.LZ4), 1 << 39)]


def binary_shapes():
    c3 = W.zipf_utf8(1_000_000, 42)
    o = c3["offsets"].astype(np.int64)
    d = c3["values"].tobytes()
    lit = sorted(set(d[o[i]:o[i + 1]] for i in range(0, 20_000)))[40]   # among the frequent words: selects a good part of the rows
    return [("c3_utf8_dict", c3, dict(max_page_size=W.PAGE, force_codec=S.DICT), lit),
            ("c3_utf8_dict_one_page", c3, dict(force_codec=S.DICT), lit),
            ("c3_utf8_none", c3, dict(max_page_size=W.PAGE, force_codec=S.NONE), lit),
            ("c3_utf8_lz4", c3, dict(max_page_size=W.PAGE, force_codec=S.LZ4), lit)]


def host_compare_le(arr, lit, rows):
    """`value <= lit` per row of a decoded binary column, on the host (the distinct values once), packed LSB-first"""
    offs = arr.offsets_numpy().view(np.int32).astype(np.int64)
    data = arr.values_numpy().tobytes()
    memo, out = {}, np.zeros(rows, bool)
    for i in range(rows):
        v = data[offs[i]:offs[i + 1]]
        r = memo.get(v)
        if r is None:
            r = memo[v] = v <= lit
        out[i] = r
    return np.packbits(out, bitorder="little")


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


def torch_filter(torch, arr, dtype, lit):
    """what a caller does today: compare the decoded values, AND with the validity, pack to bits"""
    v = arr.values.view(dtype)
    m = v < lit
    rows = m.numel()
    pad = (-rows) % 8
    if pad:
        m = torch.cat([m, torch.zeros(pad, dtype=torch.bool, device=m.device)])
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=m.device)
    bits = (m.view(-1, 8).to(torch.uint8) * w).sum(dim=1, dtype=torch.uint8)
    if arr.validity is not None:
        bits = bits & arr.validity[:bits.numel()]
    return bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="binary shapes: per-kernel times of the filter call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    dt = {S.T_I64: torch.int64, S.T_F64: torch.float64, S.T_I32: torch.int32}
    only = set(args.only.split(",")) if args.only else None
    for name, col, opt, lit in shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        preds = [sb.Predicate("lt", lit)] * args.columns
        batch = read.ReadBatch(ctx, cols)
        fbatch = sb.filter.FilterBatch(ctx, cols, preds)
        sels = fbatch.enqueue()
        ctx.synchronize()
        # B puts torch kernels of its own behind the read call: they must not run in an interval that the library issues a
        # second time (a read call whose launch hints miss after a change of shape), so the reads settle first.  (A filter
        # call has no such hazard: when its interval is issued again it is issued again in its place.)
        for _ in range(2):
            batch.enqueue()
            ctx.synchronize()

        def run_a():
            batch.enqueue()

        def run_b():
            arrs = batch.enqueue()
            with torch.cuda.stream(ctx.torch_stream):
                return [torch_filter(torch, a, dt[col["ptype"]], lit) for a in arrs]

        def run_c():
            fbatch.enqueue()

        ref = run_b()
        ctx.synchronize()
        nb = (col["rows"] + 7) // 8
        for r, s in zip(ref, sels):
            assert torch.equal(r[:nb], s.bitmap[:nb]), "%s: the filter call and the torch expression differ" % name
        res = {"shape": name, "columns": args.columns, "rows": col["rows"], "selected": sels[0].selected,
               "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
        for key, fn in (("A_read", run_a), ("B_read_then_torch", run_b), ("C_filter", run_c)):
            ms = []
            for it in range(args.warmup + args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ctx.torch_stream)
                fn()
                e1.record(ctx.torch_stream)
                ctx.synchronize()
                if it >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            res[key + "_ms"] = {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        print(json.dumps(res), flush=True)
    for name, col, opt, lit in binary_shapes():
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      offsets=col["offsets"], options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        batch = read.ReadBatch(ctx, cols)
        fbatch = sb.filter.FilterBatch(ctx, cols, [sb.Predicate("le", lit)] * args.columns)
        for _ in range(2):
            arrs = batch.enqueue()
            ctx.synchronize()
        want = host_compare_le(arrs[0], lit, col["rows"])
        sels = fbatch.enqueue()
        ctx.synchronize()
        nb = (col["rows"] + 7) // 8
        for s in sels:
            assert np.array_equal(s.bitmap[:nb].cpu().numpy(), want), "%s: the filter call and the host compare differ" % name
        res = {"shape": name, "columns": args.columns, "rows": col["rows"], "selected": sels[0].selected,
               "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
        res["A_read_ms"] = timed(torch, ctx, batch.enqueue, args.steps, args.warmup)
        res["C_filter_ms"] = timed(torch, ctx, fbatch.enqueue, args.steps, args.warmup)
        if args.profile:   # per-kernel times of the filter call alone
            ctx.profile(True)
            for _ in range(args.steps):
                fbatch.enqueue()
                ctx.synchronize()
            res["C_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
            ctx.profile(False)
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
