"""IN-list probe: what does one sb_filter_columns_in call cost next to the two ways a caller had before it?

Per page kind and list size, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A      n chained sb_filter_columns calls through prepared batches: EQ with SET, then EQ with OR, n - 1 times
  B      sb_read_columns through a prepared batch, then torch.isin on the values, ANDed with the unpacked validity and
         packed to bits (numeric columns only)
  C      one sb_filter_columns_in call through a prepared batch
A and B run on code paths the IN call does not touch; all three see the same pages.  The pages are None, RLE, Dict and Zstd
pages of an Int64 column and Dict pages of a Utf8 column, --rows rows in pages of --page-rows, --columns columns of them per
call.  The literals are half from the column and half from outside.  C's bits are compared with A's (and B's) before
anything is timed.  Prints one JSON line per case.

  python scripts/filter_in_probe.py [--steps 10] [--warmup 2] [--rows 4000000] [--page-rows 65536] [--columns 4]
                                    [--sizes 1,8,64,1024] [--only none,rle,dict,zstd,utf8]
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
from read_selected_probe import pack_bits, timed, unpack_bits   # noqa: E402


def int_column(rows, uniq, runs):
    rng = np.random.default_rng(1)
    pool = rng.integers(-(1 << 40), 1 << 40, uniq)
    v = pool[rng.integers(0, uniq, rows // runs + 1)]
    v = np.repeat(v, runs)[:rows].astype(np.int64)
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    return dict(ptype=S.T_I64, nullable=True, rows=rows, values=v, validity=validity, offsets=None), pool


def utf8_column(rows, uniq):
    rng = np.random.default_rng(2)
    pool = [("city-%06d-%s" % (i, "x" * int(rng.integers(0, 12)))).encode() for i in range(uniq)]
    idx = rng.integers(0, uniq, rows)
    lens = np.array([len(p) for p in pool], np.int64)
    offs = np.zeros(rows + 1, np.int64)
    np.cumsum(lens[idx], out=offs[1:])
    data = np.frombuffer(b"".join(pool[int(i)] for i in idx), np.uint8).copy()
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    return dict(ptype=S.T_BIN32, nullable=True, rows=rows, values=data, validity=validity, offsets=offs.astype(np.int32)), pool


def cases(rows, page_rows):
    plain, pool = int_column(rows, 2000, 1)
    runs, rpool = int_column(rows, 2000, 64)
    yield "none", plain, pool, dict(max_page_size=page_rows, force_codec=S.NONE)
    yield "rle", runs, rpool, dict(max_page_size=page_rows, force_codec=S.RLE)
    yield "dict", plain, pool, dict(max_page_size=page_rows, force_codec=S.DICT)
    yield "zstd", plain, pool, dict(max_page_size=page_rows, force_codec=S.ZSTD)
    text, tpool = utf8_column(rows // 4, 2000)
    yield "utf8", text, tpool, dict(max_page_size=page_rows, force_codec=S.DICT)


def literals(pool, n, binary):
    """n distinct literals, half of them values of the column"""
    rng = np.random.default_rng(n)
    inside = [pool[int(i)] for i in rng.permutation(len(pool))[:min((n + 1) // 2, len(pool))]]
    out = list(inside)
    k = 0
    while len(out) < n:
        out.append(("absent-%d" % k).encode() if binary else (1 << 50) + k)
        k += 1
    return [x if binary else int(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--page-rows", type=int, default=65536)
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--sizes", default="1,8,64,1024")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.filter import FilterBatch
    from strawboat_amd.filter_in import FilterInBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    for name, col, pool, opt in cases(args.rows, args.page_rows):
        if only and name not in only:
            continue
        binary = col["ptype"] == S.T_BIN32
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      offsets=col["offsets"], options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        rows = col["rows"]
        rbatch = None if binary else read.ReadBatch(ctx, cols)
        for n in [int(x) for x in args.sizes.split(",")]:
            lits = literals(pool, n, binary)
            cbatch = FilterInBatch(ctx, cols, [sb.InList(lits)] * len(cols))
            first = FilterBatch(ctx, cols, [sb.Predicate("eq", lits[0])] * len(cols))
            chain = [first] + [FilterBatch(ctx, cols, [sb.Predicate("eq", lit)] * len(cols), combine="or", out=first.selections)
                               for lit in lits[1:]]

            def run_a():
                for b in chain:
                    b.enqueue()

            def isin_of(arrs):
                with torch.cuda.stream(ctx.torch_stream):
                    want = torch.tensor(lits, dtype=torch.int64, device=ctx.torch_device)
                    out = []
                    for a in arrs:
                        hit = torch.isin(a.values.view(torch.int64), want) & unpack_bits(torch, a.validity, rows)
                        out.append((hit, pack_bits(torch, hit)))
                    return out

            def run_b():
                return isin_of(rbatch.enqueue())

            got = cbatch.enqueue()
            run_a()
            arrs = rbatch.enqueue() if rbatch is not None else None
            # (the read's buffers are final at the synchronize: its interval may be issued a second time on a launch hint
            # that missed, and torch work queued behind the first issue would have read what that left undone)
            ctx.synchronize()
            ref_b = isin_of(arrs) if rbatch is not None else None
            what = "%s %d literals" % (name, n)
            for i, g in enumerate(got):
                a = first.selections[i]
                assert torch.equal(g.bitmap, a.bitmap), "%s: the IN call and the chain differ" % what
                if ref_b is not None:
                    assert np.array_equal(g.numpy(), ref_b[i][0].cpu().numpy()), "%s: the IN call and torch.isin differ" % what
            res = {"pages": name, "literals": n, "columns": args.columns, "rows": rows, "selected": got[0].selected,
                   "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
            res["A_chained_eq_or_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
            if rbatch is not None:
                res["B_read_then_isin_ms"] = timed(torch, ctx, run_b, args.steps, args.warmup)
            res["C_filter_in_ms"] = timed(torch, ctx, cbatch.enqueue, args.steps, args.warmup)
            res["A_over_C"] = round(res["A_chained_eq_or_ms"]["median"] / res["C_filter_in_ms"]["median"], 2)
            if rbatch is not None:
                res["B_over_C"] = round(res["B_read_then_isin_ms"]["median"] / res["C_filter_in_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
