"""Substring filter probe: what do CONTAINS / ENDS_WITH of sb_filter_columns_var cost next to a read of the same pages and
next to the fixed chain of a string filter call?

Per shape and predicate, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A  sb_read_columns of the same pages: the lower bound of any read-then-search (torch has no substring search)
  F  the same filter call with "starts_with": the floor of the fixed chain (parse, plan, inflate, count)
  C  the predicate itself; with it the value bytes of the call over C's median, to hold against the 8 TB/s of HBM
Shapes: URL-like Utf8 (about 60 bytes per row, 1 M rows) as Dict pages of 64 Ki rows, Basic None and Basic LZ4; C3's zipf
column as Basic None; a column of 60 x "a" per row for the adversarial one-byte literal, which stands at every position.
Predicates on the URLs: contains with a 6-byte literal at about 1 % and about 50 % selectivity, ends_with.
Every C result (bits of the first column, `selected` of all) is compared with Python's `in` / `endswith` over the column's
own strings before anything is timed.  Prints one JSON line per shape and predicate.

  python scripts/filter_sub_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only url_none] [--profile] [--lib PATH]
--lib loads another build of the library (the per-row build, -DSB_FILTER_SUB_PER_ROW, that the scan was measured against).
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


def column_of(strings):
    lens = np.fromiter((len(s) for s in strings), np.int64, len(strings))
    offs = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(strings), np.uint8).copy()
    return dict(ptype=S.T_BIN32, nullable=False, rows=len(strings), values=data, validity=None, offsets=offs.astype(np.int32))


def url_column(rows, seed=42):
    """https://www.<host>.<tld>/<section>/<id>/<name>.<ext>: about 60 bytes per row; `google` is 1 of 100 hosts, `/items` 1 of
    2 sections, `.png` 1 of 4 extensions"""
    rng = np.random.default_rng(seed)
    hosts = [b"google"] + [b"host%02dname" % i for i in range(99)]
    tlds = [b"com", b"org", b"net", b"co.uk"]
    sections = [b"items", b"other"]
    exts = [b"png", b"html", b"jpeg", b"js"]
    h, t, s, e = (rng.integers(0, n, rows) for n in (100, 4, 2, 4))
    ident = rng.integers(0, 1_000_000, rows)
    name = rng.integers(0, 5000, rows)
    return [b"https://www.%s.%s/%s/%07d/document-%04d-final.%s" % (hosts[h[i]], tlds[t[i]], sections[s[i]], ident[i], name[i], exts[e[i]])
            for i in range(rows)]


def strings_of(col):
    o = col["offsets"].astype(np.int64)
    d = col["values"].tobytes()
    return [d[o[i]:o[i + 1]] for i in range(col["rows"])]


def shapes(rows):
    urls = url_column(rows)
    ucol = column_of(urls)
    upreds = [("contains", b"google"), ("contains", b"/items"), ("ends_with", b".png"), ("not_contains", b"google")]
    c3 = W.zipf_utf8(rows, 42)
    c3 = dict(c3, nullable=False)
    out = [("url_dict", ucol, urls, dict(max_page_size=W.PAGE, force_codec=S.DICT), upreds),
           ("url_none", ucol, urls, dict(max_page_size=W.PAGE, force_codec=S.NONE), upreds),
           ("url_lz4", ucol, urls, dict(max_page_size=W.PAGE, force_codec=S.LZ4), upreds),
           ("c3_utf8_none", c3, strings_of(c3), dict(max_page_size=W.PAGE, force_codec=S.NONE), [("contains", b"17x"), ("ends_with", b"xx")])]
    a = [b"a" * 60] * rows
    out.append(("all_a_none", column_of(a), a, dict(max_page_size=W.PAGE, force_codec=S.NONE), [("contains", b"a")]))
    return out


def host_bits(strs, op, lit):
    neg = op.startswith("not_")
    op = op[4:] if neg else op
    f = {"contains": lambda s: lit in s, "ends_with": lambda s: s.endswith(lit), "starts_with": lambda s: s.startswith(lit)}[op]
    b = np.fromiter((f(s) for s in strs), bool, len(strs))
    return ~b if neg else b


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
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the filter call (sb_ctx_profile)")
    ap.add_argument("--lib", default=None, help="another build of libstrawboat_hip.so")
    ap.add_argument("--tag", default=None, help="copied into every result line")
    args = ap.parse_args()
    import torch
    from strawboat_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    import strawboat_amd as sb
    from strawboat_amd import read
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    for name, col, strs, opt, preds in shapes(args.rows):
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      offsets=col["offsets"], options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(args.columns)]
        stage = [int(col["values"].size)] * args.columns
        batch = read.ReadBatch(ctx, cols)
        for _ in range(2):
            batch.enqueue()
            ctx.synchronize()
        a_ms = timed(torch, ctx, batch.enqueue, args.steps, args.warmup)
        for op, lit in preds:
            fbatch = sb.filter.FilterBatch(ctx, cols, [sb.Predicate(op, lit)] * args.columns, stage_capacity=stage)
            floor = sb.filter.FilterBatch(ctx, cols, [sb.Predicate("starts_with", lit)] * args.columns, stage_capacity=stage)
            sels = fbatch.enqueue()
            ctx.synchronize()
            want = host_bits(strs, op, lit)
            nb = (col["rows"] + 7) // 8
            assert np.array_equal(sels[0].bitmap[:nb].cpu().numpy(), np.packbits(want, bitorder="little")), "%s %s: bits differ from the host's" % (name, op)
            assert all(s.selected == int(want.sum()) for s in sels)
            res = {"shape": name, "op": op, "literal": lit.decode(), "columns": args.columns, "rows": col["rows"], "selected": sels[0].selected,
                   "value_bytes": int(col["values"].size), "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
            if args.tag:
                res["tag"] = args.tag
            res["A_read_ms"] = a_ms
            res["F_starts_with_ms"] = timed(torch, ctx, floor.enqueue, args.steps, args.warmup)
            res["C_filter_ms"] = timed(torch, ctx, fbatch.enqueue, args.steps, args.warmup)
            res["C_value_GBps"] = round(args.columns * col["values"].size / res["C_filter_ms"]["median"] / 1e6, 1)
            if args.profile:
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
