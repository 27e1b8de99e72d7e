"""Key-lookup probe: what does one sb_key_lookup call cost next to what an engine did before it to turn a key column
into the ids of a given list (a join against a small dimension, GROUP BY over a known key set), and next to the
discovering calls sb_key_ids / sb_key_ids_var on the same pages?

Per key type, page kind and list length, timed on the context's stream (median and min-max of --steps runs after
--warmup; device events, except where a path goes through the host, which is timed with the host's clock around its
synchronizes):
  A      Int64: sb_read_columns through a prepared batch, then torch.searchsorted over the sorted list and an equality
         mask on the device: an id per row, -1 where the row is null or its value is not in the list
         Utf8:  sb_read_columns, offsets and bytes copied to the host, np.searchsorted over the sorted list there and
         the ids copied back (the keys are 8 bytes each, so the host sees them as one fixed-width array: the cheapest
         form of that round trip)
  B      one sb_key_ids / sb_key_ids_var call through a prepared batch (max_keys 1024, ids of two bytes): it discovers
         the keys instead of being given them, and is unchanged by this call's arrival: the yardstick
  C      one sb_key_lookup call through a prepared batch (ids of two bytes)
All three see the same pages.  The column has --rows rows of 1024 distinct keys (10 % nulls) in pages of --page-rows:
plain, Dict and RLE (runs of 64) pages of Int64 keys, plain and Dict pages of Utf8 keys.  The list is the first 8 / 256 /
1024 of the keys in a random order.  C's ids are compared with A's before anything is timed.  Prints one JSON line per
case; --profile adds the per-kernel split of B and C from sb_ctx_profile.

  python scripts/key_lookup_probe.py [--steps 20] [--warmup 3] [--rows 4000000] [--page-rows 65536] [--lists 8,256,1024]
                                     [--only int64,utf8] [--profile]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import sbo as S   # noqa: E402
from read_selected_probe import timed, unpack_bits   # noqa: E402

DISTINCT = 1024


def int_column(rows, runs):
    rng = np.random.default_rng(runs)
    pool = np.unique(rng.integers(-(1 << 40), 1 << 40, 2 * DISTINCT))[:DISTINCT]
    v = np.repeat(pool[rng.integers(0, DISTINCT, rows // runs + 1)], runs)[:rows].astype(np.int64)
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    return dict(ptype=S.T_I64, nullable=True, rows=rows, values=v, validity=validity, offsets=None), pool.astype(np.int64)


def str_column(rows):
    rng = np.random.default_rng(5)
    pool = np.array([b"k%07d" % i for i in rng.permutation(10_000_000)[:DISTINCT]], "S8")
    v = pool[rng.integers(0, DISTINCT, rows)]
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    col = dict(ptype=S.T_BIN32, nullable=True, rows=rows, values=np.frombuffer(v.tobytes(), np.uint8).copy(), validity=validity,
               offsets=(np.arange(rows + 1, dtype=np.int64) * 8).astype(np.int32))
    return col, pool


def cases(rows, page_rows, only):
    if not only or "int64" in only:
        for name, runs, codec in (("plain", 1, S.NONE), ("dict", 1, S.DICT), ("rle", 64, S.RLE)):
            col, pool = int_column(rows, runs)
            yield "int64", name, col, pool, dict(max_page_size=page_rows, force_codec=codec)
    if not only or "utf8" in only:
        col, pool = str_column(rows)
        for name, codec in (("plain", S.NONE), ("dict", S.DICT)):
            yield "utf8", name, col, pool, dict(max_page_size=page_rows, force_codec=codec)


def host_timed(ctx, fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--page-rows", type=int, default=65536)
    ap.add_argument("--lists", default="8,256,1024")
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the key-id and the lookup call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.key_ids import KeyIdsBatch
    from strawboat_amd.key_ids_var import KeyIdsVarBatch
    from strawboat_amd.key_lookup import KeyLookupBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    rows = args.rows
    for ktype, name, col, pool, opt in cases(rows, args.page_rows, only):
        pages, metas = S.write_column(col["ptype"], col["nullable"], rows, col["values"], validity=col["validity"], offsets=col["offsets"],
                                      options=S.make_options(**opt))
        dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
        cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas)]
        rbatch = read.ReadBatch(ctx, cols)
        bbatch = KeyIdsBatch(ctx, cols, None, 1024, 2) if ktype == "int64" else KeyIdsVarBatch(ctx, cols, None, 1024, 2)
        for n_values in [int(x) for x in args.lists.split(",")]:
            lst = pool[np.random.default_rng(n_values).permutation(DISTINCT)[:n_values]]
            order = np.argsort(lst, kind="stable")
            cbatch = KeyLookupBatch(ctx, cols, [lst if ktype == "int64" else [bytes(x) for x in lst.tolist()]], None, None, 2)
            if ktype == "int64":
                sorted_dev = torch.from_numpy(lst[order]).to(ctx.torch_device)
                ids_of_dev = torch.from_numpy(order.astype(np.int32)).to(ctx.torch_device)

                def run_a():
                    a = rbatch.enqueue()[0]
                    with torch.cuda.stream(ctx.torch_stream):
                        vals = a.values.view(torch.int64)[:rows]
                        pos = torch.searchsorted(sorted_dev, vals).clamp_(max=n_values - 1)
                        hit = (sorted_dev[pos] == vals) & unpack_bits(torch, a.validity, rows)
                        return torch.where(hit, ids_of_dev[pos], torch.full_like(ids_of_dev[pos], -1))

                time_a = lambda: timed(torch, ctx, run_a, args.steps, args.warmup)   # noqa: E731
            else:
                sorted_host = lst[order]

                def run_a():
                    a = rbatch.enqueue()[0]
                    ctx.synchronize()
                    vals = a.values[:rows * 8].cpu().numpy().view("S8")   # (the probe's keys are 8 bytes each)
                    valid = np.unpackbits(a.validity[:(rows + 7) // 8].cpu().numpy(), bitorder="little")[:rows].astype(bool)
                    pos = np.minimum(np.searchsorted(sorted_host, vals), n_values - 1)
                    ids = np.where((sorted_host[pos] == vals) & valid, order[pos], -1).astype(np.int32)
                    return torch.from_numpy(ids).to(ctx.torch_device)

                time_a = lambda: host_timed(ctx, run_a, args.steps, args.warmup)   # noqa: E731
            want = run_a()
            got = cbatch.enqueue()[0]
            ctx.synchronize()
            mine = got.ids.view(torch.int16).to(torch.int32) & 0xFFFF
            mine = torch.where(mine == 0xFFFF, torch.full_like(mine, -1), mine)
            what = "%s %s, %d values" % (ktype, name, n_values)
            assert torch.equal(mine, want.to(torch.int32)), "%s: the ids differ" % what
            res = {"keys": ktype, "pages": name, "n_values": n_values, "rows": rows, "count": got.count, "matched": got.matched,
                   "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
            res["A_read_then_searchsorted_ms"] = time_a()
            res["B_key_ids_ms"] = timed(torch, ctx, bbatch.enqueue, args.steps, args.warmup)
            res["C_key_lookup_ms"] = timed(torch, ctx, cbatch.enqueue, args.steps, args.warmup)
            res["A_over_C"] = round(res["A_read_then_searchsorted_ms"]["median"] / res["C_key_lookup_ms"]["median"], 2)
            res["B_over_C"] = round(res["B_key_ids_ms"]["median"] / res["C_key_lookup_ms"]["median"], 2)
            if args.profile:
                for tag, batch in (("B", bbatch), ("C", cbatch)):
                    ctx.profile(True)
                    for _ in range(args.steps):
                        batch.enqueue()
                        ctx.synchronize()
                    res[tag + "_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
                    ctx.profile(False)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
