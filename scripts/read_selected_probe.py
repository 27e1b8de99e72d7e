"""Selected-read probe: what does sb_read_selected cost next to what a caller holding a selection bitmap does today?

Per shape and selection, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A  sb_read_columns alone (every row written; the same for every selection)
  B  A, then the torch compaction a caller writes today: the bitmap unpacked to a bool mask, values[mask], and the
     validity bits of the selected rows packed again
  C  sb_read_selected through a prepared batch
Shapes (those of scripts/filter_probe.py): C1 (1 M-row Int64, one plain page), C2 (1 M-row nullable Float64, RLE pages), a
Dict Int32 column and an LZ4 Int64 column (the staged path).  --columns N puts N columns of the shape into one call; all of
them share one bitmap.  Selections: random bits at 0.001 / 0.01 / 0.1 / 0.5 / 1.0, and 0.01 clustered: every bit of 1 % of
the 4096-row tiles and no other, the case the tile early-out is for.
C's bytes are compared with B's before anything is timed.  Prints one JSON line per shape and selection.

  python scripts/read_selected_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only c1,c2] [--profile]
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

TILE = 4096


def shapes():
    rng = np.random.default_rng(7)
    c1 = W.c1_int64()
    c2 = W.c2_float64()
    d = dict(ptype=S.T_I32, nullable=False, rows=1_000_000, values=rng.integers(0, 1000, 1_000_000).astype(np.int32), validity=None, offsets=None)
    z = dict(ptype=S.T_I64, nullable=False, rows=1_000_000, values=np.repeat(rng.integers(0, 1 << 40, 125_000), 8).astype(np.int64),
             validity=None, offsets=None)
    return [("c1_int64_none", c1, dict(force_codec=S.NONE)),
            ("c2_float64_rle", c2, dict(max_page_size=W.PAGE, force_codec=S.RLE)),
            ("dict_int32", d, dict(max_page_size=W.PAGE, force_codec=S.DICT)),
            ("lz4_int64", z, dict(max_page_size=W.PAGE, force_codec=S.LZ4))]


def selections(rows):
    rng = np.random.default_rng(11)
    out = [("random %g" % p, rng.random(rows) < p if p < 1.0 else np.ones(rows, bool)) for p in (0.001, 0.01, 0.1, 0.5, 1.0)]
    ntiles = (rows + TILE - 1) // TILE
    m = np.zeros(rows, bool)
    for t in rng.choice(ntiles, max(1, ntiles // 100), replace=False):
        m[t * TILE:(t + 1) * TILE] = True
    out.insert(2, ("clustered 0.01", m))
    return out


def bitmap_bytes(mask):
    bits = np.zeros((mask.size + 31) // 32 * 32, bool)
    bits[:mask.size] = mask
    return np.packbits(bits, bitorder="little")


def unpack_bits(torch, bits, rows):
    sh = torch.arange(8, dtype=torch.uint8, device=bits.device)
    return ((bits[:(rows + 7) // 8].unsqueeze(1) >> sh) & 1).bool().view(-1)[:rows]


def pack_bits(torch, m):
    pad = (-m.numel()) % 8
    if pad:
        m = torch.cat([m, torch.zeros(pad, dtype=torch.bool, device=m.device)])
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=m.device)
    return (m.view(-1, 8).to(torch.uint8) * w).sum(dim=1, dtype=torch.uint8)


def torch_compact(torch, arr, dtype, bitmap):
    """what a caller does today with a decoded column and a bitmap"""
    mask = unpack_bits(torch, bitmap, arr.rows)
    vals = arr.values.view(dtype)[mask]
    valid = pack_bits(torch, unpack_bits(torch, arr.validity, arr.rows)[mask]) if arr.validity is not None else None
    return vals, valid


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
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the selected read (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
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
        batch = read.ReadBatch(ctx, cols)
        # B puts torch kernels of its own behind the read call: they must not run in an interval that the library issues a
        # second time (launch hints that miss after a change of shape), so the reads settle first
        for _ in range(3):
            batch.enqueue()
            ctx.synchronize()
        a_ms = timed(torch, ctx, batch.enqueue, args.steps, args.warmup)
        for sel_name, mask in selections(col["rows"]):
            bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
            sbatch = ReadSelectedBatch(ctx, cols, bitmap)

            def run_b():
                arrs = batch.enqueue()
                with torch.cuda.stream(ctx.torch_stream):
                    return [torch_compact(torch, a, dt[col["ptype"]], bitmap) for a in arrs]

            ref = run_b()
            got = sbatch.enqueue()
            ctx.synchronize()
            for (rv, rb), g in zip(ref, got):
                assert g.selected == rv.numel() == int(mask.sum()), "%s %s: selected differs" % (name, sel_name)
                assert torch.equal(rv.view(torch.uint8), g.values_buf[:g.values_len]), "%s %s: values differ" % (name, sel_name)
                if rb is not None:
                    assert torch.equal(rb, g.validity), "%s %s: validity differs" % (name, sel_name)
            res = {"shape": name, "selection": sel_name, "columns": args.columns, "rows": col["rows"], "selected": got[0].selected,
                   "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup, "A_read_ms": a_ms}
            res["B_read_then_torch_ms"] = timed(torch, ctx, run_b, args.steps, args.warmup)
            res["C_read_selected_ms"] = timed(torch, ctx, sbatch.enqueue, args.steps, args.warmup)
            if args.profile:
                ctx.profile(True)
                for _ in range(args.steps):
                    sbatch.enqueue()
                    ctx.synchronize()
                res["C_kernels_ms_per_call"] = {k: round(ms / args.steps, 4) for k, (n, ms) in ctx.profile_read().items() if n}
                ctx.profile(False)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
