"""Selected-read probe for strings: what does sb_read_selected_var cost next to what a caller holding a selection bitmap
does today with a Utf8 column?

Per shape and selection, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A  sb_read_columns alone (every row's offset and bytes written; the same for every selection)
  B  A, then the torch compaction a caller writes today: lengths from the offsets, the bitmap unpacked to a bool mask,
     lengths[mask], a cumsum for the new offsets, a byte gather (repeat_interleave of the rows' source starts plus a ramp),
     and the validity bits of the selected rows packed again
  C  sb_read_selected_var through a prepared batch
Shapes: the C3 column (1 M-row Utf8, 10 000-word Zipf vocabulary, 10 % nulls, 64 Ki-row pages) as Dict pages, as plain pages
and as LZ4 pages (the staged path).  --columns N puts N columns of the shape into one call; all of them share one bitmap.
Selections: random bits at 0.001 / 0.1 / 1.0, and 0.01 clustered: every bit of 1 % of the 4096-row tiles and no other, the
case the tile early-out is for.
C's offsets, bytes and validity are compared with B's before anything is timed.  Prints one JSON line per shape and
selection.

  python scripts/read_selected_var_probe.py [--steps 20] [--warmup 3] [--columns 16] [--only dict,lz4] [--profile]
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
from scripts.read_selected_probe import bitmap_bytes, pack_bits, timed, unpack_bits   # noqa: E402

TILE = 4096


def shapes(rows):
    c3 = W.zipf_utf8(rows, 42, null_density=0.1)
    return [("dict_utf8", c3, dict(max_page_size=W.PAGE, force_codec=S.DICT)),
            ("plain_utf8", c3, dict(max_page_size=W.PAGE, force_codec=S.NONE)),
            ("lz4_utf8", c3, dict(max_page_size=W.PAGE, force_codec=S.LZ4))]


def selections(rows):
    rng = np.random.default_rng(11)
    out = [("random %g" % p, rng.random(rows) < p if p < 1.0 else np.ones(rows, bool)) for p in (0.001, 0.1, 1.0)]
    ntiles = (rows + TILE - 1) // TILE
    m = np.zeros(rows, bool)
    for t in rng.choice(ntiles, max(1, ntiles // 100), replace=False):
        m[t * TILE:(t + 1) * TILE] = True
    out.insert(1, ("clustered 0.01", m))
    return out


def torch_compact(torch, arr, bitmap):
    """what a caller does today with a decoded Utf8 column and a bitmap: (offsets int64, bytes, packed validity)"""
    offs = arr.offsets.view(torch.int32)[:arr.rows + 1].to(torch.int64)
    mask = unpack_bits(torch, bitmap, arr.rows)
    starts, lens = offs[:-1][mask], (offs[1:] - offs[:-1])[mask]
    new_offs = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
    torch.cumsum(lens, 0, out=new_offs[1:])
    total = int(new_offs[-1]) if lens.numel() else 0   # (the gather's size: one host round trip, as a caller has it)
    src = torch.repeat_interleave(starts - new_offs[:-1], lens, output_size=total) + torch.arange(total, device=lens.device)
    vals = arr.values[src]
    valid = pack_bits(torch, unpack_bits(torch, arr.validity, arr.rows)[mask]) if arr.validity is not None else None
    return new_offs, vals, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the selected read (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.read_selected_var import ReadSelectedVarBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    for name, col, opt in shapes(args.rows):
        if only and not any(name.startswith(o) for o in only):
            continue
        pages, metas = S.write_column(col["ptype"], col["nullable"], col["rows"], col["values"], validity=col["validity"],
                                      offsets=col["offsets"], options=S.make_options(**opt))
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
            # capacities that are always enough: the full read's (the default guess for `values`, 4 * pages_len, is too
            # small for Dict pages at selectivity 1)
            rows, full = col["rows"], int(col["offsets"][-1])
            out = [(torch.empty((rows + 1) * 4, dtype=torch.uint8, device=ctx.torch_device),
                    torch.empty(full, dtype=torch.uint8, device=ctx.torch_device),
                    torch.empty((rows + 31) // 32 * 4, dtype=torch.uint8, device=ctx.torch_device)) for _ in cols]
            sbatch = ReadSelectedVarBatch(ctx, cols, bitmap, out=out)

            def run_b():
                arrs = batch.enqueue()
                with torch.cuda.stream(ctx.torch_stream):
                    return [torch_compact(torch, a, bitmap) for a in arrs]

            ref = run_b()
            got = sbatch.enqueue()
            ctx.synchronize()
            for (ro, rv, rb), g in zip(ref, got):
                assert g.selected == ro.numel() - 1 == int(mask.sum()), "%s %s: selected differs" % (name, sel_name)
                assert g.values_len == rv.numel(), "%s %s: values_len differs" % (name, sel_name)
                assert torch.equal(ro, g.offsets.to(torch.int64)), "%s %s: offsets differ" % (name, sel_name)
                assert torch.equal(rv, g.values), "%s %s: values differ" % (name, sel_name)
                if rb is not None:
                    assert torch.equal(rb, g.validity), "%s %s: validity differs" % (name, sel_name)
            res = {"shape": name, "selection": sel_name, "columns": args.columns, "rows": col["rows"], "selected": got[0].selected,
                   "values_len": got[0].values_len, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup,
                   "A_read_ms": a_ms}
            res["B_read_then_torch_ms"] = timed(torch, ctx, run_b, args.steps, args.warmup)
            res["C_read_selected_var_ms"] = timed(torch, ctx, sbatch.enqueue, args.steps, args.warmup)
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
