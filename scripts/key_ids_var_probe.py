"""Key-id probe for string keys: what does one sb_key_ids_var call cost next to what an engine did before it to GROUP BY
a Binary / Utf8 key column, or to SELECT DISTINCT it?

Per page kind, distinct count, selection and column count, wall clock around enqueue .. results on the host / ids on the
device (median and min-max of --steps runs after --warmup; the host is part of what is measured):
  A      sb_read_columns through a prepared batch and a synchronize, offsets / bytes / validity to the host,
         np.unique(..., return_inverse=True) of the live rows there (selected and not null), the ids back to the device:
         keys and ids
  B      sb_read_selected_var through a prepared batch and a synchronize, its offsets / bytes / validity to the host and
         the same np.unique there: keys only, the DISTINCT use
  C      one sb_key_ids_var call through a prepared batch (max_keys 1024, ids of two bytes) and a synchronize
A and B run on code paths the new call does not touch; all three see the same pages and the same bitmap.  The host step
is given its fastest exact form: the strings zero padded to the longest with their length behind them, compared as
fixed-width records (np.unique on a void view: memcmp, which is the byte order with the prefix first).  The pages are
Dict, Freq (one value on ~90 % of the rows), None and LZ4 pages of a nullable Binary column (10 % nulls, keys of 8 .. 32
bytes), --rows rows in pages of --page-rows.  The selections are random (100 %, 10 %, 0.1 %) and clustered (10 % and 0.1 %
as one stretch of rows).  C's keys and ids are compared with A's before anything is timed.  One JSON line per case;
--profile adds the per-kernel split of C from sb_ctx_profile.

  python scripts/key_ids_var_probe.py [--steps 10] [--warmup 2] [--rows 262144] [--page-rows 65536] [--columns 1,4,16]
                                      [--distinct 16,256,1024] [--only dict,freq,none,lz4] [--profile]
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
from read_selected_probe import bitmap_bytes   # noqa: E402


def str_column(rows, uniq, freq):
    rng = np.random.default_rng(uniq)
    voc = [(b"key-%06d.host.example.com/path" % i)[:int(rng.integers(10, 33))] for i in range(uniq)]
    idx = rng.integers(0, uniq, rows)
    if freq:
        idx = np.where(rng.random(rows) < 0.9, 0, idx)
    lens = np.array([len(v) for v in voc], np.int64)[idx]
    offs = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(voc[i] for i in idx), np.uint8).copy()
    validity = np.packbits(rng.random(rows) < 0.9, bitorder="little")
    return dict(ptype=S.T_BIN32, nullable=True, rows=rows, values=data, validity=validity, offsets=offs.astype(np.int32))


def cases(rows, page_rows, uniq):
    yield "dict", str_column(rows, uniq, False), dict(max_page_size=page_rows, force_codec=S.DICT)
    yield "freq", str_column(rows, uniq, True), dict(max_page_size=page_rows, force_codec=S.FREQ)
    yield "none", str_column(rows, uniq, False), dict(max_page_size=page_rows, force_codec=S.NONE)
    yield "lz4", str_column(rows, uniq, False), dict(max_page_size=page_rows, force_codec=S.LZ4)


def selections(rows):
    rng = np.random.default_rng(3)
    yield "100%", np.ones(rows, bool)
    for p in (0.1, 0.001):
        yield "%g%% random" % (100 * p), rng.random(rows) < p
        m = np.zeros(rows, bool)
        at = int(rng.integers(0, rows - int(rows * p)))
        m[at:at + int(rows * p)] = True
        yield "%g%% clustered" % (100 * p), m


def host_unique(offs, data, live):
    """(keys as a list of bytes, the inverse of the live rows): np.unique over fixed-width records, exact"""
    offs = offs.astype(np.int64)
    start, lens = offs[:-1][live], (offs[1:] - offs[:-1])[live]
    if start.size == 0:
        return [], np.zeros(0, np.int64)
    width = int(lens.max())
    at = np.arange(width)
    rec = np.zeros((start.size, width + 4), np.uint8)
    if width:
        inside = at[None, :] < lens[:, None]
        rec[:, :width][inside] = data[(start[:, None] + at[None, :])[inside]]
    rec[:, width:] = lens.astype(">u4").view(np.uint8).reshape(-1, 4)
    u, inv = np.unique(rec.view("V%d" % (width + 4)).reshape(-1), return_inverse=True)
    u = u.view(np.uint8).reshape(-1, width + 4)
    ulen = u[:, width:].copy().view(">u4").reshape(-1)
    return [u[i, :ulen[i]].tobytes() for i in range(u.shape[0])], inv


def timed(ctx, fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--page-rows", type=int, default=65536)
    ap.add_argument("--columns", default="1,4,16")
    ap.add_argument("--distinct", default="16,256,1024")
    ap.add_argument("--only", default=None)
    ap.add_argument("--selections", default=None, help="a comma list of selection names, e.g. '100%%,10%% random'")
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the key-id call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd.key_ids_var import KeyIdsVarBatch
    from strawboat_amd.read_selected_var import ReadSelectedVarBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    S.build()
    ctx = sb.Context(0)
    only = set(args.only.split(",")) if args.only else None
    only_sel = set(args.selections.split(",")) if args.selections else None
    rows = args.rows
    for uniq in [int(x) for x in args.distinct.split(",")]:
        for name, col, opt in cases(rows, args.page_rows, uniq):
            if only and name not in only:
                continue
            pages, metas = S.write_column(col["ptype"], col["nullable"], rows, col["values"], validity=col["validity"],
                                          offsets=col["offsets"], options=S.make_options(**opt))
            seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
            dev = torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device)
            for ncols in [int(x) for x in args.columns.split(",")]:
                cols = [read.ColumnPages(col["ptype"], col["nullable"], dev, metas) for _ in range(ncols)]
                rbatch = read.ReadBatch(ctx, cols)
                for sel_name, mask in selections(rows):
                    if only_sel and sel_name not in only_sel:
                        continue
                    bitmap = torch.from_numpy(bitmap_bytes(mask)).to(ctx.torch_device)
                    selected = int(mask.sum())
                    # (values for rows of the longest key: the default, 4 * pages_len, is too little for Dict pages, and a null
                    # row of a Dict page decodes to an entry's bytes, not to the bytes the writer was given)
                    outs = [(torch.empty((rows + 1) * 4, dtype=torch.uint8, device=ctx.torch_device),
                             torch.empty(rows * 32, dtype=torch.uint8, device=ctx.torch_device),
                             torch.empty((rows + 31) // 32 * 4, dtype=torch.uint8, device=ctx.torch_device)) for _ in range(ncols)]
                    sbatch = ReadSelectedVarBatch(ctx, cols, bitmap, out=outs)
                    cbatch = KeyIdsVarBatch(ctx, cols, bitmap, 1024, 2)

                    def run_a():
                        arrs = rbatch.enqueue()
                        ctx.synchronize()
                        out = []
                        for a in arrs:
                            offs = a.offsets_numpy().view(np.int32)
                            valid = np.unpackbits(a.validity_numpy(), bitorder="little")[:rows].astype(bool)
                            live = mask & valid
                            keys, inv = host_unique(offs, a.values_numpy(), live)
                            ids = np.full(rows, 0xFFFF, np.uint16)
                            ids[live] = inv.astype(np.uint16)
                            out.append((keys, torch.from_numpy(ids.view(np.int16)).to(ctx.torch_device), ids))
                        torch.cuda.synchronize()
                        return out

                    def run_b():
                        arrs = sbatch.enqueue()
                        ctx.synchronize()
                        out = []
                        for a in arrs:
                            n = a.selected
                            offs = a.offsets_buf[:(n + 1) * 4].cpu().numpy().view(np.int32)
                            valid = np.unpackbits(a.validity_buf[:(n + 7) // 8].cpu().numpy(), bitorder="little")[:n].astype(bool)
                            out.append(host_unique(offs, a.values_buf[:a.values_len].cpu().numpy(), valid)[0])
                        return out

                    def run_c():
                        cbatch.enqueue()
                        ctx.synchronize()

                    got = cbatch.enqueue()
                    ctx.synchronize()
                    ref = run_a()
                    refb = run_b()
                    what = "%s, %d distinct, %s, %d columns" % (name, uniq, sel_name, ncols)
                    for g, (keys, _, ids), kb in zip(got, ref, refb):
                        assert not g.overflow and g.keys == keys == kb, "%s: the keys differ" % what
                        assert np.array_equal(g.ids.cpu().numpy().view(np.uint16), ids), "%s: the ids differ" % what
                    res = {"pages": name, "codecs": sorted(seen), "distinct": uniq, "selection": sel_name, "columns": ncols, "rows": rows,
                           "selected": selected, "n_keys": got[0].n_keys, "page_bytes": int(pages.size), "steps": args.steps, "warmup": args.warmup}
                    res["A_read_host_unique_ids_back_ms"] = timed(ctx, run_a, args.steps, args.warmup)
                    res["B_read_selected_var_host_unique_ms"] = timed(ctx, run_b, args.steps, args.warmup)
                    res["C_key_ids_var_ms"] = timed(ctx, run_c, args.steps, args.warmup)
                    res["A_over_C"] = round(res["A_read_host_unique_ids_back_ms"]["median"] / res["C_key_ids_var_ms"]["median"], 2)
                    res["B_over_C"] = round(res["B_read_selected_var_host_unique_ms"]["median"] / res["C_key_ids_var_ms"]["median"], 2)
                    if args.profile:
                        ctx.profile(True)
                        for _ in range(args.steps):
                            cbatch.enqueue()
                            ctx.synchronize()
                        res["C_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
                        ctx.profile(False)
                    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
