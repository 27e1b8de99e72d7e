"""Key-combine probe: what does one sb_key_combine call cost next to the routes that were there before it for the dense ids
of GROUP BY a, b?

Per shape, timed with events on the context's stream (median and min-max of --steps runs after --warmup):
  A      torch.unique(a.long() * nb + b, sorted=True, return_inverse=True) on the device, dead rows taken out first and the
         inverse scattered back into an id per row (-1 elsewhere): tuples and ids
  B      the host round trip: both id arrays copied to the host, np.unique over the pairs' codes, the ids uploaded again
         (wall time, the copies included)
  C      one sb_key_combine call through a prepared batch (max_keys 1024, ids of two bytes)
All three see the same id arrays: two-byte part ids as sb_key_ids writes them under max_keys 1024, 10 % of the rows all
ones in each part.  The shapes are two parts of 3 x 2 keys, two parts of 100 x 10 keys and four parts (8 x 6 x 5 x 4).  C's
tuples and ids are compared with A's before anything is timed.  Prints one JSON line per shape, with the bytes the call
moves per row (the parts read twice, the ids written once) and the bandwidth that makes of C's median; --profile adds the
per-kernel split of C from sb_ctx_profile.

  python scripts/key_combine_probe.py [--steps 20] [--warmup 3] [--rows 4000000] [--profile]
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

from read_selected_probe import timed   # noqa: E402

SHAPES = (("3x2", (3, 2)), ("100x10", (100, 10)), ("8x6x5x4", (8, 6, 5, 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--profile", action="store_true", help="per-kernel times of the call (sb_ctx_profile)")
    args = ap.parse_args()
    import torch
    import strawboat_amd as sb
    from strawboat_amd.key_combine import KeyCombineBatch
    assert torch.cuda.is_available(), "the probe needs a GPU"
    ctx = sb.Context(0)
    rows = args.rows
    for name, tops in SHAPES:
        rng = np.random.default_rng(len(tops) * 1000 + tops[0])
        host = []
        for top in tops:
            a = rng.integers(0, top, rows).astype(np.uint16)
            a[rng.random(rows) < 0.1] = 0xFFFF
            host.append(a)
        devs = [torch.from_numpy(a).to(ctx.torch_device) for a in host]
        batch = KeyCombineBatch(ctx, [[(d, 1024) for d in devs]], 1024, 2)

        def run_a():
            with torch.cuda.stream(ctx.torch_stream):
                live = torch.ones(rows, dtype=torch.bool, device=ctx.torch_device)
                code = torch.zeros(rows, dtype=torch.int64, device=ctx.torch_device)
                for d in devs:
                    v = d.view(torch.int16).long() & 0xFFFF
                    live &= v < 1024
                    code = code * 1024 + v
                keys, inv = torch.unique(code[live], sorted=True, return_inverse=True)
                ids = torch.full((rows,), -1, dtype=torch.int32, device=ctx.torch_device)
                ids[live] = inv.to(torch.int32)
                return keys, ids

        def run_b():
            t0 = time.perf_counter()
            hs = [d.cpu().numpy() for d in devs]
            live = np.ones(rows, bool)
            code = np.zeros(rows, np.int64)
            for h in hs:
                live &= h < 1024
                code = code * 1024 + h
            keys, inv = np.unique(code[live], return_inverse=True)
            ids = np.full(rows, 0xFFFF, np.uint16)
            ids[live] = inv.astype(np.uint16)
            dev_ids = torch.from_numpy(ids).to(ctx.torch_device)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, keys, dev_ids

        got = batch.enqueue()[0]
        ctx.synchronize()
        keys, ids = run_a()
        torch.cuda.synchronize()
        assert not got.overflow and got.n_keys == keys.numel(), "%s: n_keys differ" % name
        codes = np.zeros(got.n_keys, np.int64)
        for p in range(len(tops)):
            codes = codes * 1024 + got.tuples[:, p]
        assert np.array_equal(codes, keys.cpu().numpy()), "%s: the tuples differ" % name
        mine = got.ids.view(torch.int16).to(torch.int32) & 0xFFFF
        mine = torch.where(mine == 0xFFFF, torch.full_like(mine, -1), mine)
        assert torch.equal(mine, ids), "%s: the ids differ" % name
        bytes_per_row = 2 * 2 * len(tops) + 2
        res = {"shape": name, "parts": len(tops), "rows": rows, "n_keys": got.n_keys, "live": got.live, "steps": args.steps,
               "warmup": args.warmup, "bytes_per_row": bytes_per_row}
        res["A_torch_unique_ms"] = timed(torch, ctx, run_a, args.steps, args.warmup)
        b_ms = [run_b()[0] for _ in range(max(3, args.steps // 4))]
        res["B_host_round_trip_ms"] = {"median": round(float(np.median(b_ms)), 4), "min": round(min(b_ms), 4), "max": round(max(b_ms), 4)}
        res["C_key_combine_ms"] = timed(torch, ctx, batch.enqueue, args.steps, args.warmup)
        c = res["C_key_combine_ms"]["median"]
        res["C_GBps"] = round(rows * bytes_per_row / (c * 1e-3) / 1e9, 1)
        res["A_over_C"] = round(res["A_torch_unique_ms"]["median"] / c, 2)
        res["B_over_C"] = round(res["B_host_round_trip_ms"]["median"] / c, 2)
        if args.profile:
            ctx.profile(True)
            for _ in range(args.steps):
                batch.enqueue()
                ctx.synchronize()
            res["C_kernels_ms_per_call"] = {kn: round(ms / args.steps, 4) for kn, (n, ms) in ctx.profile_read().items() if n}
            ctx.profile(False)
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
