"""Sliced Arrow arrays through every encode kernel family: the table of tests/slice_cases.py on the device.

For every case and both fills of the poison: the presented buffers (validity_bit_offset, a Boolean values_bit_offset,
Binary offsets that do not start at 0 over the whole values buffer, a values pointer inside its buffer) are encoded on
the device; PageMeta and page bytes must equal what the oracle writes for the same presentation, the two fills must give
the same device bytes wherever the oracle's do, and the device's pages read back through read_simple must give what the
oracle reads out of its own pages.  Zstd / Snappy / parallel-LZ4 blocks are not byte-pinned: their pages are compared
codec by codec, def-level section byte for byte, and by decoding them with the oracle.

Every case is encoded in a call of its own, with the profile on for the first fill: the kernels the case names must have
been launched (a necessary condition; tests/test_slice_cases.py ties a case to its path by the codec its pages reach).
The cases of a family that share their options are encoded once more in ONE call: the column table carries per-column
offsets.

Contexts are the test's own: SB_BIN_FUSED is read when a context is created.

Teeth (scratch builds, when the file was written; both mutations only move reads to lower addresses): with
`c.validity_bit_offset + p.row0` replaced by `p.row0` in k_enc_prim_dict the prim_dict_fused family reports 156
findings (PageMeta, values read back, the poison reaching the pages; a case whose presented offset is 0 cannot see
it); with `c.values_bit_offset` dropped from the Boolean path of k_enc_emit_tiles the boolean family reports 69, all in
forced-None cases with a non-zero value offset (page bytes differ from the first block byte on)."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import slice_cases as T
from tests.test_gpu_encode import write_options

pytestmark = pytest.mark.gpu

FAMILIES = T.families()
_want = {}


def want_of(case, fill):
    """(presented, oracle pages, oracle metas, oracle read of them), computed once"""
    key = (case.name, fill)
    if key not in _want:
        p = T.present(case, fill)[0]
        pages, metas = T.oracle_write(case, p)
        _want[key] = (p, pages, metas, S.read_column(case.ptype, case.nullable, pages, metas) if case.readable else None)
    return _want[key]


def device_column(ctx, p):
    import torch
    from strawboat_amd.write import DeviceColumn
    dev = ctx.torch_device

    def up(a, skip=0):
        if a is None:
            return None
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)[skip:]
    return DeviceColumn(p["ptype"], p["nullable"], p["rows"], up(p["values_buf"], p["values_skip"]),
                        up(p["validity_buf"], p["validity_skip"]), up(p["offsets"]),
                        values_bit_offset=p["values_bit_offset"], validity_bit_offset=p["validity_bit_offset"])


def options_of(case):
    return write_options(lz4_exact=case.lz4_exact, **case.opt)


def host_encode(ctx, case, p):
    """sb_write_columns(SB_MEM_HOST): host Arrow buffers in, host page bytes out"""
    from strawboat_amd import _native as N
    from strawboat_amd.write import options_c
    lib = ctx._lib
    oc = options_c(options_of(case))
    npg = C.c_uint64()
    vlen = p["values"].size if case.kind == "bin" else 0
    bound = lib.sb_write_bound(case.ptype, int(case.nullable), case.rows, vlen, C.byref(oc), C.byref(npg))
    out = np.full(bound, 0xA5, np.uint8)
    metas = (N.PageMetaC * npg.value)()
    cw = (N.ColumnWriteC * 1)()
    cw[0].physical_type, cw[0].is_nullable, cw[0].rows = case.ptype, int(case.nullable), case.rows
    cw[0].values, cw[0].values_len = p["values"].ctypes.data, p["values"].size
    cw[0].values_bit_offset, cw[0].validity_bit_offset = p["values_bit_offset"], p["validity_bit_offset"]
    if p["validity"] is not None:
        cw[0].validity = p["validity"].ctypes.data
    if p["offsets"] is not None:
        cw[0].offsets = p["offsets"].ctypes.data
    cw[0].out_pages, cw[0].out_capacity = out.ctypes.data, out.size
    cw[0].out_metas, cw[0].n_pages_capacity = metas, npg.value
    ctx._check(lib.sb_write_columns(ctx._h, cw, 1, C.byref(oc), N.SB_MEM_HOST))
    ctx.synchronize()
    n = int(cw[0].n_pages)
    got_metas = np.array([[m.length, m.num_values] for m in metas[:n]], dtype=np.uint64).reshape(-1, 2)
    assert (out[cw[0].out_len:] == 0xA5).all(), "bytes written behind out_len"
    return out[:cw[0].out_len].copy(), got_metas


def compare(case, got, got_metas, fill):
    """device pages against the oracle's for the same presentation; returns a description of the difference or None"""
    p, pages, metas, _ = want_of(case, fill)
    if not case.decode:
        if not np.array_equal(got_metas, metas):
            return "PageMeta differ: %s, the oracle's %s" % (got_metas[:3].tolist(), metas[:3].tolist())
        if not np.array_equal(got, pages):
            bad = int(np.argmax(got != pages))
            ends = np.cumsum(metas[:, 0].astype(np.int64))
            return "page bytes differ, first at byte %d of %d (page %d of %d)" % (bad, pages.size, int(np.searchsorted(ends, bad, "right")), len(ends))
        return None
    if not np.array_equal(got_metas[:, 1], metas[:, 1]):
        return "num_values differ"
    codecs = S.stat_column(case.ptype, case.nullable, got, got_metas)[0].tolist()
    if codecs != S.stat_column(case.ptype, case.nullable, pages, metas)[0].tolist():
        return "page codecs differ: %s" % codecs
    for (a, _), (b, _) in zip(T.page_spans(got_metas), T.page_spans(metas)):
        n = T.def_section_len(pages[b:], case.nullable)
        if not np.array_equal(got[a:a + n], pages[b:b + n]):
            return "def-level sections differ"
    dec, want = S.read_column(case.ptype, case.nullable, got, got_metas), want_of(case, fill)[3]
    for key in ("values", "validity", "offsets"):
        if not np.array_equal(dec[key], want[key]):
            return "the oracle decodes other %s out of the device's pages" % key
    return None


def read_back(ctx, case, got, got_metas, fill):
    import torch
    from strawboat_amd import read
    want = want_of(case, fill)[3]
    if want is None:
        return None
    res = read.read_simple(ctx, read.ColumnPages(case.ptype, case.nullable, torch.from_numpy(got).to(ctx.torch_device), got_metas))
    if res.rows != want["rows"]:
        return "read back %d rows" % res.rows
    v, w = res.values_numpy(), want["values"]
    if case.kind == "bool":      # (the spare bits of a decoded bitmap's last byte are no rows)
        v, w = np.unpackbits(v, bitorder="little")[:case.rows], np.unpackbits(w, bitorder="little")[:case.rows]
    if not np.array_equal(v, w):
        return "values read back differ"
    if case.nullable and not np.array_equal(np.unpackbits(res.validity_numpy(), bitorder="little")[:case.rows],
                                            np.unpackbits(want["validity"], bitorder="little")[:case.rows]):
        return "validity read back differs"
    if case.kind == "bin" and not np.array_equal(res.offsets_numpy(), want["offsets"]):
        return "offsets read back differ"
    return None


def encode_one(ctx, case, p):
    from strawboat_amd import write
    if case.host:
        return host_encode(ctx, case, p)
    enc = write.write(ctx, device_column(ctx, p), options_of(case))
    return enc.pages_numpy(), enc.metas_array()


def run_cases(ctx, cases, seen_kernels):
    from strawboat_amd import write
    wrong = []
    try:
        for c in cases:
            got = {}
            for fill in T.FILLS:
                p = want_of(c, fill)[0]
                if fill == T.FILLS[0]:
                    ctx.profile(True)
                got[fill] = encode_one(ctx, c, p)
                if fill == T.FILLS[0]:
                    prof = ctx.profile_read()
                    ctx.profile(False)
                    launched = {k for k, (n, _) in prof.items() if n > 0}
                    seen_kernels |= launched
                    missing = [k for k in c.kernels if k not in launched]
                    if missing:
                        wrong.append("%s: %s not launched (launched: %s)" % (c.name, missing, sorted(launched)))
                for why in (compare(c, *got[fill], fill), read_back(ctx, c, *got[fill], fill)):
                    if why:
                        wrong.append("%s fill %d: %s" % (c.name, fill, why))
            w0, w1 = want_of(c, 0), want_of(c, 1)
            if not c.decode and np.array_equal(w0[1], w1[1]) and not (np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])):
                wrong.append("%s: the poison reaches the device's pages (the oracle's are the same for both fills)" % c.name)
    finally:
        ctx.profile(False)
    # the cases that share their options in ONE call: slices at different offsets side by side in the column table
    groups = {}
    for c in cases:
        if not c.host:
            groups.setdefault(c.group(), []).append(c)
    for cs in groups.values():
        if len(cs) < 2:
            continue
        encs = write.encode_columns(ctx, [device_column(ctx, want_of(c, 1)[0]) for c in cs], options_of(cs[0]))
        ctx.synchronize()
        for c, e in zip(cs, encs):
            why = compare(c, e.pages_numpy(), e.metas_array(), 1)
            if why:
                wrong.append("%s in a call of %d columns: %s" % (c.name, len(cs), why))
    return wrong


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_slices_of_a_family_against_the_oracle(family, monkeypatch):
    import strawboat_amd as sb
    wrong, seen = [], set()
    for fused in ("1", "0"):
        cases = [c for c in FAMILIES[family] if c.fused == fused]
        if not cases:
            continue
        monkeypatch.setenv("SB_BIN_FUSED", fused)
        ctx = sb.Context(0)
        try:
            wrong += run_cases(ctx, cases, seen)
        finally:
            ctx.close()
    print("kernels launched for %s: %s" % (family, ", ".join(sorted(seen))))
    assert not wrong, "%d findings in %d cases:\n%s" % (len(wrong), len(FAMILIES[family]), "\n".join(wrong[:40]))
    if family != "host_memory":
        assert len({(c.start, c.advance) for c in FAMILIES[family]}) >= 2, "no call with slices at different offsets"


def test_sliced_bitmaps_at_the_end_of_an_allocation(gpu_ctx):
    """A slice's validity bitmap (nullable Int64: a page kernel, the run-level kernel; Int32 for the fused Dict kernel, which
    takes no 8-byte values) and a Boolean slice's value bitmap, placed so that the byte of the slice's last bit is the last
    byte of a device allocation: the library may read ceil((offset + rows) / 8) bytes from the pointer, one more is a GPU
    fault.  (Every bitmap load of the encode kernels was read against that bound before this test ran for the first time:
    bits32 / vword_issue pull their 8-byte load back inside the bitmap, the byte loads clamp their row.)"""
    import torch
    from strawboat_amd import write
    from strawboat_amd.write import DeviceColumn
    rng = np.random.default_rng(12)
    dev = gpu_ctx.torch_device
    seg = 20 << 20   # a whole allocator segment of its own

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def ok_of(rows):
        return T.validity(rng, rows, (False, False))

    runs = T.typed(T.I64, T.run_rows(65536 + 1001, 37, 1))
    ok5 = ok_of(5005)
    shapes = [
        T.Case("end", "page_kernel_at13", T.I64, T.typed(T.I64, T.with_garbage(np.repeat(rng.integers(0, 50, 1001), 5), ok5, 1)), ok5,
               13, False, dict(max_page_size=1001, force_codec=T.RLE), T.RLE, ()),
        T.Case("end", "page_kernel_at4099adv", T.I64, T.typed(T.I64, T.with_garbage(rng.integers(0, 50, 5005), ok5, 2)), ok5,
               4099, True, dict(max_page_size=1001, force_codec=T.DICT), T.DICT, ()),
        T.Case("end", "run_level_at65", T.I64, runs, ok_of(len(runs)), 65, False,
               dict(max_page_size=65536, ratio=2.0, forbidden=(T.DICT, T.FREQ)), T.RLE, ()),
        T.Case("end", "fused_at63", T.I32, T.typed(T.I32, rng.integers(0, 40, 2002)), ok_of(2002), 63, False,
               dict(max_page_size=1001, ratio=2.0), T.DICT, ()),
        T.Case("end", "bool_none_v8", T.BOOL, rng.random(2507) < 0.5, ok_of(2507), 13, False,
               dict(max_page_size=1000, force_codec=T.NONE), T.NONE, (), bpos=8),
        T.Case("end", "bool_none_v13", T.BOOL, rng.random(2507) < 0.5, ok_of(2507), 64, True,
               dict(max_page_size=1001, force_codec=T.NONE), T.NONE, (), bpos=13),
        T.Case("end", "bool_lz4_v16", T.BOOL, rng.random(2507) < 0.2, ok_of(2507), 7, False,
               dict(max_page_size=1000, default_compression=T.LZ4), T.LZ4, (), bpos=16),
        T.Case("end", "bool_rle_v3", T.BOOL, np.repeat(rng.random(63) < 0.5, 40)[:2507], ok_of(2507), 8, False,
               dict(max_page_size=1001, force_codec=T.RLE), T.RLE, (), bpos=3)]
    for c in shapes:
        p = T.present(c, 1)[0]
        want_pages, want_metas = T.oracle_write(c, p)
        assert S.stat_column(c.ptype, True, want_pages, want_metas)[0].tolist() == [c.codec] * len(want_metas), c.name
        flush = p["values"] if c.kind == "bool" else p["validity"]
        buf = torch.zeros(seg, dtype=torch.uint8, device=dev)
        view = buf[seg - flush.size:]
        view.copy_(torch.from_numpy(flush.copy()))
        if c.kind == "bool":
            dc = DeviceColumn(c.ptype, True, c.rows, view, up(p["validity"]), None, values_bit_offset=p["values_bit_offset"],
                              validity_bit_offset=p["validity_bit_offset"])
        else:
            dc = DeviceColumn(c.ptype, True, c.rows, up(p["values"]), view, None, validity_bit_offset=p["validity_bit_offset"])
        enc = write.encode_columns(gpu_ctx, [dc], options_of(c))
        gpu_ctx.synchronize()
        assert np.array_equal(enc[0].metas_array(), want_metas), c.name
        assert np.array_equal(enc[0].pages_numpy(), want_pages), c.name
        del buf, view, dc
