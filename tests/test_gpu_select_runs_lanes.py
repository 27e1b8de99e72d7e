"""The run-level selector (sb_select_runs.h) holds a chunk's rows lane-contiguous: a wave owns 1024 rows, piece u of
lane l holds rows 1024 w + u * 64 * PR + l * PR + i (PR = 2 rows of 8 bytes, 4 rows of 4 bytes), a change is found by
comparing with the lane below (lane 0: with lane 63 of the piece before, or the row before the wave's first) and stored
from a fixed register under the compare's mask.  The shapes here are the smallest at which that addressing can go
wrong: pages that end inside a piece / a wave / a chunk, changes exactly at and next to every kind of seam, nulls across
the seams, pieces whose rows all differ, pages that leave the kernel (more than 640 changes in a chunk) early and late,
pages that do not start on a 16-byte boundary, equal keys with different bits, the sortedness flag of 4-byte integers
across the seams, a sliced column.  Every case is compared with the oracle: codecs, metas, page bytes.

`cases()` builds every case on the CPU (name, column, options, what the oracle has to choose for the case to exercise its
path); the oracle side of each was checked on the CPU when the file was written."""
import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.test_gpu_select import check

pytestmark = pytest.mark.gpu

TYPES = (S.T_F64, S.T_I64, S.T_I32, S.T_F32)
WIDE = (S.T_F64, S.T_I64)
CHUNK = 4096
RUNS_CAP = 640
ONLY_RLE = (S.DICT, S.FREQ, S.PATAS, S.BITPACK, S.DELTABP)


def col_of(vals, ptype, valid=None):
    vals = np.asarray(vals)
    if vals.dtype != gen.NP_OF[ptype]:
        vals = vals.astype(gen.NP_OF[ptype])
    validity = None if valid is None else gen.pack_bits(valid)
    return dict(ptype=ptype, nullable=validity is not None, rows=vals.size, values=vals, validity=validity, offsets=None)


def scattered(ids):
    """distinct, unordered values (exact in f32) for run ids: neighbours differ, nothing is sorted"""
    return (np.asarray(ids, np.int64) * 7919 + 13) % 65521


def run_values(rows, length, shift=0):
    """runs of `length` rows whose changes sit at k * length + shift"""
    return scattered((np.arange(rows) - shift + length) // length)


def seam_lengths(ptype):
    return (128 if ptype in WIDE else 256, 1024, 4096)   # lane 0 of every piece, wave seam, chunk seam


def changes_in_chunk(vals, chunk):
    """what the kernel counts in a chunk: its first row, and every other row whose bits differ from the row before"""
    v = np.asarray(vals)
    bits = v.view(np.uint8).reshape(v.size, -1)
    lo, hi = chunk * CHUNK, min((chunk + 1) * CHUNK, v.size)
    return 1 + int((bits[lo + 1:hi] != bits[lo:hi - 1]).any(axis=1).sum())


ROW_COUNTS = (1, 2, 3, 127, 128, 129, 255, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 12289)
OPT = dict(max_page_size=65536, ratio=2.0, forbidden=())
# A page of 65 536 rows in runs of 1024 or 4096 rows has 64 or 16 distinct values, and Dict's estimate (dict.rs:109-120) counts
# no index bytes below 256 of them: the oracle then takes Dict whatever the runs look like.  The cases that are about the
# RLE records at the seams forbid it (and Freq, which takes a page whose top value fills 90 % of it).
RLE_OPT = dict(max_page_size=65536, ratio=2.0, forbidden=(S.DICT, S.FREQ))


def cases_row_counts(ptype):
    rng = np.random.default_rng(5)
    for rows in ROW_COUNTS:
        v = run_values(rows, 5)
        yield "rows%d" % rows, col_of(v, ptype), OPT, None
        yield "rows%d_nulls" % rows, col_of(v, ptype, rng.random(rows) < 0.9), OPT, None


def cases_seams(ptype):
    rows = 65536 + 2 * CHUNK + 5
    for length in seam_lengths(ptype):
        for shift in (0, 1, -1):   # the change on lane 0 of a piece, on lane 1, on lane 63 of the piece before
            yield "runs%d%+d" % (length, shift), col_of(run_values(rows, length, shift), ptype), RLE_OPT, S.RLE
            yield "runs%d%+d_any" % (length, shift), col_of(run_values(rows, length, shift), ptype), OPT, None


def cases_null_seams(ptype):
    rows = 65536 + 2 * CHUNK + 5
    for length in seam_lengths(ptype):
        ok = np.ones(rows, bool)
        for seam in range(length, rows, length):
            ok[seam - 3:seam + 4] = False   # the run's first valid row lies in the next piece / wave / chunk
        yield "nullseam%d" % length, col_of(run_values(rows, length), ptype, ok), RLE_OPT, S.RLE
        yield "nullseam%d_any" % length, col_of(run_values(rows, length), ptype, ok), OPT, None
    v = run_values(65536, 512)
    ok = np.ones(65536, bool)
    ok[:4100] = False
    yield "first4100null", col_of(v, ptype, ok), RLE_OPT, S.RLE
    ok = np.ones(65536, bool)
    ok[-4100:] = False
    yield "last4100null", col_of(v, ptype, ok), RLE_OPT, S.RLE


def cases_dense_pieces(ptype):
    """64 runs of one row (every row of 32 / 16 lanes' pieces differs), then one run of 4032 rows, repeated: 65 changes per chunk"""
    rows = 65536 + CHUNK + 100
    i = np.arange(rows)
    ids = np.where(i % CHUNK < 64, i, (i // CHUNK) * CHUNK + 64)
    assert changes_in_chunk(scattered(ids).astype(gen.NP_OF[ptype]), 3) == 65
    yield "dense64", col_of(scattered(ids), ptype), RLE_OPT, S.RLE
    # the same 64 rows in the middle of a wave's rows and across a wave seam
    for at in (1500, 2048 - 32):
        ids = np.where((i % CHUNK >= at) & (i % CHUNK < at + 64), i, (i // CHUNK) * CHUNK + (i % CHUNK >= at + 64))
        yield "dense64at%d" % at, col_of(scattered(ids), ptype), RLE_OPT, S.RLE


def cases_fallback(ptype):
    """more than RUNS_CAP changes in one chunk: the page goes to the row-level kernel (uniformly, early or late); the
    ordinary page behind it stays"""
    rows = 65536 + 10000
    i = np.arange(rows)
    for name, first in (("early", 0), ("late", 65536 - CHUNK)):   # the page's first chunk / its last full chunk
        ids = np.where((i >= first + 100) & (i < first + 100 + 699), i, i // 2048 + (i >= first + 100 + 699) * 100000)
        v = scattered(ids).astype(gen.NP_OF[ptype])
        assert changes_in_chunk(v, first // CHUNK) >= 700 > RUNS_CAP, changes_in_chunk(v, first // CHUNK)
        assert all(changes_in_chunk(v, c) <= 4 for c in range(rows // CHUNK) if c != first // CHUNK)
        yield "fallback_" + name, col_of(v, ptype), OPT, None


def cases_speculation(ptype):
    """8192 rows of long runs, then runs of 3 rows; everything but RLE forbidden (test_rle_chosen_after_the_speculation_stopped)"""
    rng = np.random.default_rng(3)
    rows = 2 * 65536
    i = np.arange(rows)
    ids = np.where(i % 65536 < 8192, i // 1024, 1000 + i // 3)
    v = scattered(ids) + (rng.integers(0, 3, rows // 3 + 1)[i // 3] * (i % 65536 >= 8192))
    yield "spec_off", col_of(v, ptype, rng.random(rows) < 0.95), dict(max_page_size=65536, ratio=1.1, forbidden=ONLY_RLE), S.RLE


def cases_misaligned():
    """pages of 1001 f64 rows / 1003 i32 rows: page starts are not 16-byte aligned, the 16-byte loads straddle"""
    rng = np.random.default_rng(8)
    for ptype, page in ((S.T_F64, 1001), (S.T_I32, 1003)):
        v = run_values(5005, 5)
        opt = dict(max_page_size=page, ratio=2.0, forbidden=())
        yield "misaligned%d" % page, col_of(v, ptype), opt, None
        yield "misaligned%d_nulls" % page, col_of(v, ptype, rng.random(5005) < 0.9), opt, None
        yield "misaligned%d_runs40" % page, col_of(run_values(5005, 40), ptype, rng.random(5005) < 0.9), opt, None


def cases_equal_keys():
    """+0.0 / -0.0 and NaNs with two payloads: different bits, equal keys.  Periods of 2 and 3 rows (as many changes as a
    chunk can have: the page leaves the kernel at once) and of 16 and 24 rows (it stays)"""
    rng = np.random.default_rng(4)
    rows = 65536 + 5000
    i = np.arange(rows)
    for ptype, fl, ui, nan_a, nan_b in ((S.T_F64, np.float64, np.uint64, 0x7FF8000000000000, 0xFFF8000000000123),
                                        (S.T_F32, np.float32, np.uint32, 0x7FC00000, 0xFFC00123)):
        for zp, np_ in ((2, 3), (16, 24)):
            z = np.zeros(rows, fl)
            z[(i // zp) % 2 == 1] = -0.0
            nans = np.where((i // np_) % 2 == 0, nan_a, nan_b).astype(ui).view(fl)
            ok = rng.random(rows) < 0.9
            yield "zeros_every%d" % zp, col_of(z, ptype, ok), OPT, None
            yield "nans_every%d" % np_, col_of(nans, ptype, ok), OPT, None
            yield "zeros%d_nans%d" % (zp, np_), col_of(np.where((i // 3000) % 2 == 0, z, nans), ptype, ok), OPT, None


def cases_sortedness():
    """ascending runs of 64 with ONE descending step, placed on a piece / wave / chunk seam: the sortedness flag compares a
    run's value with the row before it (Bitpacking / DeltaBitpacking eligibility)"""
    opt = dict(max_page_size=65536, ratio=1.05, forbidden=())
    for ptype in (S.T_I32, S.T_U32):
        for step in (128, 1024, 4096):
            a = np.repeat(np.arange(1024) + 10, 64)
            a[step:step + 64] = a[step - 1] - 1
            assert np.count_nonzero(np.diff(a) < 0) == 1 and a[step] < a[step - 1]
            yield "descending_at%d" % step, col_of(a, ptype), opt, None
        yield "ascending", col_of(np.repeat(np.arange(1024) + 10, 64), ptype), opt, None


def sliced(ptype, start=13):
    """rows [start, start + n) of a longer column: the validity bitmap keeps its bytes and gets a bit offset, the values
    start `start` rows into their buffer (104 / 52 bytes: not 16-byte aligned)"""
    rng = np.random.default_rng(6)
    total = 65536 + 9000
    v = run_values(total, 37).astype(gen.NP_OF[ptype])
    ok = rng.random(total) < 0.85
    return v, ok, start


def cases(ptype=None):
    for t in TYPES if ptype is None else (ptype,):
        for gen_ in (cases_row_counts, cases_seams, cases_null_seams, cases_dense_pieces, cases_fallback, cases_speculation):
            for name, col, opt, want in gen_(t):
                yield "%s/type%d" % (name, t), col, opt, want
    if ptype is None:
        for gen_ in (cases_misaligned, cases_equal_keys, cases_sortedness):
            yield from gen_()


def run(ctx, it):
    for name, col, opt, want in it:
        try:
            codecs = check(ctx, col, **opt)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None
        if want is not None:
            assert (codecs == want).all(), "%s: the oracle chose %s" % (name, codecs.tolist())


@pytest.mark.parametrize("ptype", TYPES)
def test_pages_that_end_inside_a_piece_a_wave_a_chunk(gpu_ctx, ptype):
    run(gpu_ctx, cases_row_counts(ptype))


@pytest.mark.parametrize("ptype", TYPES)
def test_a_change_at_every_kind_of_seam(gpu_ctx, ptype):
    run(gpu_ctx, cases_seams(ptype))


@pytest.mark.parametrize("ptype", TYPES)
def test_nulls_across_the_seams(gpu_ctx, ptype):
    run(gpu_ctx, cases_null_seams(ptype))


@pytest.mark.parametrize("ptype", TYPES)
def test_pieces_whose_rows_all_differ(gpu_ctx, ptype):
    run(gpu_ctx, cases_dense_pieces(ptype))


@pytest.mark.parametrize("ptype", TYPES)
def test_fallback_in_the_first_and_in_the_last_full_chunk(gpu_ctx, ptype):
    run(gpu_ctx, cases_fallback(ptype))


@pytest.mark.parametrize("ptype", TYPES)
def test_speculation_switched_off_mid_page(gpu_ctx, ptype):
    run(gpu_ctx, cases_speculation(ptype))


def test_pages_that_start_off_a_16_byte_boundary(gpu_ctx):
    run(gpu_ctx, cases_misaligned())


def test_equal_keys_with_different_bits(gpu_ctx):
    run(gpu_ctx, cases_equal_keys())


def test_sortedness_of_4_byte_integers_across_the_seams(gpu_ctx):
    run(gpu_ctx, cases_sortedness())


@pytest.mark.parametrize("ptype", [S.T_F64, S.T_I32])
def test_sliced_column_with_a_validity_bit_offset(gpu_ctx, ptype):
    import torch
    from strawboat_amd import write
    from tests.test_gpu_encode import write_options
    v, ok, start = sliced(ptype)
    n = v.size - start
    dev = gpu_ctx.torch_device
    values = torch.from_numpy(v.view(np.uint8).copy()).to(dev)[start * v.itemsize:]
    validity = torch.from_numpy(gen.pack_bits(ok)[start // 8:].copy()).to(dev)
    dc = write.DeviceColumn(ptype, True, n, values, validity, validity_bit_offset=start % 8)
    enc = write.write(gpu_ctx, dc, write_options(**OPT))
    check(gpu_ctx, col_of(v[start:], ptype, ok[start:]), enc=enc, **OPT)
