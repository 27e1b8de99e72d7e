"""Writes on contexts of every launch-hint history (tests/write_hint_cases.py), against the oracle's bytes.

Every case gets a context of its own.  Every interval of its history, its probe and the probe once more are issued as the
case's entry point says; after the interval's synchronize the metas and the page bytes of every column of every call are
compared with the oracle's (lz4_exact, as tests.test_gpu_encode.write_options defaults) -- never with what the device wrote
earlier --, and sb_ctx_replays must have grown by exactly what the table's model of apply_enc_hint / EncLaunch::unused
says.  A small write of another shape closes the case: the context still works.

With SB_NO_HINTS=1 the model's counts are all 0 and nothing else changes.  With SB_BIN_FUSED=0 the model is asked for that
switch's counts; the cases whose claim rests on k_enc_bin_page (the counts differ between the two) skip themselves, as
tests/test_gpu_select.py::test_a_skipped_dict_emitter_is_replayed does.

The module prints its wall time when its last test ends (run with -s to see it).  Measured on an MI355X: 379 cases in
3.9 s (4.1 s with SB_NO_HINTS=1, 3.8 s with SB_BIN_FUSED=0), the slowest 0.1 s apart from the first, which loads the
library (2 s); the 192 tests of tests/test_gpu_hints.py took 8.5 s in the same run."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests import write_hint_cases as W
from tests.test_gpu_encode import to_device_column, write_options

pytestmark = pytest.mark.gpu


def _switches():
    """(no_hints, bin_fused) as sb_ctx_create reads them"""
    nh, bf = os.environ.get("SB_NO_HINTS"), os.environ.get("SB_BIN_FUSED")
    return nh is not None and nh[:1] != "0", not (bf is not None and bf[:1] == "0")


_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    _t0[0] = time.perf_counter()
    yield
    print("\ntests/test_gpu_write_hints.py: %.1f s for %d cases" % (time.perf_counter() - _t0[0], len(W.CASES)))


class DeviceCall:
    """one sb_write_columns call on device buffers: enqueue, and after the synchronize check every column"""

    def __init__(self, ctx, names):
        from strawboat_amd import write
        self.want = [W.written(W.VARIANT[n]) for n in names]
        options = W.VARIANT[names[0]].table.options
        assert all(W.VARIANT[n].table.options == options for n in names), "the columns of one call share its options"
        cols = [to_device_column(ctx, col) for col, _, _ in self.want]
        self.enc = write.encode_columns(ctx, cols, write_options(**options))

    def check(self, what):
        for k, ((col, pages, metas), enc) in enumerate(zip(self.want, self.enc)):
            assert np.array_equal(enc.metas_array(), metas), "%s, column %d: PageMeta differ from the oracle's" % (what, k)
            got = enc.pages_numpy()
            assert got.size == pages.size and np.array_equal(got, pages), "%s, column %d: page bytes differ from the oracle's" % (what, k)


class HostCall:
    """SB_MEM_HOST: host Arrow buffers in, host page bytes out (one primitive column: a single group)"""

    def __init__(self, ctx, names):
        from strawboat_amd import _native as N
        from strawboat_amd.write import options_c
        (name,) = names
        self.col, self.pages, self.metas = W.written(W.VARIANT[name])
        col = self.col
        assert col["offsets"] is None
        lib = ctx._lib
        self.oc = options_c(write_options(**W.VARIANT[name].table.options))
        self.vals = np.array(np.ascontiguousarray(col["values"]).view(np.uint8), copy=True)
        npg = C.c_uint64()
        bound = lib.sb_write_bound(col["ptype"], 0, col["rows"], 0, C.byref(self.oc), C.byref(npg))
        self.out = np.full(bound, 0xA5, np.uint8)
        self.m = (N.PageMetaC * npg.value)()
        self.cw = (N.ColumnWriteC * 1)()
        cw = self.cw[0]
        cw.physical_type, cw.is_nullable, cw.rows = col["ptype"], 0, col["rows"]
        cw.values, cw.values_len = self.vals.ctypes.data, self.vals.size
        cw.out_pages, cw.out_capacity = self.out.ctypes.data, self.out.size
        cw.out_metas, cw.n_pages_capacity = self.m, npg.value
        ctx._check(lib.sb_write_columns(ctx._h, self.cw, 1, C.byref(self.oc), N.SB_MEM_HOST))

    def check(self, what):
        cw = self.cw[0]
        got = np.array([[self.m[i].length, self.m[i].num_values] for i in range(cw.n_pages)], np.uint64).reshape(-1, 2)
        assert np.array_equal(got, self.metas), "%s: PageMeta differ from the oracle's" % what
        assert cw.out_len == self.pages.size and np.array_equal(self.out[:cw.out_len], self.pages), "%s: page bytes differ from the oracle's" % what


def run_interval(ctx, interval, what):
    """the interval's calls, one synchronize, every output against the oracle; returns the replays it cost"""
    r0 = ctx.replays()
    calls = [(HostCall if mem == W.MEM_HOST else DeviceCall)(ctx, names) for names, mem in interval]
    ctx.synchronize()
    for k, call in enumerate(calls):
        call.check("%s, call %d" % (what, k))
    return ctx.replays() - r0


@pytest.mark.parametrize("case", W.CASES, ids=repr)
def test_case(case):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    import strawboat_amd as sb
    no_hints, bin_fused = _switches()
    exp = case.expected(no_hints, bin_fused)
    if not bin_fused and case.expected(no_hints, True) != exp:
        pytest.skip("SB_BIN_FUSED=0: the case's claim rests on k_enc_bin_page")
    ctx = sb.Context(0)
    try:
        forks0 = ctx.side_forks()
        steps = ["history interval %d" % k for k in range(len(case.history))] + ["the probe", "the probe again"]
        for what, interval, replays in zip(steps, case.intervals(), exp):
            got = run_interval(ctx, interval, what)
            assert got == replays, "%s: %d replays, the model says %d" % (what, got, replays)
        if case.entry == "mixed":
            assert ctx.side_forks() > forks0, "the mixed-kind call did not take the side-stream path"
        assert run_interval(ctx, (W.call_of("other/uniform"),), "the closing write") == 0   # the context still works
    finally:
        ctx.close()
