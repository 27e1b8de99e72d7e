"""sb_key_buckets without a GPU: the symbol is exported, the ctypes struct has the header's layout, the preparation of
csrc/sb_key_buckets_prep.h (the checks of the bounds and ids, the order keys, the id of each bucket, the trip count, the two
keys outside which a float is a NaN) agrees with Python in a stand-alone host program, the Python layer refuses what needs
no device before a context is touched, the reference that tests/test_gpu_key_buckets.py compares the device with
(tests/key_buckets_ref.py) is checked against a plain Python loop, and every column of tests/key_buckets_cases.py carries
its codec on every page."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.key_buckets import KeyBuckets, KeyBucketsBatch, bounds_values, check_column, key_buckets
from strawboat_amd.types import PhysicalType as P
from tests import key_buckets_cases as Bc
from tests import key_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")
NONE = 0xFFFFFFFF

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, ids=64, ids_capacity=72, id_width=80, flags=84, bounds=88, bucket_ids=96, n_bounds=104,
               nan_id=112, reserved0=116, reserved=120, rows=128, selected=136, count=144, matched=152, nans=160)


def test_symbol_is_declared_and_exported():
    import strawboat_amd as sb
    assert "sb_key_buckets" in N.EXPORTS
    assert sb.key_buckets is key_buckets and sb.KeyBucketsBatch is KeyBucketsBatch and sb.KeyBuckets is KeyBuckets
    assert {"key_buckets", "KeyBucketsBatch", "KeyBuckets", "group_by_buckets", "histogram"} <= set(sb.__all__)
    assert callable(sb.group_by_buckets) and callable(sb.histogram)
    assert re.search(r"\bsb_key_buckets\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_key_buckets$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    assert C.sizeof(N.ColumnKeyBucketsC) == 168
    assert [name for name, _ in N.ColumnKeyBucketsC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnKeyBucketsC, f).offset == off, f
    # the first 84 bytes are sb_column_key_lookup's
    for f in list(OFFSETS)[:12]:
        assert getattr(N.ColumnKeyLookupC, f).offset == OFFSETS[f], f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_key_buckets));\n'
                   '    printf("MAX %u\\nCLOSED %u\\nNONE %u\\nGROUPS %u\\n", SB_BUCKET_MAX_BOUNDS, SB_BUCKET_RIGHT_CLOSED, SB_KEY_ID_NONE, SB_AGG_LARGE_MAX_GROUPS);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_key_buckets, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 168
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["MAX"]) == N.SB_BUCKET_MAX_BOUNDS == 1023 and int(got["GROUPS"]) == 1024
    assert int(got["CLOSED"]) == N.SB_BUCKET_RIGHT_CLOSED == 1 and int(got["NONE"]) == N.SB_KEY_ID_NONE == NONE
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_key_buckets_host.py)")[1].split("*/")[0]
    assert "sb_column_key_buckets 168 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_column_key_buckets 168 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


# ---- the preparation in a host program of its own.  Input, one block per case:
#   case <kind> <w> <flags> <id_width> <n> <has_ids> <nan_id>   then n words of hex (the bounds' bytes), then n + 1 ids if has_ids
# Output per case: "refused bounds", "refused ids" or "ok <n> <steps> <nan_lo> <nan_hi>" and n lines "<order key> <id>", then
# the id of the last bucket.
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "sb_key_buckets_prep.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned kind, w, flags, id_width, has_ids;
    unsigned long long n, nan_id;
    while (fscanf(f, " case %u %u %u %u %llu %u %llu", &kind, &w, &flags, &id_width, &n, &has_ids, &nan_id) == 7) {
        // every buffer of exactly its size on the heap: a load outside one is the sanitizer's
        uint8_t* bounds = n ? new uint8_t[n * w] : nullptr;
        for (unsigned long long i = 0; i < n; i++) {
            char word[64];
            if (fscanf(f, " %63s", word) != 1) return 3;
            for (unsigned b = 0; b < w; b++) {
                char hx[3] = {word[2 * b], word[2 * b + 1], 0};
                bounds[i * w + b] = (uint8_t)strtoul(hx, nullptr, 16);
            }
        }
        uint32_t* ids = has_ids ? new uint32_t[n + 1] : nullptr;
        for (unsigned long long i = 0; has_ids && i <= n; i++) {
            unsigned long long id;
            if (fscanf(f, " %llu", &id) != 1) return 3;
            ids[i] = (uint32_t)id;
        }
        const char* why = sb_buckets::check_bounds(kind, w, flags, bounds, n);
        // (more bounds than the limit: the ids are not looked at, there would be more than the buffer holds)
        if (why) {
            printf("refused bounds\n");
        } else if ((why = sb_buckets::check_ids(kind, ids, n, id_width, (uint32_t)nan_id))) {
            printf("refused ids\n");
        } else {
            const sb_buckets::Prepared pr = sb_buckets::prepare(kind, w, bounds, ids, n);
            if (pr.keys.size() != pr.n || pr.ids.size() != pr.n + 1u || pr.n != n) return 4;
            printf("ok %u %u %016llx %016llx\n", pr.n, pr.steps, (unsigned long long)pr.nan_lo, (unsigned long long)pr.nan_hi);
            for (uint32_t i = 0; i < pr.n; i++) printf("%016llx %u\n", (unsigned long long)pr.keys[i], pr.ids[i]);
            printf("%u\n", pr.ids[pr.n]);
        }
        delete[] bounds;
        delete[] ids;
    }
    fclose(f);
    return 0;
}
"""


def _build_program(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = hipcc if os.path.exists(hipcc) else (shutil.which("clang++") or shutil.which("c++") or shutil.which("g++"))
    assert cxx, "no host C++ compiler"
    src = tmp_path / "prep.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "prep"
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([cxx, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
        syms = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout + \
            subprocess.run(["nm", str(exe)], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    else:
        warnings.warn("the compiler has no sanitizer runtime (%r): the preparation is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    return exe




def _kind(dt):
    dt = np.dtype(dt)
    return 0 if dt.kind == "u" else 1 if dt.kind == "i" else 2 if dt.itemsize == 4 else 3


def _order_key(dt, raw):
    """Python's own statement of the order: unsigned as is, signed with the sign bit flipped after the sign extension,
    floats in the total order with -0.0 folded onto +0.0.  raw: the value's bits as an unsigned int."""
    dt = np.dtype(dt)
    bits = 8 * dt.itemsize
    if dt.kind == "u":
        return raw
    if dt.kind == "i":
        v = raw - (1 << bits) if raw >> (bits - 1) else raw
        return v + (1 << 63)
    if raw << 1 & ((1 << bits) - 1) == 0:
        raw = 0
    return ((1 << bits) - 1) ^ raw if raw >> (bits - 1) else raw | (1 << (bits - 1))


def _bits(arr):
    arr = np.asarray(arr)
    return [int(x) for x in arr.view("<u%d" % arr.dtype.itemsize).tolist()]


def _expect(bounds, flags, bucket_ids, id_width, nan_id):
    """what the program must print for one case"""
    dt = bounds.dtype
    n = bounds.size
    keys = [_order_key(dt, r) for r in _bits(bounds)]
    if flags & ~1 or n > 1023:
        return ["refused bounds"]
    if dt.kind == "f":
        lo = _order_key(dt, _bits(np.array([-np.inf], dt))[0])
        hi = _order_key(dt, _bits(np.array([np.inf], dt))[0])
    else:
        lo, hi = 0, (1 << 64) - 1
    if any(k < lo or k > hi for k in keys) or any(b <= a for a, b in zip(keys, keys[1:])):
        return ["refused bounds"]
    none = (1 << (8 * id_width)) - 1
    handed = [n] if bucket_ids is None else [i for i in bucket_ids if i != NONE]
    if any(i >= none for i in handed):
        return ["refused ids"]
    if nan_id != NONE and (dt.kind != "f" or nan_id >= none):
        return ["refused ids"]
    steps = 0
    while (1 << steps) < n + 1:
        steps += 1
    ids = list(range(n + 1)) if bucket_ids is None else list(bucket_ids)
    return ["ok %d %d %016x %016x" % (n, steps, lo, hi)] + ["%016x %d" % (k, i) for k, i in zip(keys, ids)] + ["%d" % ids[n]]


def _cases():
    """(bounds as a typed array, flags, bucket_ids or None, id_width, nan_id)"""
    rng = np.random.default_rng(5)
    out = []
    f64, f32, i64 = np.float64, np.float32, np.int64
    for n in (0, 1, 2, 3, 1022, 1023, 1024):                                  # the numbers of bounds, 1024 refused
        out.append((np.arange(n, dtype=i64) * 3 - 100, 0, None, 2, NONE))
        out.append((np.arange(n, dtype=f64) * 0.5 - 100, 1, None, 2, 7))
        out.append((np.arange(n, dtype=i64), 0, None, 1, NONE))               # n >= 255 does not fit one byte
    out.append((np.array([1, 2, 2, 3], i64), 0, None, 1, NONE))               # equal neighbours
    out.append((np.array([1.0, 2.0, 2.0], f64), 0, None, 1, NONE))
    out.append((np.array([3, 2, 1], i64), 0, None, 1, NONE))                  # decreasing
    out.append((np.array([1, 2, 0], np.uint8), 0, None, 1, NONE))
    out.append((np.array([-0.0, 0.0], f64), 0, None, 1, NONE))                # -0.0 == +0.0: not increasing
    out.append((np.array([0.0, -0.0], f32), 0, None, 1, NONE))
    out.append((np.array([-1.0, -0.0, 1.0], f64), 0, None, 1, NONE))          # ... alone it is a bound like any other
    out.append((np.array([-1.0, 0.0, 1.0], f32), 0, None, 1, NONE))
    for dt in (f32, f64):
        nans = Bc.nan_bits(Bc.S.T_F32 if dt is f32 else Bc.S.T_F64).view(dt)
        for x in nans:                                                        # NaN as the first and as the last bound
            out.append((np.array([x, 1.0, 2.0], dt), 0, None, 1, NONE))
            out.append((np.array([1.0, 2.0, x], dt), 0, None, 1, NONE))
        out.append((np.array([-np.inf, 0.0, np.inf], dt), 0, None, 1, 3))     # +-inf are bounds
        out.append((np.array([-np.inf, np.inf], dt), 1, [5, NONE, 5], 1, NONE))
        out.append((np.array([np.inf, -np.inf], dt), 0, None, 1, NONE))
        fi = np.finfo(dt)
        tiny = np.array([1], "<u%d" % np.dtype(dt).itemsize).view(dt)[0]
        out.append((np.array([-fi.max, -fi.tiny, -tiny, 0.0, tiny, fi.tiny, fi.max], dt), 0, None, 1, NONE))   # denormals
        out.append((np.array([-tiny, -0.0, tiny], dt), 1, None, 1, 254))
    for dt in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64):   # the extremes of the types
        info = np.iinfo(dt)
        mid = [-1, 0, 1] if info.min < 0 else [1, info.max // 2, info.max // 2 + 1]
        out.append((np.array([info.min] + mid + [info.max], dt), 0, None, 1, NONE))
        out.append((np.array([info.max, info.min], dt), 0, None, 1, NONE))    # (decreasing under the signedness)
        out.append((np.array([info.min, info.max], dt), 1, [0, 1, 0], 1, 3))  # nan_id on an integer column
    for k in range(0, 10):                                                    # the trip count at n = 2^k - 1 and 2^k
        for n in ((1 << k) - 1, 1 << k):
            out.append((np.sort(rng.permutation(5000)[:n]).astype(np.int32), 0, None, 2, NONE))
    b3 = np.array([10, 20, 30], np.int16)
    for w, largest in ((1, 254), (2, 65534), (4, 0xFFFFFFFE)):                # ids at the edge of each width
        out.append((b3, 0, [largest, 0, NONE, largest], w, NONE))
        out.append((b3, 0, [largest + 1, 0, 0, 0], w, NONE))
        out.append((b3.astype(f32), 0, [0, 0, 0, 0], w, largest))
        out.append((b3.astype(f32), 0, [0, 0, 0, 0], w, largest + 1))         # (all ones of 4 bytes is "no id": fine there)
        out.append((b3.astype(f64), 1, [NONE] * 4, w, NONE))
    out.append((np.arange(254, dtype=np.int32), 0, None, 1, NONE))            # bucket 254 is the last id of one byte
    out.append((np.arange(255, dtype=np.int32), 0, None, 1, NONE))
    out.append((b3, 2, None, 1, NONE))                                        # an unknown flag bit
    out.append((b3, 0x80000001, None, 1, NONE))
    return out


def test_preparation_in_a_stand_alone_program_against_python(tmp_path):
    exe = _build_program(tmp_path)
    lines, want = [], []
    for bounds, flags, ids, id_width, nan_id in _cases():
        w = bounds.dtype.itemsize
        # (a list beyond the limit is refused before its ids are read: none are sent)
        lines.append("case %d %d %d %d %d %d %d" % (_kind(bounds.dtype), w, flags, id_width, bounds.size, ids is not None, nan_id))
        lines += [bounds[i:i + 1].tobytes().hex() for i in range(bounds.size)]
        if ids is not None:
            lines.append(" ".join(str(i) for i in ids))
        want += _expect(bounds, flags, ids, id_width, nan_id)
    inp = tmp_path / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, "line %d: %r, want %r" % (i, g, w_)
    oks = [x[:10] for x in want if x.startswith("ok ")]
    assert {"ok 1023 10", "ok 1022 10", "ok 0 0 000", "ok 1 1 000", "ok 3 2 000", "ok 511 9 0", "ok 512 10 "} <= set(oks)
    assert want.count("refused bounds") >= 30 and want.count("refused ids") >= 12
    # the order keys of the floats: -0.0 and +0.0 are one key, and the NaNs lie outside [key(-inf), key(+inf)]
    for dt in (np.float32, np.float64):
        z = _bits(np.array([-0.0, 0.0], dt))
        assert _order_key(dt, z[0]) == _order_key(dt, z[1])
        lo, hi = (_order_key(dt, r) for r in _bits(np.array([-np.inf, np.inf], dt)))
        for r in _bits(Bc.nan_bits(Bc.S.T_F32 if dt is np.float32 else Bc.S.T_F64)):
            assert not lo <= _order_key(dt, r) <= hi
        vals = np.array([-np.inf, -1.5, -0.0, 1e-40, 2.0, np.inf], dt)
        keys = [_order_key(dt, r) for r in _bits(vals)]
        assert keys == sorted(keys) and lo == keys[0] and hi == keys[-1]


# ---- the Python layer
class Ctx:
    """a context that fails when touched: only asked where its tensors live"""

    def __getattr__(self, name):
        if name == "torch_device":
            import torch
            return torch.device("cpu")
        raise AssertionError("the context was touched (%s) before the arguments were checked" % name)


NUMERIC = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64)


def test_check_column_refuses_on_the_host():
    for ptype in NUMERIC:
        flt = ptype in (P.FLOAT32, P.FLOAT64)
        assert check_column(ptype, 33, 8, 5, None, None, None) == (None, NONE, 1)
        assert check_column(ptype, 33, None, 254, None, None, None)[2] == 1     # buckets 0 .. 254
        assert check_column(ptype, 33, None, 255, None, None, None)[2] == 2     # bucket 255 is all ones of one byte
        assert check_column(ptype, 33, None, 1023, None, None, None)[2] == 2
        assert check_column(ptype, 33, None, 0, None, None, None)[2] == 1
        ids, nan, w = check_column(ptype, 33, None, 2, [7, None, 65535], None, None)
        assert w == 4 and ids.dtype == np.uint32 and ids.tolist() == [7, NONE, 65535] and nan == NONE
        assert check_column(ptype, 33, None, 1, [NONE, NONE], None, None)[2] == 1   # every bucket dropped
        assert check_column(ptype, 33, None, 1, [0, 65534], None, None)[2] == 2
        assert check_column(ptype, 33, None, 1, None, NONE, None)[1] == NONE
        if flt:
            assert check_column(ptype, 33, None, 1, None, 300, None)[1:] == (300, 2)
            assert check_column(ptype, 33, None, 1, None, 254, 1)[1:] == (254, 1)
            for nan, w in ((255, 1), (65535, 2), (-1, 4), (1.0, 4), (True, 4), ("1", 4)):
                with pytest.raises(ValueError):
                    check_column(ptype, 33, None, 1, None, nan, w)
        else:
            with pytest.raises(ValueError):
                check_column(ptype, 33, None, 1, None, 0, None)                 # nan_id on an integer column
    for ptype in (P.BINARY, P.LARGE_BINARY, P.BOOLEAN, P.INT128, P.INT256, P.NULL):
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, 5, None, None, None)
        with pytest.raises(ValueError):
            bounds_values(ptype, [1, 2])
    with pytest.raises(ValueError):
        check_column(P.INT64, 33, 8, 1024, None, None, 2)
    for w in (0, 3, 8, "1", True, 2.0):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 5, None, None, w)
    for n, ids, w in ((255, None, 1), (2, [1, 2, 255], 1), (2, [1, 2, 65535], 2), (0, [-1], 4), (0, [1.5], 4), (1, [1], 4), (0, [True], 4),
                      (0, ["1"], 4), (0, [1 << 32], 4)):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, n, ids, None, w)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):
        with pytest.raises(ValueError):
            check_column(P.INT32, rows, nbytes, 5, None, None, 1)
    # the bounds
    assert bounds_values(P.FLOAT64, [-math.inf, -0.0, 1, math.inf]).dtype == np.float64
    assert bounds_values(P.INT8, []).size == 0 and bounds_values(P.UINT64, [0, 2 ** 64 - 1]).tolist() == [0, 2 ** 64 - 1]
    for ptype, b in ((P.FLOAT64, [-0.0, 0.0]), (P.FLOAT32, [0.0, -0.0]), (P.FLOAT64, [1.0, math.nan]), (P.FLOAT32, [math.nan]),
                     (P.INT32, [1, 1]), (P.INT32, [2, 1]), (P.INT8, [128]), (P.UINT8, [-1]), (P.INT32, [1.5]), (P.INT32, [b"a"]),
                     (P.FLOAT64, ["1"]), (P.INT32, [True]), (P.INT32, np.array([1, 2], np.int64)), (P.INT32, np.array([[1, 2]], np.int32)),
                     (P.FLOAT32, np.array([1.0], np.float64)), (P.INT32, np.arange(1024, dtype=np.int32)), (P.FLOAT64, list(range(1024)))):
        with pytest.raises(ValueError):
            bounds_values(ptype, b)


def test_bad_arguments_raise_before_a_context_is_touched():
    import torch
    from strawboat_amd import group_by_buckets, histogram
    from strawboat_amd.read import ColumnPages
    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT32, False, torch.zeros(100, dtype=torch.uint8), metas)
    fcol = ColumnPages(P.FLOAT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    ok = np.array([1, 2, 3], np.int32)
    fok = [0.5, 1.5]
    bad = [
        dict(cols=[col], bounds=[ok], selection=torch.zeros(4, dtype=torch.uint8)),        # a bitmap of 4 bytes for 40 rows
        dict(cols=[col], bounds=[ok, ok]),                                                # one list per column
        dict(cols=[col, col], bounds=[ok]),
        dict(cols=[col], bounds=[np.array([1, 2], np.int64)]),                            # not the column's dtype
        dict(cols=[col], bounds=[[1, 2 ** 31]]),                                          # does not fit int32
        dict(cols=[col], bounds=[[1.5]]),
        dict(cols=[col], bounds=[[3, 2]]),                                                # decreasing
        dict(cols=[col], bounds=[[2, 2]]),
        dict(cols=[fcol], bounds=[[-0.0, 0.0]]),
        dict(cols=[fcol], bounds=[[0.0, math.nan]]),
        dict(cols=[col], bounds=[np.arange(1024, dtype=np.int32)]),                       # more than 1023 bounds
        dict(cols=[col], bounds=[ok], bucket_ids=[[1, 2, 3]]),                            # three ids for four buckets
        dict(cols=[col], bounds=[ok], bucket_ids=[[1, 2, 3, 255]], id_width=1),           # all ones of the width
        dict(cols=[col], bounds=[ok], bucket_ids=[[1, 2, 3, -3]]),
        dict(cols=[col], bounds=[ok], bucket_ids=[None, None]),
        dict(cols=[col], bounds=[np.arange(255, dtype=np.int32)], id_width=1),            # bucket 255 does not fit
        dict(cols=[col], bounds=[ok], id_width=3),
        dict(cols=[col], bounds=[ok], id_width=[1, 1]),
        dict(cols=[col], bounds=[ok], nan_id=0),                                          # nan_id on an integer column
        dict(cols=[fcol], bounds=[fok], nan_id=255, id_width=1),
        dict(cols=[fcol], bounds=[fok], nan_id=[1, 2]),
        dict(cols=[fcol], bounds=[fok], right_closed=1),
        dict(cols=[fcol], bounds=[fok], right_closed=[True, False]),
        dict(cols=[col, col], bounds=[ok, ok], selection=[torch.zeros(8, dtype=torch.uint8)]),
        dict(cols=[col], bounds=[ok], out=[torch.zeros(40, dtype=torch.int32)]),           # id_width 1 writes uint8
        dict(cols=[col], bounds=[ok], out=[torch.zeros(39, dtype=torch.uint8)]),
        dict(cols=[col], bounds=[ok], out=[None, None]),
        dict(cols=[ColumnPages(P.BINARY, False, col.pages, metas)], bounds=[[b"a"]]),
        dict(cols=[ColumnPages(P.BOOLEAN, False, col.pages, metas)], bounds=[[1]]),
        dict(cols=[ColumnPages(P.INT128, False, col.pages, metas)], bounds=[[1]]),
        dict(cols=[ColumnPages(P.NULL, False, col.pages, metas)], bounds=[[]]),
        dict(cols=[object()], bounds=[ok]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            key_buckets(Ctx(), **kw)
    with pytest.raises(TypeError):    # not a bitmap
        key_buckets(Ctx(), [col], [ok], selection=[np.zeros(8, np.uint8)])
    for kw in (dict(n_groups=0), dict(n_groups=1025), dict(n_groups=3), dict(n_groups=2.0), dict(bucket_ids=[0, 1, 5, 0], n_groups=5),
               dict(bucket_ids=[0, 1, 5], n_groups=6), dict(nan_id=1), dict(right_closed="yes"), dict(ops=("median",))):
        with pytest.raises(ValueError):   # the buckets hand out the id 3 (or 5): it needs a group
            group_by_buckets(Ctx(), col, ok, [col], **kw)
    with pytest.raises(ValueError):
        group_by_buckets(Ctx(), fcol, fok, [fcol], nan_id=3, n_groups=3)
    with pytest.raises(ValueError):       # a value column the aggregate refuses: before the key call is made
        group_by_buckets(Ctx(), col, ok, [ColumnPages(P.BINARY, False, col.pages, metas)], ops=("sum",))
    for b in ([2, 1], np.arange(1024, dtype=np.int32), [1.5]):
        with pytest.raises(ValueError):
            histogram(Ctx(), col, b)
    with pytest.raises(ValueError):
        histogram(Ctx(), fcol, [math.nan])


# ---- the reference against a plain Python loop
def _loop(vals, live, bounds, bucket_ids, right_closed, nan_id, id_width):
    none = (1 << (8 * id_width)) - 1
    ids, matched, nans = [], 0, 0
    for x, on in zip(vals.tolist(), live.tolist()):
        i = none
        if on:
            if isinstance(x, float) and x != x:
                nans += 1
                i = none if nan_id is None else nan_id
            else:
                b = sum(1 for t in bounds if (t < x if right_closed else t <= x))   # Python compares ints and floats exactly
                i = b if bucket_ids is None else bucket_ids[b]
                i = none if i in (None, NONE) else i
            matched += i != none
        ids.append(i)
    return ids, matched, nans


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reference_against_a_plain_loop(seed):
    rng = np.random.default_rng(seed)
    live = rng.random(500) < 0.6
    cols = [
        (rng.integers(-20, 20, 500).astype(np.int16), np.array([-15, -3, 0, 1, 19], np.int16)),
        (rng.integers(0, 2 ** 64, 500, dtype=np.uint64), np.array([1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], np.uint64)),
        (rng.integers(-2 ** 63, 2 ** 63, 500, dtype=np.int64), np.array([-2 ** 63, -1, 0, 2 ** 53 + 1, 2 ** 63 - 1], np.int64)),
        (rng.choice(np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 1.0, np.inf, np.nan, -np.nan, 5e-324]), 500),
         np.array([-np.inf, -1.5, 0.0, 1.0, np.inf])),
        (rng.choice(np.array([-2.0, -0.0, 0.0, 1.0, np.nan, 3.5], np.float32), 500), np.array([-0.0, 1.0], np.float32)),
    ]
    cols[1][0][:4] = cols[1][1]   # (values equal to the bounds, the extremes among them)
    cols[2][0][:5] = cols[2][1]
    for vals, bounds in cols:
        n = bounds.size
        flt = vals.dtype.kind == "f"
        for bucket_ids in (None, [3] * (n + 1), list(range(n + 1, 0, -1)), [None] + list(range(n - 1)) + [NONE]):
            for right_closed in (False, True):
                for nan_id in ((None, 7) if flt else (None,)):
                    for id_width in (1, 2, 4):
                        w = R.bucket_values(vals, live, 123, bounds, bucket_ids, right_closed, nan_id, id_width)
                        ids, matched, nans = _loop(vals, live, bounds.tolist(), bucket_ids, right_closed, nan_id, id_width)
                        assert w.ids.dtype == R.ID_NP[id_width] and w.ids.tolist() == ids
                        assert (w.rows, w.selected, w.count, w.matched, w.nans) == (500, 123, int(live.sum()), matched, nans)
        w = R.bucket_values(vals, live, 0, bounds[:0], None, False, None, 1)     # no bounds: every value in bucket 0
        nan = live & np.isnan(vals) if flt else np.zeros(500, bool)
        assert (w.ids[live & ~nan] == 0).all() and (w.ids[~live | nan] == 255).all() and w.matched == int((live & ~nan).sum())
        w = R.bucket_values(vals, np.zeros(500, bool), 0, bounds, None, False, None, 2)
        assert (w.ids == 65535).all() and (w.count, w.matched, w.nans) == (0, 0, 0)
    # the two closednesses differ exactly on the rows that equal a bound
    v = np.array([1, 2, 3, 4, 5, 6, 7], np.int8)
    b = np.array([2, 4, 6], np.int8)
    left = R.bucket_values(v, np.ones(7, bool), 7, b, None, False, None, 1).ids
    right = R.bucket_values(v, np.ones(7, bool), 7, b, None, True, None, 1).ids
    assert left.tolist() == [0, 1, 1, 2, 2, 3, 3] and right.tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert ((left != right) == np.isin(v, b)).all()


# ---- the columns of the GPU tests carry their codec on every page
def test_every_case_of_the_gpu_tests_carries_its_codec_on_every_page():
    import time
    from oracle import sbo as S
    assert len(Bc.ALL) > 80 and len(Bc.CASES) > 20
    for name in Bc.ALL:
        t = time.perf_counter()
        b = Bc.build(name)   # (asserts the codec of every page)
        assert not b.binary, name
        if name == "big_u8":
            assert b.rows == 4096 * 4096 + 1 and time.perf_counter() - t < 60
    assert {Bc.CASES[n][0] for n in Bc.CASES} == {S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.ONEVALUE, S.RLE, S.DICT, S.PATAS, S.FREQ}
    assert {Bc.Kc.CASES[n][0] for n in Bc.INT_CASES} == {S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.ONEVALUE, S.RLE, S.DICT, S.BITPACK, S.DELTABP, S.FREQ}
    for D in (Bc.FILTER_DICT_BITS, Bc.FILTER_DICT_BITS + 1):   # the two sides of the LDS table
        assert Bc.dict_entries(Bc.build("dict_%d" % D)) == D and Bc.dict_entries(Bc.build("f64_dict_%d" % D)) == D
        fb = Bc.build("f64_dict_%d" % D)
        assert np.isnan(fb.ref.vals[:fb.rows][fb.ref.valid]).any()   # a NaN is a dictionary entry
    for r in Bc.ROW_COUNTS:
        assert Bc.build("f64_rows_%d" % r).rows == r
        for p in (2, 9):
            assert Bc.build("rows_%d_%d" % (r, p)).rows == r
    assert Bc.build("f64_rle_long").metas.shape[0] == 1 and Bc.build("f64_rle_long").rows >= 1 << 18
    for name in ("f64_rle", "f32_rle", "f64_dict", "f64_none", "f64_patas"):   # NaNs of both signs, +-0.0 and +-inf among the live rows
        b = Bc.build(name)
        v = b.ref.vals[:b.rows][b.ref.valid]
        assert np.isnan(v).any() and np.isinf(v).any() and (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any(), name
        assert (np.signbit(v) & np.isnan(v)).any() and (~np.signbit(v) & np.isnan(v)).any(), name
    one = Bc.build("f64_onevalue_nan")
    assert np.isnan(one.ref.vals[:one.rows][one.ref.valid]).all()
    assert re.search(r"FILTER_DICT_BITS = %d;" % Bc.FILTER_DICT_BITS, open(os.path.join(CSRC, "sb_filter.h")).read())
