"""sb_key_combine without a GPU: the symbol is exported, the ctypes struct has the header's layout, comb_pack / comb_unpack
(csrc/sb_common.h) agree with Python in a stand-alone host program, the Python layer refuses what needs no device before a
context is touched, and the reference that tests/test_gpu_key_combine.py compares the device with
(tests/key_combine_ref.py) is checked against a plain Python dict-of-tuples group-by."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.key_combine import KeyCombineBatch, check_parts, key_combine
from strawboat_amd.types import PhysicalType as P
from tests import key_combine_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(rows=0, n_parts=8, id_width=12, part_ids=16, part_capacity=48, part_width=80, part_keys=96, ids=112,
               ids_capacity=120, max_keys=128, reserved=132, tuples=136, live=144, n_keys=152, overflow=160)


def test_symbol_is_declared_and_exported():
    assert "sb_key_combine" in N.EXPORTS
    assert re.search(r"\bsb_key_combine\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_key_combine$", out, re.M)


def test_ctypes_struct_has_the_headers_layout_and_the_constants_match(tmp_path):
    assert C.sizeof(N.KeyCombineItemC) == 168
    assert [name for name, _ in N.KeyCombineItemC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.KeyCombineItemC, f).offset == off, f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_key_combine_item));\n'
                   '    printf("MAX %u\\nNONE %u\\nPARTS %u\\n", SB_KEY_MAX_KEYS, SB_KEY_ID_NONE, SB_KEY_COMBINE_MAX_PARTS);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_key_combine_item, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 168
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["MAX"]) == N.SB_KEY_MAX_KEYS == 1024 == 1 << K.FIELD_BITS
    assert int(got["NONE"]) == N.SB_KEY_ID_NONE == 0xFFFFFFFF
    assert int(got["PARTS"]) == N.SB_KEY_COMBINE_MAX_PARTS == 4
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_key_combine_host.py)")[1].split("*/")[0]
    assert "sb_key_combine_item 168 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_key_combine_item 168 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


# ---- comb_pack / comb_unpack in a host program of their own: it reads tuples, prints code and the unpacked parts
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "sb_common.h"

int main() {
    unsigned n_parts, id[4];
    static_assert(sb::COMB_MAX_PARTS == 4 && sb::COMB_FIELD_BITS == 10, "the code word");
    while (scanf("%u %u %u %u %u", &n_parts, &id[0], &id[1], &id[2], &id[3]) == 5) {
        uint32_t in[4] = {id[0], id[1], id[2], id[3]}, out[4] = {77, 77, 77, 77};
        const uint64_t code = sb::comb_pack(in, n_parts);
        sb::comb_unpack(code, n_parts, out);
        printf("%llu %u %u %u %u\n", (unsigned long long)code, out[0], out[1], out[2], out[3]);
    }
    return 0;
}
"""


def _tuples_for_the_program():
    rng = np.random.default_rng(5)
    cases = []
    for n in (2, 3, 4):
        cases.append((n, (0,) * n))
        cases.append((n, (1023,) * n))
        for p in range(n):   # one-hot: every bit of every field alone, and the full field alone
            for bit in range(10):
                cases.append((n, tuple((1 << bit) if q == p else 0 for q in range(n))))
            cases.append((n, tuple(1023 if q == p else 0 for q in range(n))))
        for _ in range(300):
            cases.append((n, tuple(int(v) for v in rng.integers(0, 1024, n))))
        for _ in range(100):   # near neighbours: tuples that differ in one part by one
            t = [int(v) for v in rng.integers(1, 1023, n)]
            cases.append((n, tuple(t)))
            p = int(rng.integers(0, n))
            t[p] += 1
            cases.append((n, tuple(t)))
    return cases


def test_pack_and_unpack_against_python(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them):
    all-0, all-1023, one-hot and random tuples of 2, 3 and 4 parts; the codes are Python's, unpack inverts pack and
    writes 0 into the unused parts, and the codes order as the tuples do"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "pack.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "pack"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): comb_pack is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    cases = _tuples_for_the_program()
    text = "".join("%d %d %d %d %d\n" % ((n,) + t + (0,) * (4 - n)) for n, t in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    by_parts = {2: [], 3: [], 4: []}
    for (n, t), line in zip(cases, lines):
        got = [int(x) for x in line.split()]
        assert got[0] == K.pack(t), (n, t, got)
        assert tuple(got[1:1 + n]) == t == K.unpack(got[0], n) and got[1 + n:] == [0] * (4 - n), (n, t, got)
        by_parts[n].append((t, got[0]))
    for n, pairs in by_parts.items():   # the order of the codes is the lexicographic order of the tuples
        assert [t for t, _ in sorted(pairs)] == [t for t, _ in sorted(pairs, key=lambda x: x[1])], n
        assert max(c for _, c in pairs) == (1 << (10 * n)) - 1 and min(c for _, c in pairs) == 0


# ---- refusals of the Python layer
class _Untouchable:
    """a context that fails if anything but the place of its tensors is asked of it"""

    def __getattr__(self, name):
        if name == "torch_device":
            import torch
            return torch.device("cpu")
        raise AssertionError("the context was touched: %s" % name)


def test_check_parts():
    check_parts([1, 2], [255, 1024], 1024, 2)
    check_parts([4, 4, 1, 2], [1, 1, 1, 1], 255, 1)
    for widths, bounds in (([1], [5]), ([1] * 5, [5] * 5), ([], []), ([1, 2], [5])):
        with pytest.raises(ValueError):
            check_parts(widths, bounds, 5, 1)
    for w in (0, 3, 8, None, True, "1"):
        with pytest.raises(ValueError):
            check_parts([1, w], [5, 5], 5, 1)
        with pytest.raises(ValueError):
            check_parts([1, 1], [5, 5], 5, w)
    for b in (0, 1025, -1, 2.0, None, True, 1 << 32):
        with pytest.raises(ValueError):
            check_parts([1, 1], [5, b], 5, 1)
    for mk, w in ((0, 1), (256, 1), (1025, 2), (1025, 4), (2.5, 2), (None, 2), (True, 1)):
        with pytest.raises(ValueError):
            check_parts([1, 1], [5, 5], mk, w)


def test_bad_arguments_raise_before_a_context_is_touched():
    import torch
    ctx = _Untouchable()
    a8 = torch.zeros(40, dtype=torch.uint8)
    a16 = torch.zeros(40, dtype=torch.uint16)
    a32 = torch.zeros(40, dtype=torch.int32)
    for parts in ([(a8, 5)], [(a8, 5)] * 5, []):                         # n_parts
        with pytest.raises(ValueError):
            key_combine(ctx, parts)
    for bad in (torch.zeros(40, dtype=torch.int64), torch.zeros(40, dtype=torch.float32), torch.zeros(40, dtype=torch.int16)):
        with pytest.raises(ValueError):                                   # widths: the dtype says them
            key_combine(ctx, [(a8, 5), (bad, 5)])
    with pytest.raises(ValueError):                                       # no part at all
        key_combine(ctx, [(a8, 5), np.zeros(40, np.uint8)])
    for bound in (0, 1025, -3, 2.5, None):                                # bounds
        with pytest.raises(ValueError):
            key_combine(ctx, [(a8, 5), (a16, bound)])
    for mk, w in ((0, None), (1025, None), (256, 1), (1025, 4), (2.5, None)):   # max_keys against id_width
        with pytest.raises(ValueError):
            key_combine(ctx, [(a8, 5), (a32, 5)], max_keys=mk, id_width=w)
    for w in (3, 8, "2"):
        with pytest.raises(ValueError):
            key_combine(ctx, [(a8, 5), (a32, 5)], max_keys=5, id_width=w)
    with pytest.raises(ValueError):                                       # parts of different lengths
        key_combine(ctx, [(a8, 5), (torch.zeros(39, dtype=torch.uint8), 5)])
    with pytest.raises(ValueError):                                       # a part on another device
        key_combine(ctx, [(a8, 5), (torch.zeros(40, dtype=torch.uint8, device="meta"), 5)])
    # out: of the width's dtype, on the device, long enough
    with pytest.raises(ValueError):
        key_combine(ctx, [(a8, 5), (a16, 5)], max_keys=5, out=torch.zeros(40, dtype=torch.int32))
    with pytest.raises(ValueError):
        key_combine(ctx, [(a8, 5), (a16, 5)], max_keys=5, id_width=4, out=torch.zeros(40, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError):
        key_combine(ctx, [(a8, 5), (a16, 5)], max_keys=5, out=torch.zeros(39, dtype=torch.uint8))
    with pytest.raises(ValueError):
        key_combine(ctx, [(a8, 5), (a16, 5)], max_keys=5, out=np.zeros(40, np.uint8))
    with pytest.raises(ValueError):                                       # one out per item
        KeyCombineBatch(ctx, [[(a8, 5), (a16, 5)]] * 2, max_keys=5, out=[torch.zeros(40, dtype=torch.uint8)])
    with pytest.raises(ValueError):                                       # one max_keys per item
        KeyCombineBatch(ctx, [[(a8, 5), (a16, 5)]] * 2, max_keys=[5])


def test_group_by_refuses_bad_key_lists_before_any_call():
    import torch
    from strawboat_amd.group_by import group_by
    from strawboat_amd.read import ColumnPages
    ctx = _Untouchable()
    metas = np.array([[100, 40]], np.uint64)
    pages = torch.zeros(100, dtype=torch.uint8)
    i64 = ColumnPages(P.INT64, False, pages, metas)
    utf8 = ColumnPages(P.BINARY, False, pages, metas)
    f64 = ColumnPages(P.FLOAT64, False, pages, metas)
    for key in ([i64], [i64] * 5, [], (utf8,), [i64, f64], [f64, utf8], [i64, utf8, ColumnPages(P.BOOLEAN, False, pages, metas)],
                [i64, "b"]):
        with pytest.raises(ValueError):
            group_by(ctx, key, [i64])
    for mk in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            group_by(ctx, [i64, utf8], [i64], max_keys=mk)


# ---- the reference against a dict-of-tuples group-by
def _dict_group_by(parts, bounds):
    """Python tuples in a dict: the distinct live tuples in ascending order, and a row's id by dictionary lookup"""
    rows = list(zip(*[p.tolist() for p in parts]))
    live = [all(v < b for v, b in zip(t, bounds)) for t in rows]
    order = sorted({t for t, on in zip(rows, live) if on})
    place = {t: i for i, t in enumerate(order)}
    return order, [place[t] if on else None for t, on in zip(rows, live)], live


@pytest.mark.parametrize("n_parts,seed", [(2, 1), (3, 2), (4, 3)])
def test_the_reference_against_a_dict_group_by(n_parts, seed):
    rng = np.random.default_rng(seed)
    bounds = [7, 300, 1024, 2][:n_parts]
    dts = [np.uint8, np.uint16, np.uint32, np.uint8][:n_parts]
    parts = []
    for b, dt in zip(bounds, dts):
        a = rng.integers(0, min(b, 4), 400).astype(dt)
        a[rng.random(400) < 0.1] = np.iinfo(dt).max      # all ones
        a[rng.random(400) < 0.03] = min(b, np.iinfo(dt).max - 1)   # at the bound, not all ones (but for the 2-key byte part)
        parts.append(a)
    order, ids, live = _dict_group_by(parts, bounds)
    assert 0 < len(order) and not all(live)
    for id_width in (1, 2, 4):
        w = K.combine(parts, bounds, 255, id_width)
        none = (1 << (8 * id_width)) - 1
        assert not w.overflow and w.n_keys == len(order) and [tuple(t) for t in w.tuples.tolist()] == order
        assert w.ids.tolist() == [none if i is None else i for i in ids]
        assert (w.rows, w.live) == (400, sum(live))
        tw = w.tuple_words
        assert tw.shape == (255, 4) and tw.dtype == np.uint32 and not tw[len(order):].any() and not tw[:, n_parts:].any()
        assert [tuple(t) for t in tw[:len(order), :n_parts].tolist()] == order
    # exactly max_keys tuples fit; one more is an overflow, and nothing else is stated then
    assert not K.combine(parts, bounds, len(order), 2).overflow
    w = K.combine(parts, bounds, len(order) - 1, 2)
    assert w.overflow and w.tuples is None and w.ids is None and w.n_keys is None and w.live == sum(live)
    # no live row: no tuple, every id all ones
    dead = [np.full(50, 255, np.uint8)] * n_parts
    w = K.combine(dead, [255] * n_parts, 4, 1)
    assert (w.n_keys, w.live) == (0, 0) and (w.ids == 255).all() and not w.tuple_words.any()
    # no row at all
    w = K.combine([np.zeros(0, np.uint16)] * n_parts, [9] * n_parts, 4, 2)
    assert (w.rows, w.n_keys, w.live, w.overflow) == (0, 0, 0, False) and w.ids.size == 0
