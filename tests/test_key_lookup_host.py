"""sb_key_lookup without a GPU: the symbol is exported, the ctypes struct has the header's layout, the list preparation of
csrc/sb_key_lookup_prep.h (sort, dedup that keeps the first occurrence, the id of each sorted position, the checks, the
trip count) agrees with Python in a stand-alone host program, the Python layer refuses what needs no device before a
context is touched, the reference that tests/test_gpu_key_lookup.py compares the device with (tests/key_lookup_ref.py) is
checked against a dict-based lookup, and every column of tests/key_lookup_cases.py carries its codec on every page."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.key_lookup import KeyLookup, KeyLookupBatch, check_column, key_lookup, narrowest_id_width
from strawboat_amd.types import PhysicalType as P
from tests import key_lookup_cases as Kc
from tests import key_lookup_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, ids=64, ids_capacity=72, id_width=80, reserved0=84, values=88, value_offsets=96,
               value_ids=104, n_values=112, stage_capacity=120, reserved=128, rows=136, selected=144, count=152, matched=160)


def test_symbol_is_declared_and_exported():
    import strawboat_amd as sb
    assert "sb_key_lookup" in N.EXPORTS
    assert sb.key_lookup is key_lookup and sb.KeyLookupBatch is KeyLookupBatch and sb.KeyLookup is KeyLookup
    assert {"key_lookup", "KeyLookupBatch", "KeyLookup", "group_by_keys"} <= set(sb.__all__) and callable(sb.group_by_keys)
    assert re.search(r"\bsb_key_lookup\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_key_lookup$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    assert C.sizeof(N.ColumnKeyLookupC) == 168
    assert [name for name, _ in N.ColumnKeyLookupC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnKeyLookupC, f).offset == off, f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_key_lookup));\n'
                   '    printf("MAX %u\\nNONE %u\\n", SB_KEY_MAX_KEYS, SB_KEY_ID_NONE);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_key_lookup, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 168
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["MAX"]) == N.SB_KEY_MAX_KEYS == 1024 and int(got["NONE"]) == N.SB_KEY_ID_NONE == 0xFFFFFFFF
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_key_lookup_host.py)")[1].split("*/")[0]
    assert "sb_column_key_lookup 168 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_column_key_lookup 168 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


# ---- the list preparation in a host program of its own.  Input, one list per block:
#   list <binary> <w> <signed> <id_width> <n> <has_ids>      then n lines "<hex of the value's bytes or -> [id]"
# Output per list: "refused <list|ids>" or "ok <n> <steps>" and n lines "<hex or -> <id>" in sorted order.
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "sb_key_lookup_prep.h"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (s[0] == '-') return out;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        char b[3] = {s[i], s[i + 1], 0};
        out.push_back((uint8_t)strtoul(b, nullptr, 16));
    }
    return out;
}
static void put_hex(const uint8_t* p, size_t n) {
    if (!n) printf("-");
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int binary, w, is_signed, id_width, has_ids;
    unsigned long long n;
    while (fscanf(f, " list %d %d %d %d %llu %d", &binary, &w, &is_signed, &id_width, &n, &has_ids) == 6) {
        // every buffer of exactly its size on the heap: a load outside one is the sanitizer's
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> offsets(1, 0);
        std::vector<uint32_t> ids;
        static char word[1 << 16];
        for (unsigned long long i = 0; i < n; i++) {
            if (fscanf(f, " %65535s", word) != 1) return 3;
            const std::vector<uint8_t> v = unhex(word);
            bytes.insert(bytes.end(), v.begin(), v.end());
            offsets.push_back(bytes.size());
            if (has_ids) {
                unsigned long long id;
                if (fscanf(f, " %llu", &id) != 1) return 3;
                ids.push_back((uint32_t)id);
            }
        }
        uint8_t* vals = new uint8_t[bytes.size() ? bytes.size() : 1];
        if (bytes.size()) memcpy(vals, bytes.data(), bytes.size());
        uint64_t* offs = new uint64_t[offsets.size()];
        memcpy(offs, offsets.data(), offsets.size() * 8);
        uint32_t* vid = has_ids ? new uint32_t[ids.size() ? ids.size() : 1] : nullptr;
        if (has_ids && ids.size()) memcpy(vid, ids.data(), ids.size() * 4);
        const char* why = sb_lookup::check_list(binary != 0, vals, binary ? offs : nullptr, n);
        if (why) {
            printf("refused list\n");
        } else if ((why = sb_lookup::check_ids(vid, n, (uint32_t)id_width))) {
            printf("refused ids\n");
        } else {
            const sb_lookup::Prepared pr = binary ? sb_lookup::prepare_binary(vals, offs, vid, n)
                                                  : sb_lookup::prepare_numeric(vals, (uint32_t)w, is_signed != 0, vid, n);
            printf("ok %u %u\n", pr.n, pr.steps);
            if (pr.ids.size() != pr.n || pr.words.size() != pr.n + (binary ? 1u : 0u)) return 4;
            if (binary && (pr.bytes.size() != pr.words[pr.n] + 8 || pr.words[0] != 0)) return 4;
            for (uint32_t i = 0; i < pr.n; i++) {
                if (binary) {
                    put_hex(pr.bytes.data() + pr.words[i], pr.words[i + 1] - pr.words[i]);
                } else {   // the order key back to the value's bytes
                    uint64_t raw = is_signed ? pr.words[i] ^ (1ull << 63) : pr.words[i];
                    if (sb_lookup::order_key(is_signed != 0, (uint32_t)w, raw & (w == 8 ? ~0ull : (1ull << (8 * w)) - 1)) != pr.words[i]) return 5;
                    put_hex((const uint8_t*)&raw, (size_t)w);
                }
                printf(" %u\n", pr.ids[i]);
            }
            for (size_t i = 0; binary && i < 8; i++)
                if (pr.bytes[pr.words[pr.n] + i]) return 6;   // 8 zero bytes behind the literals
        }
        delete[] vals;
        delete[] offs;
        delete[] vid;
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
        warnings.warn("the compiler has no sanitizer runtime (%r): the list preparation is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    return exe


def _hex(b):
    return b.hex() if len(b) else "-"


def _expect(kind, values, value_ids, id_width):
    """what the program must print for one list: Python's own sort, dedup that keeps the first occurrence, ids and steps"""
    n = len(values)
    if n > 1024:
        return ["refused list"]
    none = (1 << (8 * id_width)) - 1
    handed = list(value_ids) if value_ids is not None else ([n - 1] if n else [])
    if any(i >= none for i in handed):
        return ["refused ids"]
    first = {}
    for i, v in enumerate(values):
        first.setdefault(v, i if value_ids is None else value_ids[i])
    keys = sorted(first)   # (Python orders ints by value and bytes unsigned, the prefix first)
    steps = 0
    while (1 << steps) < len(keys) + 1:
        steps += 1
    out = ["ok %d %d" % (len(keys), steps)]
    for k in keys:
        if kind == "bytes":
            out.append("%s %d" % (_hex(k), first[k]))
        else:
            w, signed = kind
            out.append("%s %d" % (int(k).to_bytes(w, "little", signed=signed).hex(), first[k]))
    return out


def _lists():
    """(kind, values, value_ids, id_width): kind "bytes" or (width, signed)"""
    rng = np.random.default_rng(5)
    out = []
    i64, u8, i8, u64, i16 = (8, True), (1, False), (1, True), (8, False), (2, True)
    out.append((i64, [], None, 1))                                         # empty
    out.append((i64, [], [], 2))
    out.append((i64, [42], None, 1))                                       # single
    out.append((i64, [42], [254], 1))
    out.append((i64, [42], [255], 1))                                      # all ones of the width: refused
    out.append((i64, [42], [65535], 2))
    out.append((i64, [42], [65534], 2))
    out.append((i64, [42], [0xFFFFFFFE], 4))
    out.append((i64, [42], [0xFFFFFFFF], 4))
    out.append((i64, [7] * 50, None, 1))                                   # all duplicates: the first occurrence wins
    out.append((i64, [7] * 50, list(range(50, 100)), 1))
    out.append((i64, list(range(1000, 0, -1)), None, 2))                   # reversed
    out.append((i64, list(range(1000, 0, -1)), None, 1))                   # ... 999 does not fit one byte
    out.append((i64, [5, 3, 5, 9, 3, 3, 1], [10, 11, 12, 13, 14, 15, 16], 1))   # duplicates with ids: 5 -> 10, 3 -> 11
    out.append((i64, [-2 ** 63, 2 ** 63 - 1, 0, -1, 1, -2 ** 63], None, 1))      # signed extremes
    out.append((i8, [-128, 127, 0, -1, 1], [4, 3, 2, 1, 0], 1))
    out.append((i16, [-32768, 32767, -1, 0], None, 4))
    out.append((u8, [255, 0, 128, 127], None, 1))
    out.append((u64, [2 ** 64 - 1, 0, 2 ** 63, 2 ** 63 - 1], None, 2))
    full = rng.permutation(np.arange(-512, 512)).tolist()
    out.append((i64, full, None, 2))                                       # 1024 values
    out.append((i64, full, (rng.integers(0, 5, 1024)).tolist(), 1))        # many-to-one
    out.append((i64, full + [9999], None, 2))                              # 1025: refused
    for k in range(0, 11):                                                 # the trip count at n = 2^k - 1 and 2^k
        for n in ((1 << k) - 1, 1 << k):
            out.append((i64, rng.permutation(np.arange(n) * 3).tolist(), None, 2))
    edge = [b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"abcdefgX", b"abc", b"", b"a", b"a\x00", b"a\x00\x00", b"\xff", b"\x80", b"b",
            b"abcdefgh" + b"q" * 32, b"abcdefgh" + b"q" * 31 + b"r", b"\x00"]
    out.append(("bytes", [], None, 1))
    out.append(("bytes", [b""], None, 1))                                  # the empty string is a value
    out.append(("bytes", edge, None, 1))                                   # shared prefix, proper prefix, trailing zero byte
    out.append(("bytes", edge[::-1], list(range(100, 100 + len(edge))), 1))
    out.append(("bytes", [b"a", b"a\x00", b"a", b"", b"a\x00", b""], [1, 2, 3, 4, 5, 6], 1))   # a -> 1, a\0 -> 2, "" -> 4
    out.append(("bytes", [b"x"] * 20, None, 1))
    out.append(("bytes", [b"k%04d" % i for i in rng.permutation(1024)], None, 2))
    out.append(("bytes", [b"k%04d" % i for i in range(1025)], None, 2))
    for n in (1, 2, 3, 4, 255, 256):
        out.append(("bytes", [b"s%d" % i for i in rng.permutation(n)], None, 2))
    return out


def test_list_preparation_in_a_stand_alone_program_against_python(tmp_path):
    exe = _build_program(tmp_path)
    lists = _lists()
    lines, want = [], []
    for kind, values, value_ids, id_width in lists:
        binary = kind == "bytes"
        w, signed = (0, False) if binary else kind
        lines.append("list %d %d %d %d %d %d" % (binary, w, signed, id_width, len(values), value_ids is not None))
        for i, v in enumerate(values):
            hx = _hex(v) if binary else int(v).to_bytes(w, "little", signed=signed).hex()
            lines.append(hx if value_ids is None else "%s %d" % (hx, value_ids[i]))
        want += _expect(kind, values, value_ids, id_width)
    inp = tmp_path / "lists.txt"
    inp.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, "line %d: %r, want %r" % (i, g, w_)
    # the trip count is ceil(log2(n + 1)): 2^k - 1 keys take k probes, 2^k take k + 1
    oks = [x for x in want if x.startswith("ok ")]
    assert "ok 1023 10" in oks and "ok 1024 11" in oks and "ok 0 0" in oks and "ok 1 1" in oks and "ok 3 2" in oks and "ok 4 3" in oks


# ---- the Python layer
class Ctx:
    """a context that fails when touched: only asked where its tensors live"""

    def __getattr__(self, name):
        if name == "torch_device":
            import torch
            return torch.device("cpu")
        raise AssertionError("the context was touched (%s) before the arguments were checked" % name)


def test_check_column_refuses_on_the_host():
    ints = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64)
    for ptype in ints + (P.BINARY, P.LARGE_BINARY):
        assert check_column(ptype, 33, 8, 5, None, None) == (None, 1)
        assert check_column(ptype, 33, None, 255, None, None)[1] == 1     # ids 0 .. 254
        assert check_column(ptype, 33, None, 256, None, None)[1] == 2     # 255 is all ones of one byte
        assert check_column(ptype, 33, None, 1024, None, None)[1] == 2
        assert check_column(ptype, 33, None, 0, None, None)[1] == 1
        ids, w = check_column(ptype, 33, None, 3, [7, 7, 65535], None)
        assert w == 4 and ids.dtype == np.uint32 and ids.tolist() == [7, 7, 65535]
        assert check_column(ptype, 33, None, 2, [0, 65534], None)[1] == 2
    for ptype in (P.FLOAT32, P.FLOAT64, P.BOOLEAN, P.INT128, P.INT256, P.NULL):
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, 5, None, None)
    with pytest.raises(ValueError):
        check_column(P.INT64, 33, 8, 1025, None, 2)
    for w in (0, 3, 8, "1", True, 2.0):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 5, None, w)
    for n, ids, w in ((256, None, 1), (3, [1, 2, 255], 1), (3, [1, 2, 65535], 2), (1, [0xFFFFFFFF], 4), (1, [-1], 4), (1, [1.5], 4),
                      (2, [1], 4), (1, [True], 4), (1, ["1"], 4)):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, n, ids, w)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):
        with pytest.raises(ValueError):
            check_column(P.INT32, rows, nbytes, 5, None, 1)
    assert [narrowest_id_width(i) for i in (0, 254, 255, 65534, 65535, 1 << 20)] == [1, 1, 2, 2, 4, 4]


def test_bad_arguments_raise_before_a_context_is_touched():
    import torch
    from strawboat_amd import group_by_keys
    from strawboat_amd.read import ColumnPages
    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT32, False, torch.zeros(100, dtype=torch.uint8), metas)
    scol = ColumnPages(P.BINARY, False, torch.zeros(100, dtype=torch.uint8), metas)
    ok = np.array([1, 2, 3], np.int32)
    bad = [
        dict(columns=[col], values=[ok], selection=torch.zeros(4, dtype=torch.uint8)),       # a bitmap of 4 bytes for 40 rows
        dict(columns=[col], values=[ok, ok]),                                               # one list per column
        dict(columns=[col, col], values=[ok]),
        dict(columns=[col], values=[np.array([1, 2], np.int64)]),                           # not the column's dtype
        dict(columns=[col], values=[np.array([[1, 2]], np.int32)]),
        dict(columns=[col], values=[[1, 2 ** 31]]),                                         # does not fit int32
        dict(columns=[col], values=[[1.5]]),
        dict(columns=[col], values=[[b"a"]]),
        dict(columns=[scol], values=[[1, 2]]),                                              # a number on a binary column
        dict(columns=[scol], values=[np.array([1], np.int32)]),
        dict(columns=[col], values=[np.arange(1025, dtype=np.int32)]),                      # more than 1024 values
        dict(columns=[scol], values=[[b"%d" % i for i in range(1025)]]),
        dict(columns=[col], values=[ok], value_ids=[[1, 2]]),                               # two ids for three values
        dict(columns=[col], values=[ok], value_ids=[[1, 2, 255]], id_width=1),              # all ones of the width
        dict(columns=[col], values=[ok], value_ids=[[1, 2, 0xFFFFFFFF]]),
        dict(columns=[col], values=[ok], value_ids=[[1, 2, -3]]),
        dict(columns=[col], values=[ok], value_ids=[None, None]),
        dict(columns=[col], values=[np.arange(256, dtype=np.int32)], id_width=1),           # the position 255 does not fit
        dict(columns=[col], values=[ok], id_width=3),
        dict(columns=[col], values=[ok], id_width=[1, 1]),
        dict(columns=[col, col], values=[ok, ok], selection=[torch.zeros(8, dtype=torch.uint8)]),
        dict(columns=[col], values=[ok], out=[torch.zeros(40, dtype=torch.int32)]),          # id_width 1 writes uint8
        dict(columns=[col], values=[ok], out=[torch.zeros(39, dtype=torch.uint8)]),
        dict(columns=[col], values=[ok], out=[None, None]),
        dict(columns=[ColumnPages(P.FLOAT32, False, col.pages, metas)], values=[[1.0]]),
        dict(columns=[ColumnPages(P.BOOLEAN, False, col.pages, metas)], values=[[1]]),
        dict(columns=[ColumnPages(P.INT128, False, col.pages, metas)], values=[[1]]),
        dict(columns=[ColumnPages(P.NULL, False, col.pages, metas)], values=[[]]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            key_lookup(Ctx(), **kw)
    with pytest.raises(TypeError):    # not a bitmap
        key_lookup(Ctx(), [col], [ok], selection=[np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):
        KeyLookupBatch(Ctx(), [col], [ok], stage_capacity=[1, 2])
    for kw in (dict(n_groups=0), dict(n_groups=1025), dict(n_groups=2), dict(n_groups=2.0), dict(value_ids=[0, 1, 5], n_groups=5)):
        with pytest.raises(ValueError):   # the list hands out the id 2 (or 5): it needs a group
            group_by_keys(Ctx(), col, ok, [col], **kw)


# ---- the reference against a dict-based lookup
def _dict_lookup(rowv, live, values, value_ids):
    first = {}
    for i, v in enumerate(values):
        if v not in first:
            first[v] = i if value_ids is None else value_ids[i]
    return [first.get(v) if on else None for v, on in zip(rowv, live.tolist())]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reference_against_a_dict_lookup(seed):
    rng = np.random.default_rng(seed)
    live = rng.random(500) < 0.6
    vals = rng.integers(-20, 20, 500).astype(np.int16)
    pool = [b"", b"a", b"a\x00", b"ab", b"a\xff", b"b", b"\x80", b"abcdefgh", b"abcdefgh\x00", b"abcdefgi", b"x" * 40, b"x" * 39 + b"y"]
    strs = np.empty(500, object)
    for i, k in enumerate(rng.integers(0, len(pool), 500)):
        strs[i] = pool[k]
    num_list = [5, -20, 19, 5, 0, -20, 7, 100, -100]       # duplicates; values the column does not hold
    str_list = [b"a\x00", b"", b"abcdefgh", b"a\x00", b"x" * 40, b"nope", b"abcdefg"]
    for column, lst in ((vals, num_list), (strs, str_list)):
        rowv = column.tolist()
        for value_ids in (None, [3] * len(lst), list(range(len(lst), 0, -1))):
            want = _dict_lookup(rowv, live, lst, value_ids)
            for id_width in (1, 2, 4):
                w = L.lookup_values(column, live, 123, lst, value_ids, id_width)
                none = (1 << (8 * id_width)) - 1
                assert w.ids.dtype == L.ID_NP[id_width] and w.ids.tolist() == [none if x is None else x for x in want]
                assert (w.rows, w.selected, w.count, w.matched) == (500, 123, int(live.sum()), sum(x is not None for x in want))
        w = L.lookup_values(column, live, 0, [], None, 1)
        assert (w.ids == 255).all() and w.matched == 0 and w.count == int(live.sum())
        w = L.lookup_values(column, np.zeros(500, bool), 0, lst, None, 2)
        assert (w.ids == 65535).all() and (w.count, w.matched) == (0, 0)
    # the lower bound alone is no match: values between, below and above the list's entries get all ones
    w = L.lookup_values(np.array([1, 2, 3, 4, 5, 6, 7], np.int8), np.ones(7, bool), 7, np.array([6, 2, 4], np.int8), None, 1)
    assert w.ids.tolist() == [255, 1, 255, 2, 255, 0, 255] and w.matched == 3


# ---- the columns of the GPU tests carry their codec on every page
def test_every_case_of_the_gpu_tests_carries_its_codec_on_every_page():
    import time
    from oracle import sbo as S
    assert len(Kc.CASES) > 90
    for name in Kc.CASES:
        t = time.perf_counter()
        b = Kc.build(name)   # (asserts the codec of every page)
        if name == "big_u8":
            assert b.rows == 4096 * 4096 + 1 and time.perf_counter() - t < 60
    codecs = {Kc.CASES[n][0] for n in Kc.CASES if not Kc.build(n).binary}
    assert codecs == {S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.ONEVALUE, S.RLE, S.DICT, S.BITPACK, S.DELTABP, S.FREQ}
    assert {Kc.CASES[n][0] for n in Kc.CASES if Kc.build(n).binary} == {S.NONE, S.LZ4, S.DICT, S.FREQ, S.ONEVALUE}
    for D in (Kc.FILTER_DICT_BITS, Kc.FILTER_DICT_BITS + 1):   # the two sides of the LDS table
        assert Kc.dict_entries(Kc.build("dict_%d" % D)) == D and Kc.dict_entries(Kc.build("bin_dict_%d" % D)) == D
    for r in Kc.ROW_COUNTS:
        for p in (2, 9):
            b = Kc.build("rows_%d_%d" % (r, p))
            # (64 rows in pages of 8 are eight pages: equal pages do not always come out as nine)
            assert b.rows == r and min(p, r) - 1 <= b.metas.shape[0] <= p and (r < 2 or b.metas.shape[0] >= 2), (r, p, b.metas.shape[0])
    assert Kc.build("rle_long").metas.shape[0] == 1 and Kc.build("rle_long").rows >= 1 << 18
    assert re.search(r"FILTER_DICT_BITS = %d;" % Kc.FILTER_DICT_BITS, open(os.path.join(CSRC, "sb_filter.h")).read())
