"""sb_key_ids_var without a GPU: the symbol is exported, the ctypes struct has the header's layout, the Python layer refuses
what needs no device before a context is touched, the byte-order compare, the prefix, the hash and the lower bound of
csrc/sb_common.h (kv_rel / kv_prefix / kv_hash / kv_lower_bound: the host's and the device's alike) agree with
std::lexicographical_compare / std::lower_bound in a stand-alone host program, and the reference that
tests/test_gpu_key_ids_var.py compares the device with (tests/key_ids_var_ref.py) is checked against a dict-based group-by."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.key_ids_var import KeyIdsVarBatch, check_column, key_ids_var
from strawboat_amd.types import PhysicalType as P
from tests import key_ids_var_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, ids=64, ids_capacity=72, id_width=80, max_keys=84, key_offsets=88, keys=96,
               keys_capacity=104, stage_capacity=112, reserved=120, rows=128, selected=136, count=144, n_keys=152,
               keys_len=160, overflow=168)


def test_symbol_is_declared_and_exported():
    import strawboat_amd as sb
    assert "sb_key_ids_var" in N.EXPORTS
    assert sb.key_ids_var is key_ids_var and sb.KeyIdsVarBatch is KeyIdsVarBatch and "KeyIdsVar" in sb.__all__
    assert re.search(r"\bsb_key_ids_var\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_key_ids_var$", out, re.M)


def test_ctypes_struct_has_the_headers_layout_and_the_constants_match(tmp_path):
    assert C.sizeof(N.ColumnKeyIdsVarC) == 176
    assert [name for name, _ in N.ColumnKeyIdsVarC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnKeyIdsVarC, f).offset == off, f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_key_ids_var));\n'
                   '    printf("BYTES %u\\nOK %u\\nOB %u\\nMAX %u\\n", SB_KEY_VAR_MAX_BYTES, SB_KEY_OVERFLOW_KEYS, SB_KEY_OVERFLOW_BYTES, SB_KEY_MAX_KEYS);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_key_ids_var, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 176
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["BYTES"]) == N.SB_KEY_VAR_MAX_BYTES == 1 << 20
    assert (int(got["OK"]), int(got["OB"])) == (N.SB_KEY_OVERFLOW_KEYS, N.SB_KEY_OVERFLOW_BYTES) == (1, 2)
    assert int(got["MAX"]) == N.SB_KEY_MAX_KEYS == 1024
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_key_ids_var_host.py)")[1].split("*/")[0]
    assert "sb_column_key_ids_var 176 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_column_key_ids_var 176 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


def test_unsupported_types_bad_widths_bad_max_keys_bad_key_bytes_and_short_bitmaps_are_refused_on_the_host():
    every = (P.BINARY, P.LARGE_BINARY, P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32,
             P.FLOAT64, P.BOOLEAN, P.INT128, P.INT256, P.NULL)
    for ptype in every[:2]:
        for mk, w in ((1, 1), (255, 1), (256, 2), (1024, 2), (1024, 4), (7, 4)):
            for kb in (0, 1, 65536, 1 << 20):
                check_column(ptype, 33, 8, mk, w, kb)
                check_column(ptype, 33, None, mk, w, kb)
    for ptype in every[2:]:
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, 5, 1, 64)
    for mk, w in ((0, 1), (-1, 2), (256, 1), (1025, 2), (1025, 4), (1 << 32, 4), (2.0, 2), ("3", 2), (None, 2), (True, 1)):
        with pytest.raises(ValueError):
            check_column(P.BINARY, 33, 8, mk, w, 64)
    for w in (0, 3, 8, None, "1", True):
        with pytest.raises(ValueError):
            check_column(P.BINARY, 33, 8, 5, w, 64)
    for kb in (-1, (1 << 20) + 1, 2.5, "64", None, True):
        with pytest.raises(ValueError):
            check_column(P.LARGE_BINARY, 33, 8, 5, 1, kb)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):
        with pytest.raises(ValueError):
            check_column(P.BINARY, rows, nbytes, 5, 1, 64)


def test_bad_arguments_raise_before_a_context_is_touched():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.BINARY, False, torch.zeros(100, dtype=torch.uint8), metas)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        key_ids_var(Ctx(), [col], selection=torch.zeros(4, dtype=torch.uint8))
    for ptype in (P.INT32, P.INT64, P.FLOAT32, P.BOOLEAN, P.INT128, P.NULL):
        with pytest.raises(ValueError):
            key_ids_var(Ctx(), [ColumnPages(ptype, False, col.pages, metas)])
    for mk in (0, 1025, [5], [5, 5, 5], 2.5):
        with pytest.raises(ValueError):
            key_ids_var(Ctx(), [col, col], max_keys=mk)
    with pytest.raises(ValueError):   # 256 keys do not fit ids of one byte
        key_ids_var(Ctx(), [col], max_keys=256, id_width=1)
    for w in (3, 8, [1], "2"):
        with pytest.raises(ValueError):
            key_ids_var(Ctx(), [col, col], max_keys=5, id_width=w)
    for kb in ((1 << 20) + 1, -1, [64], 1.5):
        with pytest.raises(ValueError):
            key_ids_var(Ctx(), [col, col], max_keys=5, key_bytes=kb)
    with pytest.raises(ValueError):   # one selection per column
        key_ids_var(Ctx(), [col, col], selection=[torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(TypeError):    # not a bitmap
        key_ids_var(Ctx(), [col], selection=[np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):
        KeyIdsVarBatch(Ctx(), [col, col], out=[torch.zeros(40, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        key_ids_var(Ctx(), [col], max_keys=5, out=[torch.zeros(40, dtype=torch.int32)])
    with pytest.raises(ValueError):
        key_ids_var(Ctx(), [col], max_keys=5, out=[torch.zeros(39, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        KeyIdsVarBatch(Ctx(), [col], stage_capacity=[1, 2])


# ---- kv_rel / kv_prefix / kv_hash / kv_lower_bound in a host program of their own
PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "sb_common.h"

typedef std::vector<unsigned char> Str;
static int fails = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
// every string in a heap block of exactly its length: a load before its first or behind its last byte is the sanitizer's
struct Exact {
    std::vector<uint8_t*> p;
    std::vector<uint32_t> n;
    ~Exact() { for (uint8_t* q : p) delete[] q; }
    void add(const Str& s) {
        uint8_t* q = new uint8_t[s.size() ? s.size() : 1];
        if (s.size()) memcpy(q, s.data(), s.size());
        p.push_back(q), n.push_back((uint32_t)s.size());
    }
};
static bool less_std(const Str& a, const Str& b) { return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end()); }
int main() {
    std::vector<Str> pool;
    const uint32_t lens[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 200};
    const unsigned char alphabet[] = {0x00, 0x01, 'a', 'b', 0x7F, 0x80, 0xFF};
    for (uint32_t L : lens)
        for (int k = 0; k < 6; k++) {
            Str s(L, (unsigned char)'a');
            if (k == 1) for (uint32_t i = 0; i < L; i++) s[i] = alphabet[rnd() % 7];
            if (k == 2 && L) s[L - 1] = 0xFF;                 // differs in the last byte only
            if (k == 3 && L) s[L - 1] = 0x00;                 // "a" against "a\0": the shorter is the prefix
            if (k == 4 && L > 8) s[8] = 0x80;                 // differs at byte 8 only
            if (k == 5 && L) s[0] = 0x80;                     // bytes >= 0x80 are greater than ASCII
            pool.push_back(s);
        }
    Exact ex;
    for (const Str& s : pool) ex.add(s);
    const size_t m = pool.size();
    for (size_t i = 0; i < m; i++)
        for (size_t j = 0; j < m; j++) {
            const uint32_t want = less_std(pool[i], pool[j]) ? 0u : pool[i] == pool[j] ? 1u : 2u;
            const uint32_t got = sb::kv_rel(ex.p[i], ex.n[i], ex.p[j], ex.n[j]);
            if (got != want && fails++ < 10) printf("kv_rel %zu %zu: %u, want %u\n", i, j, got, want);
            if (sb::kv_equal(ex.p[i], ex.n[i], ex.p[j], ex.n[j]) != (want == 1u) && fails++ < 10) printf("kv_equal %zu %zu\n", i, j);
            // prefixes that differ order the strings; equal strings share prefix and hash
            const uint64_t pi = sb::kv_prefix(ex.p[i], ex.n[i]), pj = sb::kv_prefix(ex.p[j], ex.n[j]);
            if (pi != pj && (pi < pj) != (want == 0u) && fails++ < 10) printf("kv_prefix %zu %zu\n", i, j);
            if (want == 1u && (pi != pj || sb::kv_hash(ex.p[i], ex.n[i]) != sb::kv_hash(ex.p[j], ex.n[j])) && fails++ < 10) printf("hash/prefix of equal strings %zu %zu\n", i, j);
        }
    // the lower bound over sorted distinct sets of 0, 1, 2, 3, 255, 256, 1023 and 1024 keys: every pool string and every key probed
    const uint32_t sizes[] = {0, 1, 2, 3, 255, 256, 1023, 1024};
    for (uint32_t n : sizes) {
        std::vector<Str> keys(pool.begin(), pool.end());
        for (;;) {   // the pool and random strings over the same alphabet, until n distinct ones are there
            std::sort(keys.begin(), keys.end(), less_std);
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            if (keys.size() >= n) break;
            for (int k = 0; k < 64; k++) {
                Str s(rnd() % 20, 0);
                for (auto& c : s) c = alphabet[rnd() % 7];
                keys.push_back(s);
            }
        }
        if (keys.size() > n) {   // (both ends stay)
            const size_t cut = keys.size() - n;
            keys.erase(keys.begin() + n / 2, keys.begin() + n / 2 + cut);
        }
        if (keys.size() != n) { fails++; printf("set of %u: %zu\n", n, keys.size()); continue; }
        Exact kx;
        for (const Str& s : keys) kx.add(s);
        std::vector<uint64_t> pre(n), ptr(n);
        for (uint32_t i = 0; i < n; i++) pre[i] = sb::kv_prefix(kx.p[i], kx.n[i]), ptr[i] = (uint64_t)(uintptr_t)kx.p[i];
        std::vector<Str> probes(pool.begin(), pool.end());
        probes.insert(probes.end(), keys.begin(), keys.end());
        Exact px;
        for (const Str& s : probes) px.add(s);
        for (size_t q = 0; q < probes.size(); q++) {
            const uint32_t want = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), probes[q], less_std) - keys.begin());
            const uint32_t got = sb::kv_lower_bound(pre.data(), ptr.data(), kx.n.data(), n, sb::key_steps(n), px.p[q], px.n[q]);
            if (got != want && fails++ < 10) printf("n %u probe %zu: %u, want %u\n", n, q, got, want);
        }
    }
    // the slot's word: never 0, its fields come back
    const uint64_t w = sb::kv_word(sb::KEYV_ROW, (1u << sb::KEYV_PAGE_BITS) - 1, (1u << sb::KEYV_INDEX_BITS) - 1, ~0ull);
    if (w != ~0ull - (1ull << 8) || sb::kv_word(sb::KEYV_ENTRY, 0, 0, 0) == 0) fails++, printf("kv_word\n");
    if (sb::KEYV_TAG_BITS != 8) fails++, printf("the tag has 8 bits (tests/test_gpu_key_ids_var.py says so)\n");
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
"""


def test_compare_prefix_hash_and_lower_bound_against_the_standard_library(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them):
    strings of 0 .. 200 bytes in heap blocks of exactly their length, so a load outside a string is an error of its own"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "kv.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "kv"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
        syms = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout + \
            subprocess.run(["nm", str(exe)], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): the helpers are compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("fails 0"), run.stdout + run.stderr


# ---- the reference against a dict-based group-by
def test_numpy_orders_bytes_objects_unsigned_with_the_prefix_first():
    a = np.empty(8, object)
    a[:] = [b"b", b"\x80", b"a\xff", b"", b"ab", b"a\x00", b"a", b"a"]
    assert list(np.unique(a)) == [b"", b"a", b"a\x00", b"ab", b"a\xff", b"b", b"\x80"]


def _dict_group_by(strs, live):
    seen = {}
    for s, on in zip(strs, live.tolist()):
        if on:
            seen[s] = True
    keys = sorted(seen)   # (Python orders bytes unsigned, the prefix first)
    place = {k: i for i, k in enumerate(keys)}
    return keys, [place[s] if on else None for s, on in zip(strs, live.tolist())]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reference_against_a_dict_group_by(seed):
    rng = np.random.default_rng(seed)
    pool = [b"", b"a", b"a\x00", b"ab", b"a\xff", b"b", b"\x80", b"abcdefgh", b"abcdefgh\x00", b"abcdefgi", b"x" * 40, b"x" * 39 + b"y"]
    strs = np.empty(300, object)
    for i, k in enumerate(rng.integers(0, len(pool), 300)):
        strs[i] = pool[k]
    live = rng.random(300) < 0.6
    keys, ids = _dict_group_by(strs, live)
    for id_width in (1, 2, 4):
        w = K.key_ids_values(strs, live, 123, 16, id_width, 256)
        none = (1 << (8 * id_width)) - 1
        assert w.overflow == 0 and w.n_keys == len(keys) and w.keys == keys
        assert w.ids.tolist() == [none if i is None else i for i in ids]
        assert (w.rows, w.selected, w.count) == (300, 123, int(live.sum()))
        assert w.keys_len == sum(len(k) for k in keys) and w.key_bytes == b"".join(keys) + bytes(256 - w.keys_len)
        assert w.key_offsets[0] == 0 and (w.key_offsets[len(keys):] == w.keys_len).all() and w.key_offsets.size == 17
        assert [w.key_bytes[int(w.key_offsets[i]):int(w.key_offsets[i + 1])] for i in range(len(keys))] == keys
    n, total = len(keys), sum(len(k) for k in keys)
    assert K.key_ids_values(strs, live, 0, n, 2, total).overflow == 0
    w = K.key_ids_values(strs, live, 0, n - 1, 2, total)
    assert w.overflow == K.OVER_KEYS and w.keys is None and w.ids is None and w.n_keys is None and w.count == int(live.sum())
    w = K.key_ids_values(strs, live, 0, n, 2, total - 1)   # the bytes alone do not fit: everything else is stated
    assert w.overflow == K.OVER_BYTES and w.n_keys == n and w.keys_len == total and w.ids is not None
    w = K.key_ids_values(strs, np.zeros(300, bool), 0, 4, 1, 8)
    assert (w.n_keys, w.count, w.keys_len) == (0, 0, 0) and (w.ids == 255).all() and w.key_bytes == bytes(8) and not w.key_offsets.any()
