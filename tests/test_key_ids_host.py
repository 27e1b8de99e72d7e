"""sb_key_ids without a GPU: the symbol is exported, the ctypes struct has the header's layout, the Python layer refuses
what needs no device before a context is touched, key_lower_bound / in_key (csrc/sb_common.h) agree with std::lower_bound
in a stand-alone host program, and the reference that tests/test_gpu_key_ids.py compares the device with
(tests/key_ids_ref.py) is checked against a plain Python dict-based group-by."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from oracle import sbo as S
from strawboat_amd import _native as N
from strawboat_amd.key_ids import (ID_DTYPES, KeyIdsBatch, check_column, key_ids, max_keys_limit, narrowest_id_width)
from strawboat_amd.types import PhysicalType as P
from tests import key_ids_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, ids=64, ids_capacity=72, id_width=80, max_keys=84, keys=88, reserved=96, rows=104,
               selected=112, count=120, n_keys=128, overflow=136)


def test_symbol_is_declared_and_exported():
    assert "sb_key_ids" in N.EXPORTS
    assert re.search(r"\bsb_key_ids\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_key_ids$", out, re.M)


def test_ctypes_struct_has_the_headers_layout_and_the_constants_match(tmp_path):
    assert C.sizeof(N.ColumnKeyIdsC) == 144
    assert [name for name, _ in N.ColumnKeyIdsC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnKeyIdsC, f).offset == off, f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_key_ids));\n'
                   '    printf("MAX %u\\nNONE %u\\nIN_MAX %u\\n", SB_KEY_MAX_KEYS, SB_KEY_ID_NONE, SB_IN_MAX_VALUES);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_key_ids, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 144
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["MAX"]) == N.SB_KEY_MAX_KEYS == int(got["IN_MAX"]) == 1024
    assert int(got["NONE"]) == N.SB_KEY_ID_NONE == 0xFFFFFFFF
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_key_ids_host.py)")[1].split("*/")[0]
    assert "sb_column_key_ids 144 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_column_key_ids 144 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


def test_widths_and_limits():
    assert [narrowest_id_width(m) for m in (1, 255, 256, 1024)] == [1, 1, 2, 2]
    assert [max_keys_limit(w) for w in (1, 2, 4)] == [255, 1024, 1024]
    assert ID_DTYPES == {1: "uint8", 2: "uint16", 4: "int32"}


def test_unsupported_types_bad_widths_bad_max_keys_and_short_bitmaps_are_refused_on_the_host():
    every = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
             P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)
    for ptype in every[:8]:
        for mk, w in ((1, 1), (255, 1), (256, 2), (1024, 2), (1024, 4), (7, 4)):
            check_column(ptype, 33, 8, mk, w)
            check_column(ptype, 33, None, mk, w)
    for ptype in every[8:]:
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, 5, 1)
    for mk, w in ((0, 1), (-1, 2), (256, 1), (1025, 2), (1025, 4), (1 << 32, 4), (2.0, 2), ("3", 2), (None, 2), (True, 1)):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, mk, w)
    for w in (0, 3, 8, None, "1", True):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 5, w)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):   # (1250 = ceil(rows/8): whole words are asked for)
        with pytest.raises(ValueError):
            check_column(P.INT64, rows, nbytes, 5, 1)


def test_bad_arguments_raise_before_a_context_is_touched():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        key_ids(Ctx(), [col], selection=torch.zeros(4, dtype=torch.uint8))
    for ptype in (P.FLOAT32, P.FLOAT64, P.BOOLEAN, P.BINARY, P.LARGE_BINARY, P.INT128, P.INT256, P.NULL):
        with pytest.raises(ValueError):
            key_ids(Ctx(), [ColumnPages(ptype, False, col.pages, metas)])
    for mk in (0, 1025, [5], [5, 5, 5], 2.5):   # out of range; not one per column; no int
        with pytest.raises(ValueError):
            key_ids(Ctx(), [col, col], max_keys=mk)
    with pytest.raises(ValueError):   # 256 keys do not fit ids of one byte
        key_ids(Ctx(), [col], max_keys=256, id_width=1)
    for w in (3, 8, [1], "2"):
        with pytest.raises(ValueError):
            key_ids(Ctx(), [col, col], max_keys=5, id_width=w)
    with pytest.raises(ValueError):   # one selection per column
        key_ids(Ctx(), [col, col], selection=[torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(TypeError):    # not a bitmap
        key_ids(Ctx(), [col], selection=[np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):   # a bitmap on another device
        key_ids(Ctx(), [col], selection=torch.zeros(8, dtype=torch.uint8, device="meta"))
    # out: one per column, of the width's dtype, long enough, on the device
    with pytest.raises(ValueError):
        KeyIdsBatch(Ctx(), [col, col], out=[torch.zeros(40, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        key_ids(Ctx(), [col], max_keys=5, out=[torch.zeros(40, dtype=torch.int32)])
    with pytest.raises(ValueError):
        key_ids(Ctx(), [col], max_keys=5, out=[torch.zeros(39, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        key_ids(Ctx(), [col], max_keys=5, id_width=4, out=[torch.zeros(40, dtype=torch.int32, device="meta")])
    with pytest.raises(ValueError):
        key_ids(Ctx(), [col], max_keys=5, out=[np.zeros(40, np.uint8)])


# ---- key_lower_bound and in_key in a host program of their own, against std::lower_bound
PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "sb_common.h"

static int fails = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
static void probe(const std::vector<uint64_t>& keys, uint64_t x) {
    const uint32_t n = (uint32_t)keys.size();
    const uint32_t want = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), x) - keys.begin());
    const uint32_t got = sb::key_lower_bound(keys.data(), n, sb::key_steps(n), x);
    if (got != want && fails++ < 10) printf("n %u x %llu: %u, want %u\n", n, (unsigned long long)x, got, want);
}
static void check_set(std::vector<uint64_t> keys) {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint32_t n = (uint32_t)keys.size();
    uint32_t steps = 0;
    while ((1ull << steps) < (uint64_t)n + 1) steps++;
    if (sb::key_steps(n) != steps) fails++, printf("steps of %u: %u, want %u\n", n, sb::key_steps(n), steps);
    probe(keys, 0), probe(keys, ~0ull), probe(keys, 1ull << 63), probe(keys, (1ull << 63) - 1);
    for (uint32_t i = 0; i < n; i++) {   // below, at, between and above every key
        probe(keys, keys[i]);
        probe(keys, keys[i] - 1);
        probe(keys, keys[i] + 1);
        if (i + 1 < n) probe(keys, keys[i] + (keys[i + 1] - keys[i]) / 2);
    }
}
int main() {
    const uint32_t sizes[] = {0, 1, 2, 3, 255, 256, 1023, 1024};
    for (uint32_t n : sizes)
        for (int shape = 0; shape < 4; shape++) {
            std::vector<uint64_t> keys;
            // dense from 0, random over 64 bits, packed against ~0, and the order keys of the signed extremes of every width
            for (uint32_t i = 0; keys.size() < n; i++) {
                const uint64_t k = shape == 0 ? i : shape == 1 ? rnd() : shape == 2 ? ~0ull - i : 0;
                if (shape < 3) {
                    keys.push_back(k);
                } else {
                    for (uint32_t w = 1; w <= 8; w *= 2) {
                        const uint64_t top = 1ull << (8 * w - 1);
                        const uint64_t raws[] = {top, top - 1, 0, (top - 1) | top, (uint64_t)i + 1, top + i + 1};   // min, max, 0, -1, ...
                        for (uint64_t raw : raws) keys.push_back(sb::in_key(1u, w, raw));
                    }
                    std::sort(keys.begin(), keys.end());
                    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
                }
            }
            if (keys.size() > n) keys.erase(keys.begin() + n / 2, keys.begin() + n / 2 + (keys.size() - n));   // (both ends stay)
            check_set(keys);
        }
    // in_key orders every width by signedness: min < -1 < 0 < max for signed, 0 < max for unsigned
    for (uint32_t w = 1; w <= 8; w *= 2) {
        const uint64_t top = 1ull << (8 * w - 1), ones = top | (top - 1);
        const uint64_t smin = sb::in_key(1u, w, top), sm1 = sb::in_key(1u, w, ones), s0 = sb::in_key(1u, w, 0), smax = sb::in_key(1u, w, top - 1);
        if (!(smin < sm1 && sm1 < s0 && s0 < smax)) fails++, printf("signed order, width %u\n", w);
        if (w == 8 && !(smin == 0 && smax == ~0ull)) fails++, printf("64-bit extremes: keys 0 and ~0\n");
        if (!(sb::in_key(0u, w, 0) == 0 && sb::in_key(0u, w, ones) == ones && sb::in_key(0u, w, top) == top)) fails++, printf("unsigned, width %u\n", w);
        // the 64-bit extremes land on both ends of a set
        std::vector<uint64_t> keys = {smin, sm1, s0, smax};
        check_set(keys);
    }
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
"""


def test_key_lower_bound_and_in_key_against_std_lower_bound(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has
    them): sorted sets of 0, 1, 2, 3, 255, 256, 1023 and 1024 keys, probes below, at, between and above every key,
    0, ~0 and the signed extremes of every width among them"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "lower_bound.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "lower_bound"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    # Does the compiler have the sanitizers' host runtime?  It names the file either way; where the file exists the
    # sanitized build MUST succeed and the program must carry the runtime.  Only a toolchain that ships none builds the
    # comparison alone, and says so in the test's warnings.
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
        syms = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout + \
            subprocess.run(["nm", str(exe)], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): key_lower_bound is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("fails 0"), run.stdout + run.stderr


# ---- the reference against a dict-based group-by
def _dict_group_by(vals, live):
    """Python ints in a dict: the distinct live values in ascending order, and a row's id by dictionary lookup"""
    seen = {}
    for v, on in zip(vals.tolist(), live.tolist()):
        if on:
            seen[v] = True
    keys = sorted(seen)
    place = {k: i for i, k in enumerate(keys)}
    return keys, [place[v] if on else None for v, on in zip(vals.tolist(), live.tolist())]


@pytest.mark.parametrize("ptype,seed", [(S.T_I8, 1), (S.T_I64, 2), (S.T_U64, 3)])
def test_the_reference_against_a_dict_group_by(ptype, seed):
    dt = np.dtype(K.NP[ptype])
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    pool = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1, 5, 77] + ([-1, -77] if info.min < 0 else []), dt)
    vals = pool[rng.integers(0, pool.size, 300)]
    live = rng.random(300) < 0.6
    for id_width in (1, 2, 4):
        w = K.key_ids_values(vals, live, 123, 16, id_width)
        keys, ids = _dict_group_by(vals, live)
        none = (1 << (8 * id_width)) - 1
        assert not w.overflow and w.n_keys == len(keys) and w.keys.tolist() == keys
        assert w.ids.tolist() == [none if i is None else i for i in ids]
        assert (w.rows, w.selected, w.count) == (300, 123, int(live.sum()))
        kb = np.frombuffer(w.key_bytes, np.uint8).reshape(16, 8)
        assert kb[:len(keys), :dt.itemsize].tobytes() == np.array(keys, dt).tobytes()
        assert not kb[:, dt.itemsize:].any() and not kb[len(keys):].any()
    # exactly max_keys keys fit; one more is an overflow, and nothing else is stated then
    n = len(_dict_group_by(vals, live)[0])
    assert not K.key_ids_values(vals, live, 0, n, 2).overflow
    w = K.key_ids_values(vals, live, 0, n - 1, 2)
    assert w.overflow and w.keys is None and w.ids is None and w.n_keys is None and w.count == int(live.sum())
    # no live row: no key, every id all ones
    w = K.key_ids_values(vals, np.zeros(300, bool), 0, 4, 1)
    assert (w.n_keys, w.count) == (0, 0) and (w.ids == 255).all() and w.key_bytes == bytes(32)
