// The bounds check of a page inside its column's `pages` bytes.  Plain C++ without HIP includes: the host tables of a
// read call use it (fill_read_tables, sb_api.hip) and tests/test_buffer_cases.py compiles it with the host compiler.
#pragma once
#include <cstdint>

// [in_off, in_off + len) lies inside [0, pages_len).  Both in_off (page_offsets, or the running sum of the lengths before
// the page) and len (PageMeta.length) come from a file: no sum of them is formed, so nothing can wrap.
static inline bool page_span_ok(uint64_t in_off, uint64_t len, uint64_t pages_len) {
    return in_off <= pages_len && len <= pages_len - in_off;
}
