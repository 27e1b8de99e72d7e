// strawboat-hip: sb_key_lookup — the list of a column as the kernels search it (sb_key_lookup.h), prepared on the host.
// Host only and nothing but the standard library, so that a stand-alone program can compile it
// (tests/test_key_lookup_host.py does): the checks of the list, the sort, the dedup that keeps the first occurrence, the
// id of each sorted position and the trip count of the search.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace sb_lookup {

constexpr uint64_t MAX_VALUES = 1024;   // SB_KEY_MAX_KEYS
constexpr uint64_t MAX_LIST_BYTES = 1ull << 30;

// the trip count of the search over n sorted keys: ceil(log2(n + 1)) (key_steps, sb_common.h)
inline uint32_t steps_of(uint32_t n) {
    uint32_t s = 0;
    while ((1ull << s) < (uint64_t)n + 1) s++;
    return s;
}

// the order key of an integer of w bytes (in_key, sb_common.h): unsigned as is, signed sign-extended with the sign bit flipped
inline uint64_t order_key(bool is_signed, uint32_t w, uint64_t raw) {
    if (!is_signed) return raw;
    const uint32_t sh = 64 - 8 * w;
    return (uint64_t)((int64_t)(raw << sh) >> sh) ^ (1ull << 63);
}

// What the entry point refuses of a list, in the order it looks: null = fine.  `binary`: the column's type.
inline const char* check_list(bool binary, const uint8_t* values, const uint64_t* value_offsets, uint64_t n_values) {
    if (n_values > MAX_VALUES) return "n_values exceeds SB_KEY_MAX_KEYS";
    if (!binary) {
        if (value_offsets) return "value_offsets on a numeric column";
        if (n_values && !values) return "values is null";
        return nullptr;
    }
    if (!n_values) return nullptr;
    if (!value_offsets) return "value_offsets is null";
    if (value_offsets[0] != 0) return "value_offsets[0] is not 0";
    for (uint64_t j = 0; j < n_values; j++)
        if (value_offsets[j + 1] < value_offsets[j]) return "value_offsets descend";
    if (value_offsets[n_values] > MAX_LIST_BYTES) return "the values of a column have at most 2^30 bytes";
    if (value_offsets[n_values] && !values) return "values is null";
    return nullptr;
}
// Every id the list can hand out is below all ones of id_width (1, 2 or 4): value_ids[i], or n_values - 1 without them
inline const char* check_ids(const uint32_t* value_ids, uint64_t n_values, uint32_t id_width) {
    const uint64_t none = id_width >= 4 ? 0xFFFFFFFFull : (1ull << (8 * id_width)) - 1;
    if (!value_ids) return n_values && n_values - 1 >= none ? "n_values - 1 does not fit below all ones of id_width" : nullptr;
    for (uint64_t j = 0; j < n_values; j++)
        if ((uint64_t)value_ids[j] >= none) return "a value_ids entry is all ones or does not fit id_width";
    return nullptr;
}

struct Prepared {
    std::vector<uint64_t> words;   // numeric: n order keys, ascending; binary: n + 1 ascending offsets into `bytes`
    std::vector<uint32_t> ids;     // n: the id of each sorted position
    std::vector<uint8_t> bytes;    // binary: the values in byte-string order, back to back, then 8 zero bytes
    uint32_t n = 0, steps = 0;
};

// a list that check_list passed; w: bytes per value.  A value that repeats keeps the id of its first occurrence.
inline Prepared prepare_numeric(const uint8_t* values, uint32_t w, bool is_signed, const uint32_t* value_ids, uint64_t n_values) {
    Prepared out;
    std::vector<uint64_t> key(n_values);
    for (uint64_t j = 0; j < n_values; j++) {
        uint64_t raw = 0;
        memcpy(&raw, values + j * w, w);
        key[j] = order_key(is_signed, w, raw);
    }
    std::vector<uint32_t> at(n_values);
    std::iota(at.begin(), at.end(), 0u);
    std::sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    for (uint32_t j : at) {
        if (!out.words.empty() && out.words.back() == key[j]) continue;   // (a later occurrence: sorted behind the first)
        out.words.push_back(key[j]);
        out.ids.push_back(value_ids ? value_ids[j] : j);
    }
    out.n = (uint32_t)out.words.size();
    out.steps = steps_of(out.n);
    return out;
}

// bytes unsigned, lexicographic, a proper prefix before the longer string
inline int compare_bytes(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t m = std::min(la, lb);
    const int r = m ? memcmp(a, b, m) : 0;
    return r ? r : la < lb ? -1 : la > lb ? 1 : 0;
}
inline Prepared prepare_binary(const uint8_t* values, const uint64_t* value_offsets, const uint32_t* value_ids, uint64_t n_values) {
    Prepared out;
    auto cmp = [&](uint32_t a, uint32_t b) {
        return compare_bytes(values + value_offsets[a], value_offsets[a + 1] - value_offsets[a], values + value_offsets[b],
                             value_offsets[b + 1] - value_offsets[b]);
    };
    std::vector<uint32_t> at(n_values);
    std::iota(at.begin(), at.end(), 0u);
    std::sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) {
        const int r = cmp(a, b);
        return r ? r < 0 : a < b;
    });
    out.words.push_back(0);
    uint32_t last = 0;
    for (uint32_t j : at) {
        if (!out.ids.empty() && cmp(last, j) == 0) continue;
        last = j;
        const uint64_t len = value_offsets[j + 1] - value_offsets[j];
        if (len) out.bytes.insert(out.bytes.end(), values + value_offsets[j], values + value_offsets[j] + len);
        out.words.push_back(out.bytes.size());
        out.ids.push_back(value_ids ? value_ids[j] : j);
    }
    out.bytes.insert(out.bytes.end(), 8, (uint8_t)0);
    out.n = (uint32_t)out.ids.size();
    out.steps = steps_of(out.n);
    return out;
}

}  // namespace sb_lookup
