// strawboat-hip: sb_key_buckets — the bounds of a column as the kernels search them (sb_key_buckets.h), prepared on the host.
// Host only and nothing but the standard library, so that a stand-alone program can compile it
// (tests/test_key_buckets_host.py does): the checks of the bounds and the ids, the bounds as order keys, the id of each
// bucket, the trip count of the search and the two order keys outside which a float is a NaN.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace sb_buckets {

constexpr uint64_t MAX_BOUNDS = 1023;          // SB_BUCKET_MAX_BOUNDS
constexpr uint32_t RIGHT_CLOSED = 1u;          // SB_BUCKET_RIGHT_CLOSED
constexpr uint32_t ID_NONE = 0xFFFFFFFFu;      // SB_KEY_ID_NONE
enum Kind : uint32_t { UNSIGNED = 0, SIGNED = 1, F32 = 2, F64 = 3 };   // FK_UNSIGNED .. FK_F64 (sb_common.h)

// the trip count of the search over n sorted keys: ceil(log2(n + 1)) (key_steps, sb_common.h)
inline uint32_t steps_of(uint32_t n) {
    uint32_t s = 0;
    while ((1ull << s) < (uint64_t)n + 1) s++;
    return s;
}

// the order key of a value of w bytes (in_key, sb_common.h): unsigned as is, signed sign-extended with the sign bit flipped,
// floats in the total order with -0.0 folded onto +0.0
inline uint64_t order_key(uint32_t kind, uint32_t w, uint64_t raw) {
    if (kind == UNSIGNED) return raw;
    if (kind == SIGNED) {
        const uint32_t sh = 64 - 8 * w;
        return (uint64_t)((int64_t)(raw << sh) >> sh) ^ (1ull << 63);
    }
    if (kind == F32) {
        uint32_t b = (uint32_t)raw;
        if ((b << 1) == 0) b = 0;
        return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
    }
    if ((raw << 1) == 0) raw = 0;
    return (raw >> 63) ? ~raw : (raw | (1ull << 63));
}
// the order keys of -inf and +inf: a float whose key is below the first or above the second is a NaN.  Integers: every key
// lies between them.
inline uint64_t nan_lo_of(uint32_t kind) { return kind == F32 ? order_key(F32, 4, 0xFF800000u) : kind == F64 ? order_key(F64, 8, 0xFFF0000000000000ull) : 0; }
inline uint64_t nan_hi_of(uint32_t kind) { return kind == F32 ? order_key(F32, 4, 0x7F800000u) : kind == F64 ? order_key(F64, 8, 0x7FF0000000000000ull) : ~0ull; }

inline uint64_t load_raw(const uint8_t* p, uint32_t w) {
    uint64_t raw = 0;
    memcpy(&raw, p, w);
    return raw;
}

// What the entry point refuses of the flags and the bounds, in the order it looks: null = fine
inline const char* check_bounds(uint32_t kind, uint32_t w, uint32_t flags, const uint8_t* bounds, uint64_t n_bounds) {
    if (flags & ~RIGHT_CLOSED) return "unknown flags bits";
    if (n_bounds > MAX_BOUNDS) return "n_bounds exceeds SB_BUCKET_MAX_BOUNDS";
    if (n_bounds && !bounds) return "bounds is null";
    const uint64_t lo = nan_lo_of(kind), hi = nan_hi_of(kind);
    uint64_t last = 0;
    for (uint64_t j = 0; j < n_bounds; j++) {
        const uint64_t k = order_key(kind, w, load_raw(bounds + j * w, w));
        if (k < lo || k > hi) return "a bound is NaN";
        if (j && k <= last) return "bounds are not strictly increasing";
        last = k;
    }
    return nullptr;
}
// Every id the call can hand out is below all ones of id_width (1, 2 or 4): bucket_ids[i] unless it is SB_KEY_ID_NONE, or
// n_bounds without them; nan_id likewise, and only on a float column
inline const char* check_ids(uint32_t kind, const uint32_t* bucket_ids, uint64_t n_bounds, uint32_t id_width, uint32_t nan_id) {
    const uint64_t none = id_width >= 4 ? 0xFFFFFFFFull : (1ull << (8 * id_width)) - 1;
    if (!bucket_ids) {
        if (n_bounds >= none) return "n_bounds does not fit below all ones of id_width";
    } else {
        for (uint64_t j = 0; j <= n_bounds; j++)
            if (bucket_ids[j] != ID_NONE && (uint64_t)bucket_ids[j] >= none) return "a bucket_ids entry does not fit id_width";
    }
    if (nan_id != ID_NONE) {
        if (kind != F32 && kind != F64) return "nan_id on an integer column";
        if ((uint64_t)nan_id >= none) return "nan_id does not fit id_width";
    }
    return nullptr;
}

struct Prepared {
    std::vector<uint64_t> keys;   // n order keys, ascending
    std::vector<uint32_t> ids;    // n + 1: the id of each bucket (SB_KEY_ID_NONE: none)
    uint64_t nan_lo = 0, nan_hi = ~0ull;
    uint32_t n = 0, steps = 0;
};

// bounds and ids that check_bounds and check_ids passed; w: bytes per value
inline Prepared prepare(uint32_t kind, uint32_t w, const uint8_t* bounds, const uint32_t* bucket_ids, uint64_t n_bounds) {
    Prepared out;
    out.keys.resize(n_bounds);
    out.ids.resize(n_bounds + 1);
    for (uint64_t j = 0; j < n_bounds; j++) out.keys[j] = order_key(kind, w, load_raw(bounds + j * w, w));
    for (uint64_t j = 0; j <= n_bounds; j++) out.ids[j] = bucket_ids ? bucket_ids[j] : (uint32_t)j;
    out.nan_lo = nan_lo_of(kind);
    out.nan_hi = nan_hi_of(kind);
    out.n = (uint32_t)n_bounds;
    out.steps = steps_of(out.n);
    return out;
}

}  // namespace sb_buckets
