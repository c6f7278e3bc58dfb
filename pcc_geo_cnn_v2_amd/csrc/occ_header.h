// The header of an "occ1" string against its length: shared by the host check (pcc_occ_check_strings), the decode
// kernel and the stand-alone sanitizer program tools/occ_header_check.cpp.  Plain C++: no HIP header is needed to compile it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OCC_HD __host__ __device__
#else
#define OCC_HD
#endif

constexpr int kOccBuckets = 32;                  // K
constexpr int kOccMaxLanes = 64;
constexpr int64_t kOccMaxVoxels = (int64_t)1 << 28;

// bytes of the longest string of an n-voxel block: lane byte, K entries, 64 states, one word per voxel
OCC_HD inline int64_t occ_stream_cap(int64_t n) { return 1 + 2 * kOccBuckets + 4 * kOccMaxLanes + 2 * n; }

// What a reader knows WITHOUT x_hat: byte 0 is log2 L <= 6, and entries (2 bytes each), states (4 L bytes) and words (2 bytes each)
// leave len - 1 - 4 L even, non-negative and at most 2 (K + n).  `used` (the number of entries) and m (the coded voxels) follow from
// x_hat, so only the device can validate a string fully (occ_split below).  get(q) returns byte q; it is only called with q < len.
template <class Get>
OCC_HD inline bool occ_parse_lanes(Get get, int64_t len, int64_t n, int32_t& L) {
    if (n <= 0) return n == 0 && len == 0;
    if (len < 1) return false;
    const uint32_t lg = get(0);
    if (lg > 6) return false;
    L = 1 << lg;
    const int64_t rest = len - 1 - 4 * (int64_t)L;
    return rest >= 0 && (rest & 1) == 0 && rest <= 2 * (kOccBuckets + n);
}

// With `used` known: the string is 1 + 2 used + 4 L + 2 n_words bytes.  (n_words <= m is the caller's test: m needs the entries.)
OCC_HD inline bool occ_split(int64_t len, int32_t L, int32_t used, int64_t& n_words) {
    const int64_t rest = len - 1 - 2 * (int64_t)used - 4 * (int64_t)L;
    if (rest < 0 || (rest & 1)) return false;
    n_words = rest / 2;
    return true;
}

// Host: the first string of a batch whose lane byte or length cannot be right, or -1.  Negative off / len / n count as bad.
inline int32_t occ_first_bad_string(int32_t n_streams, const uint8_t* str, const int64_t* off, const int32_t* len, int64_t n) {
    for (int32_t s = 0; s < n_streams; ++s) {
        if (off[s] < 0 || len[s] < 0 || n < 0) return s;
        const uint8_t* sp = str + off[s];
        int32_t L = 0;
        if (!occ_parse_lanes([&](int64_t q) { return (uint32_t)sp[q]; }, len[s], n, L)) return s;
    }
    return -1;
}
