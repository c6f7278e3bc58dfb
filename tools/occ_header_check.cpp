// Stand-alone check of the host-only part of the occ1 coder (csrc/occ_header.h: what pcc_occ_check_strings runs) on damaged strings.
// Every string lives in a heap block of exactly its length, so a read past it is an AddressSanitizer report.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/occ_header_check.cpp -o occ_header_check && ./occ_header_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pcc_geo_cnn_v2_amd/csrc/occ_header.h"

static int failures = 0;

static void expect(const char* what, const std::vector<std::vector<uint8_t>>& strings, int64_t n, int32_t want) {
    // the strings back to back in one exact-size block, as the wrapper uploads them
    size_t total = 0;
    for (const auto& s : strings) total += s.size();
    uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    size_t pos = 0;
    for (const auto& s : strings) {
        if (!s.empty()) memcpy(blob + pos, s.data(), s.size());
        off.push_back((int64_t)pos);
        len.push_back((int32_t)s.size());
        pos += s.size();
    }
    const int32_t got = occ_first_bad_string((int32_t)strings.size(), blob, off.data(), len.data(), n);
    if (got != want) {
        printf("FAIL %s: first bad string %d, expected %d\n", what, got, want);
        ++failures;
    }
    free(blob);
}

int main() {
    // a string of the right form for n = 64 voxels in one bucket: L = 2, one entry, two states, three words
    std::vector<uint8_t> good = {1, 0x00, 0x80, 0, 0, 1, 0, 0, 0, 1, 0, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0xff};
    const int64_t n = 64;
    auto cut = [&](size_t k) { return std::vector<uint8_t>(good.begin(), good.end() - (long)k); };
    auto more = good;
    more.push_back(0);
    more.push_back(0);
    auto lane7 = good;
    lane7[0] = 7;

    expect("the string as it is", {good}, n, -1);
    expect("truncated by one byte (parity)", {good, cut(1)}, n, 1);
    expect("truncated by two bytes (the device's to refuse: used and m need x_hat)", {cut(2)}, n, -1);
    expect("two bytes appended (the device's to refuse)", {more}, n, -1);
    expect("lane byte 7", {good, good, lane7}, n, 2);
    expect("the empty string for n > 0", {{}}, n, 0);
    expect("shorter than its states", {std::vector<uint8_t>{6, 1, 2}}, n, 0);
    expect("a lane byte alone", {std::vector<uint8_t>{0}}, n, 0);
    expect("longer than any block of n voxels codes to", {std::vector<uint8_t>(1 + 4 + 2 * (kOccBuckets + 1) + 2, 0)}, 1, 0);
    expect("the longest string of n = 1", {std::vector<uint8_t>(1 + 4 + 2 * (kOccBuckets + 1), 0)}, 1, -1);
    expect("n = 0 takes the empty string only", {{}}, 0, -1);
    expect("bytes for n = 0", {good}, 0, 0);
    expect("a negative voxel count", {good}, -1, 0);
    expect("no strings", {}, n, -1);
    // every prefix and every lane byte: nothing may read outside the string
    for (size_t k = 0; k <= good.size(); ++k)
        for (int lg = 0; lg < 256; lg += (lg < 8 ? 1 : 31)) {
            auto s = cut(k);
            if (!s.empty()) s[0] = (uint8_t)lg;
            int64_t off = 0;
            int32_t len = (int32_t)s.size();
            uint8_t* p = (uint8_t*)malloc(s.size() ? s.size() : 1);
            if (!s.empty()) memcpy(p, s.data(), s.size());
            (void)occ_first_bad_string(1, p, &off, &len, n);
            int64_t n_words = 0;
            (void)occ_split(len, 1 << (lg & 7), 3, n_words);
            free(p);
        }
    if (occ_stream_cap(64) != 1 + 64 + 256 + 128) { printf("FAIL occ_stream_cap\n"); ++failures; }
    printf(failures ? "occ_header_check: %d failure(s)\n" : "occ_header_check: ok\n", failures);
    return failures ? 1 : 0;
}
