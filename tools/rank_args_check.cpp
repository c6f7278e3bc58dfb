// Stand-alone check of the host side of the rank levels and the count-indexed search entries (csrc/rank_levels.hip, and the argument tests
// of pcc_d1_count_stats / pcc_d12_count_stats in csrc/search_d1.hip / search_d2.hip) under AddressSanitizer and UBSan: the workspace
// arithmetic and the refusals in front of the launches.  Every call here returns before the first HIP call that needs a device, so no GPU
// is needed (without one the sort's temporary-storage query answers nothing and counts as 0 bytes).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/rank_args_check.cpp pcc_geo_cnn_v2_amd/csrc/rank_levels.hip pcc_geo_cnn_v2_amd/csrc/search_d1.hip \
//         pcc_geo_cnn_v2_amd/csrc/search_d2.hip -o rank_args_check && ./rank_args_check
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../include/pcc_geo.h"

// (the library's own lives in ctx.hip)
void pcc_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
}

static int failures = 0;
#define EXPECT(cond)                                        \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("FAIL line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                     \
        }                                                   \
    } while (0)

int main() {
    const int64_t top = 1LL << 28, items = (1LL << 31) - 1;
    // the workspace: 0 outside the contract (B in [1, 65535], n in [0, 2^28], B n < 2^31), else at least the two key and the two value
    // buffers of the sort and the two per-block counters, monotone in n, no overflow at the largest shapes
    EXPECT(pcc_rank_levels_workspace_bytes(0, 64) == 0 && pcc_rank_levels_workspace_bytes(-1, 64) == 0 && pcc_rank_levels_workspace_bytes(1, -1) == 0);
    EXPECT(pcc_rank_levels_workspace_bytes(1, top + 1) == 0 && pcc_rank_levels_workspace_bytes(1, INT64_MAX) == 0);
    EXPECT(pcc_rank_levels_workspace_bytes(65536, 1) == 0 && pcc_rank_levels_workspace_bytes(INT32_MAX, 1) == 0);
    EXPECT(pcc_rank_levels_workspace_bytes(8, top) == 0 && pcc_rank_levels_workspace_bytes(65535, 32769) == 0);      // B n >= 2^31
    EXPECT(pcc_rank_levels_workspace_bytes(7, top) != 0 && pcc_rank_levels_workspace_bytes(65535, 32768) != 0);
    size_t last = 0;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)4097, (int64_t)262144, top - 1, top}) {
        for (int32_t B : {1, 2, 7}) {
            const size_t ws = pcc_rank_levels_workspace_bytes(B, n);
            EXPECT(ws >= (size_t)B * (size_t)n * 24 + (size_t)B * 8 && ws % 256 == 0);
        }
        const size_t one = pcc_rank_levels_workspace_bytes(1, n);
        EXPECT(one >= last);
        last = one;
    }
    EXPECT(pcc_rank_levels_workspace_bytes(65535, items / 65535) != 0);
    // refusals of pcc_rank_levels, each before anything is launched: a fake context pointer is never dereferenced on these paths
    pcc_ctx* ctx = (pcc_ctx*)&failures;
    float x[8] = {};
    uint8_t lev[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    int32_t counts[3] = {3, 2, 1}, tcount[1] = {-1};
    char ws[1];
    EXPECT(pcc_rank_levels(nullptr, x, 8, 1, 8, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, -1, 8, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 65536, 8, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, -8, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, top + 1, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, INT64_MAX, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, top, 8, top, counts, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);           // B n >= 2^31
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, 8, counts, 0, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, 8, counts, 256, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, 8, counts, -1, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, 8, nullptr, 3, lev, tcount, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, x, 8, 1, 8, counts, 3, lev, nullptr, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_rank_levels(ctx, nullptr, 0, 0, 8, nullptr, 3, nullptr, nullptr, nullptr, 0, nullptr) == PCC_OK);           // B = 0
    EXPECT(tcount[0] == -1 && lev[0] == 9);
    // ... and of the two statistics entries: their own argument tests come before the device is selected
    int32_t pts[3] = {0, 0, 0}, block_of[1] = {0}, block_start[2] = {0, 1};
    float normals[3] = {0, 0, 1};
    uint64_t s_ab[256], hsum[256], hcnt[256];
    double d2_ab[256], d2_ba[256];
    char w1[1], w2[1];
#define D1(ctx_, x_, B_, D_, counts_, J_, rws_) \
    pcc_d1_count_stats(ctx_, x_, B_, D_, 2, 2, counts_, J_, pts, block_of, 1, w1, rws_, sizeof ws, s_ab, hsum, hcnt, tcount, nullptr)
    EXPECT(D1(nullptr, x, 1, 2, counts, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, nullptr, 1, 2, counts, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 1, 2, nullptr, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 1, 2, counts, 3, nullptr) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 0, 2, counts, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 65536, 2, counts, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 1, 129, counts, 3, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 1, 2, counts, 0, ws) == PCC_ERR_ARG);
    EXPECT(D1(ctx, x, 1, 2, counts, 256, ws) == PCC_ERR_ARG);
#define D12(normals_, w2_, J_) \
    pcc_d12_count_stats(ctx, x, 1, 2, 2, 2, counts, J_, pts, block_of, block_start, 1, normals_, w1, w2_, ws, sizeof ws, s_ab, hsum, hcnt, tcount, \
                        d2_ab, d2_ba, nullptr)
    EXPECT(D12(nullptr, w2, 3) == PCC_ERR_ARG);
    EXPECT(D12(normals, nullptr, 3) == PCC_ERR_ARG);
    EXPECT(D12(normals, w2, 0) == PCC_ERR_ARG);
    EXPECT(D12(normals, w2, 256) == PCC_ERR_ARG);
    EXPECT(tcount[0] == -1);
    printf(failures ? "%d check(s) failed\n" : "rank_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
