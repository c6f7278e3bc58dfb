// Stand-alone check of the host side of the top-k selection (csrc/topk_select.hip: the workspace arithmetic and the argument tests in
// front of the launches) under AddressSanitizer and UBSan.  Every call here returns before the first HIP call, so no GPU is needed.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/topk_args_check.cpp pcc_geo_cnn_v2_amd/csrc/topk_select.hip -o topk_args_check && ./topk_args_check
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
    const int64_t top = 1LL << 28;
    // the workspace: 0 outside the contract, else proportional to B and monotone in n, no overflow at the largest shapes
    EXPECT(pcc_topk_workspace_bytes(0, 64) == 0 && pcc_topk_workspace_bytes(-1, 64) == 0 && pcc_topk_workspace_bytes(1, -1) == 0);
    EXPECT(pcc_topk_workspace_bytes(1, top + 1) == 0 && pcc_topk_workspace_bytes(1, INT64_MAX) == 0);
    size_t last = 0;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)4097, (int64_t)262144, top - 1, top}) {
        const size_t one = pcc_topk_workspace_bytes(1, n);
        EXPECT(one >= 3 * 2048 * 4 + 32 + 8 * (size_t)((n + 4095) / 4096) && one >= last && one % 16 == 0);
        for (int32_t B : {65535, INT32_MAX}) {              // (the segment part is rounded up to 16 bytes once per call)
            const size_t many = pcc_topk_workspace_bytes(B, n);
            EXPECT(many <= (size_t)B * one && many >= (size_t)B * (one - 15) && many % 16 == 0);
        }
        last = one;
    }
    // refusals, each before anything is launched: a fake context pointer is never dereferenced on these paths
    pcc_ctx* ctx = (pcc_ctx*)&failures;
    float x[8] = {}, xyz[24];
    int32_t k[1] = {3}, counts[1] = {-1};
    char ws[1];
    EXPECT(pcc_topk_compact(nullptr, x, 8, 1, 2, 2, 2, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, -1, 2, 2, 2, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 65536, 2, 2, 2, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, -2, 2, 2, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, 2, 2, 2, k, xyz, counts, -1, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, 1024, 1024, 257, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, INT32_MAX, INT32_MAX, INT32_MAX, k, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, 2, 2, 2, nullptr, xyz, counts, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, x, 8, 1, 2, 2, 2, k, xyz, nullptr, 8, ws, sizeof ws, nullptr) == PCC_ERR_ARG);
    EXPECT(pcc_topk_compact(ctx, nullptr, 0, 0, 2, 2, 2, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == PCC_OK);      // B = 0
    EXPECT(counts[0] == -1);
    printf(failures ? "%d check(s) failed\n" : "topk_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
