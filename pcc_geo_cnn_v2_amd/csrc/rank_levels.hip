// Rank levels of libpcc_geo_hip.so: the level grid of the per-block D1/D2 search (search_d1.hip, search_d2.hip) built from RANKS instead of
// score thresholds, so that the engines score the top-c[j] sets of a block -- the sets pcc_topk_compact (topk_select.hip) decodes -- for a
// whole row of candidate counts at once (include/pcc_geo.h "rank levels").
//
// Per block: key(i) = raw bits of x[i] where x[i] > 0, else 0; rank(i) = position of voxel i among the P voxels with key > 0 in the order
// (key descending, i ascending); lev(i) = #{j : rank(i) < c[j]} for key(i) > 0, else 0; tcount = #{j : c[j] >= 1} when P >= 1, else 0.
//
//   keys      every voxel writes a 64-bit sort key and its own index as the value: block << 31 | (0x7fffffff - key) for key > 0, else a pad
//             key that carries the block number B and so sorts behind every block; the positive voxels of a segment are counted by ballot
//             and popcount and added to the block's P (one integer atomic per workgroup; the zero bulk behind the ReLU is one compare per
//             voxel here, but takes part in the sort: see the open gap in DESIGN.md 4.20)
//   sort      ONE stable radix sort (hipcub, as in search_d2.hip) of all B n pairs on the 31 + bits(B) low bits: ascending keys are blocks
//             in order and inside a block keys descending; stability keeps equal keys in ascending voxel index, the order they were written in
//   start     one workgroup: exclusive prefix of P over the blocks = the first sorted position of every block; tcount
//   store     a workgroup owns 4096 consecutive ranks of one block and holds the block's row in LDS: rank r stores #{j : r < c[j]} at the voxel
//             the sorted value names.  The count walks the whole row (LDS broadcast reads), so it is the formula for ANY row, ordered or not.
// Nothing score-valued is accumulated; every store into lev is under the test index < n.  The result of a block depends on its scores and its
// row alone: the sort is a total order on (block, key, index).
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSeg = 4096, kPer = kSeg / kThreads;      // voxels (keys) / ranks (store) per workgroup, per thread
constexpr int kMaxJ = 255;
constexpr int64_t kMaxVoxels = 1LL << 28;
constexpr int64_t kMaxItems = (1LL << 31) - 1;          // the sort counts its items in an int

struct Layout {
    size_t keys0, keys1, vals0, vals1, P, start, sort_tmp, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// (B >= 1, 0 <= n <= kMaxVoxels, B n <= kMaxItems: no overflow below)
inline Layout layout_of(int32_t B, int64_t n, size_t sort_tmp_bytes) {
    const size_t items = (size_t)B * (size_t)n;
    Layout l;
    size_t o = 0;
    l.keys0 = o; o += up256(items * 8);
    l.keys1 = o; o += up256(items * 8);
    l.vals0 = o; o += up256(items * 4);
    l.vals1 = o; o += up256(items * 4);
    l.P = o;     o += up256((size_t)B * 4);
    l.start = o; o += up256((size_t)B * 4);
    l.sort_tmp = o; o += up256(sort_tmp_bytes + 256);
    l.total = o;
    return l;
}

inline bool shape_ok(int32_t B, int64_t n) { return B >= 1 && B <= 65535 && n >= 0 && n <= kMaxVoxels && (int64_t)B * n <= kMaxItems; }

inline int sort_bits(int32_t B) {                       // the pad key carries block number B
    int bits = 0;
    while ((B >> bits) != 0) ++bits;
    return 31 + bits;
}

// temporary storage of the sort for `items` pairs (0 when it cannot be asked, e.g. without a device: the call itself checks again)
inline size_t sort_tmp_bytes_of(size_t items, int end_bit) {
    size_t bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs((void*)nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                           (const unsigned*)nullptr, (unsigned*)nullptr, (int)(items ? items : 1), 0, end_bit,
                                           (hipStream_t)0) != hipSuccess)
        return 0;
    return bytes;
}

__global__ __launch_bounds__(kThreads) void rank_keys_kernel(const float* __restrict__ x, int64_t x_stride, int n, int B,
                                                             unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                             int* __restrict__ P) {
    __shared__ int wcnt[kWaves];
    const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float* xb = x + (int64_t)b * x_stride;
    const unsigned long long pad = ((unsigned long long)B << 31) | 0x7fffffffull, head = (unsigned long long)b << 31;
    const size_t out = (size_t)b * (size_t)n;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = g * kSeg + j * kThreads + tid;
        const float v = i < n ? xb[i] : 0.0f;
        const bool pos = v > 0.0f;                          // NaN, -0, +0 and negatives have key 0
        cnt += __popcll(__ballot(pos));
        if (i < n) {
            keys[out + i] = pos ? head | (unsigned long long)(0x7fffffffu - __float_as_uint(v)) : pad;
            vals[out + i] = (unsigned)i;
        }
    }
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wcnt[w];
        if (s) atomicAdd(&P[b], s);
    }
}

// one workgroup: start[b] = sum of P over the blocks before b; tcount[b] = #{j : c[b][j] >= 1} when P[b] >= 1, else 0
__global__ __launch_bounds__(kThreads) void rank_start_kernel(const int* __restrict__ P, int B, const int32_t* __restrict__ counts, int J,
                                                              int* __restrict__ start, int32_t* __restrict__ tcount) {
    __shared__ int lds[kThreads];
    const int tid = (int)threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += kThreads) {
        const int b = b0 + tid;
        const int p = b < B ? P[b] : 0;
        lds[tid] = p;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {      // inclusive scan in place
            const int t = tid >= off ? lds[tid - off] : 0;
            __syncthreads();
            lds[tid] += t;
            __syncthreads();
        }
        if (b < B) {
            start[b] = carry + lds[tid] - p;
            int live = 0;
            if (p >= 1)
                for (int j = 0; j < J; ++j) live += counts[(size_t)b * J + j] >= 1;
            tcount[b] = live;
        }
        carry += lds[kThreads - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void rank_store_kernel(const unsigned* __restrict__ vals, const int* __restrict__ P,
                                                              const int* __restrict__ start, const int32_t* __restrict__ counts, int J, int n,
                                                              unsigned char* __restrict__ lev) {
    __shared__ int row[kMaxJ + 1];
    const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int Pb = P[b], r0 = g * kSeg;
    if (r0 >= Pb) return;                                   // (uniform: the ranks of this workgroup do not exist)
    if (tid < J) {
        const int c = counts[(size_t)b * J + tid];
        row[tid] = c < 0 ? 0 : c;
    }
    __syncthreads();
    const unsigned* vb = vals + start[b];
    unsigned char* lb = lev + (size_t)b * (size_t)n;
#pragma unroll 1
    for (int e = 0; e < kPer; ++e) {
        const int r = r0 + e * kThreads + tid;
        if (r >= Pb) break;
        int l = 0;
        for (int j = 0; j < J; ++j) l += r < row[j];
        const unsigned i = vb[r];
        if (i < (unsigned)n) lb[i] = (unsigned char)l;      // l <= J <= 255
    }
}

}  // namespace

PCC_API size_t pcc_rank_levels_workspace_bytes(int32_t B, int64_t n) {
    if (!shape_ok(B, n)) return 0;
    return layout_of(B, n, sort_tmp_bytes_of((size_t)B * (size_t)n, sort_bits(B))).total;
}

PCC_API int pcc_rank_levels(pcc_ctx* ctx, const float* x, int64_t x_stride, int32_t B, int64_t n, const int32_t* counts, int32_t J,
                            unsigned char* lev, int32_t* tcount, void* workspace, size_t workspace_bytes, void* stream) {
    PCC_REQUIRE(ctx, "pcc_rank_levels: NULL context");
    PCC_REQUIRE(B >= 0 && B <= 65535 && n >= 0, "pcc_rank_levels: bad dimension");
    PCC_REQUIRE(n <= kMaxVoxels, "pcc_rank_levels: %lld voxels per block (at most 2^28)", (long long)n);
    PCC_REQUIRE(J >= 1 && J <= kMaxJ, "pcc_rank_levels: %d candidate counts per block (1 to 255)", (int)J);
    if (B == 0) return PCC_OK;
    PCC_REQUIRE((int64_t)B * n <= kMaxItems, "pcc_rank_levels: %lld voxels in one call (below 2^31)", (long long)((int64_t)B * n));
    PCC_REQUIRE(tcount && counts, "pcc_rank_levels: NULL pointer");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        PCC_CHECK_HIP(hipMemsetAsync(tcount, 0, (size_t)B * sizeof(int32_t), st));
        return PCC_OK;
    }
    PCC_REQUIRE(x && lev && workspace, "pcc_rank_levels: NULL pointer");
    PCC_REQUIRE(B == 1 || x_stride >= n, "pcc_rank_levels: stride %lld below n = %lld", (long long)x_stride, (long long)n);
    const size_t items = (size_t)B * (size_t)n;
    const int end_bit = sort_bits(B);
    size_t tmp = 0;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                     (const unsigned*)nullptr, (unsigned*)nullptr, (int)items, 0, end_bit, st));
    const Layout l = layout_of(B, n, tmp);
    PCC_REQUIRE(workspace_bytes >= l.total, "pcc_rank_levels: workspace %zu < pcc_rank_levels_workspace_bytes (%zu)", workspace_bytes, l.total);
    char* ws = (char*)workspace;
    unsigned long long *keys0 = (unsigned long long*)(ws + l.keys0), *keys1 = (unsigned long long*)(ws + l.keys1);
    unsigned *vals0 = (unsigned*)(ws + l.vals0), *vals1 = (unsigned*)(ws + l.vals1);
    int *P = (int*)(ws + l.P), *start = (int*)(ws + l.start);
    const int G = (int)((n + kSeg - 1) / kSeg);
    const dim3 grid((unsigned)G, (unsigned)B), threads(kThreads);
    PCC_CHECK_HIP(hipMemsetAsync(P, 0, (size_t)B * sizeof(int), st));
    PCC_CHECK_HIP(hipMemsetAsync(lev, 0, items, st));
    hipLaunchKernelGGL(rank_keys_kernel, grid, threads, 0, st, x, x_stride, (int)n, (int)B, keys0, vals0, P);
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(ws + l.sort_tmp), tmp, keys0, keys1, vals0, vals1, (int)items, 0, end_bit, st));
    hipLaunchKernelGGL(rank_start_kernel, dim3(1), threads, 0, st, P, (int)B, counts, (int)J, start, tcount);
    hipLaunchKernelGGL(rank_store_kernel, grid, threads, 0, st, vals1, P, start, counts, (int)J, (int)n, lev);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
