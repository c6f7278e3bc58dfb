// Tree and contexts of the octree anchor codec (include/pcc_geo.h "octree anchor"): everything of
// anchor_octree.py that is data parallel.  The entropy coder itself is sequential and stays on the host (anchor_coder.cpp).
//
// Encoder (pcc_anchor_tree; one stream, nothing read back by the call):
//   k_keys      q = (2 p num + den) / (2 den) per coordinate, exact in 64 bits, and the Morton key of q (cell_index.h's order);
//   hipCUB      radix sort of the keys;
//   k_mark      marks the first of every run of equal key >> shift (that is: the highest differing bit of a key and its
//               predecessor is at or above `shift`); an exclusive scan of the marks numbers the runs;
//   k_compact   writes each run's key >> shift to its number.  shift 0 merges duplicate points; shift 3 turns the nodes of level
//               l + 1 into the nodes of level l, and the run -- contiguous, at most 8 long -- is OR-ed into the node's occupancy byte;
//   k_n6        for every node of a level, six binary searches in the level's own sorted keys (cell_index.h's lower_bound): the
//               face-neighbour mask.  Lanes of a wave hold neighbouring Morton keys, so their searches walk the same cache lines.
//               The same pass marks the level for the next step.
// The levels go bottom-up from the leaves, level l into the slot of min(n, 8^l) bytes the host reserved for it; the number of nodes
// of every level stays on the device, in the header the caller copies back together with the bytes.
//
// Decoder, per level (the host has decoded the level's occupancy bytes and knows every count):
//   k_popc + scan + k_expand   child keys (parent << 3 | c) in ascending order, so the next level is sorted as it is written;
//   k_n6                        the next level's contexts;
//   k_leaves (pcc_anchor_points) after the last level: keys back to coordinates, p = min((2 q den + num) / (2 num), resolution - 1).
//
// Every index is checked against the count or the capacity it belongs to: a wrong count can give wrong bytes, never an access
// outside the buffers.  The only atomics: none.
#include <hipcub/hipcub.hpp>

#include "cell_index.h"

namespace {

constexpr int kMaxDepth = 21;
constexpr int kBlock = 256;

struct TreeHdr {                      // what the caller reads back in front of the bytes (int64[PCC_ANCHOR_HDR_WORDS])
    long long cnt[kMaxDepth + 1];     // nodes of level l; cnt[depth] = distinct quantised points
    long long pad[PCC_ANCHOR_HDR_WORDS - kMaxDepth - 1];
};
static_assert(sizeof(TreeHdr) == 8 * PCC_ANCHOR_HDR_WORDS, "header layout");

__device__ __forceinline__ unsigned compact3(unsigned long long x) {           // inverse of spread3
    x &= 0x1249249249249249ull;
    x = (x | x >> 2) & 0x10c30c30c30c30c3ull;
    x = (x | x >> 4) & 0x100f00f00f00f00full;
    x = (x | x >> 8) & 0x1f0000ff0000ffull;
    x = (x | x >> 16) & 0x1f00000000ffffull;
    x = (x | x >> 32) & 0x1fffffull;
    return (unsigned)x;
}

long long level_bound(long long n, int l) {                   // min(n, 8^l)
    return 3 * l >= 62 || (1ll << (3 * l)) > n ? n : 1ll << (3 * l);
}
long long slot_offset(long long n, int l) {                   // first byte of level l in occ / n6
    long long o = 0;
    for (int j = 0; j < l; ++j) o += level_bound(n, j);
    return o;
}
unsigned grid_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__global__ void __launch_bounds__(kBlock) k_keys(const int32_t* __restrict__ pts, long long n, unsigned long long num, unsigned long long den,
                                                 int depth, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int3 p = load_pt(pts, i);
    const int mask = (int)((1u << depth) - 1);                // depth = bit_length(max q): a no-op for a caller that kept the contract
    const int qx = (int)((2ull * (unsigned)p.x * num + den) / (2ull * den)) & mask;
    const int qy = (int)((2ull * (unsigned)p.y * num + den) / (2ull * den)) & mask;
    const int qz = (int)((2ull * (unsigned)p.z * num + den) / (2ull * den)) & mask;
    keys[i] = morton(qx, qy, qz);
}

// mark[i] = 1 where key[i] >> shift starts a run, for i < *count; 0 from there to `bound`
__global__ void __launch_bounds__(kBlock) k_mark(const unsigned long long* __restrict__ keys, const long long* __restrict__ count, long long fixed,
                                                 long long bound, int shift, unsigned* __restrict__ mark) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound) return;
    long long c = count ? *count : fixed;
    c = c < bound ? c : bound;
    mark[i] = i < c && (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift));
}

// run r (numbered by pos) -> dst[r] = key >> shift; occ (shift 3 only): OR of 1 << (key & 7) over the run; *dst_count = runs
__global__ void __launch_bounds__(kBlock) k_compact(const unsigned long long* __restrict__ keys, const long long* __restrict__ count, long long fixed,
                                                    long long bound, int shift, const unsigned* __restrict__ mark, const unsigned* __restrict__ pos,
                                                    unsigned long long* __restrict__ dst, long long dst_cap, uint8_t* __restrict__ occ,
                                                    long long* __restrict__ dst_count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long c = count ? *count : fixed;
    c = c < bound ? c : bound;
    if (i >= c) return;
    const unsigned m = mark[i];
    const long long r = pos[i];
    if (i == c - 1) *dst_count = r + m;
    if (!m || r >= dst_cap) return;
    const unsigned long long k = keys[i] >> shift;
    dst[r] = k;
    if (occ) {
        unsigned b = 0;
        for (long long j = i; j < c && j < i + 8; ++j) {
            const unsigned long long kj = keys[j];
            if ((kj >> 3) != k) break;
            b |= 1u << (unsigned)(kj & 7);
        }
        occ[r] = (uint8_t)b;
    }
}

// face-neighbour mask of every node of one level (bit 0 / 1: -x / +x, 2 / 3: -y / +y, 4 / 5: -z / +z; outside [0, 2^level): 0), and
// optionally the marks of the next step towards the root
__global__ void __launch_bounds__(kBlock) k_n6(const unsigned long long* __restrict__ keys, const long long* __restrict__ count, long long fixed,
                                               long long bound, int level, uint8_t* __restrict__ n6, unsigned* __restrict__ mark) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound) return;
    long long c = count ? *count : fixed;
    c = c < bound ? c : bound;
    if (i >= c) {
        if (mark) mark[i] = 0;
        return;
    }
    const unsigned long long k = keys[i];
    if (mark) mark[i] = i == 0 || (k >> 3) != (keys[i - 1] >> 3);
    const int x = (int)compact3(k >> 2), y = (int)compact3(k >> 1), z = (int)compact3(k);
    const int top = (int)((1u << level) - 1);
    unsigned b = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int d = (f & 1) ? 1 : -1;
        const int nx = x + (f >> 1 == 0 ? d : 0), ny = y + (f >> 1 == 1 ? d : 0), nz = z + (f >> 1 == 2 ? d : 0);
        if (nx < 0 || ny < 0 || nz < 0 || nx > top || ny > top || nz > top) continue;
        const unsigned long long nk = morton(nx, ny, nz);
        const long long p = lower_bound(keys, c, nk);
        if (p < c && keys[p] == nk) b |= 1u << f;
    }
    n6[i] = (uint8_t)b;
}

__global__ void __launch_bounds__(kBlock) k_popc(const uint8_t* __restrict__ occ, long long n, unsigned* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = (unsigned)__popc((unsigned)occ[i]);
}

__global__ void __launch_bounds__(kBlock) k_expand(const unsigned long long* __restrict__ parents, const uint8_t* __restrict__ occ, long long n,
                                                   const unsigned* __restrict__ pos, unsigned long long* __restrict__ children, long long nchildren) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = parents[i] << 3;
    const unsigned b = occ[i];
    long long o = pos[i];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (b >> c & 1) {
            if (o < nchildren) children[o] = k | (unsigned)c;
            ++o;
        }
}

__global__ void __launch_bounds__(kBlock) k_leaves(const unsigned long long* __restrict__ keys, long long n, unsigned long long num,
                                                   unsigned long long den, int top, int32_t* __restrict__ pts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const unsigned long long q[3] = {compact3(k >> 2), compact3(k >> 1), compact3(k)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned long long p = (2ull * q[a] * den + num) / (2ull * num);
        pts[3 * i + a] = (int32_t)(p < (unsigned long long)top ? p : (unsigned long long)top);
    }
}

struct TreeLayout { size_t keys0, keys1, mark, pos, tmp, tmp_bytes, total; };

TreeLayout tree_layout(long long n) {
    TreeLayout l;
    const size_t N = (size_t)n;
    size_t o = 0, a = 0, b = 0;
    l.keys0 = o; o += al256(N * 8);
    l.keys1 = o; o += al256(N * 8);
    l.mark = o; o += al256(N * 4);
    l.pos = o; o += al256(N * 4);
    (void)hipcub::DeviceRadixSort::SortKeys((void*)nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, 0, 63,
                                            (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, b, (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, (hipStream_t)0);
    l.tmp_bytes = a > b ? a : b;
    l.tmp = o; o += al256(l.tmp_bytes + 256);
    l.total = o;
    return l;
}

size_t expand_tmp_bytes(long long n) {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, b, (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, (hipStream_t)0);
    return b;
}

bool valid_count(int64_t n) { return n >= 1 && n < (1ll << 31); }
bool valid_scale(int64_t num, int64_t den) { return num >= 1 && num <= den && den < (1ll << 31); }

}  // namespace

PCC_API int64_t pcc_anchor_tree_capacity(int64_t npts, int32_t depth) {
    if (!valid_count(npts) || depth < 1 || depth > kMaxDepth) return 0;
    return slot_offset(npts, depth);
}

PCC_API int64_t pcc_anchor_tree_level_offset(int64_t npts, int32_t level) {
    if (!valid_count(npts) || level < 0 || level > kMaxDepth) return -1;
    return slot_offset(npts, level);
}

PCC_API size_t pcc_anchor_tree_workspace_bytes(int64_t npts) {
    if (!valid_count(npts)) return 0;
    return tree_layout(npts).total;
}

PCC_API int pcc_anchor_tree(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int64_t num, int64_t den, int32_t depth, int64_t* hdr, uint8_t* occ,
                            uint8_t* n6, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && pts && hdr && occ && n6 && workspace, "pcc_anchor_tree: NULL argument");
    PCC_REQUIRE(valid_count(npts), "pcc_anchor_tree: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(valid_scale(num, den), "pcc_anchor_tree: scale %lld / %lld: need 0 < num <= den < 2^31", (long long)num, (long long)den);
    PCC_REQUIRE(depth >= 1 && depth <= kMaxDepth, "pcc_anchor_tree: depth = %d outside [1, %d]", depth, kMaxDepth);
    hipStream_t st = (hipStream_t)stream;
    const TreeLayout l = tree_layout(npts);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long* bufs[2] = {(unsigned long long*)(w + l.keys0), (unsigned long long*)(w + l.keys1)};
    unsigned *mark = (unsigned*)(w + l.mark), *pos = (unsigned*)(w + l.pos);
    void* tmp = (void*)(w + l.tmp);
    TreeHdr* H = (TreeHdr*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, sizeof(TreeHdr), st));
    hipLaunchKernelGGL(k_keys, dim3(grid_for(npts)), dim3(kBlock), 0, st, pts, (long long)npts, (unsigned long long)num, (unsigned long long)den,
                       (int)depth, bufs[0]);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, bytes, (const unsigned long long*)bufs[0], bufs[1], (int)npts, 0, 3 * depth, st));
    // duplicates: sorted keys in bufs[1] -> distinct leaves in bufs[0]
    hipLaunchKernelGGL(k_mark, dim3(grid_for(npts)), dim3(kBlock), 0, st, (const unsigned long long*)bufs[1], (const long long*)nullptr,
                       (long long)npts, (long long)npts, 0, mark);
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const unsigned*)mark, pos, (int)npts, st));
    hipLaunchKernelGGL(k_compact, dim3(grid_for(npts)), dim3(kBlock), 0, st, (const unsigned long long*)bufs[1], (const long long*)nullptr,
                       (long long)npts, (long long)npts, 0, (const unsigned*)mark, (const unsigned*)pos, bufs[0], (long long)npts, (uint8_t*)nullptr,
                       &H->cnt[depth]);
    hipLaunchKernelGGL(k_mark, dim3(grid_for(npts)), dim3(kBlock), 0, st, (const unsigned long long*)bufs[0], (const long long*)&H->cnt[depth],
                       0ll, (long long)npts, 3, mark);
    int cur = 0;                                          // bufs[cur]: the nodes of level lv + 1, marked for the step to level lv
    for (int lv = depth - 1; lv >= 0; --lv) {
        const long long cb = level_bound(npts, lv + 1), pb = level_bound(npts, lv), off = slot_offset(npts, lv);
        bytes = l.tmp_bytes;
        PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const unsigned*)mark, pos, (int)cb, st));
        hipLaunchKernelGGL(k_compact, dim3(grid_for(cb)), dim3(kBlock), 0, st, (const unsigned long long*)bufs[cur], (const long long*)&H->cnt[lv + 1],
                           0ll, cb, 3, (const unsigned*)mark, (const unsigned*)pos, bufs[cur ^ 1], pb, occ + off, &H->cnt[lv]);
        cur ^= 1;
        hipLaunchKernelGGL(k_n6, dim3(grid_for(pb)), dim3(kBlock), 0, st, (const unsigned long long*)bufs[cur], (const long long*)&H->cnt[lv], 0ll,
                           pb, lv, n6 + off, lv > 0 ? mark : (unsigned*)nullptr);
    }
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_anchor_expand_workspace_bytes(int64_t nparents) {
    if (!valid_count(nparents)) return 0;
    return 2 * al256((size_t)nparents * 4) + al256(expand_tmp_bytes(nparents) + 256);
}

PCC_API int pcc_anchor_expand(pcc_ctx* ctx, const uint64_t* parents, const uint8_t* occ, int64_t nparents, int32_t child_level, uint64_t* children,
                              int64_t nchildren, uint8_t* n6, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && parents && occ && children && workspace, "pcc_anchor_expand: NULL argument");
    PCC_REQUIRE(valid_count(nparents) && valid_count(nchildren) && nchildren >= nparents && nchildren <= 8 * nparents,
                "pcc_anchor_expand: %lld parents, %lld children", (long long)nparents, (long long)nchildren);
    PCC_REQUIRE(child_level >= 1 && child_level <= kMaxDepth, "pcc_anchor_expand: child level %d outside [1, %d]", child_level, kMaxDepth);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned *cnt = (unsigned*)w, *pos = (unsigned*)(w + al256((size_t)nparents * 4));
    void* tmp = (void*)(w + 2 * al256((size_t)nparents * 4));
    hipLaunchKernelGGL(k_popc, dim3(grid_for(nparents)), dim3(kBlock), 0, st, occ, (long long)nparents, cnt);
    size_t bytes = expand_tmp_bytes(nparents);
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const unsigned*)cnt, pos, (int)nparents, st));
    hipLaunchKernelGGL(k_expand, dim3(grid_for(nparents)), dim3(kBlock), 0, st, (const unsigned long long*)parents, occ, (long long)nparents,
                       (const unsigned*)pos, (unsigned long long*)children, (long long)nchildren);
    if (n6)
        hipLaunchKernelGGL(k_n6, dim3(grid_for(nchildren)), dim3(kBlock), 0, st, (const unsigned long long*)children, (const long long*)nullptr,
                           (long long)nchildren, (long long)nchildren, (int)child_level, n6, (unsigned*)nullptr);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_anchor_points(pcc_ctx* ctx, const uint64_t* keys, int64_t n, int64_t num, int64_t den, int32_t resolution, int32_t* pts, void* stream) {
    PCC_REQUIRE(ctx && keys && pts, "pcc_anchor_points: NULL argument");
    PCC_REQUIRE(valid_count(n), "pcc_anchor_points: n = %lld outside [1, 2^31)", (long long)n);
    PCC_REQUIRE(valid_scale(num, den), "pcc_anchor_points: scale %lld / %lld: need 0 < num <= den < 2^31", (long long)num, (long long)den);
    PCC_REQUIRE(resolution >= 1 && resolution <= (1 << 21), "pcc_anchor_points: resolution = %d outside [1, 2^21]", resolution);
    hipLaunchKernelGGL(k_leaves, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, (const unsigned long long*)keys, (long long)n,
                       (unsigned long long)num, (unsigned long long)den, (int)resolution - 1, pts);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
