// Transform of the colour anchor codec (include/pcc_geo.h "colour anchor"): an integer weighted-Haar lifting over the
// binary Morton tree of a voxelised cloud (the class of G-PCC's RAHT; NOT RAHT-conformant).  Integers only: no float reaches a
// result (isqrt starts from a double sqrt and is corrected to the exact floor), no result depends on an atomic's order or on the
// launch geometry.  The entropy coder is sequential and stays on the host (anchor_coder.cpp).
//
// Leaves 0 .. N - 1 are the points in ascending Morton order.  Leaf i >= 1 owns the one coefficient of the node whose right child
// starts at i: step s = d(i) = the highest bit in which key[i - 1] and key[i] differ.  The node's leaves are [p0, p1), the keys that
// agree with key[i] above bit s; the children are [p0, i) and [i, p1), their weights the leaf counts.
//
//   pcc_color_anchor_plan     k_keys (Morton key, row), hipCUB radix sort over the 3 D key bits, k_d (d(i) of every i >= 1 and the
//                             number of adjacent equal keys = duplicate positions), a stable 6-bit radix sort of the leaf indices by
//                             d: the leaves of one step are one contiguous, ascending segment; k_offsets finds the 65 segment bounds
//                             by binary search (hdr[s] = leaves of step s).  The plan stays in the workspace.
//   pcc_color_anchor_forward  k_leaves (RGB -> YCoCg-R in leaf order), then ONE launch per step s = 0 .. 3 D - 1 over that step's
//                             segment (its bounds are read from the device: the host never waits): h = val[i] - val[p0], val[p0] +=
//                             floor(wR h / w), quantise in the same lane, int16 c[3] straight to the coefficient's place in coding
//                             order (steps descending, i ascending inside a step).  The leaves of one step touch disjoint pairs
//                             (p0, i) and kernel boundaries order the steps.  val[0] ends as the DC triple.
//   pcc_color_anchor_inverse  val[0] = DC, one launch per step descending: aL = val[p0] - floor(wR h^ / w), val[p0] = aL, val[i] = aL
//                             + h^; k_colors turns the leaves back into RGB, clipped, in the caller's row order.
//
// The transform runs in place on one N x 3 int32 array.  Every index is checked against its count: a workspace that no plan filled
// gives wrong values, never an access outside the buffers.
#include <hipcub/hipcub.hpp>

#include "cell_index.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSteps = 64;                    // d(i) < 63; bin 63 stays empty, off[64] = N - 1
constexpr int kHdrDup = 64, kHdrDc = 65;

unsigned grid_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }
bool valid_count(int64_t n) { return n >= 1 && n < (1ll << 31); }
bool valid_depth(int32_t d) { return d >= 1 && d <= 21; }
bool valid_q(int32_t q) { return q >= 1 && q <= 255; }

__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ long long isqrt(long long x) {                        // floor(sqrt(x)), 0 <= x < 2^52
    long long r = (long long)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) k_keys(const int32_t* __restrict__ pts, long long n, int bits, unsigned long long* __restrict__ keys,
                                                 unsigned* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int3 p = load_pt(pts, i);
    keys[i] = morton(p.x, p.y, p.z) & ((1ull << bits) - 1);      // bits <= 63; a coordinate above the stated depth is masked
    rows[i] = (unsigned)i;
}

// entry t = leaf t + 1.  The duplicate count is a sum of integers: it does not depend on the order of the atomics.
__global__ void __launch_bounds__(kBlock) k_d(const unsigned long long* __restrict__ keys, long long n, uint8_t* __restrict__ d,
                                              unsigned* __restrict__ idx, long long* __restrict__ hdr) {
    __shared__ unsigned dup;
    if (threadIdx.x == 0) dup = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n - 1) {
        const unsigned long long x = keys[t] ^ keys[t + 1];
        if (x == 0) atomicAdd(&dup, 1u);
        d[t] = x ? (uint8_t)(63 - __clzll((long long)x)) : 0;
        idx[t] = (unsigned)(t + 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && dup) atomicAdd((unsigned long long*)&hdr[kHdrDup], (unsigned long long)dup);
}

// off[s] = the first entry of the sorted d that is >= s, s = 0 .. 64; hdr[s] = off[s + 1] - off[s]
__global__ void __launch_bounds__(128) k_offsets(const uint8_t* __restrict__ d, long long m, long long* __restrict__ off, long long* __restrict__ hdr) {
    __shared__ long long o[kSteps + 1];
    const int s = threadIdx.x;
    if (s <= kSteps) {
        long long lo = 0, hi = m;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((int)d[mid] < s) lo = mid + 1; else hi = mid;
        }
        o[s] = lo;
        off[s] = lo;
    }
    __syncthreads();
    if (s < kSteps) hdr[s] = o[s + 1] - o[s];
}

// ---- transform -------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) k_leaves(const uint8_t* __restrict__ colors, const unsigned* __restrict__ rows, long long n,
                                                   int32_t* __restrict__ val) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long r = rows[j];
    if (r >= n) return;
    const int R = colors[3 * r], G = colors[3 * r + 1], B = colors[3 * r + 2];
    const int co = R - B, t = B + (co >> 1), cg = G - t;
    val[3 * j] = t + (cg >> 1);
    val[3 * j + 1] = co;
    val[3 * j + 2] = cg;
}

struct Node { long long i, p0, wl, wr, step, pos; bool ok; };

// the node of entry t of step s: its leaves, weights, quantiser step and place in coding order
__device__ __forceinline__ Node node_of(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ order, long long n, int s, int q,
                                        long long t, long long lo, long long hi) {
    Node nd;
    nd.ok = false;
    nd.i = order[t];
    if (nd.i < 1 || nd.i >= n) return nd;
    const unsigned long long base = keys[nd.i] >> (s + 1) << (s + 1), top = base + (1ull << (s + 1));     // s + 1 <= 63, keys < 2^63
    // the run around i: gallop to a bracket, then cell_index.h's lower_bound inside it
    long long a = nd.i, g = 1;                                      // keys[a] >= base throughout
    while (a - g >= 0 && keys[a - g] >= base) { a -= g; g <<= 1; }
    const long long a0 = a - g >= 0 ? a - g + 1 : 0;                // keys[a - g] < base, or the array starts here
    nd.p0 = a0 + lower_bound(keys + a0, a - a0, base);
    long long b = nd.i;                                             // keys[b] < top throughout
    g = 1;
    while (b + g < n && keys[b + g] < top) { b += g; g <<= 1; }
    const long long b1 = b + g < n ? b + g : n;                     // keys[b + g] >= top, or the array ends here
    const long long p1 = b + 1 + lower_bound(keys + b + 1, b1 - (b + 1), top);
    nd.wl = nd.i - nd.p0;
    nd.wr = p1 - nd.i;
    if (nd.wl < 1 || nd.wr < 1) return nd;
    const long long st = isqrt((long long)q * q * (nd.wl + nd.wr) / (nd.wl * nd.wr));
    nd.step = st < 1 ? 1 : st;
    nd.pos = (n - 1 - hi) + (t - lo);
    nd.ok = nd.pos >= 0 && nd.pos < n - 1;
    return nd;
}

// the segment of step s, clamped to the n - 1 entries
__device__ __forceinline__ void segment(const long long* __restrict__ off, int s, long long n, long long& lo, long long& hi) {
    lo = off[s];
    hi = off[s + 1];
    lo = lo < 0 ? 0 : lo > n - 1 ? n - 1 : lo;
    hi = hi < lo ? lo : hi > n - 1 ? n - 1 : hi;
}

__global__ void __launch_bounds__(kBlock) k_forward(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ order,
                                                    const long long* __restrict__ off, long long n, int s, int q, int32_t* __restrict__ val,
                                                    int16_t* __restrict__ coef) {
    long long lo, hi;
    segment(off, s, n, lo, hi);
    for (long long t = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < hi; t += (long long)gridDim.x * blockDim.x) {
        const Node nd = node_of(keys, order, n, s, q, t, lo, hi);
        if (!nd.ok) continue;
        const long long w = nd.wl + nd.wr;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long left = val[3 * nd.p0 + ch], h = (long long)val[3 * nd.i + ch] - left;
            val[3 * nd.p0 + ch] = (int32_t)(left + floor_div(nd.wr * h, w));
            const long long mag = (2 * (h < 0 ? -h : h) + nd.step) / (2 * nd.step);
            coef[3 * nd.pos + ch] = (int16_t)(h < 0 ? -mag : mag);
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_inverse(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ order,
                                                    const long long* __restrict__ off, long long n, int s, int q, int32_t* __restrict__ val,
                                                    const int16_t* __restrict__ coef) {
    long long lo, hi;
    segment(off, s, n, lo, hi);
    for (long long t = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < hi; t += (long long)gridDim.x * blockDim.x) {
        const Node nd = node_of(keys, order, n, s, q, t, lo, hi);
        if (!nd.ok) continue;
        const long long w = nd.wl + nd.wr;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long h = (long long)coef[3 * nd.pos + ch] * nd.step;
            const long long left = (long long)val[3 * nd.p0 + ch] - floor_div(nd.wr * h, w);
            val[3 * nd.p0 + ch] = (int32_t)left;
            val[3 * nd.i + ch] = (int32_t)(left + h);
        }
    }
}

__global__ void k_get_dc(const int32_t* __restrict__ val, long long* __restrict__ hdr) {
    if (threadIdx.x < 3) hdr[kHdrDc + threadIdx.x] = val[threadIdx.x];
}

__global__ void k_set_dc(int32_t* __restrict__ val, int y, int co, int cg) {
    val[0] = y; val[1] = co; val[2] = cg;
}

__device__ __forceinline__ uint8_t clip8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ void __launch_bounds__(kBlock) k_colors(const int32_t* __restrict__ val, const unsigned* __restrict__ rows, long long n,
                                                   uint8_t* __restrict__ colors) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long r = rows[j];
    if (r >= n) return;
    const int y = val[3 * j], co = val[3 * j + 1], cg = val[3 * j + 2];
    const int t = y - (cg >> 1), G = cg + t, B = t - (co >> 1), R = B + co;
    colors[3 * r] = clip8(R); colors[3 * r + 1] = clip8(G); colors[3 * r + 2] = clip8(B);
}

// ---- workspace: the plan (keys, rows, order, off), the N x 3 values, and what the plan's two sorts need
struct Layout { size_t keys, rows, order, off, val, keys0, rows0, d0, d1, tmp, tmp_bytes, total; };

Layout layout(long long n) {
    Layout l;
    const size_t N = (size_t)n;
    size_t a = 0, b = 0, o = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, 0, 63, (hipStream_t)0);
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, b, (const uint8_t*)nullptr, (uint8_t*)nullptr, (const unsigned*)nullptr,
                                             (unsigned*)nullptr, (int)n, 0, 6, (hipStream_t)0);
    l.keys = o; o += al256(N * 8);
    l.rows = o; o += al256(N * 4);
    l.order = o; o += al256(N * 4);
    l.off = o; o += al256((kSteps + 1) * 8);
    l.val = o; o += al256(N * 12);
    l.keys0 = o; o += al256(N * 8);
    l.rows0 = o; o += al256(N * 4);          // row numbers, then the leaf indices before their sort
    l.d0 = o; o += al256(N);
    l.d1 = o; o += al256(N);
    l.tmp_bytes = a > b ? a : b;
    l.tmp = o; o += al256(l.tmp_bytes + 256);
    l.total = o;
    return l;
}

unsigned step_grid(const pcc_ctx* ctx, long long n) {
    const unsigned blocks = grid_for(n > 1 ? n - 1 : 1), cap = 8u * (unsigned)(ctx->num_cu > 0 ? ctx->num_cu : 256);
    return blocks < cap ? blocks : cap;
}

}  // namespace

PCC_API size_t pcc_color_anchor_workspace_bytes(int64_t npts) { return valid_count(npts) ? layout(npts).total : 0; }

PCC_API int pcc_color_anchor_plan(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t depth, int64_t* hdr, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && pts && hdr && workspace, "pcc_color_anchor_plan: NULL argument");
    PCC_REQUIRE(valid_count(npts), "pcc_color_anchor_plan: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(valid_depth(depth), "pcc_color_anchor_plan: depth = %d outside [1, 21]", depth);
    hipStream_t st = (hipStream_t)stream;
    const long long n = npts;
    const Layout l = layout(n);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *keys = (unsigned long long*)(w + l.keys), *keys0 = (unsigned long long*)(w + l.keys0);
    unsigned *rows = (unsigned*)(w + l.rows), *rows0 = (unsigned*)(w + l.rows0), *order = (unsigned*)(w + l.order);
    uint8_t *d0 = (uint8_t*)(w + l.d0), *d1 = (uint8_t*)(w + l.d1);
    long long *off = (long long*)(w + l.off), *H = (long long*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, 8 * PCC_COLOR_HDR_WORDS, st));
    PCC_CHECK_HIP(hipMemsetAsync(off, 0, (kSteps + 1) * 8, st));
    hipLaunchKernelGGL(k_keys, dim3(grid_for(n)), dim3(kBlock), 0, st, pts, n, 3 * (int)depth, keys0, rows0);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.tmp), bytes, (const unsigned long long*)keys0, keys, (const unsigned*)rows0, rows,
                                                     (int)n, 0, 3 * (int)depth, st));
    if (n > 1) {
        hipLaunchKernelGGL(k_d, dim3(grid_for(n - 1)), dim3(kBlock), 0, st, (const unsigned long long*)keys, n, d0, rows0, H);
        bytes = l.tmp_bytes;
        PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.tmp), bytes, (const uint8_t*)d0, d1, (const unsigned*)rows0, order, (int)(n - 1),
                                                         0, 6, st));
        hipLaunchKernelGGL(k_offsets, dim3(1), dim3(128), 0, st, (const uint8_t*)d1, n - 1, off, H);
    }
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_color_anchor_forward(pcc_ctx* ctx, const uint8_t* colors, int64_t npts, int32_t depth, int32_t qstep, int64_t* hdr, int16_t* coef,
                                     void* workspace, void* stream) {
    PCC_REQUIRE(ctx && colors && hdr && workspace && (coef || npts == 1), "pcc_color_anchor_forward: NULL argument");
    PCC_REQUIRE(valid_count(npts), "pcc_color_anchor_forward: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(valid_depth(depth), "pcc_color_anchor_forward: depth = %d outside [1, 21]", depth);
    PCC_REQUIRE(valid_q(qstep), "pcc_color_anchor_forward: qstep = %d outside [1, 255]", qstep);
    hipStream_t st = (hipStream_t)stream;
    const long long n = npts;
    const Layout l = layout(n);
    unsigned char* w = (unsigned char*)workspace;
    const unsigned long long* keys = (const unsigned long long*)(w + l.keys);
    const unsigned *rows = (const unsigned*)(w + l.rows), *order = (const unsigned*)(w + l.order);
    const long long* off = (const long long*)(w + l.off);
    int32_t* val = (int32_t*)(w + l.val);
    hipLaunchKernelGGL(k_leaves, dim3(grid_for(n)), dim3(kBlock), 0, st, colors, rows, n, val);
    if (n > 1) {
        PCC_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)(n - 1) * 6, st));
        const unsigned grid = step_grid(ctx, n);
        for (int s = 0; s < 3 * depth; ++s) hipLaunchKernelGGL(k_forward, dim3(grid), dim3(kBlock), 0, st, keys, order, off, n, s, (int)qstep, val, coef);
    }
    hipLaunchKernelGGL(k_get_dc, dim3(1), dim3(64), 0, st, (const int32_t*)val, (long long*)hdr);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_color_anchor_inverse(pcc_ctx* ctx, const int16_t* coef, const int32_t* dc, int64_t npts, int32_t depth, int32_t qstep,
                                     uint8_t* colors, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && dc && colors && workspace && (coef || npts == 1), "pcc_color_anchor_inverse: NULL argument");
    PCC_REQUIRE(valid_count(npts), "pcc_color_anchor_inverse: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(valid_depth(depth), "pcc_color_anchor_inverse: depth = %d outside [1, 21]", depth);
    PCC_REQUIRE(valid_q(qstep), "pcc_color_anchor_inverse: qstep = %d outside [1, 255]", qstep);
    PCC_REQUIRE(dc[0] >= 0 && dc[0] <= 255 && dc[1] >= -255 && dc[1] <= 255 && dc[2] >= -255 && dc[2] <= 255,
                "pcc_color_anchor_inverse: DC (%d, %d, %d) outside Y [0, 255], Co, Cg [-255, 255]", dc[0], dc[1], dc[2]);
    hipStream_t st = (hipStream_t)stream;
    const long long n = npts;
    const Layout l = layout(n);
    unsigned char* w = (unsigned char*)workspace;
    const unsigned long long* keys = (const unsigned long long*)(w + l.keys);
    const unsigned *rows = (const unsigned*)(w + l.rows), *order = (const unsigned*)(w + l.order);
    const long long* off = (const long long*)(w + l.off);
    int32_t* val = (int32_t*)(w + l.val);
    PCC_CHECK_HIP(hipMemsetAsync(val, 0, (size_t)n * 12, st));
    PCC_CHECK_HIP(hipMemsetAsync(colors, 0, (size_t)n * 3, st));
    hipLaunchKernelGGL(k_set_dc, dim3(1), dim3(1), 0, st, val, (int)dc[0], (int)dc[1], (int)dc[2]);
    if (n > 1) {
        const unsigned grid = step_grid(ctx, n);
        for (int s = 3 * depth - 1; s >= 0; --s)
            hipLaunchKernelGGL(k_inverse, dim3(grid), dim3(kBlock), 0, st, keys, order, off, n, s, (int)qstep, val, coef);
    }
    hipLaunchKernelGGL(k_colors, dim3(grid_for(n)), dim3(kBlock), 0, st, (const int32_t*)val, rows, n, colors);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
