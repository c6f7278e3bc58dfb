// Count-matched thresholding of libpcc_geo_hip.so: the k voxels of a block with the highest occupancy score, in voxel order
// (include/pcc_geo.h "top-k selection").
//
// The rule works on a 31-bit key per voxel: 0 unless x > 0 (NaN, -0, +0, negatives), else the raw bits of x -- positive floats order like
// their bits.  With P = #{key > 0} and k_eff = clamp(k, 0, P), the selection is the k_eff first voxels by (key descending, index
// ascending): every voxel above the k_eff-th largest key T, and the first r = k_eff - #{key > T} voxels with key == T.
//
// A block of n voxels is cut into segments of kSeg voxels, one workgroup each, so a chunk of 32 blocks of 64^3 is 2048 workgroups.
// Everything the workgroups of a block share lives in the workspace and is an integer:
//   hist<0..2> + select<0..2>  radix select of T over the digits 11 | 10 | 10 bits, most significant first: a segment histograms the digit
//                              of its keys that carry the digits chosen so far in LDS and adds the used bins to the block's histogram
//                              (integer atomics: the sums do not depend on the order); one workgroup per block then walks the bins from the
//                              top.  A segment without a key that takes part -- the zero bulk behind the ReLU -- costs one compare per
//                              voxel and touches neither LDS nor the workspace.
//   count                      per segment #{key > T} and #{key == T} (ballot + popcount)
//   segscan                    per block the exclusive prefixes of both over the segments -> first output row and first tie rank of
//                              every segment; counts[b] = k_eff
//   write                      a wave owns 1024 consecutive voxels of its segment: rank among the equal keys and output row by ballot and
//                              prefix popcount behind the prefixes of the waves and segments before it
// A store goes to xyz + b * cap * 3 + 3 * j under the test j < min(k_eff, cap), whatever the scores and k hold.
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSeg = 4096, kPer = kSeg / kThreads;      // voxels per workgroup / per thread
constexpr int kPasses = 3, kBins = 2048;                // digits of the key, bins of the widest one
constexpr int64_t kMaxVoxels = 1LL << 28;
constexpr uint32_t kNoKey = 0xffffffffu;                // T of a block that selects nothing: above every key

__host__ __device__ constexpr int shift_of(int pass) { return pass == 0 ? 20 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int bits_of(int pass) { return pass == 0 ? 11 : 10; }

struct BlockState {
    uint32_t T;            // the k_eff-th largest key (kNoKey: k_eff = 0)
    int32_t r;             // voxels with key == T to take, lowest index first
    int32_t k_eff, P;
    uint32_t prefix;       // the digits of T chosen so far
    int32_t k_rem;         // rank of T among the keys that carry them
    int32_t pad[2];
};

struct Layout {
    uint32_t* hist;        // [B][kPasses][kBins]
    BlockState* state;     // [B]
    int32_t* seg;          // [B][2][G]: count -> #{key > T}, #{key == T}; segscan -> first output row, first tie rank
    size_t hist_bytes;
};

inline int segments_of(int64_t n) { return (int)((n + kSeg - 1) / kSeg); }

inline size_t hist_bytes_of(int32_t B) { return (size_t)B * kPasses * kBins * sizeof(uint32_t); }
inline size_t seg_offset_of(int32_t B) { return hist_bytes_of(B) + (size_t)B * sizeof(BlockState); }
inline size_t workspace_bytes_of(int32_t B, int64_t n) {
    return seg_offset_of(B) + ((size_t)B * 2 * (size_t)segments_of(n) * sizeof(int32_t) + 15) / 16 * 16;
}

inline Layout layout_of(char* ws, int32_t B, int64_t n) {
    Layout l;
    l.hist_bytes = hist_bytes_of(B);
    l.hist = (uint32_t*)ws;
    l.state = (BlockState*)(ws + l.hist_bytes);
    l.seg = (int32_t*)(ws + seg_offset_of(B));
    return l;
}

__device__ __forceinline__ uint32_t key_of(float v) { return v > 0.0f ? __float_as_uint(v) : 0u; }

__device__ __forceinline__ int count_of(bool p) { return __popcll(__ballot(p)); }

// the keys of segment g, wave w of the workgroup on the 64 * kPer consecutive voxels w of it; a voxel past n has key 0
__device__ __forceinline__ void load_keys(const float* __restrict__ xb, int g, int n, uint32_t (&key)[kPer]) {
    const int base = g * kSeg + ((int)threadIdx.x >> 6) * (64 * kPer) + ((int)threadIdx.x & 63);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = base + j * 64;
        key[j] = i < n ? key_of(xb[i]) : 0u;
    }
}

// exclusive prefix of v over the workgroup in thread order, *total = the sum; lds: kWaves ints, reusable after the call
__device__ __forceinline__ int block_excl_scan(int v, int* total, int* lds) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const int c = lds[i];
        base += i < w ? c : 0;
        tot += c;
    }
    *total = tot;
    return base + incl - v;
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void topk_hist_kernel(const float* __restrict__ x, int64_t x_stride, int n, uint32_t* __restrict__ hist,
                                                             const BlockState* __restrict__ state) {
    __shared__ uint32_t h[kBins];
    const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
    constexpr int bins = 1 << bits_of(PASS), shift = shift_of(PASS);
    uint32_t prefix = 0;
    if (PASS > 0) {
        if (state[b].k_eff == 0) return;
        prefix = state[b].prefix;
    }
    uint32_t key[kPer];
    load_keys(x + (int64_t)b * x_stride, g, n, key);
    bool any = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        // (key > 0 also under a zero prefix: the zero bulk never takes part)
        if (!(key[j] != 0u && (PASS == 0 || (key[j] >> (shift + bits_of(PASS))) == prefix))) key[j] = 0u;
        any |= key[j] != 0u;
    }
    if (!__syncthreads_or(any)) return;
    for (int t = tid; t < bins; t += kThreads) h[t] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        if (key[j] != 0u) atomicAdd(&h[(key[j] >> shift) & (bins - 1)], 1u);
    __syncthreads();
    uint32_t* hb = hist + ((size_t)b * kPasses + PASS) * kBins;
    for (int t = tid; t < bins; t += kThreads)
        if (h[t]) atomicAdd(&hb[t], h[t]);
}

// one workgroup per block: the digit of T in histogram PASS, walking the bins from the top
template <int PASS>
__global__ __launch_bounds__(kThreads) void topk_select_kernel(const uint32_t* __restrict__ hist, const int32_t* __restrict__ k, BlockState* __restrict__ state) {
    __shared__ int lds[kWaves];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    constexpr int bins = 1 << bits_of(PASS), per = bins / kThreads;
    const uint32_t* hb = hist + ((size_t)b * kPasses + PASS) * kBins;
    BlockState s = {};
    if (PASS > 0) {
        s = state[b];
        if (s.k_eff == 0) return;
    }
    int c[per], sum = 0;
#pragma unroll
    for (int e = 0; e < per; ++e) {
        c[e] = (int)hb[bins - 1 - (tid * per + e)];
        sum += c[e];
    }
    int total;
    int run = block_excl_scan(sum, &total, lds);
    if (PASS == 0) {
        const int want = k[b];
        s.P = total;
        s.k_eff = want < 0 ? 0 : want > total ? total : want;
        s.k_rem = s.k_eff;
        if (s.k_eff == 0) {
            if (tid == 0) {
                s.T = kNoKey;
                state[b] = s;
            }
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < per; ++e) {
        if (run < s.k_rem && s.k_rem <= run + c[e]) {          // exactly one bin of one thread: 1 <= k_rem <= total
            s.prefix = (s.prefix << bits_of(PASS)) | (uint32_t)(bins - 1 - (tid * per + e));
            s.k_rem -= run;
            s.T = PASS == kPasses - 1 ? s.prefix : kNoKey;
            s.r = s.k_rem;
            state[b] = s;
            break;
        }
        run += c[e];
    }
}

__global__ __launch_bounds__(kThreads) void topk_count_kernel(const float* __restrict__ x, int64_t x_stride, int n, int G,
                                                              const BlockState* __restrict__ state, int32_t* __restrict__ seg) {
    __shared__ int wgt[kWaves], weq[kWaves];
    const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x;
    int32_t* sb = seg + (size_t)b * 2 * G;
    if (state[b].k_eff == 0) {
        if (tid == 0) sb[g] = sb[G + g] = 0;
        return;
    }
    const uint32_t T = state[b].T;
    uint32_t key[kPer];
    load_keys(x + (int64_t)b * x_stride, g, n, key);
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        gt += count_of(key[j] > T);
        eq += count_of(key[j] == T);
    }
    if ((tid & 63) == 0) { wgt[tid >> 6] = gt; weq[tid >> 6] = eq; }
    __syncthreads();
    if (tid == 0) {
        gt = eq = 0;
        for (int w = 0; w < kWaves; ++w) { gt += wgt[w]; eq += weq[w]; }
        sb[g] = gt;
        sb[G + g] = eq;
    }
}

// one workgroup per block: (#{key > T}, #{key == T}) per segment -> (first output row, first tie rank) per segment
__global__ __launch_bounds__(kThreads) void topk_segscan_kernel(int G, const BlockState* __restrict__ state, int32_t* __restrict__ seg,
                                                                int32_t* __restrict__ counts) {
    __shared__ int lds[kWaves];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int r = state[b].r, k_eff = state[b].k_eff;
    if (tid == 0) counts[b] = k_eff;
    if (k_eff == 0) return;
    int32_t* sb = seg + (size_t)b * 2 * G;
    int out_carry = 0, eq_carry = 0;
    for (int g0 = 0; g0 < G; g0 += kThreads) {
        const int g = g0 + tid;
        const int gt = g < G ? sb[g] : 0, eq = g < G ? sb[G + g] : 0;
        int eq_total, out_total;
        const int eq_off = eq_carry + block_excl_scan(eq, &eq_total, lds);
        const int left = r - eq_off;
        const int take = left < 0 ? 0 : left > eq ? eq : left;
        const int out_off = out_carry + block_excl_scan(gt + take, &out_total, lds);
        if (g < G) {
            sb[g] = out_off;
            sb[G + g] = eq_off;
        }
        out_carry += out_total;
        eq_carry += eq_total;
    }
}

__global__ __launch_bounds__(kThreads) void topk_write_kernel(const float* __restrict__ x, int64_t x_stride, int n, int G, int H, int W,
                                                              const BlockState* __restrict__ state, const int32_t* __restrict__ seg,
                                                              float* __restrict__ xyz, int64_t cap) {
    __shared__ int wgt[kWaves], weq[kWaves];
    const int b = (int)blockIdx.y, g = (int)blockIdx.x, tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int k_eff = state[b].k_eff;
    if (k_eff == 0) return;
    const uint32_t T = state[b].T;
    const int r = state[b].r;
    const int lim = (int64_t)k_eff < cap ? k_eff : (int)cap;       // rows of this block that exist
    int pos = seg[(size_t)b * 2 * G + g], eq_before = seg[(size_t)b * 2 * G + G + g];
    if (pos >= lim) return;
    uint32_t key[kPer];
    load_keys(x + (int64_t)b * x_stride, g, n, key);
    int gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        gt += count_of(key[j] > T);
        eq += count_of(key[j] == T);
    }
    if (lane == 0) { wgt[w] = gt; weq[w] = eq; }
    __syncthreads();
    for (int v = 0; v < w; ++v) {                                   // the waves of this segment before this one
        const int e = weq[v], left = r - eq_before;
        pos += wgt[v] + (left < 0 ? 0 : left > e ? e : left);
        eq_before += e;
    }
    float* ob = xyz + (size_t)b * (size_t)cap * 3;
    const uint64_t below = (1ull << lane) - 1;
    const int HW = H * W;
    const int base = g * kSeg + w * (64 * kPer) + lane;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const bool is_eq = key[j] == T;
        const uint64_t m_eq = __ballot(is_eq);
        const bool sel = key[j] > T || (is_eq && eq_before + __popcll(m_eq & below) < r);
        const uint64_t m_sel = __ballot(sel);
        const int p = pos + __popcll(m_sel & below);
        if (sel && p < lim) {
            const int i = base + j * 64, d = i / HW, rem = i - d * HW;
            ob[(size_t)p * 3 + 0] = (float)d;
            ob[(size_t)p * 3 + 1] = (float)(rem / W);
            ob[(size_t)p * 3 + 2] = (float)(rem % W);
        }
        pos += __popcll(m_sel);
        eq_before += __popcll(m_eq);
    }
}

}  // namespace

PCC_API size_t pcc_topk_workspace_bytes(int32_t B, int64_t n) {
    return B <= 0 || n < 0 || n > kMaxVoxels ? 0 : workspace_bytes_of(B, n);
}

PCC_API int pcc_topk_compact(pcc_ctx* ctx, const float* x, int64_t x_stride, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* k,
                             float* xyz, int32_t* counts, int64_t cap, void* workspace, size_t workspace_bytes, void* stream) {
    PCC_REQUIRE(ctx, "pcc_topk_compact: NULL context");
    PCC_REQUIRE(B >= 0 && B <= 65535 && D >= 0 && H >= 0 && W >= 0 && cap >= 0, "pcc_topk_compact: bad dimension");
    int64_t n = (int64_t)D * H;                          // (no overflow: two 31-bit factors at a time)
    n = W == 0 ? 0 : n > kMaxVoxels ? n : n * W;
    PCC_REQUIRE(n <= kMaxVoxels, "pcc_topk_compact: %lld voxels per block (at most 2^28)", (long long)n);
    if (B == 0) return PCC_OK;
    PCC_REQUIRE(counts && k, "pcc_topk_compact: NULL pointer");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        PCC_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * sizeof(int32_t), st));
        return PCC_OK;
    }
    PCC_REQUIRE(x && workspace && (xyz || cap == 0), "pcc_topk_compact: NULL pointer");
    PCC_REQUIRE(B == 1 || x_stride >= n, "pcc_topk_compact: stride %lld below n = %lld", (long long)x_stride, (long long)n);
    PCC_REQUIRE(workspace_bytes >= workspace_bytes_of(B, n), "pcc_topk_compact: workspace %zu < pcc_topk_workspace_bytes (%zu)", workspace_bytes,
                workspace_bytes_of(B, n));
    const Layout l = layout_of((char*)workspace, B, n);
    const int G = segments_of(n);
    const dim3 grid((unsigned)G, (unsigned)B), blocks((unsigned)B), threads(kThreads);
    PCC_CHECK_HIP(hipMemsetAsync(l.hist, 0, l.hist_bytes, st));
    hipLaunchKernelGGL(topk_hist_kernel<0>, grid, threads, 0, st, x, x_stride, (int)n, l.hist, l.state);
    hipLaunchKernelGGL(topk_select_kernel<0>, blocks, threads, 0, st, l.hist, k, l.state);
    hipLaunchKernelGGL(topk_hist_kernel<1>, grid, threads, 0, st, x, x_stride, (int)n, l.hist, l.state);
    hipLaunchKernelGGL(topk_select_kernel<1>, blocks, threads, 0, st, l.hist, k, l.state);
    hipLaunchKernelGGL(topk_hist_kernel<2>, grid, threads, 0, st, x, x_stride, (int)n, l.hist, l.state);
    hipLaunchKernelGGL(topk_select_kernel<2>, blocks, threads, 0, st, l.hist, k, l.state);
    hipLaunchKernelGGL(topk_count_kernel, grid, threads, 0, st, x, x_stride, (int)n, G, l.state, l.seg);
    hipLaunchKernelGGL(topk_segscan_kernel, blocks, threads, 0, st, G, l.state, l.seg, counts);
    hipLaunchKernelGGL(topk_write_kernel, grid, threads, 0, st, x, x_stride, (int)n, G, H, W, l.state, l.seg, xyz, cap);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
