// Variable rate from one checkpoint: the per-block latent step of the hyperprior models.
//   * the stepped twins of the fused quantise / index / pack kernels of elementwise.hip: block n works on y / step and sigma / step,
//     step = pcc_latent_step(q[n]); the quotient is a correctly rounded fp32 division, the dequantiser one fp32 multiply;
//   * the rate ladder: the exact size of every block's y string under every step of a ladder, as integer sums of a cost table.
// Everything is deterministic: the element-wise kernels have no reductions beyond the tile maxima, the ladder adds integers.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPackT = 64;      // the pack tile of elementwise.hip: the same tile_max entries

// step(q) = (8 + (q & 7)) * 2^((q >> 3) - 5), q in [0, 63], assembled from its bits: 8 + m = 1.m * 2^3, so the biased exponent is
// 127 + 3 + (q >> 3) - 5 and the three mantissa bits are q & 7.  0.25 ... 60, step(16) = 1.
__device__ __forceinline__ float step_of(int q) {
    q &= 63;
    return __builtin_bit_cast(float, (uint32_t)((125 + (q >> 3)) << 23) | (uint32_t)((q & 7) << 20));
}

// as scale_row of elementwise.hip: idx = (L-1) - #{j < L-1 : sigma <= table[j]}, by bisection when the table ascends
__device__ __forceinline__ int scale_row(float sg, const float* tab, int L, bool ascending) {
    if (!(sg >= tab[0])) sg = tab[0];
    if (ascending) {
        int lo = 0, n = L - 1;
        while (n > 0) {
            const int half = n >> 1;
            if (tab[lo + half] < sg) { lo += half + 1; n -= half + 1; } else n = half;
        }
        return lo;
    }
    int id = L - 1;
    for (int j = 0; j < L - 1; ++j) id -= (sg <= tab[j]) ? 1 : 0;
    return id;
}

// the scale table into LDS; returns whether it ascends (all threads of the workgroup call it)
__device__ __forceinline__ bool load_table(float* tab, const float* table, int L) {
    for (int j = threadIdx.x; j < L; j += kThreads) tab[j] = table[j];
    __syncthreads();
    int ok = 1;
    for (int j = threadIdx.x; j + 1 < L; j += kThreads) ok &= tab[j] <= tab[j + 1];
    return __syncthreads_and(ok) != 0;
}

__device__ __forceinline__ float quantize_step(float v, float step, float m, int mode) {
    const float t = __fdiv_rn(v, step);
    return mode == PCC_ROUND_FLOOR_HALF ? floorf(t + (0.5f - m)) : rintf(t - m);      // as k_quantize on t
}

// deq = float(sym) * step (+ medians[c]): two separately rounded operations, never one fused multiply-add
__device__ __forceinline__ float dequantize_step(int32_t sym, float step, float m) {
    return __fadd_rn(__fmul_rn((float)sym, step), m);
}

enum { SRC_QUANT = 1, SRC_INDEX = 2 };
struct StepSrc {
    const float* fsrc;        // SRC_QUANT: values; SRC_INDEX: sigma
    const float* med;         // SRC_QUANT: medians (C) or NULL
    int32_t* sym;             // int32 NDHWC output
    float* deq;               // SRC_QUANT: dequantised output (may be NULL)
    const float* table;       // SRC_INDEX: scale table
    const uint8_t* q;         // ladder index of every block
    int mode, L;
};

template <typename T, int SRC>
__global__ void __launch_bounds__(kThreads) k_step_pack(StepSrc ps, T* __restrict__ dst, int vox, int C, int vtiles, int ctiles,
                                                         int channels_first, int32_t* __restrict__ tile_max) {
    __shared__ int32_t tile[kPackT][kPackT + 1];
    __shared__ int32_t wmax[kThreads / 64];
    __shared__ float tab[SRC == SRC_INDEX ? 256 : 1];
    bool ascending = false;
    if constexpr (SRC == SRC_INDEX) ascending = load_table(tab, ps.table, ps.L);
    int t = blockIdx.x;
    const int ct = t % ctiles; t /= ctiles;
    const int vt = t % vtiles;
    const int n = t / vtiles;
    const int v0 = vt * kPackT, c0 = ct * kPackT;
    const int nv = min(kPackT, vox - v0), nc = min(kPackT, C - c0);
    const size_t g0 = ((size_t)n * vox + v0) * C + c0;        // NDHWC index of the tile's first element
    const float step = step_of(ps.q[n]);
    int32_t m = 0;
    for (int i = threadIdx.x; i < nv * kPackT; i += kThreads) {
        const int v = i / kPackT, c = i % kPackT;
        if (c < nc) {
            const size_t gi = g0 + (size_t)v * C + c;
            int32_t x;
            if constexpr (SRC == SRC_QUANT) {
                const float md = ps.med ? ps.med[c0 + c] : 0.f;
                x = (int32_t)quantize_step(ps.fsrc[gi], step, md, ps.mode);
                if (ps.deq) ps.deq[gi] = dequantize_step(x, step, md);
            } else {
                x = scale_row(__fdiv_rn(ps.fsrc[gi], step), tab, ps.L, ascending);
            }
            ps.sym[gi] = x;
            if (channels_first) tile[c][v] = x; else if (dst) dst[gi] = (T)x;
            m = max(m, abs(x));
        }
    }
    if (channels_first && dst) {                              // (dst NULL: no packed copy is wanted, uniform over the launch)
        __syncthreads();
        T* db = dst + ((size_t)n * C + c0) * vox + v0;
        for (int i = threadIdx.x; i < nc * kPackT; i += kThreads) {
            const int c = i / kPackT, v = i % kPackT;
            if (v < nv) db[(size_t)c * vox + v] = (T)tile[c][v];
        }
    }
    if (tile_max) {
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) tile_max[blockIdx.x] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) k_step_unpack(const T* __restrict__ src, int32_t* __restrict__ dst, int vox, int C, int vtiles,
                                                           int ctiles, int channels_first, const float* __restrict__ med,
                                                           float* __restrict__ deq, const uint8_t* __restrict__ q) {
    __shared__ int32_t tile[kPackT][kPackT + 1];
    int t = blockIdx.x;
    const int ct = t % ctiles; t /= ctiles;
    const int vt = t % vtiles;
    const int n = t / vtiles;
    const int v0 = vt * kPackT, c0 = ct * kPackT;
    const int nv = min(kPackT, vox - v0), nc = min(kPackT, C - c0);
    const size_t g0 = ((size_t)n * vox + v0) * C + c0;
    const float step = step_of(q[n]);
    if (channels_first) {
        const T* sb = src + ((size_t)n * C + c0) * vox + v0;
        for (int i = threadIdx.x; i < nc * kPackT; i += kThreads) {
            const int c = i / kPackT, v = i % kPackT;
            if (v < nv) tile[c][v] = (int32_t)sb[(size_t)c * vox + v];
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < nv * kPackT; i += kThreads) {
        const int v = i / kPackT, c = i % kPackT;
        if (c < nc) {
            const size_t gi = g0 + (size_t)v * C + c;
            const int32_t x = channels_first ? tile[c][v] : (int32_t)src[gi];
            dst[gi] = x;
            deq[gi] = dequantize_step(x, step, med ? med[c0 + c] : 0.f);
        }
    }
}

// ---- rate ladder -------------------------------------------------------------------------------------------------------------------
// One workgroup takes tiles of kRateE * 256 elements of one block; a tile's (y, sigma) pairs stay in registers while the J steps run
// over them.  The cost rows are read through L2 (a 64-row Gaussian table is some hundreds of KB, beyond the 160 KB of LDS; the bins
// near zero that almost every symbol takes stay cached); the scale table and the per-row offset and last bin live in LDS.  Per step the
// workgroup adds into an LDS slot, and once at its end into bits16 with one 64-bit atomic per step: integer sums, any order.
constexpr int kRateE = 8;
constexpr int kRateTile = kRateE * kThreads;
struct StepList { uint8_t q[64]; };

__global__ void __launch_bounds__(kThreads) k_rate_ladder(const float* __restrict__ y, const float* __restrict__ sigma,
                                                           const float* __restrict__ table, int L, int mode, StepList steps, int J,
                                                           const uint32_t* __restrict__ cost, int cost_stride,
                                                           const int32_t* __restrict__ offset, const int32_t* __restrict__ cdf_size, int ow,
                                                           long long per_block, int tiles, unsigned long long* __restrict__ bits16) {
    __shared__ float tab[256];
    __shared__ int32_t s_off[256], s_last[256];
    __shared__ unsigned long long s_acc[64];
    for (int j = threadIdx.x; j < L; j += kThreads) {
        s_off[j] = offset[j];
        s_last[j] = min(max(cdf_size[j] - 2, 0), cost_stride - 1);      // the escape bin m (bounded: nothing is read past a row)
    }
    if (threadIdx.x < 64) s_acc[threadIdx.x] = 0ull;
    const bool ascending = load_table(tab, table, L);                   // (its barriers also publish s_off / s_last / s_acc)
    const int n = blockIdx.y;
    const float* yb = y + (size_t)n * (size_t)per_block;
    const float* sb = sigma + (size_t)n * (size_t)per_block;
    const uint32_t omax = (1u << ow) - 1u;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        float yv[kRateE], sv[kRateE];
        bool ok[kRateE];
#pragma unroll
        for (int e = 0; e < kRateE; ++e) {
            const long long i = (long long)tile * kRateTile + e * kThreads + threadIdx.x;
            ok[e] = i < per_block;
            yv[e] = ok[e] ? yb[i] : 0.f;
            sv[e] = ok[e] ? sb[i] : 1.f;
        }
        for (int j = 0; j < J; ++j) {
            const float step = step_of(steps.q[j]);
            unsigned long long acc = 0ull;
#pragma unroll
            for (int e = 0; e < kRateE; ++e) {
                if (!ok[e]) continue;
                const int32_t sym = (int32_t)quantize_step(yv[e], step, 0.f, mode);
                const int row = scale_row(__fdiv_rn(sv[e], step), tab, L, ascending);
                const long long v = (long long)sym - s_off[row];
                const int m = s_last[row];
                const uint32_t* cr = cost + (size_t)row * cost_stride;
                if (v >= 0 && v < m) {
                    acc += cr[v];
                } else {                                                // the escape of encode_stream (range_coder.cpp)
                    const uint32_t overflow = v < 0 ? (uint32_t)(-2 * v - 1) : (uint32_t)(2 * (v - m));
                    int widths = 0;
                    while (widths * ow < 32 && (overflow >> (widths * ow)) != 0) ++widths;
                    acc += cr[m] + 65536ull * (unsigned)ow * (unsigned long long)(widths / (int)omax + 1 + widths);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if ((threadIdx.x & 63) == 0) atomicAdd(&s_acc[j], acc);
        }
    }
    __syncthreads();
    if (threadIdx.x < J && s_acc[threadIdx.x]) atomicAdd(&bits16[(size_t)n * J + threadIdx.x], s_acc[threadIdx.x]);
}

template <int SRC>
int launch_step_pack(pcc_ctx* ctx, const StepSrc& ps, int32_t N, int64_t vox, int32_t C, int32_t channels_first, void* dst, int32_t dst_bytes,
                     int32_t* tile_max, void* stream, const char* who) {
    PCC_REQUIRE(ctx && ps.q, "%s: NULL argument", who);
    PCC_REQUIRE(N > 0 && vox > 0 && vox < (1LL << 31) && C > 0, "%s: bad dimension", who);
    PCC_REQUIRE(dst_bytes == 1 || dst_bytes == 2 || dst_bytes == 4, "%s: dst_bytes must be 1, 2 or 4", who);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    const int vt = (int)((vox + kPackT - 1) / kPackT), ct = (C + kPackT - 1) / kPackT;
    const size_t tiles = (size_t)N * vt * ct;
    PCC_REQUIRE(tiles < (1ull << 31), "%s: too many tiles for one launch", who);
    hipStream_t st = (hipStream_t)stream;
    if (dst_bytes == 1)
        hipLaunchKernelGGL((k_step_pack<uint8_t, SRC>), dim3((unsigned)tiles), dim3(kThreads), 0, st, ps, (uint8_t*)dst, (int)vox, C, vt, ct, channels_first, tile_max);
    else if (dst_bytes == 2)
        hipLaunchKernelGGL((k_step_pack<int16_t, SRC>), dim3((unsigned)tiles), dim3(kThreads), 0, st, ps, (int16_t*)dst, (int)vox, C, vt, ct, channels_first, tile_max);
    else
        hipLaunchKernelGGL((k_step_pack<int32_t, SRC>), dim3((unsigned)tiles), dim3(kThreads), 0, st, ps, (int32_t*)dst, (int)vox, C, vt, ct, channels_first, tile_max);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

}  // namespace

PCC_API int pcc_quantize_step_pack(pcc_ctx* ctx, const float* v, const float* medians, int32_t* sym, float* deq, int32_t N, int64_t vox,
                                   int32_t C, int32_t mode, int32_t channels_first, void* dst, int32_t dst_bytes, int32_t* tile_max,
                                   const uint8_t* q, void* stream) {
    PCC_REQUIRE(v && sym && (mode == PCC_ROUND_FLOOR_HALF || mode == PCC_ROUND_HALF_EVEN), "pcc_quantize_step_pack: bad argument");
    StepSrc ps = {};
    ps.fsrc = v; ps.med = medians; ps.sym = sym; ps.deq = deq; ps.mode = mode; ps.q = q;
    return launch_step_pack<SRC_QUANT>(ctx, ps, N, vox, C, channels_first, dst, dst_bytes, tile_max, stream, "pcc_quantize_step_pack");
}

PCC_API int pcc_index_pack_step(pcc_ctx* ctx, const float* sigma, const float* table, int32_t L, int32_t* idx, int32_t N, int64_t vox,
                                int32_t C, int32_t channels_first, void* dst, int32_t dst_bytes, const uint8_t* q, void* stream) {
    PCC_REQUIRE(sigma && table && idx && L >= 1 && L <= 256, "pcc_index_pack_step: bad argument");
    StepSrc ps = {};
    ps.fsrc = sigma; ps.table = table; ps.L = L; ps.sym = idx; ps.q = q;
    return launch_step_pack<SRC_INDEX>(ctx, ps, N, vox, C, channels_first, dst, dst_bytes, nullptr, stream, "pcc_index_pack_step");
}

PCC_API int pcc_unpack_dequantize_step(pcc_ctx* ctx, const void* src, int32_t src_bytes, int32_t N, int64_t vox, int32_t C,
                                       int32_t channels_first, int32_t* sym, const float* medians, float* deq, const uint8_t* q,
                                       void* stream) {
    PCC_REQUIRE(ctx && src && sym && deq && q, "pcc_unpack_dequantize_step: NULL argument");
    PCC_REQUIRE(N > 0 && vox > 0 && vox < (1LL << 31) && C > 0, "pcc_unpack_dequantize_step: bad dimension");
    PCC_REQUIRE(src_bytes == 1 || src_bytes == 2 || src_bytes == 4, "pcc_unpack_dequantize_step: src_bytes must be 1, 2 or 4");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    const int vt = (int)((vox + kPackT - 1) / kPackT), ct = (C + kPackT - 1) / kPackT;
    const size_t tiles = (size_t)N * vt * ct;
    PCC_REQUIRE(tiles < (1ull << 31), "pcc_unpack_dequantize_step: too many tiles for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (src_bytes == 1)
        hipLaunchKernelGGL(k_step_unpack<uint8_t>, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const uint8_t*)src, sym, (int)vox, C, vt, ct, channels_first, medians, deq, q);
    else if (src_bytes == 2)
        hipLaunchKernelGGL(k_step_unpack<int16_t>, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const int16_t*)src, sym, (int)vox, C, vt, ct, channels_first, medians, deq, q);
    else
        hipLaunchKernelGGL(k_step_unpack<int32_t>, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const int32_t*)src, sym, (int)vox, C, vt, ct, channels_first, medians, deq, q);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_rate_ladder(pcc_ctx* ctx, const float* y, const float* sigma, int32_t N, int64_t vox, int32_t C, const float* table,
                            int32_t L, int32_t mode, const uint8_t* steps, int32_t J, const uint32_t* cost16, int32_t cost_stride,
                            const int32_t* offset, const int32_t* cdf_size, int32_t overflow_width, int32_t groups_per_block,
                            int64_t* bits16, void* stream) {
    PCC_REQUIRE(ctx && y && sigma && table && steps && cost16 && offset && cdf_size && bits16, "pcc_rate_ladder: NULL argument");
    PCC_REQUIRE(N > 0 && N <= 65535 && vox > 0 && C > 0 && vox < (1LL << 31) / C, "pcc_rate_ladder: bad dimension (at most 65535 blocks of fewer than 2^31 elements)");
    PCC_REQUIRE(L >= 1 && L <= 256 && cost_stride >= 2, "pcc_rate_ladder: a scale table of 1 to 256 entries, one cost row of at least 2 bins for each");
    PCC_REQUIRE(mode == PCC_ROUND_FLOOR_HALF || mode == PCC_ROUND_HALF_EVEN, "pcc_rate_ladder: bad round mode");
    PCC_REQUIRE(J >= 1 && J <= 64, "pcc_rate_ladder: a ladder of 1 to 64 steps, not %d", J);
    PCC_REQUIRE(overflow_width >= 1 && overflow_width <= 8, "pcc_rate_ladder: overflow_width %d not in [1, 8]", overflow_width);
    PCC_REQUIRE(groups_per_block >= 0, "pcc_rate_ladder: groups_per_block < 0");
    StepList sl = {};
    for (int j = 0; j < J; ++j) {
        PCC_REQUIRE(steps[j] <= 63, "pcc_rate_ladder: steps[%d] = %d is beyond the ladder (0 to 63)", j, (int)steps[j]);
        sl.q[j] = steps[j];
    }
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const long long per_block = (long long)vox * C;
    const int tiles = (int)((per_block + kRateTile - 1) / kRateTile);
    int groups = groups_per_block > 0 ? groups_per_block : tiles;      // the sums do not depend on it
    if (groups > tiles) groups = tiles;
    PCC_CHECK_HIP(hipMemsetAsync(bits16, 0, (size_t)N * J * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_rate_ladder, dim3((unsigned)groups, (unsigned)N), dim3(kThreads), 0, st, y, sigma, table, L, mode, sl, J, cost16,
                       cost_stride, offset, cdf_size, overflow_width, per_block, tiles, reinterpret_cast<unsigned long long*>(bits16));
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
