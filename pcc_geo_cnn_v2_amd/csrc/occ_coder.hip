// Lossless occupancy layer of libpcc_geo_hip.so: the "occ1" string format (include/pcc_geo.h "occupancy coder (DEVICE)").
//
// One string codes the true occupancy of a block given the decoder's x_hat: every voxel falls into one of K = 32 buckets of x_hat, a
// bucket's share of occupied voxels is sent as a 16-bit probability, and the voxels of the buckets that hold an occupied voxel are coded
// with rans1's interleaved rANS (rans_common.h), without escapes.  One workgroup of 16 waves codes one block; a launch codes a chunk.
//
//   encoder  histogram (all waves; wave w owns the contiguous voxel segment w): tot / on per bucket -> the entries, m, the cost -> L
//            pass 1 (all waves): the coded voxels compacted in voxel order into the workspace as (start << 16 | freq); a wave's first
//            slot is the number of coded voxels of the segments before it, known from the per-wave histograms
//            pass 2 (wave 0, steps descending): the rANS recurrence, the next step's workspace load in flight
//            pass 3 (all waves): lane byte, entries, states, words, and the length
//   decoder  histogram of tot; lane byte and length against the entries; compaction of (voxel index, f) into the workspace; the
//            recurrence on wave 0, steps ascending; the grid is zeroed first and the occupied voxels are stored as 1.0f
//
// Every store is a plain C++ store of a vector lane.  A store of the decoder goes to out[i] with i < n by construction, whatever the
// string says; every read of the string is made under the length test of occ_header.h.
#include "common.h"
#include "occ_header.h"
#include "rans_common.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, K = kOccBuckets;
constexpr uint32_t kTotal = 1u << 16;

__device__ __forceinline__ int bucket_of(float x) {
    if (!(x > 0.0f)) return 0;                       // NaN, -0 and negatives
    if (x >= 1.0f) return K - 1;
    const int b = 1 + (int)(x * 30.0f);              // one fp32 multiply, then truncation
    return b > K - 2 ? K - 2 : b;                    // ((1 - 2^-24) * 30 rounds to 30)
}

struct Shared {
    uint32_t wtot[kWaves][K], won[kWaves][K];        // per wave segment
    uint32_t tot[K], on[K], f[K];                    // f: the entry of a used bucket, 0 for an empty or skipped one
    uint32_t wcoded[kWaves];                         // coded voxels per wave segment
    int32_t wcount;                                  // words of the encoder's pass 2
};

struct Segment { int32_t lo, hi; };
// the voxels of wave w: contiguous, a multiple of 64 long, so that every step of a wave's loop is one coalesced row
__device__ __forceinline__ Segment segment_of(int32_t n, int w) {
    const int32_t seg = (n + kThreads - 1) / kThreads * 64;
    const int64_t lo = (int64_t)w * seg;
    const int32_t l = lo < n ? (int32_t)lo : n;
    return Segment{l, n - l < seg ? n : l + seg};
}

// tot (and, with occ, on) per bucket into sh.tot / sh.on, per wave segment into sh.wtot / sh.won.  Bucket 0 -- after the ReLU the bulk of
// a block -- is counted in registers; the others with LDS atomics on the wave's own row.
__device__ __forceinline__ void histogram(Shared& sh, const float* __restrict__ x, const float* __restrict__ occ, int32_t n) {
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = lane_id();
    for (int j = tid; j < kWaves * K; j += kThreads) { (&sh.wtot[0][0])[j] = 0; (&sh.won[0][0])[j] = 0; }
    __syncthreads();
    const Segment sg = segment_of(n, w);
    int64_t c0 = 0, o0 = 0;
    for (int32_t i = sg.lo + lane; i < sg.hi; i += 64) {
        const int b = bucket_of(x[i]);
        const bool o = occ && occ[i] != 0.0f;
        if (b == 0) {
            ++c0;
            o0 += o ? 1 : 0;
        } else {
            atomicAdd(&sh.wtot[w][b], 1u);
            if (o) atomicAdd(&sh.won[w][b], 1u);
        }
    }
    c0 = wave_sum(c0);
    o0 = wave_sum(o0);
    if (lane == 0) { sh.wtot[w][0] = (uint32_t)c0; sh.won[w][0] = (uint32_t)o0; }
    __syncthreads();
    if (tid < K) {
        uint32_t t = 0, o = 0;
        for (int v = 0; v < kWaves; ++v) { t += sh.wtot[v][tid]; o += sh.won[v][tid]; }
        sh.tot[tid] = t;
        sh.on[tid] = o;
    }
    __syncthreads();
}

// with sh.f final: the coded voxels of every wave segment -> sh.wcoded; returns the first slot of this thread's wave
__device__ __forceinline__ uint32_t wave_base(Shared& sh) {
    const int tid = (int)threadIdx.x, w = tid >> 6;
    if (tid < kWaves) {
        uint32_t c = 0;
        for (int b = 0; b < K; ++b) c += sh.f[b] ? sh.wtot[tid][b] : 0u;
        sh.wcoded[tid] = c;
    }
    __syncthreads();
    uint32_t base = 0;
    for (int v = 0; v < w; ++v) base += sh.wcoded[v];
    return base;
}

inline size_t ws_stride_of(int64_t n) { return ((size_t)n * 6 + 15) / 16 * 16; }

__global__ __launch_bounds__(kThreads) void occ_encode_kernel(const float* __restrict__ x_hat, int64_t x_stride, const float* __restrict__ occ,
                                                              int64_t occ_stride, int32_t n, int32_t forced, uint8_t* __restrict__ out, int64_t cap,
                                                              int32_t* __restrict__ out_len, int32_t* __restrict__ status, uint8_t* __restrict__ ws,
                                                              int64_t ws_stride) {
    __shared__ Shared sh;
    const int s = (int)blockIdx.x, tid = (int)threadIdx.x, w = tid >> 6, lane = lane_id();
    if (n <= 0 || n > kOccMaxVoxels) {
        if (tid == 0) { out_len[s] = 0; status[s] = n == 0 ? 0 : kBadShape; }
        return;
    }
    x_hat += (int64_t)s * x_stride;
    occ += (int64_t)s * occ_stride;
    uint32_t* bins = (uint32_t*)(ws + (int64_t)s * ws_stride);          // n packed bins, then n words
    uint16_t* words = (uint16_t*)(bins + n);
    uint8_t* o = out + (int64_t)s * cap;

    histogram(sh, x_hat, occ, n);
    if (tid < K) {
        const int64_t t = sh.tot[tid], on = sh.on[tid];
        int64_t f = 0;
        if (on > 0) {
            f = (on * 65536 + t / 2) / t;
            f = f < 1 ? 1 : f > 65535 ? 65535 : f;
        }
        sh.f[tid] = (uint32_t)f;
    }
    __syncthreads();
    // (every thread, from LDS broadcasts) the entries in front of the states, the coded voxels and their integer cost -> L
    int used = 0;
    int64_t m = 0, cost = 0;
    for (int b = 0; b < K; ++b) {
        const uint32_t t = sh.tot[b], f = sh.f[b];
        used += t ? 1 : 0;
        if (f) {
            m += t;
            cost += (int64_t)sh.on[b] * cost256(f) + (int64_t)(t - sh.on[b]) * cost256(kTotal - f);
        }
    }
    const int L = forced ? forced : lane_rule((cost + 2047) >> 11);

    // pass 1
    {
        uint32_t pos = wave_base(sh);
        const Segment sg = segment_of(n, w);
        for (int32_t i0 = sg.lo; i0 < sg.hi; i0 += 64) {
            const int32_t i = i0 + lane;
            bool coded = false;
            uint32_t sf = 0;
            if (i < sg.hi) {
                const uint32_t f = sh.f[bucket_of(x_hat[i])];
                if (f) {
                    coded = true;
                    sf = occ[i] != 0.0f ? (((kTotal - f) << 16) | f) : (kTotal - f);
                }
            }
            const uint64_t mask = __ballot(coded);
            if (coded) bins[pos + prefix_rank(mask)] = sf;
            pos += (uint32_t)__popcll(mask);
        }
    }
    __syncthreads();

    // pass 2 (wave 0): steps descending; the words of step t lie before those of step t + 1, ascending lane order inside a step
    uint32_t x = kLow;
    if (w == 0) {
        const int32_t steps = (int32_t)((m + L - 1) / L);
        int32_t wcount = 0;                                              // words so far; they occupy words[n - wcount, n)
        uint32_t next = 1u;
        if (steps > 0 && lane < L && (int64_t)(steps - 1) * L + lane < m) next = bins[(int64_t)(steps - 1) * L + lane];
        for (int32_t tstep = steps - 1; tstep >= 0; --tstep) {
            const bool active = lane < L && (int64_t)tstep * L + lane < m;
            const uint32_t sf = next;
            if (tstep > 0 && lane < L) next = bins[(int64_t)(tstep - 1) * L + lane];      // (does not depend on the state: in flight during the update)
            const uint32_t f = sf & 0xffffu, start = sf >> 16;
            const bool emit = active && x >= (f << 16);
            const uint64_t mask = __ballot(emit);
            const int k = __popcll(mask);
            if (emit) {
                words[n - wcount - k + prefix_rank(mask)] = (uint16_t)x;
                x >>= 16;
            }
            wcount += k;
            if (active) x = ((x / f) << 16) + (x % f) + start;
        }
        if (lane == 0) sh.wcount = wcount;
    }
    __syncthreads();

    // pass 3
    const int32_t wcount = sh.wcount;
    if (tid == 0) o[0] = (uint8_t)(31 - __clz(L));
    if (tid < K && sh.tot[tid]) {
        int slot = 0;
        for (int b = 0; b < tid; ++b) slot += sh.tot[b] ? 1 : 0;
        put16(o + 1 + 2 * slot, sh.f[tid]);
    }
    uint8_t* os = o + 1 + 2 * used;
    if (w == 0 && lane < L) put32(os + 4 * lane, x);
    uint8_t* ow = os + 4 * L;
    for (int32_t j = tid; j < wcount; j += kThreads) put16(ow + 2 * (int64_t)j, words[n - wcount + j]);
    if (tid == 0) {
        out_len[s] = (int32_t)(1 + 2 * used + 4 * L + 2 * (int64_t)wcount);
        status[s] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void occ_decode_kernel(const float* __restrict__ x_hat, int64_t x_stride, int32_t n,
                                                              const uint8_t* __restrict__ str, int64_t str_bytes, const int64_t* __restrict__ off_arr,
                                                              const int32_t* __restrict__ len_arr, float* __restrict__ out, int64_t out_stride,
                                                              int32_t* __restrict__ status, uint8_t* __restrict__ ws, int64_t ws_stride) {
    __shared__ Shared sh;
    const int s = (int)blockIdx.x, tid = (int)threadIdx.x, w = tid >> 6, lane = lane_id();
    int32_t flags = 0;
    if (n < 0 || n > kOccMaxVoxels) { flags = kBadShape; n = 0; }
    const int64_t off = off_arr[s];
    int64_t len = len_arr[s];
    if (off < 0 || len < 0 || off > str_bytes || len > str_bytes - off) { flags |= kCorrupt; len = 0; }      // the string inside the buffer
    if (n == 0) {
        if (len_arr[s] != 0 && flags == 0) flags = kCorrupt;             // bytes for an empty block
        if (tid == 0) status[s] = flags;
        return;
    }
    const uint8_t* sp = str + off;
    x_hat += (int64_t)s * x_stride;
    out += (int64_t)s * out_stride;
    for (int32_t i = tid; i < n; i += kThreads) out[i] = 0.0f;
    histogram(sh, x_hat, nullptr, n);

    // the header against the length (all threads take the same way: everything below is uniform over the workgroup)
    int32_t L = 1;
    int64_t n_words = 0;
    int used = 0;
    for (int b = 0; b < K; ++b) used += sh.tot[b] ? 1 : 0;
    bool ok = flags == 0 && occ_parse_lanes([&](int64_t q) { return (uint32_t)sp[q]; }, len, n, L) && occ_split(len, L, used, n_words);
    // from here on (ok): 1 + 2 used + 4 L + 2 n_words == len, so entries, states and words [0, n_words) lie inside the string
    if (tid < K) {
        int slot = 0;
        for (int b = 0; b < tid; ++b) slot += sh.tot[b] ? 1 : 0;
        sh.f[tid] = ok && sh.tot[tid] ? get16(sp + 1 + 2 * slot) : 0u;
    }
    __syncthreads();
    int64_t m = 0;
    for (int b = 0; b < K; ++b) m += sh.f[b] ? sh.tot[b] : 0u;
    if (!ok || n_words > m) {
        if (tid == 0) status[s] = flags | kCorrupt;
        return;
    }

    // the coded voxels in voxel order: index and probability
    uint32_t* idx = (uint32_t*)(ws + (int64_t)s * ws_stride);           // n indexes, then n probabilities
    uint16_t* prob = (uint16_t*)(idx + n);
    {
        uint32_t pos = wave_base(sh);
        const Segment sg = segment_of(n, w);
        for (int32_t i0 = sg.lo; i0 < sg.hi; i0 += 64) {
            const int32_t i = i0 + lane;
            const uint32_t f = i < sg.hi ? sh.f[bucket_of(x_hat[i])] : 0u;
            const uint64_t mask = __ballot(f != 0);
            if (f) {
                const uint32_t p = pos + prefix_rank(mask);
                idx[p] = (uint32_t)i;
                prob[p] = (uint16_t)f;
            }
            pos += (uint32_t)__popcll(mask);
        }
    }
    __syncthreads();                                                     // (also orders the zeroes above before the ones below)
    if (w != 0) return;

    const uint8_t* ps = sp + 1 + 2 * used;
    const uint8_t* pw = ps + 4 * L;
    uint32_t x = kLow;
    if (lane < L) x = get16(ps + 4 * lane) | (get16(ps + 4 * lane + 2) << 16);
    int64_t wcur = 0;
    const int32_t steps = (int32_t)((m + L - 1) / L);
    uint32_t next_i = 0, next_f = 1;
    if (lane < L && lane < m) { next_i = idx[lane]; next_f = prob[lane]; }
    for (int32_t tstep = 0; tstep < steps; ++tstep) {
        const int64_t j = (int64_t)tstep * L + lane;
        const bool active = lane < L && j < m;
        const uint32_t i = next_i, f = next_f;
        if (lane < L && j + L < m) { next_i = idx[j + L]; next_f = prob[j + L]; }        // (does not depend on the state)
        bool refill = false;
        if (active) {
            const uint32_t slot = x & 0xffffu;
            const bool bit = slot >= kTotal - f;
            const uint32_t freq = bit ? f : kTotal - f, start = bit ? kTotal - f : 0u;
            x = freq * (x >> 16) + slot - start;
            refill = x < kLow;
            if (bit) out[i] = 1.0f;
        }
        const uint64_t rmask = __ballot(refill);
        if (refill) {
            const int64_t wd = wcur + prefix_rank(rmask);
            uint32_t word = 0;
            if (wd < n_words) word = get16(pw + 2 * wd); else flags |= kCorrupt;
            x = (x << 16) | word;
        }
        wcur += __popcll(rmask);
    }
    if (wcur != n_words || (lane < L && x != kLow)) flags |= kCorrupt;   // the string ends where its symbols do
    flags = wave_or(flags);
    if (lane == 0) status[s] = flags;
}

int args_ok(const char* who, int32_t n_streams, int64_t n, int64_t stride_a, int64_t stride_b, int32_t lanes) {
    PCC_REQUIRE(n_streams >= 0 && n >= 0 && n <= kOccMaxVoxels, "%s: %d streams of %lld voxels (at most 2^28)", who, n_streams, (long long)n);
    PCC_REQUIRE(n_streams <= 1 || (stride_a >= n && stride_b >= n), "%s: a stride (%lld, %lld) below n = %lld", who, (long long)stride_a,
                (long long)stride_b, (long long)n);
    PCC_REQUIRE(lanes >= 0 && lanes <= kMaxLanes && (lanes & (lanes - 1)) == 0, "%s: lanes %d (0 or a power of two <= 64)", who, lanes);
    return PCC_OK;
}

}  // namespace

PCC_API size_t pcc_occ_stream_cap(int64_t n) { return n < 0 ? 0 : (size_t)occ_stream_cap(n); }

PCC_API size_t pcc_occ_workspace_bytes(int32_t n_streams, int64_t n) { return n_streams <= 0 || n < 0 ? 0 : (size_t)n_streams * ws_stride_of(n); }

PCC_API int pcc_occ_check_strings(int32_t n_streams, const uint8_t* str, const int64_t* off, const int32_t* len, int64_t n) {
    PCC_REQUIRE(n_streams >= 0 && (n_streams == 0 || (str && off && len)), "pcc_occ_check_strings: bad argument");
    const int32_t bad = occ_first_bad_string(n_streams, str, off, len, n);
    if (bad >= 0) {
        pcc_set_error("pcc_occ_check_strings: string %d (%d bytes for %lld voxels) has no valid lane byte or an impossible length", bad, len[bad],
                      (long long)n);
        return PCC_ERR_CORRUPT;
    }
    return PCC_OK;
}

PCC_API int pcc_occ_encode_batch(pcc_ctx* ctx, const float* x_hat, int64_t x_hat_stride, const float* occ, int64_t occ_stride, int32_t n_streams,
                                 int64_t n, int32_t lanes, uint8_t* out, size_t cap, int32_t* out_len, int32_t* status, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    PCC_REQUIRE(ctx, "pcc_occ_encode_batch: bad argument");
    if (int rc = args_ok("pcc_occ_encode_batch", n_streams, n, x_hat_stride, occ_stride, lanes)) return rc;
    if (n_streams == 0) return PCC_OK;
    PCC_REQUIRE(x_hat && occ && out && out_len && status && workspace, "pcc_occ_encode_batch: NULL pointer");
    if (cap < pcc_occ_stream_cap(n) || workspace_bytes < pcc_occ_workspace_bytes(n_streams, n)) {
        pcc_set_error("pcc_occ_encode_batch: cap %zu < pcc_occ_stream_cap (%zu) or workspace %zu < pcc_occ_workspace_bytes (%zu)", cap,
                      pcc_occ_stream_cap(n), workspace_bytes, pcc_occ_workspace_bytes(n_streams, n));
        return PCC_ERR_SPACE;
    }
    hipLaunchKernelGGL(occ_encode_kernel, dim3((unsigned)n_streams), dim3(kThreads), 0, (hipStream_t)stream, x_hat, x_hat_stride, occ, occ_stride,
                       (int32_t)n, lanes, out, (int64_t)cap, out_len, status, (uint8_t*)workspace, (int64_t)ws_stride_of(n));
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_occ_decode_batch(pcc_ctx* ctx, const float* x_hat, int64_t x_hat_stride, int32_t n_streams, int64_t n, const uint8_t* str,
                                 size_t str_bytes, const int64_t* off, const int32_t* len, float* occ_out, int64_t out_stride, int32_t* status,
                                 int32_t* status_host, void* workspace, size_t workspace_bytes, void* stream) {
    PCC_REQUIRE(ctx, "pcc_occ_decode_batch: bad argument");
    if (int rc = args_ok("pcc_occ_decode_batch", n_streams, n, x_hat_stride, out_stride, 0)) return rc;
    if (n_streams == 0) return PCC_OK;
    PCC_REQUIRE(x_hat && str && off && len && occ_out && status && workspace, "pcc_occ_decode_batch: NULL pointer");
    if (workspace_bytes < pcc_occ_workspace_bytes(n_streams, n)) {
        pcc_set_error("pcc_occ_decode_batch: workspace %zu < pcc_occ_workspace_bytes (%zu)", workspace_bytes, pcc_occ_workspace_bytes(n_streams, n));
        return PCC_ERR_SPACE;
    }
    hipLaunchKernelGGL(occ_decode_kernel, dim3((unsigned)n_streams), dim3(kThreads), 0, (hipStream_t)stream, x_hat, x_hat_stride, (int32_t)n, str,
                       (int64_t)str_bytes, off, len, occ_out, out_stride, status, (uint8_t*)workspace, (int64_t)ws_stride_of(n));
    PCC_CHECK_HIP(hipGetLastError());
    if (status_host) {
        PCC_CHECK_HIP(hipMemcpyAsync(status_host, status, (size_t)n_streams * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        PCC_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int s = 0; s < n_streams; ++s) {
            if (status_host[s] & kBadShape) { pcc_set_error("pcc_occ_decode_batch: stream %d: bad voxel count", s); return PCC_ERR_ARG; }
            if (status_host[s]) { pcc_set_error("pcc_occ_decode_batch: string %d is corrupt", s); return PCC_ERR_CORRUPT; }
        }
    }
    return PCC_OK;
}
