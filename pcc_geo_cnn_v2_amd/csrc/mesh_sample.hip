// Mesh -> voxelised point cloud (include/pcc_geo.h "mesh sampling"): the reference's dataset step
// src/ds_mesh_to_pc.py (pyntcloud's mesh_random sampler, one scalar min / max over all axes, rint onto vg^3, drop duplicates),
// reproducible from a seed.  The numpy restatement utils/mesh_sampling.py is the definition; tests/test_mesh_gpu.py pins these
// kernels to it bit for bit.
//
// One stream, no host synchronisation:
//   1. k_area: float64 area of every triangle (as its bit pattern: non-negative doubles order like unsigned integers) and the
//      largest one (integer atomicMax, one per workgroup);
//   2. k_weights: w_i = floor(ldexp(area_i / A_max, 32)) in place, then a hipCUB uint64 inclusive scan -> C (exact integers);
//   3. k_sample: Philox4x64-10 per sample, binary search of umul64hi(r0, W) in C, the float64 barycentric point rounded to float32;
//      the min and max of all coordinates (order-preserving uint32 images, integer atomicMin / atomicMax, one per workgroup);
//   4. k_keys: the float32 voxel of every sample and its key x | y << b | z << 2b;
//   5. hipCUB stable radix sort of (key, sample) over 3b bits; k_first marks the first sample of every run of equal keys;
//   6. hipCUB exclusive scan of the marks; k_compact writes the marked voxels in sample order and the count.
// Only integer min / max atomics: the result does not depend on dispatch order.
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int kBlock = 256;

struct MeshHdr {
    unsigned long long amax;          // bits of the largest area
    unsigned pmin, pmax;              // order-preserving images of the smallest / largest sample coordinate
};

size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// float32 <-> uint32 with the order of the floats (no NaN arrives: the samples are finite)
__device__ __forceinline__ unsigned fkey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op) {
    __shared__ T s[kBlock / 64];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, (T)__shfl_xor(v, off));
    __syncthreads();                                      // s may still be read by a previous call
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) v = op(v, s[w]);
    return v;
}

struct MaxOp {
    template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct MinOp {
    template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};

__global__ void k_init(MeshHdr* H) {
    H->amax = 0;
    H->pmin = 0xffffffffu;
    H->pmax = 0;
}

__device__ __forceinline__ double3 vert(const double* __restrict__ v, int i) {
    return make_double3(v[3 * (long long)i], v[3 * (long long)i + 1], v[3 * (long long)i + 2]);
}

__global__ void __launch_bounds__(kBlock) k_area(const double* __restrict__ verts, const int32_t* __restrict__ tris, long long F,
                                                 unsigned long long* __restrict__ abits, MeshHdr* H) {
#pragma clang fp contract(off)
    unsigned long long m = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < F; i += (long long)gridDim.x * blockDim.x) {
        const double3 a = vert(verts, tris[3 * i]), b = vert(verts, tris[3 * i + 1]), c = vert(verts, tris[3 * i + 2]);
        const double e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
        const double e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const double area = 0.5 * __dsqrt_rn((cx * cx + cy * cy) + cz * cz);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(area);
        abits[i] = bits;
        m = bits > m ? bits : m;
    }
    m = block_reduce(m, MaxOp());
    if (threadIdx.x == 0) atomicMax(&H->amax, m);
}

// in place: area bits -> integer weight.  A_max == 0 (a mesh the caller should have refused) gives w = 0 everywhere.
__global__ void __launch_bounds__(kBlock) k_weights(unsigned long long* __restrict__ w, long long F, const MeshHdr* __restrict__ H) {
    const double amax = __longlong_as_double((long long)H->amax);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < F; i += (long long)gridDim.x * blockDim.x) {
        const double r = amax > 0.0 ? __ddiv_rn(__longlong_as_double((long long)w[i]), amax) : 0.0;
        w[i] = (unsigned long long)floor(r * 4294967296.0);             // ldexp(r, 32): exact
    }
}

struct U64x4 {
    unsigned long long v[4];
};

// Philox4x64-10 (Salmon et al., SC'11) of counter (s, 0, 0, 0) and key (k0, 0)
__device__ __forceinline__ U64x4 philox4x64_10(unsigned long long s, unsigned long long k0) {
    unsigned long long c0 = s, c1 = 0, c2 = 0, c3 = 0, k1 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        const unsigned long long h0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), l0 = 0xD2E7470EE14C6C93ull * c0;
        const unsigned long long h1 = __umul64hi(0xCA5A826395121157ull, c2), l1 = 0xCA5A826395121157ull * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    }
    return U64x4{{c0, c1, c2, c3}};
}

__global__ void __launch_bounds__(kBlock) k_sample(const double* __restrict__ verts, const int32_t* __restrict__ tris,
                                                   const unsigned long long* __restrict__ C, long long F, long long n,
                                                   unsigned long long seed, float* __restrict__ P, MeshHdr* H) {
#pragma clang fp contract(off)
    const unsigned long long W = C[F - 1];
    unsigned lo = 0xffffffffu, hi = 0;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x) {
        const U64x4 r = philox4x64_10((unsigned long long)s, seed);
        const unsigned long long t = __umul64hi(r.v[0], W);
        long long a = 0, b = F - 1;                     // smallest i with C[i] > t (t < W = C[F-1]; clamped for W = 0)
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (C[mid] > t) b = mid; else a = mid + 1;
        }
        const double u = (double)(r.v[1] >> 11) * 0x1p-53;
        const double v = (1.0 - u) * ((double)(r.v[2] >> 11) * 0x1p-53);
        const double g = 1.0 - (u + v);
        const double3 p1 = vert(verts, tris[3 * a]), p2 = vert(verts, tris[3 * a + 1]), p3 = vert(verts, tris[3 * a + 2]);
        const float x = __double2float_rn((p1.x * u + p2.x * v) + g * p3.x);
        const float y = __double2float_rn((p1.y * u + p2.y * v) + g * p3.y);
        const float z = __double2float_rn((p1.z * u + p2.z * v) + g * p3.z);
        P[3 * s] = x; P[3 * s + 1] = y; P[3 * s + 2] = z;
        const unsigned kx = fkey(x), ky = fkey(y), kz = fkey(z);
        lo = min(lo, min(kx, min(ky, kz)));
        hi = max(hi, max(kx, max(ky, kz)));
    }
    lo = block_reduce(lo, MinOp());
    hi = block_reduce(hi, MaxOp());
    if (threadIdx.x == 0) {
        atomicMin(&H->pmin, lo);
        atomicMax(&H->pmax, hi);
    }
}

__global__ void __launch_bounds__(kBlock) k_keys(const float* __restrict__ P, long long n, int vg, int b, const MeshHdr* __restrict__ H,
                                                 unsigned long long* __restrict__ keys, unsigned* __restrict__ rows) {
    const float mn = fval(H->pmin);
    const float mx = __fsub_rn(fval(H->pmax), mn);
    const float scale = (float)(vg - 1);                // exact: vg <= 2^21
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x) {
        unsigned long long key = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = mx == 0.0f ? 0.0f : rintf(__fmul_rn(__fdiv_rn(__fsub_rn(P[3 * s + c], mn), mx), scale));
            key |= (unsigned long long)(unsigned)q << (c * b);        // q in [0, vg - 1]: rounding is monotonic
        }
        keys[s] = key;
        rows[s] = (unsigned)s;
    }
}

// keep[sample] = 1 for the first sample of every run of equal keys (the sort is stable: the lowest sample of the run)
__global__ void __launch_bounds__(kBlock) k_first(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ rows,
                                                  long long n, unsigned* __restrict__ keep) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x)
        keep[rows[j]] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_compact(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ keep,
                                                    const unsigned* __restrict__ pos, long long n, int b, float* __restrict__ out,
                                                    int64_t* __restrict__ count) {
    const unsigned long long mask = (1ull << b) - 1;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x) {
        if (s == n - 1) *count = (int64_t)pos[s] + keep[s];
        if (!keep[s]) continue;
        const unsigned long long k = keys[s];
        const long long o = 3 * (long long)pos[s];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[o + c] = (float)((k >> (c * b)) & mask);
    }
}

int key_bits(int vg) {                                  // max(1, ceil(log2 vg))
    int b = 1;
    while ((1 << b) < vg) ++b;
    return b;
}

bool valid_count(int64_t n) { return n > 0 && n < ((int64_t)1 << 31); }

struct MeshLayout {
    size_t hdr, w, cum, pts, keys, keys_s, rows, rows_s, keep, pos, tmp, tmp_bytes, total;
};

MeshLayout mesh_layout(long long F, long long n) {
    MeshLayout l;
    const size_t f = (size_t)F, m = (size_t)n;
    size_t o = 0;
    l.hdr = o; o += al256(sizeof(MeshHdr));
    l.w = o; o += al256(f * 8);
    l.cum = o; o += al256(f * 8);
    l.pts = o; o += al256(m * 12);
    l.keys = o; o += al256(m * 8);
    l.keys_s = o; o += al256(m * 8);
    l.rows = o; o += al256(m * 4);
    l.rows_s = o; o += al256(m * 4);
    l.keep = o; o += al256(m * 4);
    l.pos = o; o += al256(m * 4);
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceScan::InclusiveSum((void*)nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)F,
                                           (hipStream_t)0);
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, 0, 63, (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, c, (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, (hipStream_t)0);
    l.tmp_bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
    l.tmp = o; o += al256(l.tmp_bytes + 256);
    l.total = o;
    return l;
}

unsigned grid_for(long long n, unsigned cap) {
    const long long b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b < (long long)cap ? b : cap);
}

}  // namespace

PCC_API size_t pcc_mesh_sample_workspace_bytes(int64_t ntris, int64_t n) {
    if (!valid_count(ntris) || !valid_count(n)) return 0;
    return mesh_layout(ntris, n).total;
}

PCC_API int pcc_mesh_to_points(pcc_ctx* ctx, const double* verts, int64_t nverts, const int32_t* tris, int64_t ntris, int64_t n, uint64_t seed,
                               int32_t vg, float* samples, float* points, int64_t* npoints_dev, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && verts && tris && points && npoints_dev && workspace, "pcc_mesh_to_points: NULL argument");
    PCC_REQUIRE(nverts > 0 && valid_count(ntris) && valid_count(n), "pcc_mesh_to_points: nverts = %lld, ntris = %lld, n = %lld: need nverts >= 1 "
                "and ntris, n in [1, 2^31)", (long long)nverts, (long long)ntris, (long long)n);
    PCC_REQUIRE(vg >= 1 && vg <= (1 << 21), "pcc_mesh_to_points: vg = %d outside [1, 2^21]", (int)vg);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const MeshLayout l = mesh_layout(ntris, n);
    unsigned char* w = (unsigned char*)workspace;
    MeshHdr* H = (MeshHdr*)(w + l.hdr);
    unsigned long long *wts = (unsigned long long*)(w + l.w), *cum = (unsigned long long*)(w + l.cum);
    unsigned long long *keys = (unsigned long long*)(w + l.keys), *keys_s = (unsigned long long*)(w + l.keys_s);
    unsigned *rows = (unsigned*)(w + l.rows), *rows_s = (unsigned*)(w + l.rows_s);
    unsigned *keep = (unsigned*)(w + l.keep), *pos = (unsigned*)(w + l.pos);
    float* P = samples ? samples : (float*)(w + l.pts);
    void* tmp = (void*)(w + l.tmp);
    const unsigned cap = 4u * (unsigned)(ctx->num_cu > 0 ? ctx->num_cu : 256);     // workgroups of the kernels with atomics
    const int b = key_bits(vg);

    hipLaunchKernelGGL(k_init, dim3(1), dim3(1), 0, st, H);
    hipLaunchKernelGGL(k_area, dim3(grid_for(ntris, cap)), dim3(kBlock), 0, st, verts, tris, (long long)ntris, wts, H);
    hipLaunchKernelGGL(k_weights, dim3(grid_for(ntris, 1u << 20)), dim3(kBlock), 0, st, wts, (long long)ntris, (const MeshHdr*)H);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::InclusiveSum(tmp, bytes, (const unsigned long long*)wts, cum, (int)ntris, st));
    hipLaunchKernelGGL(k_sample, dim3(grid_for(n, cap)), dim3(kBlock), 0, st, verts, tris, (const unsigned long long*)cum, (long long)ntris,
                       (long long)n, (unsigned long long)seed, P, H);
    const unsigned g = grid_for(n, 1u << 20);
    hipLaunchKernelGGL(k_keys, dim3(g), dim3(kBlock), 0, st, (const float*)P, (long long)n, (int)vg, b, (const MeshHdr*)H, keys, rows);
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const unsigned long long*)keys, keys_s, (const unsigned*)rows, rows_s,
                                                     (int)n, 0, 3 * b, st));
    hipLaunchKernelGGL(k_first, dim3(g), dim3(kBlock), 0, st, (const unsigned long long*)keys_s, (const unsigned*)rows_s, (long long)n, keep);
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const unsigned*)keep, pos, (int)n, st));
    hipLaunchKernelGGL(k_compact, dim3(g), dim3(kBlock), 0, st, (const unsigned long long*)keys, (const unsigned*)keep, (const unsigned*)pos,
                       (long long)n, b, points, npoints_dev);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
