// Point normals of a voxelised cloud (include/pcc_geo.h "point normals", DESIGN.md "Point normals").
//
// Definition (pinned by tests/test_normals_gpu.py against a numpy / scipy restatement):
//   - points are integers in [0, 2^21); the neighbourhood of point i is the k_eff = min(k, N) points j with the smallest
//     (|p_j - p_i|^2, j) in lexicographic order (i itself is a candidate like any other);
//   - M = k_eff * sum q q^T - (sum q)(sum q)^T over the neighbours, q = p_j - p_i, exact in int64;
//   - the normal is the unit eigenvector of the smallest eigenvalue of M (double, cyclic Jacobi with a fixed sweep count),
//     stored as float32; M == 0 gives exactly (0, 0, 1);
//   - otherwise its sign makes n . (p_i - o) >= 0, o = the viewpoint or the centroid (exact int64 sums / N); a product of
//     exactly 0 makes the first non-zero component positive.
//
// Pipeline, all on one stream, no host synchronisation:
//   1. k_prepare: 63-bit Morton code of every point, bounding box and exact coordinate sums (integer atomics, one set per
//      workgroup);
//   2. hipCUB radix sort of (code, row index); k_records gathers (x, y, z, row) in that order and histograms the highest
//      differing Morton bit of adjacent codes, which gives the number of occupied cells of edge 2^L for every L at once;
//   3. k_params picks the base cell level: the smallest L with about k/2 or more points per occupied cell;
//   4. k_knn, one lane per query in Morton order (a wave's lanes are neighbours in space): the cells of edge 2^L are
//      contiguous ranges of the sorted array (found by binary search); the search visits the cube of cells of Chebyshev
//      radius 1 around the query, then radius 2, then radius 2 at the next coarser levels, until the k-th best squared
//      distance is STRICTLY below the squared distance from the query to the outside of the visited box (an equidistant
//      point with a lower row index could still be outside on equality), or the box holds the whole cloud.  The top k live
//      in registers as packed 64-bit keys (squared distance << 32 | row), sorted, insertion by an unrolled min/max chain;
//      integer order of the keys is exactly the tie rule.  A query whose k-th squared distance does not fit 32 bits
//      (far outliers) is re-run by the same kernel with 128-bit keys (the "wide" pass over the flagged queries).
//   5. the same lane computes M, solves, orients and writes the normal (and its neighbour rows when asked).
// No floating-point atomics: every output is bit-reproducible from call to call.
#include <hipcub/hipcub.hpp>

#include <type_traits>

#include "common.h"

namespace {

constexpr int kCoordMask = (1 << 21) - 1;
constexpr int kLevels = 22;         // cell edge 2^L, L = 0 .. 21 (L = 21: one cell holds the whole domain)
constexpr int kJacobiSweeps = 10;   // 3x3 cyclic Jacobi converges to machine precision in ~5

struct NormParams {
    int bmin[3], bmax[3];            // bounding box of the cloud
    unsigned long long sum[3];       // exact coordinate sums
    unsigned hist[kLevels];          // adjacent sorted pairs by floor(highest differing Morton bit / 3)
    int level;                       // base cell level of the search
    int nflag;                       // queries for the wide pass
};

__device__ __forceinline__ unsigned long long spread3(unsigned v) {
    unsigned long long x = v & kCoordMask;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ unsigned long long morton(int x, int y, int z) {
    return spread3((unsigned)x) << 2 | spread3((unsigned)y) << 1 | spread3((unsigned)z);
}

// coordinates outside [0, 2^21) are a precondition violation (the Python layer refuses them); masking keeps every cell
// computation inside the domain whatever arrives
__device__ __forceinline__ int3 load_pt(const int32_t* pts, long long i) {
    return make_int3(pts[3 * i] & kCoordMask, pts[3 * i + 1] & kCoordMask, pts[3 * i + 2] & kCoordMask);
}

__global__ void k_init(NormParams* P) {
    for (int a = 0; a < 3; ++a) { P->bmin[a] = kCoordMask; P->bmax[a] = 0; P->sum[a] = 0; }
    for (int l = 0; l < kLevels; ++l) P->hist[l] = 0;
    P->level = 0;
    P->nflag = 0;
}

// grid-stride over the points, one set of atomics per workgroup: thousands of same-address atomics serialise (a launch with one set
// per wave cost 1.4 ms at 1e6 points)
__global__ void __launch_bounds__(256) k_prepare(const int32_t* __restrict__ pts, long long n, unsigned long long* __restrict__ codes,
                                                 unsigned* __restrict__ rows, NormParams* P) {
    __shared__ int slo[4][3], shi[4][3];
    __shared__ unsigned long long ssum[4][3];
    int lo[3] = {kCoordMask, kCoordMask, kCoordMask}, hi[3] = {0, 0, 0};
    unsigned long long s[3] = {0, 0, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int3 p = load_pt(pts, i);
        codes[i] = morton(p.x, p.y, p.z);
        rows[i] = (unsigned)i;
        lo[0] = min(lo[0], p.x); lo[1] = min(lo[1], p.y); lo[2] = min(lo[2], p.z);
        hi[0] = max(hi[0], p.x); hi[1] = max(hi[1], p.y); hi[2] = max(hi[2], p.z);
        s[0] += p.x; s[1] += p.y; s[2] += p.z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], off));
            hi[a] = max(hi[a], __shfl_xor(hi[a], off));
            s[a] += __shfl_xor(s[a], off);
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { slo[wave][a] = lo[a]; shi[wave][a] = hi[a]; ssum[wave][a] = s[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        int l = slo[0][a], h = shi[0][a];
        unsigned long long t = ssum[0][a];
        for (int w = 1; w < 4; ++w) { l = min(l, slo[w][a]); h = max(h, shi[w][a]); t += ssum[w][a]; }
        atomicMin(&P->bmin[a], l);
        atomicMax(&P->bmax[a], h);
        atomicAdd(&P->sum[a], t);
    }
}

__global__ void __launch_bounds__(256) k_records(const int32_t* __restrict__ pts, long long n, const unsigned long long* __restrict__ codes,
                                                 const unsigned* __restrict__ rows, int4* __restrict__ recs, NormParams* P) {
    __shared__ unsigned h[kLevels];
    if (threadIdx.x < kLevels) h[threadIdx.x] = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const unsigned r = rows[t];
        const int3 p = load_pt(pts, r);
        recs[t] = make_int4(p.x, p.y, p.z, (int)r);
        if (t > 0) {
            const unsigned long long d = codes[t] ^ codes[t - 1];
            if (d) atomicAdd(&h[(63 - __clzll((long long)d)) / 3], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLevels && h[threadIdx.x]) atomicAdd(&P->hist[threadIdx.x], h[threadIdx.x]);
}

// base level: the smallest L whose occupied cells hold k_eff / 2 points or more on average (L = 21 always qualifies)
__global__ void k_params(long long n, int keff, NormParams* P) {
    unsigned long long occ = 1;                 // occupied cells of edge 1: one more than the adjacent pairs that differ
    for (int l = 0; l < kLevels; ++l) occ += P->hist[l];
    int level = kLevels - 1;
    for (int l = 0; l < kLevels; ++l) {
        if (2ull * (unsigned long long)n >= (unsigned long long)keff * occ) { level = l; break; }
        occ -= P->hist[l];                      // pairs that differ at level l but not above: merged one level up
    }
    P->level = level;
}

__device__ __forceinline__ long long lower_bound(const unsigned long long* __restrict__ codes, long long n, unsigned long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <class K>
struct KeyOps;
template <>
struct KeyOps<unsigned long long> {            // squared distance saturated to 32 bits: exact while the k-th one fits
    static constexpr unsigned long long kMax = ~0ull;
    __device__ static unsigned long long pack(unsigned long long d2, unsigned row) {
        return (d2 < 0xffffffffull ? d2 : 0xffffffffull) << 32 | row;
    }
};
template <>
struct KeyOps<unsigned __int128> {             // squared distance < 3 * 2^42: always exact
    static constexpr unsigned __int128 kMax = ~(unsigned __int128)0;
    __device__ static unsigned __int128 pack(unsigned long long d2, unsigned row) { return (unsigned __int128)d2 << 32 | row; }
};
template <class K>
__device__ __forceinline__ unsigned long long key_d2(K key) {
    const K d = key >> 32;
    return d > (K)~0ull ? ~0ull : (unsigned long long)d;
}

template <int KC, class K>
__device__ __forceinline__ void insert(K (&a)[KC], K key) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const K lo = a[j] < key ? a[j] : key;
        key = a[j] < key ? key : a[j];
        a[j] = lo;
    }
}

// one Jacobi rotation of the symmetric A (upper triangle kept in sync) zeroing A[p][q], accumulated into V
template <int p, int q, int r>
__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p][p] -= t * apq;
    A[q][q] += t * apq;
    A[p][q] = A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = c * vp - s * vq;
        V[i][q] = s * vp + c * vq;
    }
}

// One lane per query.  WIDE = false: every query, in sorted order; a query whose k-th key saturated is appended to `flagged`.
// WIDE = true: the flagged queries, with 128-bit keys.
template <int KC, bool WIDE>
__global__ void __launch_bounds__(256) k_knn(const int4* __restrict__ recs, const unsigned long long* __restrict__ codes,
                                             const int32_t* __restrict__ pts, long long n, int k, NormParams* P,
                                             const double* __restrict__ viewpoint, float* __restrict__ normals,
                                             int32_t* __restrict__ knn, int* __restrict__ flagged) {
    using K = typename std::conditional<WIDE, unsigned __int128, unsigned long long>::type;
    const long long count = WIDE ? (long long)P->nflag : n;
    const int keff = (long long)k < n ? k : (int)n;
    const int base = P->level;
    int bmin[3], bmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { bmin[a] = P->bmin[a]; bmax[a] = P->bmax[a]; }
    for (long long job = (long long)blockIdx.x * blockDim.x + threadIdx.x; job < count; job += (long long)gridDim.x * blockDim.x) {
        const long long t = WIDE ? (long long)flagged[job] : job;
        const int4 qr = recs[t];
        const int qc[3] = {qr.x, qr.y, qr.z};
        K a[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) a[j] = j < KC - keff ? (K)0 : KeyOps<K>::kMax;   // zero sentinels in front of the k_eff slots
        int level = base, rad = 1;
        bool have_prev = false;
        int plo[3] = {0, 0, 0}, phi[3] = {0, 0, 0};
        for (;;) {
            const int e = 1 << level;
            int c[3], clo[3], chi[3], blo[3], bhi[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                c[ax] = qc[ax] >> level;
                clo[ax] = max(c[ax] - rad, bmin[ax] >> level);
                chi[ax] = min(c[ax] + rad, bmax[ax] >> level);
                blo[ax] = (c[ax] - rad) * e;
                bhi[ax] = (c[ax] + rad + 1) * e - 1;
            }
            for (int cx = clo[0]; cx <= chi[0]; ++cx)
                for (int cy = clo[1]; cy <= chi[1]; ++cy)
                    for (int cz = clo[2]; cz <= chi[2]; ++cz) {
                        if (have_prev && cx * e >= plo[0] && (cx + 1) * e - 1 <= phi[0] && cy * e >= plo[1] && (cy + 1) * e - 1 <= phi[1] &&
                            cz * e >= plo[2] && (cz + 1) * e - 1 <= phi[2])
                            continue;                                        // visited at the previous stage
                        const unsigned long long key0 = morton(cx, cy, cz) << (3 * level);
                        for (long long pos = lower_bound(codes, n, key0); pos < n; ++pos) {
                            const int4 r = recs[pos];
                            if ((r.x >> level) != cx || (r.y >> level) != cy || (r.z >> level) != cz) break;
                            if (have_prev && r.x >= plo[0] && r.x <= phi[0] && r.y >= plo[1] && r.y <= phi[1] && r.z >= plo[2] && r.z <= phi[2])
                                continue;
                            const long long dx = r.x - qc[0], dy = r.y - qc[1], dz = r.z - qc[2];
                            const K key = KeyOps<K>::pack((unsigned long long)(dx * dx + dy * dy + dz * dz), (unsigned)r.w);
                            if (key < a[KC - 1]) insert<KC, K>(a, key);
                        }
                    }
            // nearest possible unvisited point: just outside a face of the box; faces beyond the cloud's box hide nothing
            long long gap = -1;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (blo[ax] > bmin[ax]) { const long long g = qc[ax] - blo[ax] + 1; gap = gap < 0 || g < gap ? g : gap; }
                if (bhi[ax] < bmax[ax]) { const long long g = bhi[ax] + 1 - qc[ax]; gap = gap < 0 || g < gap ? g : gap; }
            }
            if (gap < 0 || key_d2(a[KC - 1]) < (unsigned long long)(gap * gap)) break;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { plo[ax] = blo[ax]; phi[ax] = bhi[ax]; }
            have_prev = true;
            if (rad == 1) rad = 2; else ++level;
        }
        if (!WIDE && key_d2(a[KC - 1]) >= 0xffffffffull) {              // saturated: exact only with wide keys
            flagged[atomicAdd(&P->nflag, 1)] = (int)t;
            continue;
        }
        // exact moments of q = p_j - p_i over the neighbours
        const long long row = qr.w;
        long long s0 = 0, s1 = 0, s2 = 0, m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            if (j < KC - keff) continue;
            const unsigned nb = (unsigned)(a[j] & 0xffffffffu);
            if (knn) knn[row * k + (j - (KC - keff))] = (int32_t)nb;
            const int3 p = load_pt(pts, nb);
            const long long q0 = p.x - qc[0], q1 = p.y - qc[1], q2 = p.z - qc[2];
            s0 += q0; s1 += q1; s2 += q2;
            m00 += q0 * q0; m01 += q0 * q1; m02 += q0 * q2; m11 += q1 * q1; m12 += q1 * q2; m22 += q2 * q2;
        }
        if (knn)
            for (int j = keff; j < k; ++j) knn[row * k + j] = -1;
        const long long M[6] = {keff * m00 - s0 * s0, keff * m01 - s0 * s1, keff * m02 - s0 * s2,
                                keff * m11 - s1 * s1, keff * m12 - s1 * s2, keff * m22 - s2 * s2};
        double nrm[3] = {0.0, 0.0, 1.0};
        if (M[0] | M[1] | M[2] | M[3] | M[4] | M[5]) {
            double amax = 0.0;
#pragma unroll
            for (int u = 0; u < 6; ++u) amax = fmax(amax, fabs((double)M[u]));
            const double sc = 1.0 / amax;
            double A[3][3] = {{M[0] * sc, M[1] * sc, M[2] * sc}, {M[1] * sc, M[3] * sc, M[4] * sc}, {M[2] * sc, M[4] * sc, M[5] * sc}};
            double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
            for (int sw = 0; sw < kJacobiSweeps; ++sw) {
                jacobi_rot<0, 1, 2>(A, V);
                jacobi_rot<0, 2, 1>(A, V);
                jacobi_rot<1, 2, 0>(A, V);
            }
            int m = 0;
            if (A[1][1] < A[m][m]) m = 1;
            if (A[2][2] < (m == 0 ? A[0][0] : A[1][1])) m = 2;
            const double v0 = m == 0 ? V[0][0] : m == 1 ? V[0][1] : V[0][2];
            const double v1 = m == 0 ? V[1][0] : m == 1 ? V[1][1] : V[1][2];
            const double v2 = m == 0 ? V[2][0] : m == 1 ? V[2][1] : V[2][2];
            const double inv = 1.0 / sqrt(v0 * v0 + v1 * v1 + v2 * v2);
            nrm[0] = v0 * inv; nrm[1] = v1 * inv; nrm[2] = v2 * inv;
            double o[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) o[ax] = viewpoint ? viewpoint[ax] : (double)P->sum[ax] / (double)n;
            const double dot = nrm[0] * (qc[0] - o[0]) + nrm[1] * (qc[1] - o[1]) + nrm[2] * (qc[2] - o[2]);
            const double first = nrm[0] != 0.0 ? nrm[0] : nrm[1] != 0.0 ? nrm[1] : nrm[2];
            if (dot < 0.0 || (dot == 0.0 && first < 0.0)) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
        }
        normals[3 * row] = (float)nrm[0];
        normals[3 * row + 1] = (float)nrm[1];
        normals[3 * row + 2] = (float)nrm[2];
    }
}

struct NormLayout {
    size_t codes0, codes1, rows0, rows1, recs, flagged, params, sort_tmp, sort_tmp_bytes, total;
};

NormLayout norm_layout(long long n) {
    NormLayout l;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t N = (size_t)n;
    size_t o = 0;
    l.codes0 = o; o += al(N * 8);
    l.codes1 = o; o += al(N * 8);
    l.rows0 = o; o += al(N * 4);
    l.rows1 = o; o += al(N * 4);
    l.recs = o; o += al(N * 16);
    l.flagged = o; o += al(N * 4);
    l.params = o; o += al(sizeof(NormParams));
    size_t tmp = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)(n > 0 ? n : 1), 0, 63, (hipStream_t)0);
    l.sort_tmp_bytes = tmp;
    l.sort_tmp = o; o += al(tmp + 256);
    l.total = o;
    return l;
}

template <int KC>
void launch_knn(unsigned grid, unsigned wide_grid, hipStream_t st, const int4* recs, const unsigned long long* codes, const int32_t* pts,
                long long n, int k, NormParams* P, const double* viewpoint, float* normals, int32_t* knn, int* flagged) {
    hipLaunchKernelGGL((k_knn<KC, false>), dim3(grid), dim3(256), 0, st, recs, codes, pts, n, k, P, viewpoint, normals, knn, flagged);
    hipLaunchKernelGGL((k_knn<KC, true>), dim3(wide_grid), dim3(256), 0, st, recs, codes, pts, n, k, P, viewpoint, normals, knn, flagged);
}

}  // namespace

PCC_API size_t pcc_normals_workspace_bytes(int64_t npts, int32_t k) {
    (void)k;
    if (npts <= 0 || npts >= ((int64_t)1 << 31)) return 0;
    return norm_layout(npts).total;
}

PCC_API int pcc_estimate_normals(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t k, const double* viewpoint, float* normals,
                                 int32_t* knn, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && pts && normals && workspace, "pcc_estimate_normals: NULL argument");
    PCC_REQUIRE(npts > 0 && npts < ((int64_t)1 << 31), "pcc_estimate_normals: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(k >= 3 && k <= 64, "pcc_estimate_normals: k = %d outside [3, 64]", k);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const long long n = npts;
    const NormLayout l = norm_layout(n);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *codes0 = (unsigned long long*)(w + l.codes0), *codes1 = (unsigned long long*)(w + l.codes1);
    unsigned *rows0 = (unsigned*)(w + l.rows0), *rows1 = (unsigned*)(w + l.rows1);
    int4* recs = (int4*)(w + l.recs);
    int* flagged = (int*)(w + l.flagged);
    NormParams* P = (NormParams*)(w + l.params);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_init, dim3(1), dim3(1), 0, st, P);
    const unsigned cus = (unsigned)(ctx->num_cu > 0 ? ctx->num_cu : 256);
    hipLaunchKernelGGL(k_prepare, dim3(blocks < cus ? blocks : cus), dim3(256), 0, st, pts, n, codes0, rows0, P);
    size_t tmp = l.sort_tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.sort_tmp), tmp, (const unsigned long long*)codes0, codes1,
                                                     (const unsigned*)rows0, rows1, (int)n, 0, 63, st));
    hipLaunchKernelGGL(k_records, dim3(blocks), dim3(256), 0, st, pts, n, (const unsigned long long*)codes1, (const unsigned*)rows1, recs, P);
    const int keff = (long long)k < n ? k : (int)n;
    hipLaunchKernelGGL(k_params, dim3(1), dim3(1), 0, st, n, keff, P);
    const unsigned wide_grid = cus;
    if (k <= 8) launch_knn<8>(blocks, wide_grid, st, recs, codes1, pts, n, k, P, viewpoint, normals, knn, flagged);
    else if (k <= 16) launch_knn<16>(blocks, wide_grid, st, recs, codes1, pts, n, k, P, viewpoint, normals, knn, flagged);
    else if (k <= 32) launch_knn<32>(blocks, wide_grid, st, recs, codes1, pts, n, k, P, viewpoint, normals, knn, flagged);
    else launch_knn<64>(blocks, wide_grid, st, recs, codes1, pts, n, k, P, viewpoint, normals, knn, flagged);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
