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
//   1. the cell index of cell_index.h over the cloud, base level for k_eff / 2 points per occupied cell;
//   2. k_knn, one lane per query in Morton order: the index search from Chebyshev radius 1 keeps the top k in registers as packed
//      64-bit keys (squared distance << 32 | row), sorted, insertion by an unrolled min/max chain; integer order of the keys is
//      exactly the tie rule.  A query whose k-th squared distance does not fit 32 bits (far outliers) is re-run by the same kernel
//      with 128-bit keys (the "wide" pass over the flagged queries).
//   3. the same lane computes M, solves, orients and writes the normal (and its neighbour rows when asked).
// No floating-point atomics: every output is bit-reproducible from call to call.
#include <type_traits>

#include "cell_index.h"

namespace {

constexpr int kJacobiSweeps = 10;   // 3x3 cyclic Jacobi converges to machine precision in ~5

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

// the top k of a query as sorted keys; the first KC - k_eff slots hold zero sentinels, so the last k_eff are the answer
template <int KC, class K>
struct TopK {
    K a[KC];
    __device__ __forceinline__ explicit TopK(int keff) {
#pragma unroll
        for (int j = 0; j < KC; ++j) a[j] = j < KC - keff ? (K)0 : KeyOps<K>::kMax;
    }
    __device__ __forceinline__ void consider(unsigned long long d2, unsigned row) {
        const K key = KeyOps<K>::pack(d2, row);
        if (key < a[KC - 1]) insert<KC, K>(a, key);
    }
    __device__ __forceinline__ unsigned long long bound() const { return key_d2(a[KC - 1]); }
};

// One lane per query.  WIDE = false: every query, in sorted order; a query whose k-th key saturated is appended to `flagged`.
// WIDE = true: the flagged queries, with 128-bit keys.  pts: the index's row-order copy of the points.
template <int KC, bool WIDE>
__global__ void __launch_bounds__(256) k_knn(const IndexHdr* H, const int4* __restrict__ recs, const unsigned long long* __restrict__ codes,
                                             const int32_t* __restrict__ pts, long long n, int k, const double* __restrict__ viewpoint,
                                             float* __restrict__ normals, int32_t* __restrict__ knn, int* __restrict__ flagged, int* nflag) {
    using K = typename std::conditional<WIDE, unsigned __int128, unsigned long long>::type;
    const long long count = WIDE ? (long long)*nflag : n;
    const int keff = (long long)k < n ? k : (int)n;
    const Cells g = cells(H, codes, recs, n);
    for (long long job = (long long)blockIdx.x * blockDim.x + threadIdx.x; job < count; job += (long long)gridDim.x * blockDim.x) {
        const long long t = WIDE ? (long long)flagged[job] : job;
        const int4 qr = recs[t];
        const int qc[3] = {qr.x, qr.y, qr.z};
        const TopK<KC, K> top = search(g, qc, 1, TopK<KC, K>(keff));
        if (!WIDE && top.bound() >= 0xffffffffull) {                     // saturated: exact only with wide keys
            flagged[atomicAdd(nflag, 1)] = (int)t;
            continue;
        }
        // exact moments of q = p_j - p_i over the neighbours
        const long long row = qr.w;
        long long s0 = 0, s1 = 0, s2 = 0, m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            if (j < KC - keff) continue;
            const unsigned nb = (unsigned)(top.a[j] & 0xffffffffu);
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
            for (int ax = 0; ax < 3; ++ax) o[ax] = viewpoint ? viewpoint[ax] : (double)H->sum[ax] / (double)n;
            const double dot = nrm[0] * (qc[0] - o[0]) + nrm[1] * (qc[1] - o[1]) + nrm[2] * (qc[2] - o[2]);
            const double first = nrm[0] != 0.0 ? nrm[0] : nrm[1] != 0.0 ? nrm[1] : nrm[2];
            if (dot < 0.0 || (dot == 0.0 && first < 0.0)) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
        }
        normals[3 * row] = (float)nrm[0];
        normals[3 * row + 1] = (float)nrm[1];
        normals[3 * row + 2] = (float)nrm[2];
    }
}

struct NormLayout {                   // the cell index, then the flagged queries of the wide pass and their count
    size_t flagged, nflag, total;
};

NormLayout norm_layout(long long n) {
    NormLayout l;
    l.flagged = index_layout(n).total;
    l.nflag = l.flagged + al256((size_t)n * 4);
    l.total = l.nflag + al256(sizeof(int));
    return l;
}

template <int KC>
void launch_knn(unsigned grid, unsigned wide_grid, hipStream_t st, const IndexView& v, int k, const double* viewpoint, float* normals,
                int32_t* knn, int* flagged, int* nflag) {
    hipLaunchKernelGGL((k_knn<KC, false>), dim3(grid), dim3(256), 0, st, v.hdr, v.recs, v.codes, v.pts, v.n, k, viewpoint, normals, knn,
                       flagged, nflag);
    hipLaunchKernelGGL((k_knn<KC, true>), dim3(wide_grid), dim3(256), 0, st, v.hdr, v.recs, v.codes, v.pts, v.n, k, viewpoint, normals,
                       knn, flagged, nflag);
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
    int* flagged = (int*)(w + l.flagged);
    int* nflag = (int*)(w + l.nflag);
    const int keff = (long long)k < n ? k : (int)n;
    const int rc = index_build(ctx, pts, n, w, keff, st);
    if (rc != PCC_OK) return rc;
    PCC_CHECK_HIP(hipMemsetAsync(nflag, 0, sizeof(int), st));
    const IndexView v = index_view(w, n);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const unsigned wide_grid = (unsigned)(ctx->num_cu > 0 ? ctx->num_cu : 256);
    if (k <= 8) launch_knn<8>(blocks, wide_grid, st, v, k, viewpoint, normals, knn, flagged, nflag);
    else if (k <= 16) launch_knn<16>(blocks, wide_grid, st, v, k, viewpoint, normals, knn, flagged, nflag);
    else if (k <= 32) launch_knn<32>(blocks, wide_grid, st, v, k, viewpoint, normals, knn, flagged, nflag);
    else launch_knn<64>(blocks, wide_grid, st, v, k, viewpoint, normals, knn, flagged, nflag);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
