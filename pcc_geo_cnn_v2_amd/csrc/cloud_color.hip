// Colour transfer and colour distortion across two voxelised clouds (include/pcc_geo.h "cloud colours").
//
// Definition (pinned by tests/test_color_gpu.py against the numpy / scipy restatement in tests/_color_ref.py):
//   - the indexed points of a query q in order: the rows j sorted by (|p_j - q|^2, j), exact integers, lexicographic;
//   - map: the colour (and row) of the rank-th point of that order, rank 1 or 2 (rank 1 is pcc_cloud_nearest's row; rank 2 is the
//     reference's map_color.py, which takes the second of a k = 2 KD-tree query);
//   - distortion: over ALL indexed points at the smallest squared distance, the exact integer sums S of R, G, B and their count;
//     m = S / count and d = c_q - m in float64, then the BT.709 terms eY = (0.2126 dR + 0.7152 dG) + 0.0722 dB,
//     eU = (-0.1146 dR - 0.3854 dG) + 0.5 dB, eV = (0.5 dR - 0.4542 dG) - 0.0458 dB, every operation rounded (no contraction);
//     tally float64[6] = the sums of eY^2, eU^2, eV^2 for A -> B (each A point against B), then for B -> A;
//   - transfer (pinned by tests/test_transfer_gpu.py against utils/pc_metric.transfer_colors_host): the colour of a row of B that
//     minimises the A -> B sums above, the mean of the rows of A that have it in their tie set, rounded half up in integers.
//
// Search: the cell index of cell_index.h (built by pcc_cloud_index_build), one lane per query, queries in the query cloud's
// Morton order (its index records), as k_query<true> of cloud_metrics.hip.  Tally: the per-point terms are written by row and
// summed by k_ctally / k_cfinish in an order fixed by the sizes (the grid and the tree of cloud_tally.h); nothing synchronises with
// the host.
#include "cell_index.h"
#include "cloud_tally.h"

namespace {

// ---- map -----------------------------------------------------------------------------------------------------------------------

// the two lowest (squared distance, row) pairs so far; bound: the RANK-th best, ~0 until RANK points have been seen
template <int RANK>
struct TwoBest {
    unsigned long long d0 = ~0ull, d1 = ~0ull;
    unsigned r0 = ~0u, r1 = ~0u;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d < d1 || (d == d1 && r < r1)) {
            if (d < d0 || (d == d0 && r < r0)) { d1 = d0; r1 = r0; d0 = d; r0 = r; }
            else { d1 = d; r1 = r; }
        }
    }
    __device__ __forceinline__ unsigned long long bound() const { return RANK == 1 ? d0 : d1; }
};

// One lane per query record (Morton order); writes out[3 * row ..] and rows[row] (may be NULL) for the record's row.
template <int RANK>
__global__ void __launch_bounds__(256) k_map(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                             const int4* __restrict__ recs, long long n, const uint8_t* __restrict__ colours,
                                             const int4* __restrict__ qrecs, long long nq, uint8_t* __restrict__ out,
                                             int32_t* __restrict__ rows) {
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        const TwoBest<RANK> best = search(g, qc, 0, TwoBest<RANK>());
        const long long r = RANK == 1 ? best.r0 : best.r1;    // n >= RANK: the search has seen at least RANK points
        const long long row = q.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * row + c] = colours[3 * r + c];
        if (rows) rows[row] = (int32_t)r;
    }
}

// ---- distortion ----------------------------------------------------------------------------------------------------------------

struct ColourSums {                   // over the tie set: the exact sums of R, G, B
    const uint8_t* colours;
    unsigned long long s[3] = {0, 0, 0};
    __device__ __forceinline__ void reset() { s[0] = s[1] = s[2] = 0; }
    __device__ __forceinline__ void add(unsigned r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += colours[3 * (long long)r + c];
    }
};
using TieSet = TieVisitor<ColourSums>;

// One lane per query record of the source cloud against the destination index: terms[3 * row ..] = (eY^2, eU^2, eV^2).
__global__ void __launch_bounds__(256) k_cterms(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                                const int4* __restrict__ recs, long long n, const uint8_t* __restrict__ colours,
                                                const int4* __restrict__ qrecs, const uint8_t* __restrict__ qcolours, long long nq,
                                                double* __restrict__ terms) {
#pragma clang fp contract(off)
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        TieSet init;
        init.over.colours = colours;
        const TieSet ties = search(g, qc, 0, init);
        const long long row = q.w;
        const double cnt = (double)ties.count;                  // exact: count < 2^31, sums < 2^39
        const double dR = (double)qcolours[3 * row] - (double)ties.over.s[0] / cnt;
        const double dG = (double)qcolours[3 * row + 1] - (double)ties.over.s[1] / cnt;
        const double dB = (double)qcolours[3 * row + 2] - (double)ties.over.s[2] / cnt;
        const double eY = (0.2126 * dR + 0.7152 * dG) + 0.0722 * dB;
        const double eU = (-0.1146 * dR - 0.3854 * dG) + 0.5 * dB;
        const double eV = (0.5 * dR - 0.4542 * dG) - 0.0458 * dB;
        terms[3 * row] = eY * eY;
        terms[3 * row + 1] = eU * eU;
        terms[3 * row + 2] = eV * eV;
    }
}

// Grid-stride over the rows on tally_blocks(n) workgroups, then the fixed tree in each: partial[3 * block ..].
__global__ void __launch_bounds__(256) k_ctally(const double* __restrict__ terms, long long n, double* __restrict__ partial) {
    __shared__ Slots<double, 3> sh[256];
    Slots<double, 3> acc = {{0.0, 0.0, 0.0}};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc.v[c] += terms[3 * i + c];
    }
    const Slots<double, 3> sum = tree256(acc, sh, EachSlot<Sum>());
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) partial[3 * blockIdx.x + c] = sum.v[c];
    }
}

// one workgroup: the partials of A -> B (ga of them) and B -> A (gb), each direction summed in a fixed order
__global__ void __launch_bounds__(256) k_cfinish(const double* __restrict__ pab, int ga, const double* __restrict__ pba, int gb,
                                                 double* __restrict__ tally) {
    __shared__ Slots<double, 6> sh[256];
    Slots<double, 6> acc = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double* p = side ? pba : pab;
        const int g = side ? gb : ga;
        for (int b = threadIdx.x; b < g; b += 256) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc.v[3 * side + c] += p[3 * b + c];
        }
    }
    const Slots<double, 6> sum = tree256(acc, sh, EachSlot<Sum>());
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) tally[k] = sum.v[k];
    }
}

struct ColorLayout {
    size_t terms_a, terms_b, pab, pba, total;
};

ColorLayout color_layout(long long na, long long nb) {
    ColorLayout l;
    Carver w;
    l.terms_a = w.take((size_t)na * 24);
    l.terms_b = w.take((size_t)nb * 24);
    l.pab = w.take(kTallyBlocks * 24);
    l.pba = w.take(kTallyBlocks * 24);
    l.total = w.o;
    return l;
}

// ---- transfer ------------------------------------------------------------------------------------------------------------------
// Least-squares recolouring (DESIGN.md §4.9 "Colour transfer"): every row of A votes for ALL rows of B at its smallest squared
// distance; a row of B takes the mean of its voters' colours, or, with no voter, of its own equidistant nearest rows of A; the mean
// is rounded half up in integers, (2 S + n) / (2 n).  The accumulators are integers and only ever added to, so the bits do not
// depend on the order in which the votes arrive: 64-bit sums (255 * N_A < 2^39) and a 32-bit vote count (<= N_A < 2^31), exact for
// every size the entry point accepts.

struct TransferLayout {
    size_t sums, votes, total;          // unsigned long long[3 * nb], unsigned[nb]
};

TransferLayout transfer_layout(long long nb) {
    TransferLayout l;
    Carver w;
    l.sums = w.take((size_t)nb * 24);
    l.votes = w.take((size_t)nb * 4);
    l.total = w.o;
    return l;
}

// Second visit of a query whose smallest squared distance is known: the bound is that distance from the start, so the search covers
// every row at it (each once) and stops as the first one did or earlier; every such row receives the query's colour and one vote.
struct VoteScatter {
    unsigned long long d2;
    unsigned c[3];
    unsigned long long* sums;
    unsigned* votes;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d != d2) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(&sums[3 * (long long)r + k], (unsigned long long)c[k]);
        atomicAdd(&votes[r], 1u);
    }
    __device__ __forceinline__ unsigned long long bound() const { return d2; }
};

// One lane per record of A (Morton order) against B's index: two searches, the first for the distance, the second scatters.
__global__ void __launch_bounds__(256) k_vote(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                              const int4* __restrict__ recs, long long n, const int4* __restrict__ qrecs,
                                              const uint8_t* __restrict__ qcolours, long long nq, unsigned long long* __restrict__ sums,
                                              unsigned* __restrict__ votes) {
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        const TieVisitor<> best = search(g, qc, 0, TieVisitor<>());
        const long long row = q.w;
        VoteScatter sc;
        sc.d2 = best.d2;
#pragma unroll
        for (int k = 0; k < 3; ++k) sc.c[k] = qcolours[3 * row + k];
        sc.sums = sums;
        sc.votes = votes;
        search(g, qc, 0, sc);
    }
}

// One lane per record of B: the rounded mean of its votes, or of its own tie set in A's index when nobody voted for it.
__global__ void __launch_bounds__(256) k_transfer(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                                  const int4* __restrict__ recs, long long n, const uint8_t* __restrict__ colours,
                                                  const int4* __restrict__ qrecs, long long nq,
                                                  const unsigned long long* __restrict__ sums, const unsigned* __restrict__ votes,
                                                  uint8_t* __restrict__ out, int32_t* __restrict__ out_votes) {
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const long long row = q.w;
        const unsigned v = votes[row];
        unsigned long long s[3], cnt = v;
        if (v) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = sums[3 * row + k];
        } else {
            const int qc[3] = {q.x, q.y, q.z};
            TieSet init;
            init.over.colours = colours;
            const TieSet ties = search(g, qc, 0, init);
            cnt = ties.count;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = ties.over.s[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * row + k] = (uint8_t)((2 * s[k] + cnt) / (2 * cnt));
        if (out_votes) out_votes[row] = (int32_t)v;
    }
}

}  // namespace

PCC_API size_t pcc_cloud_transfer_workspace_bytes(int64_t na, int64_t nb) {
    if (!valid_n(na) || !valid_n(nb)) return 0;
    return transfer_layout(nb).total;
}

PCC_API int pcc_cloud_transfer_colors(pcc_ctx* ctx, const void* index_a, int64_t na, const uint8_t* a_colours, const void* index_b,
                                      int64_t nb, uint8_t* out_colours, int32_t* votes, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && index_a && a_colours && index_b && out_colours && workspace, "pcc_cloud_transfer_colors: NULL argument");
    PCC_REQUIRE(valid_n(na) && valid_n(nb), "pcc_cloud_transfer_colors: na = %lld, nb = %lld outside [1, 2^31)", (long long)na,
                (long long)nb);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const IndexView A = index_view(index_a, na), B = index_view(index_b, nb);
    const TransferLayout l = transfer_layout(nb);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long* sums = (unsigned long long*)(w + l.sums);
    unsigned* cnt = (unsigned*)(w + l.votes);
    PCC_CHECK_HIP(hipMemsetAsync(w, 0, l.total, st));
    hipLaunchKernelGGL(k_vote, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, a_colours, A.n,
                       sums, cnt);
    hipLaunchKernelGGL(k_transfer, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, A.hdr, A.codes, A.recs, A.n, a_colours, B.recs,
                       B.n, (const unsigned long long*)sums, (const unsigned*)cnt, out_colours, votes);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_cloud_map_colors(pcc_ctx* ctx, const void* index, int64_t npts, const uint8_t* colours, const void* query_index, int64_t nq,
                                 int32_t rank, uint8_t* out_colours, int32_t* rows, void* stream) {
    PCC_REQUIRE(ctx && index && colours && query_index && out_colours, "pcc_cloud_map_colors: NULL argument");
    PCC_REQUIRE(valid_n(npts) && valid_n(nq), "pcc_cloud_map_colors: npts = %lld, nq = %lld outside [1, 2^31)", (long long)npts,
                (long long)nq);
    PCC_REQUIRE(rank == 1 || rank == 2, "pcc_cloud_map_colors: rank = %d, must be 1 or 2", (int)rank);
    PCC_REQUIRE(npts >= rank, "pcc_cloud_map_colors: rank %d needs at least %d indexed points, got %lld", (int)rank, (int)rank,
                (long long)npts);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    const IndexView v = index_view(index, npts), q = index_view(query_index, nq);
    const dim3 grid((unsigned)((nq + 255) / 256));
    if (rank == 1)
        hipLaunchKernelGGL(k_map<1>, grid, dim3(256), 0, (hipStream_t)stream, v.hdr, v.codes, v.recs, v.n, colours, q.recs, q.n,
                           out_colours, rows);
    else
        hipLaunchKernelGGL(k_map<2>, grid, dim3(256), 0, (hipStream_t)stream, v.hdr, v.codes, v.recs, v.n, colours, q.recs, q.n,
                           out_colours, rows);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_cloud_color_workspace_bytes(int64_t na, int64_t nb) {
    if (!valid_n(na) || !valid_n(nb)) return 0;
    return color_layout(na, nb).total;
}

PCC_API int pcc_cloud_color_distortion(pcc_ctx* ctx, const void* index_a, int64_t na, const uint8_t* a_colours, const void* index_b,
                                       int64_t nb, const uint8_t* b_colours, double* tally, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && index_a && a_colours && index_b && b_colours && tally && workspace, "pcc_cloud_color_distortion: NULL argument");
    PCC_REQUIRE(valid_n(na) && valid_n(nb), "pcc_cloud_color_distortion: na = %lld, nb = %lld outside [1, 2^31)", (long long)na,
                (long long)nb);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const IndexView A = index_view(index_a, na), B = index_view(index_b, nb);
    const ColorLayout l = color_layout(na, nb);
    unsigned char* w = (unsigned char*)workspace;
    double *terms_a = (double*)(w + l.terms_a), *terms_b = (double*)(w + l.terms_b);
    double *pab = (double*)(w + l.pab), *pba = (double*)(w + l.pba);
    hipLaunchKernelGGL(k_cterms, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, b_colours, A.recs,
                       a_colours, A.n, terms_a);
    hipLaunchKernelGGL(k_cterms, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, A.hdr, A.codes, A.recs, A.n, a_colours, B.recs,
                       b_colours, B.n, terms_b);
    const int ta = tally_blocks(na), tb = tally_blocks(nb);
    hipLaunchKernelGGL(k_ctally, dim3(ta), dim3(256), 0, st, (const double*)terms_a, (long long)na, pab);
    hipLaunchKernelGGL(k_ctally, dim3(tb), dim3(256), 0, st, (const double*)terms_b, (long long)nb, pba);
    hipLaunchKernelGGL(k_cfinish, dim3(1), dim3(256), 0, st, (const double*)pab, ta, (const double*)pba, tb, tally);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
