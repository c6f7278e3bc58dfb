// Whole-cloud D1 / D2 distortion with Hausdorff terms (include/pcc_geo.h "cloud metrics", DESIGN.md "Cloud metrics on the GPU").
//
// Definition (pinned by tests/test_cloud_metrics_gpu.py against the numpy / scipy restatement in tests/_metrics_ref.py):
//   - clouds are integer points in [0, 2^21); the nearest indexed point of a query q is the row j with the smallest
//     (|p_j - q|^2, j) in lexicographic order: exact integer distances, ties to the lowest row (the normals kNN rule at k = 1);
//   - with A = original, B = decoded, to_b[i] = nearest B row of A point i, to_a[j] = nearest A row of B point j, the tally is
//     float64[9] = (N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA) as utils/pc_metric.pair_tally writes the first five:
//     D1 sums exact in 128-bit integers (converted once, correctly rounded), per-point D2 terms ((g.x*n.x + g.y*n.y) + g.z*n.z)^2
//     in float64 without contraction (the same bits as numpy), the H slots the maxima of the per-point D1 / D2 terms;
//   - the normal of decoded point j on the A->B side is pc_metric.transfer_normals: the mean of a_normals[i] over to_b[i] == j,
//     summed in float64 in increasing i, or a_normals[to_a[j]] when no original point links to j.
//
// Index: the cell index of cell_index.h, base level for two points per occupied cell.
// Query (k_query), one lane per query: the index search from Chebyshev radius 0, keeping the best (squared distance, row) pair.
// Tally: a stable radix sort of (to_b[i], i) makes every decoded point's original points a segment in increasing i (k_segments,
// k_bnormals: one sequential float64 sum per segment, numpy bincount's order); k_tally reduces each direction into per-block
// partials, k_finish adds the partials in a fixed order.  The only atomics are the index build's integer ones (bounding box,
// coordinate sums, histogram); nothing synchronises with the host: the same inputs give the same bits on every call.
#include <hipcub/hipcub.hpp>

#include "cell_index.h"

namespace {

constexpr int kTallyBlocks = 1024;    // upper bound of the partials of one direction (fixed per n: the sum order depends on n only)

struct Partial {                      // one workgroup's share of one direction
    unsigned long long d1_lo, d1_hi;  // exact sum of the squared distances (128 bits)
    unsigned long long h1;            // max squared distance
    double d2, h2;                    // sum / max of the per-point plane terms
};

// ---- query ---------------------------------------------------------------------------------------------------------------------

struct Nearest {                      // the lowest (squared distance, row) so far
    unsigned long long d2 = ~0ull;
    unsigned row = ~0u;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d < d2 || (d == d2 && r < row)) { d2 = d; row = r; }
    }
    __device__ __forceinline__ unsigned long long bound() const { return d2; }
};

// One lane per query.  RECS: the queries are another index's records (Morton order: a wave's lanes are neighbours in space, and
// the result goes to the record's row); otherwise row-order points.  Writes nn[row] and sqd[row] (either may be NULL).
template <bool RECS>
__global__ void __launch_bounds__(256) k_query(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                               const int4* __restrict__ recs, long long n, const int4* __restrict__ qrecs,
                                               const int32_t* __restrict__ qpts, long long nq, int32_t* __restrict__ nn,
                                               long long* __restrict__ sqd) {
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        int qc[3];
        long long row;
        if (RECS) {
            const int4 q = qrecs[t];
            qc[0] = q.x; qc[1] = q.y; qc[2] = q.z;
            row = q.w;
        } else {
            const int3 q = load_pt(qpts, t);
            qc[0] = q.x; qc[1] = q.y; qc[2] = q.z;
            row = t;
        }
        const Nearest best = search(g, qc, 0, Nearest());
        if (nn) nn[row] = (int32_t)best.row;
        if (sqd) sqd[row] = (long long)best.d2;
    }
}

// ---- tally ---------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_link_keys(const int32_t* __restrict__ to_b, long long na, unsigned* __restrict__ keys,
                                                   unsigned* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) { keys[i] = (unsigned)to_b[i]; vals[i] = (unsigned)i; }
}

// segment [lo[j], hi[j]) of the sorted links holds the original points whose nearest decoded point is j (both zero: none)
__global__ void __launch_bounds__(256) k_segments(const unsigned* __restrict__ keys, long long na, unsigned* __restrict__ lo,
                                                  unsigned* __restrict__ hi) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    const unsigned k = keys[t];
    if (t == 0 || keys[t - 1] != k) lo[k] = (unsigned)t;
    if (t == na - 1 || keys[t + 1] != k) hi[k] = (unsigned)(t + 1);
}

// pc_metric.transfer_normals: one sequential float64 sum per segment (increasing i, as bincount), divided by the count
__global__ void __launch_bounds__(256) k_bnormals(const unsigned* __restrict__ lo, const unsigned* __restrict__ hi,
                                                  const unsigned* __restrict__ vals, const double* __restrict__ an,
                                                  const int32_t* __restrict__ to_a, long long nb, double* __restrict__ bn) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const unsigned s = lo[j], e = hi[j];
    double acc[3] = {0.0, 0.0, 0.0}, votes = 1.0;
    if (e > s) {
        for (unsigned t = s; t < e; ++t) {
            const long long i = vals[t];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += an[3 * i + c];
        }
        votes = (double)(e - s);
    } else {
        const long long i = to_a[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += an[3 * i + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) bn[3 * j + c] = acc[c] / votes;
}

// ((gx*nx + gy*ny) + gz*nz)^2 rounded after every operation, numpy's order
__device__ __forceinline__ double plane_term(double gx, double gy, double gz, const double* __restrict__ nrm) {
#pragma clang fp contract(off)
    const double p = (gx * nrm[0] + gy * nrm[1]) + gz * nrm[2];
    return p * p;
}

// One direction: src point s links to dst row link[s]; nrm (NULL: no D2) is indexed by that row.  Grid-stride with a grid fixed by
// n: every per-thread sum visits the same points in the same order on every call.
__global__ void __launch_bounds__(256) k_tally(const int32_t* __restrict__ src, long long ns, const int32_t* __restrict__ dst,
                                               const int32_t* __restrict__ link, const long long* __restrict__ sqd,
                                               const double* __restrict__ nrm, Partial* __restrict__ out) {
    __shared__ unsigned __int128 s_d1[256];
    __shared__ unsigned long long s_h1[256];
    __shared__ double s_d2[256], s_h2[256];
    unsigned __int128 d1 = 0;
    unsigned long long h1 = 0;
    double d2 = 0.0, h2 = 0.0;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (long long)gridDim.x * blockDim.x) {
        const unsigned long long d = (unsigned long long)sqd[s];
        d1 += d;
        h1 = d > h1 ? d : h1;
        if (nrm) {
            const long long j = link[s];
            const double v = plane_term((double)(src[3 * s] - dst[3 * j]), (double)(src[3 * s + 1] - dst[3 * j + 1]),
                                        (double)(src[3 * s + 2] - dst[3 * j + 2]), nrm + 3 * j);
            d2 += v;
            h2 = v > h2 ? v : h2;
        }
    }
    const int t = threadIdx.x;
    s_d1[t] = d1; s_h1[t] = h1; s_d2[t] = d2; s_h2[t] = h2;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            s_d1[t] += s_d1[t + w];
            s_h1[t] = s_h1[t + w] > s_h1[t] ? s_h1[t + w] : s_h1[t];
            s_d2[t] += s_d2[t + w];
            s_h2[t] = s_h2[t + w] > s_h2[t] ? s_h2[t + w] : s_h2[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        Partial p;
        p.d1_lo = (unsigned long long)s_d1[0];
        p.d1_hi = (unsigned long long)(s_d1[0] >> 64);
        p.h1 = s_h1[0];
        p.d2 = s_d2[0];
        p.h2 = s_h2[0];
        out[blockIdx.x] = p;
    }
}

// correctly rounded double of a 128-bit unsigned integer
__device__ __forceinline__ double u128_to_double(unsigned __int128 v) {
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    if (!hi) return (double)lo;
    const int s = 64 - __clzll((long long)hi);                  // 1 .. 64: bits of hi
    const unsigned __int128 top = v >> s;                       // the highest 64 bits
    const unsigned long long sticky = (v & (((unsigned __int128)1 << s) - 1)) != 0;
    return ldexp((double)((unsigned long long)top | sticky), s);
}

// one workgroup: the partials of A->B (ga of them) and B->A (gb), each direction summed in a fixed order
__global__ void __launch_bounds__(256) k_finish(const Partial* __restrict__ pab, int ga, const Partial* __restrict__ pba, int gb,
                                                long long nb, double* __restrict__ tally) {
    __shared__ unsigned __int128 s_d1[2][256];
    __shared__ unsigned long long s_h1[2][256];
    __shared__ double s_d2[2][256], s_h2[2][256];
    const int t = threadIdx.x;
    for (int side = 0; side < 2; ++side) {
        const Partial* p = side ? pba : pab;
        const int g = side ? gb : ga;
        unsigned __int128 d1 = 0;
        unsigned long long h1 = 0;
        double d2 = 0.0, h2 = 0.0;
        for (int b = t; b < g; b += 256) {
            d1 += (unsigned __int128)p[b].d1_hi << 64 | p[b].d1_lo;
            h1 = p[b].h1 > h1 ? p[b].h1 : h1;
            d2 += p[b].d2;
            h2 = p[b].h2 > h2 ? p[b].h2 : h2;
        }
        s_d1[side][t] = d1; s_h1[side][t] = h1; s_d2[side][t] = d2; s_h2[side][t] = h2;
    }
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                s_d1[side][t] += s_d1[side][t + w];
                s_h1[side][t] = s_h1[side][t + w] > s_h1[side][t] ? s_h1[side][t + w] : s_h1[side][t];
                s_d2[side][t] += s_d2[side][t + w];
                s_h2[side][t] = s_h2[side][t + w] > s_h2[side][t] ? s_h2[side][t + w] : s_h2[side][t];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        tally[0] = (double)nb;
        tally[1] = u128_to_double(s_d1[0][0]);
        tally[2] = u128_to_double(s_d1[1][0]);
        tally[3] = s_d2[0][0];
        tally[4] = s_d2[1][0];
        tally[5] = (double)s_h1[0][0];
        tally[6] = (double)s_h1[1][0];
        tally[7] = s_h2[0][0];
        tally[8] = s_h2[1][0];
    }
}

// ---- tie-averaged D2 (pcc_cloud_distortion_ties, tie_mode mean; DESIGN.md "Tie-averaged D2") --------------------------------------
// A -> B: k_tie_count counts every original point's tie set T_B(a), an exclusive scan places it, k_tie_emit writes its (b, a) pairs
// (a second search with the known smallest distance as its bound), the stable sort by b makes every decoded point's votes a segment
// in increasing a, k_bnormals_ties averages them (or takes the orphan mean of k_tie_ba), k_terms_ab walks each point's own pairs.
// B -> A: one search, k_tie_ba, whose visitor accumulates the plane terms and the normals of T_A(b) as it meets them.
// The pair count is only known on the device: k_total compares it with the caller's capacity; past it every later kernel returns
// early and k_overflow turns the D2 / H2 slots into NaN (status tells the caller the capacity to come back with).

struct TieCtl {                       // written by k_total
    unsigned long long pairs;         // sum of |T_B(a)| over the original points
    int overflow;                     // pairs > capacity: nothing below k_total touches the pair arrays
};

// ((gx*nx + gy*ny) + gz*nz)^2 rounded after every operation, as plane_term (kept apart so the kernels of the default rule compile
// from the same text as before)
__device__ __forceinline__ double tie_plane_term(double gx, double gy, double gz, const double* __restrict__ nrm) {
#pragma clang fp contract(off)
    const double p = (gx * nrm[0] + gy * nrm[1]) + gz * nrm[2];
    return p * p;
}

struct TieCount {                     // the size of the tie set so far and its lowest row
    unsigned long long d2 = ~0ull;
    unsigned count = 0, row = ~0u;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d > d2) return;
        if (d < d2) { d2 = d; count = 0; row = ~0u; }
        ++count;
        row = r < row ? r : row;
    }
    __device__ __forceinline__ unsigned long long bound() const { return d2; }
};

struct TieEmit {                      // writes the rows at squared distance `target` (the smallest, known from k_tie_count)
    unsigned* out;
    unsigned long long target;
    unsigned cap, n = 0;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d == target && n < cap) out[n++] = r;
    }
    __device__ __forceinline__ unsigned long long bound() const { return target; }
};

struct TiePlane {                     // over the tie set so far: sum of e(q - p_r, nrm[r]), sum of nrm[r], count, lowest row
    const int32_t* pts;               // the indexed cloud in row order
    const double* nrm;                // its normals
    int q[3];
    unsigned long long d2 = ~0ull;
    unsigned count = 0, row = ~0u;
    double e = 0.0, s[3] = {0.0, 0.0, 0.0};
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
#pragma clang fp contract(off)
        if (d > d2) return;
        if (d < d2) { d2 = d; count = 0; row = ~0u; e = 0.0; s[0] = s[1] = s[2] = 0.0; }
        ++count;
        row = r < row ? r : row;
        const long long j = r;
        const double* n = nrm + 3 * j;
        e += tie_plane_term((double)(q[0] - pts[3 * j]), (double)(q[1] - pts[3 * j + 1]), (double)(q[2] - pts[3 * j + 2]), n);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += n[c];
    }
    __device__ __forceinline__ unsigned long long bound() const { return d2; }
};

// One lane per original point (A's records, Morton order) against B's index: nn[row] the lowest tied row, sqd[row], cnt[row] = |T_B|.
__global__ void __launch_bounds__(256) k_tie_count(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                                   const int4* __restrict__ recs, long long n, const int4* __restrict__ qrecs, long long nq,
                                                   int32_t* __restrict__ nn, long long* __restrict__ sqd,
                                                   unsigned long long* __restrict__ cnt) {
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        const TieCount best = search(g, qc, 0, TieCount());
        const long long row = q.w;
        nn[row] = (int32_t)best.row;
        sqd[row] = (long long)best.d2;
        cnt[row] = best.count;
    }
}

__global__ void k_total(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off, long long na,
                        unsigned long long cap, TieCtl* __restrict__ ctl, long long* __restrict__ status) {
    const unsigned long long pairs = off[na - 1] + cnt[na - 1];
    ctl->pairs = pairs;
    ctl->overflow = pairs > cap;
    status[0] = (long long)pairs;
    status[1] = pairs > cap;
}

// The pairs of original point `row` at [off[row], off[row] + cnt[row]): keys = the tied decoded rows in visiting order, vals = row.
__global__ void __launch_bounds__(256) k_tie_emit(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                                  const int4* __restrict__ recs, long long n, const int4* __restrict__ qrecs, long long nq,
                                                  const long long* __restrict__ sqd, const unsigned long long* __restrict__ cnt,
                                                  const unsigned long long* __restrict__ off, const TieCtl* __restrict__ ctl,
                                                  unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    if (ctl->overflow) return;
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        const long long row = q.w;
        const unsigned long long o = off[row];
        TieEmit init;
        init.out = keys + o;
        init.target = (unsigned long long)sqd[row];
        init.cap = (unsigned)cnt[row];
        const TieEmit done = search(g, qc, 0, init);
        for (unsigned k = 0; k < done.n; ++k) vals[o + k] = (unsigned)row;
    }
}

// the unused tail of the pair arrays sorts behind every decoded row (key nb)
__global__ void __launch_bounds__(256) k_tie_pad(const TieCtl* __restrict__ ctl, unsigned long long cap, unsigned nb,
                                                 unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    if (ctl->overflow) return;
    const unsigned long long t = ctl->pairs + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cap) { keys[t] = nb; vals[t] = 0; }
}

__global__ void __launch_bounds__(256) k_segments_ties(const unsigned* __restrict__ keys, const TieCtl* __restrict__ ctl, unsigned nb,
                                                       unsigned* __restrict__ lo, unsigned* __restrict__ hi) {
    if (ctl->overflow) return;
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ctl->pairs) return;
    const unsigned k = keys[t];
    if (k >= nb) return;
    if (t == 0 || keys[t - 1] != k) lo[k] = (unsigned)t;
    if (t == ctl->pairs - 1 || keys[t + 1] != k) hi[k] = (unsigned)(t + 1);
}

// One lane per decoded point (B's records) against A's index: nn / sqd as k_tie_count, terms[row] = the mean plane term over T_A(b),
// orphan[3 * row ..] = the mean original normal over T_A(b) (the decoded point's normal when nobody votes for it).
__global__ void __launch_bounds__(256) k_tie_ba(const IndexHdr* __restrict__ H, const unsigned long long* __restrict__ codes,
                                                const int4* __restrict__ recs, long long n, const int32_t* __restrict__ pts,
                                                const double* __restrict__ nrm, const int4* __restrict__ qrecs, long long nq,
                                                int32_t* __restrict__ nn, long long* __restrict__ sqd, double* __restrict__ terms,
                                                double* __restrict__ orphan) {
#pragma clang fp contract(off)
    const Cells g = cells(H, codes, recs, n);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const int qc[3] = {q.x, q.y, q.z};
        TiePlane init;
        init.pts = pts;
        init.nrm = nrm;
        init.q[0] = q.x; init.q[1] = q.y; init.q[2] = q.z;
        const TiePlane ties = search(g, qc, 0, init);
        const long long row = q.w;
        const double c = (double)ties.count;
        nn[row] = (int32_t)ties.row;
        sqd[row] = (long long)ties.d2;
        terms[row] = ties.e / c;
#pragma unroll
        for (int k = 0; k < 3; ++k) orphan[3 * row + k] = ties.s[k] / c;
    }
}

// the normal of decoded point j: the mean of its votes' normals (one sequential float64 sum in increasing a), else its orphan mean
__global__ void __launch_bounds__(256) k_bnormals_ties(const unsigned* __restrict__ lo, const unsigned* __restrict__ hi,
                                                       const unsigned* __restrict__ vals, const double* __restrict__ an,
                                                       const double* __restrict__ orphan, const TieCtl* __restrict__ ctl, long long nb,
                                                       double* __restrict__ bn) {
#pragma clang fp contract(off)
    if (ctl->overflow) return;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const unsigned s = lo[j], e = hi[j];
    if (e > s) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (unsigned t = s; t < e; ++t) {
            const long long i = vals[t];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += an[3 * i + c];
        }
        const double votes = (double)(e - s);
#pragma unroll
        for (int c = 0; c < 3; ++c) bn[3 * j + c] = acc[c] / votes;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) bn[3 * j + c] = orphan[3 * j + c];
    }
}

// One lane per original point (A's records): terms[row] = the mean of e(a - b, bn[b]) over its own pairs, in their emitted order.
__global__ void __launch_bounds__(256) k_terms_ab(const int4* __restrict__ qrecs, long long nq, const int32_t* __restrict__ bpts,
                                                  const double* __restrict__ bn, const unsigned* __restrict__ keys,
                                                  const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                                  const TieCtl* __restrict__ ctl, double* __restrict__ terms) {
#pragma clang fp contract(off)
    if (ctl->overflow) return;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (long long)gridDim.x * blockDim.x) {
        const int4 q = qrecs[t];
        const long long row = q.w;
        const unsigned long long o = off[row], c = cnt[row];
        double e = 0.0;
        for (unsigned long long k = 0; k < c; ++k) {
            const long long j = keys[o + k];
            e += tie_plane_term((double)(q.x - bpts[3 * j]), (double)(q.y - bpts[3 * j + 1]), (double)(q.z - bpts[3 * j + 2]), bn + 3 * j);
        }
        terms[row] = e / (double)c;
    }
}

// k_tally over per-point terms that are already computed (NULL: no D2): the same grid rule, per-thread order and tree
__global__ void __launch_bounds__(256) k_tally_terms(long long ns, const long long* __restrict__ sqd, const double* __restrict__ terms,
                                                     Partial* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ unsigned __int128 s_d1[256];
    __shared__ unsigned long long s_h1[256];
    __shared__ double s_d2[256], s_h2[256];
    unsigned __int128 d1 = 0;
    unsigned long long h1 = 0;
    double d2 = 0.0, h2 = 0.0;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (long long)gridDim.x * blockDim.x) {
        const unsigned long long d = (unsigned long long)sqd[s];
        d1 += d;
        h1 = d > h1 ? d : h1;
        if (terms) {
            const double v = terms[s];
            d2 += v;
            h2 = v > h2 ? v : h2;
        }
    }
    const int t = threadIdx.x;
    s_d1[t] = d1; s_h1[t] = h1; s_d2[t] = d2; s_h2[t] = h2;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            s_d1[t] += s_d1[t + w];
            s_h1[t] = s_h1[t + w] > s_h1[t] ? s_h1[t + w] : s_h1[t];
            s_d2[t] += s_d2[t + w];
            s_h2[t] = s_h2[t + w] > s_h2[t] ? s_h2[t + w] : s_h2[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        Partial p;
        p.d1_lo = (unsigned long long)s_d1[0];
        p.d1_hi = (unsigned long long)(s_d1[0] >> 64);
        p.h1 = s_h1[0];
        p.d2 = s_d2[0];
        p.h2 = s_h2[0];
        out[blockIdx.x] = p;
    }
}

// past the pair capacity the D2 / H2 slots say so instead of holding numbers made from unwritten pairs
__global__ void k_overflow(const TieCtl* __restrict__ ctl, double* __restrict__ tally) {
    if (!ctl->overflow) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    tally[3] = nan; tally[4] = nan; tally[7] = nan; tally[8] = nan;
}

int tally_blocks(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < kTallyBlocks ? b : kTallyBlocks);
}

int key_bits(long long nb) {                    // bits of the largest decoded row, nb - 1 (at least 1)
    int bits = 1;
    while (bits < 31 && ((long long)1 << bits) < nb) ++bits;
    return bits;
}

struct DistLayout {
    size_t nn_ab, d_ab, nn_ba, d_ba, keys0, vals0, keys1, vals1, seg_lo, seg_hi, bn, pab, pba, sort_tmp, sort_tmp_bytes, total;
};

DistLayout dist_layout(long long na, long long nb) {
    DistLayout l;
    const size_t A = (size_t)na, B = (size_t)nb;
    size_t o = 0;
    l.nn_ab = o; o += al256(A * 4);
    l.d_ab = o; o += al256(A * 8);
    l.nn_ba = o; o += al256(B * 4);
    l.d_ba = o; o += al256(B * 8);
    l.keys0 = o; o += al256(A * 4);
    l.vals0 = o; o += al256(A * 4);
    l.keys1 = o; o += al256(A * 4);
    l.vals1 = o; o += al256(A * 4);
    l.seg_lo = o; o += al256(B * 4);
    l.seg_hi = o; o += al256(B * 4);
    l.bn = o; o += al256(B * 24);
    l.pab = o; o += al256(kTallyBlocks * sizeof(Partial));
    l.pba = o; o += al256(kTallyBlocks * sizeof(Partial));
    size_t tmp = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, tmp, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                             (unsigned*)nullptr, (int)(na > 0 ? na : 1), 0, key_bits(nb), (hipStream_t)0);
    l.sort_tmp_bytes = tmp;
    l.sort_tmp = o; o += al256(tmp + 256);
    l.total = o;
    return l;
}

struct TieLayout {
    size_t nn_ab, d_ab, nn_ba, d_ba, cnt, off, keys0, vals0, keys1, vals1, seg_lo, seg_hi, bn, orphan, terms_a, terms_b, pab, pba, ctl,
        scan_tmp, scan_tmp_bytes, sort_tmp, sort_tmp_bytes, total;
};

TieLayout tie_layout(long long na, long long nb, long long cap) {
    TieLayout l;
    const size_t A = (size_t)na, B = (size_t)nb, P = (size_t)cap;
    size_t o = 0;
    l.nn_ab = o; o += al256(A * 4);
    l.d_ab = o; o += al256(A * 8);
    l.nn_ba = o; o += al256(B * 4);
    l.d_ba = o; o += al256(B * 8);
    l.cnt = o; o += al256(A * 8);
    l.off = o; o += al256(A * 8);
    l.keys0 = o; o += al256(P * 4);
    l.vals0 = o; o += al256(P * 4);
    l.keys1 = o; o += al256(P * 4);
    l.vals1 = o; o += al256(P * 4);
    l.seg_lo = o; o += al256(B * 4);
    l.seg_hi = o; o += al256(B * 4);
    l.bn = o; o += al256(B * 24);
    l.orphan = o; o += al256(B * 24);
    l.terms_a = o; o += al256(A * 8);
    l.terms_b = o; o += al256(B * 8);
    l.pab = o; o += al256(kTallyBlocks * sizeof(Partial));
    l.pba = o; o += al256(kTallyBlocks * sizeof(Partial));
    l.ctl = o; o += al256(sizeof(TieCtl));
    size_t tmp = 0;
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)na,
                                           (hipStream_t)0);
    l.scan_tmp_bytes = tmp;
    l.scan_tmp = o; o += al256(tmp + 256);
    tmp = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, tmp, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                             (unsigned*)nullptr, (int)cap, 0, key_bits(nb + 1), (hipStream_t)0);
    l.sort_tmp_bytes = tmp;
    l.sort_tmp = o; o += al256(tmp + 256);
    l.total = o;
    return l;
}

bool valid_n(int64_t n) { return n > 0 && n < ((int64_t)1 << 31); }

}  // namespace

PCC_API size_t pcc_cloud_index_bytes(int64_t npts) {
    if (!valid_n(npts)) return 0;
    return index_layout(npts).total;
}

PCC_API int pcc_cloud_index_build(pcc_ctx* ctx, const int32_t* pts, int64_t npts, void* index, void* stream) {
    PCC_REQUIRE(ctx && pts && index, "pcc_cloud_index_build: NULL argument");
    PCC_REQUIRE(valid_n(npts), "pcc_cloud_index_build: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    return index_build(ctx, pts, npts, index, 4, (hipStream_t)stream);
}

PCC_API int pcc_cloud_nearest(pcc_ctx* ctx, const void* index, int64_t npts, const int32_t* queries, int64_t nq, int32_t* nn,
                              int64_t* sqdist, void* stream) {
    PCC_REQUIRE(ctx && index && queries, "pcc_cloud_nearest: NULL argument");
    PCC_REQUIRE(valid_n(npts), "pcc_cloud_nearest: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31), "pcc_cloud_nearest: nq = %lld outside [0, 2^31)", (long long)nq);
    if (nq == 0) return PCC_OK;
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    const IndexView v = index_view(index, npts);
    hipLaunchKernelGGL(k_query<false>, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v.hdr, v.codes, v.recs,
                       v.n, (const int4*)nullptr, queries, (long long)nq, nn, (long long*)sqdist);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_cloud_distortion_workspace_bytes(int64_t na, int64_t nb) {
    if (!valid_n(na) || !valid_n(nb)) return 0;
    return dist_layout(na, nb).total;
}

PCC_API int pcc_cloud_distortion(pcc_ctx* ctx, const void* index_a, int64_t na, const void* index_b, int64_t nb, const double* a_normals,
                                 double* tally, int32_t* to_b, int32_t* to_a, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && index_a && index_b && tally && workspace, "pcc_cloud_distortion: NULL argument");
    PCC_REQUIRE(valid_n(na) && valid_n(nb), "pcc_cloud_distortion: na = %lld, nb = %lld outside [1, 2^31)", (long long)na, (long long)nb);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const IndexView A = index_view(index_a, na), B = index_view(index_b, nb);
    const DistLayout l = dist_layout(na, nb);
    unsigned char* w = (unsigned char*)workspace;
    int32_t* nn_ab = to_b ? to_b : (int32_t*)(w + l.nn_ab);
    int32_t* nn_ba = to_a ? to_a : (int32_t*)(w + l.nn_ba);
    long long *d_ab = (long long*)(w + l.d_ab), *d_ba = (long long*)(w + l.d_ba);
    Partial *pab = (Partial*)(w + l.pab), *pba = (Partial*)(w + l.pba);
    const unsigned ga = (unsigned)((na + 255) / 256), gb = (unsigned)((nb + 255) / 256);
    // queries in the other index's Morton order
    hipLaunchKernelGGL(k_query<true>, dim3(ga), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, (const int32_t*)nullptr, A.n,
                       nn_ab, d_ab);
    hipLaunchKernelGGL(k_query<true>, dim3(gb), dim3(256), 0, st, A.hdr, A.codes, A.recs, A.n, B.recs, (const int32_t*)nullptr, B.n,
                       nn_ba, d_ba);
    const double* bn = nullptr;
    if (a_normals) {
        unsigned *keys0 = (unsigned*)(w + l.keys0), *vals0 = (unsigned*)(w + l.vals0);
        unsigned *keys1 = (unsigned*)(w + l.keys1), *vals1 = (unsigned*)(w + l.vals1);
        unsigned *seg_lo = (unsigned*)(w + l.seg_lo), *seg_hi = (unsigned*)(w + l.seg_hi);
        hipLaunchKernelGGL(k_link_keys, dim3(ga), dim3(256), 0, st, (const int32_t*)nn_ab, (long long)na, keys0, vals0);
        size_t tmp = l.sort_tmp_bytes;                     // LSD radix sort: stable, so every segment stays in increasing i
        PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.sort_tmp), tmp, (const unsigned*)keys0, keys1, (const unsigned*)vals0,
                                                         vals1, (int)na, 0, key_bits(nb), st));
        PCC_CHECK_HIP(hipMemsetAsync(seg_lo, 0, (size_t)nb * 4, st));
        PCC_CHECK_HIP(hipMemsetAsync(seg_hi, 0, (size_t)nb * 4, st));
        hipLaunchKernelGGL(k_segments, dim3(ga), dim3(256), 0, st, (const unsigned*)keys1, (long long)na, seg_lo, seg_hi);
        hipLaunchKernelGGL(k_bnormals, dim3(gb), dim3(256), 0, st, (const unsigned*)seg_lo, (const unsigned*)seg_hi, (const unsigned*)vals1,
                           a_normals, (const int32_t*)nn_ba, (long long)nb, (double*)(w + l.bn));
        bn = (const double*)(w + l.bn);
    }
    const int ta = tally_blocks(na), tb = tally_blocks(nb);
    hipLaunchKernelGGL(k_tally, dim3(ta), dim3(256), 0, st, A.pts, (long long)na, B.pts, (const int32_t*)nn_ab, (const long long*)d_ab, bn, pab);
    hipLaunchKernelGGL(k_tally, dim3(tb), dim3(256), 0, st, B.pts, (long long)nb, A.pts, (const int32_t*)nn_ba, (const long long*)d_ba,
                       a_normals, pba);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, st, (const Partial*)pab, ta, (const Partial*)pba, tb, (long long)nb, tally);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_cloud_distortion_ties_workspace_bytes(int64_t na, int64_t nb, int32_t tie_mode, int64_t max_pairs) {
    if (!valid_n(na) || !valid_n(nb)) return 0;
    if (tie_mode == PCC_TIES_PICK) return dist_layout(na, nb).total;
    if (tie_mode != PCC_TIES_MEAN || !valid_n(max_pairs)) return 0;
    const size_t pick = dist_layout(na, nb).total, mean = tie_layout(na, nb, max_pairs).total;      // without normals mean runs pick's pass
    return mean > pick ? mean : pick;
}

PCC_API int pcc_cloud_distortion_ties(pcc_ctx* ctx, const void* index_a, int64_t na, const void* index_b, int64_t nb, const double* a_normals,
                                      int32_t tie_mode, int64_t max_pairs, double* tally, int64_t* status, int32_t* to_b, int32_t* to_a,
                                      void* workspace, void* stream) {
    PCC_REQUIRE(ctx && index_a && index_b && tally && status && workspace, "pcc_cloud_distortion_ties: NULL argument");
    PCC_REQUIRE(valid_n(na) && valid_n(nb), "pcc_cloud_distortion_ties: na = %lld, nb = %lld outside [1, 2^31)", (long long)na,
                (long long)nb);
    PCC_REQUIRE(tie_mode == PCC_TIES_PICK || tie_mode == PCC_TIES_MEAN, "pcc_cloud_distortion_ties: tie_mode = %d, must be 0 (pick) or 1 (mean)",
                (int)tie_mode);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (tie_mode == PCC_TIES_PICK || !a_normals) {      // the D1 / H1 slots do not depend on the rule: no pairs without normals
        PCC_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st));
        return pcc_cloud_distortion(ctx, index_a, na, index_b, nb, a_normals, tally, to_b, to_a, workspace, stream);
    }
    PCC_REQUIRE(valid_n(max_pairs), "pcc_cloud_distortion_ties: max_pairs = %lld outside [1, 2^31)", (long long)max_pairs);
    const IndexView A = index_view(index_a, na), B = index_view(index_b, nb);
    const TieLayout l = tie_layout(na, nb, max_pairs);
    unsigned char* w = (unsigned char*)workspace;
    int32_t* nn_ab = to_b ? to_b : (int32_t*)(w + l.nn_ab);
    int32_t* nn_ba = to_a ? to_a : (int32_t*)(w + l.nn_ba);
    long long *d_ab = (long long*)(w + l.d_ab), *d_ba = (long long*)(w + l.d_ba);
    unsigned long long *cnt = (unsigned long long*)(w + l.cnt), *off = (unsigned long long*)(w + l.off);
    unsigned *keys0 = (unsigned*)(w + l.keys0), *vals0 = (unsigned*)(w + l.vals0);
    unsigned *keys1 = (unsigned*)(w + l.keys1), *vals1 = (unsigned*)(w + l.vals1);
    unsigned *seg_lo = (unsigned*)(w + l.seg_lo), *seg_hi = (unsigned*)(w + l.seg_hi);
    double *bn = (double*)(w + l.bn), *orphan = (double*)(w + l.orphan);
    double *terms_a = (double*)(w + l.terms_a), *terms_b = (double*)(w + l.terms_b);
    Partial *pab = (Partial*)(w + l.pab), *pba = (Partial*)(w + l.pba);
    TieCtl* ctl = (TieCtl*)(w + l.ctl);
    const unsigned long long cap = (unsigned long long)max_pairs;
    const unsigned ga = (unsigned)((na + 255) / 256), gb = (unsigned)((nb + 255) / 256), gp = (unsigned)((cap + 255) / 256);
    hipLaunchKernelGGL(k_tie_count, dim3(ga), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, A.n, nn_ab, d_ab, cnt);
    hipLaunchKernelGGL(k_tie_ba, dim3(gb), dim3(256), 0, st, A.hdr, A.codes, A.recs, A.n, A.pts, a_normals, B.recs, B.n, nn_ba, d_ba,
                       terms_b, orphan);
    size_t tmp = l.scan_tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum((void*)(w + l.scan_tmp), tmp, (const unsigned long long*)cnt, off, (int)na, st));
    hipLaunchKernelGGL(k_total, dim3(1), dim3(1), 0, st, (const unsigned long long*)cnt, (const unsigned long long*)off, (long long)na, cap,
                       ctl, (long long*)status);
    hipLaunchKernelGGL(k_tie_emit, dim3(ga), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, A.n, (const long long*)d_ab,
                       (const unsigned long long*)cnt, (const unsigned long long*)off, (const TieCtl*)ctl, keys0, vals0);
    hipLaunchKernelGGL(k_tie_pad, dim3(gp), dim3(256), 0, st, (const TieCtl*)ctl, cap, (unsigned)nb, keys0, vals0);
    tmp = l.sort_tmp_bytes;                                // LSD radix sort: stable, so every segment stays in increasing a
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.sort_tmp), tmp, (const unsigned*)keys0, keys1, (const unsigned*)vals0,
                                                     vals1, (int)cap, 0, key_bits(nb + 1), st));
    PCC_CHECK_HIP(hipMemsetAsync(seg_lo, 0, (size_t)nb * 4, st));
    PCC_CHECK_HIP(hipMemsetAsync(seg_hi, 0, (size_t)nb * 4, st));
    hipLaunchKernelGGL(k_segments_ties, dim3(gp), dim3(256), 0, st, (const unsigned*)keys1, (const TieCtl*)ctl, (unsigned)nb, seg_lo, seg_hi);
    hipLaunchKernelGGL(k_bnormals_ties, dim3(gb), dim3(256), 0, st, (const unsigned*)seg_lo, (const unsigned*)seg_hi, (const unsigned*)vals1,
                       a_normals, (const double*)orphan, (const TieCtl*)ctl, (long long)nb, bn);
    hipLaunchKernelGGL(k_terms_ab, dim3(ga), dim3(256), 0, st, A.recs, A.n, B.pts, (const double*)bn, (const unsigned*)keys0,
                       (const unsigned long long*)cnt, (const unsigned long long*)off, (const TieCtl*)ctl, terms_a);
    const int ta = tally_blocks(na), tb = tally_blocks(nb);
    hipLaunchKernelGGL(k_tally_terms, dim3(ta), dim3(256), 0, st, (long long)na, (const long long*)d_ab, (const double*)terms_a, pab);
    hipLaunchKernelGGL(k_tally_terms, dim3(tb), dim3(256), 0, st, (long long)nb, (const long long*)d_ba, (const double*)terms_b, pba);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, st, (const Partial*)pab, ta, (const Partial*)pba, tb, (long long)nb, tally);
    hipLaunchKernelGGL(k_overflow, dim3(1), dim3(1), 0, st, (const TieCtl*)ctl, tally);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
