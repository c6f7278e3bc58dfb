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
// partials, k_finish adds the partials in a fixed order (the grid and the tree of cloud_tally.h).  The only atomics are the index build's integer ones (bounding box,
// coordinate sums, histogram); nothing synchronises with the host: the same inputs give the same bits on every call.
#include <hipcub/hipcub.hpp>

#include "cell_index.h"
#include "cloud_tally.h"

namespace {

struct Partial {                      // one direction's sums and maxima: a thread's, a workgroup's (in the workspace), the cloud's
    unsigned long long d1_lo, d1_hi;  // exact sum of the squared distances (128 bits)
    unsigned long long h1;            // max squared distance
    double d2, h2;                    // sum / max of the per-point plane terms
    __device__ __forceinline__ static Partial zero() { return Partial{0, 0, 0, 0.0, 0.0}; }
    __device__ __forceinline__ unsigned __int128 d1() const { return (unsigned __int128)d1_hi << 64 | d1_lo; }
    __device__ __forceinline__ void add_d1(unsigned __int128 v) {
        v += d1();
        d1_lo = (unsigned long long)v;
        d1_hi = (unsigned long long)(v >> 64);
    }
    __device__ __forceinline__ void distance(unsigned long long d) { add_d1(d); h1 = d > h1 ? d : h1; }
    __device__ __forceinline__ void term(double v) { d2 += v; h2 = v > h2 ? v : h2; }
};
struct Merge {
    __device__ __forceinline__ Partial operator()(Partial a, const Partial& b) const {
        a.add_d1(b.d1());
        a.h1 = b.h1 > a.h1 ? b.h1 : a.h1;
        a.d2 += b.d2;
        a.h2 = b.h2 > a.h2 ? b.h2 : a.h2;
        return a;
    }
};

// ---- query ---------------------------------------------------------------------------------------------------------------------

using Nearest = TieVisitor<>;         // the lowest (squared distance, row): the tie set's lowest row, its count unused

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

// How many sorted (decoded row, original row) pairs there are: all na links of the default rule, or the device's count of tie pairs
// (then the tail of the arrays is padding with key nb, and past the capacity nothing is done).
struct AllLinks {
    static constexpr bool kPadded = false;
    long long n;
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ unsigned long long count() const { return (unsigned long long)n; }
};
struct TiePairs {
    static constexpr bool kPadded = true;
    const TieCtl* ctl;
    __device__ __forceinline__ bool live() const { return !ctl->overflow; }
    __device__ __forceinline__ unsigned long long count() const { return ctl->pairs; }
};

// segment [lo[j], hi[j]) of the sorted pairs holds the original points that link to (vote for) decoded point j (both zero: none)
template <class Pairs>
__global__ void __launch_bounds__(256) k_segments(const unsigned* __restrict__ keys, Pairs pairs, unsigned nb, unsigned* __restrict__ lo,
                                                  unsigned* __restrict__ hi) {
    if (!pairs.live()) return;
    const unsigned long long n = pairs.count(), t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned k = keys[t];
    if (Pairs::kPadded && k >= nb) return;
    if (t == 0 || keys[t - 1] != k) lo[k] = (unsigned)t;
    if (t == n - 1 || keys[t + 1] != k) hi[k] = (unsigned)(t + 1);
}

// The normal of a decoded point nobody links to.  Default rule: that of its nearest original point, through the sum and the division
// of a one-vote segment ((0.0 + n) / 1.0: -0.0 becomes +0.0).  Tie-averaged: the mean over T_A(b) that k_tie_ba left, copied as is.
struct OrphanNearest {
    const double* an;
    const int32_t* to_a;
    __device__ __forceinline__ bool live() const { return true; }
    __device__ __forceinline__ double get(long long j, int c) const { return (0.0 + an[3 * (long long)to_a[j] + c]) / 1.0; }
};
struct OrphanMean {
    const double* orphan;
    const TieCtl* ctl;
    __device__ __forceinline__ bool live() const { return !ctl->overflow; }
    __device__ __forceinline__ double get(long long j, int c) const { return orphan[3 * j + c]; }
};

// pc_metric.transfer_normals: one sequential float64 sum per segment (increasing original row, as bincount), divided by the count
template <class Orphan>
__global__ void __launch_bounds__(256) k_bnormals(const unsigned* __restrict__ lo, const unsigned* __restrict__ hi,
                                                  const unsigned* __restrict__ vals, const double* __restrict__ an, Orphan orphan,
                                                  long long nb, double* __restrict__ bn) {
#pragma clang fp contract(off)
    if (!orphan.live()) return;
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
        for (int c = 0; c < 3; ++c) bn[3 * j + c] = orphan.get(j, c);
    }
}

// Where the plane term of point s of one direction comes from.  LinkTerm: src point s links to dst row link[s], nrm is indexed by
// that row.  StoredTerm: computed already.  Either with a NULL array: no D2.
struct LinkTerm {
    const int32_t *src, *dst, *link;
    const double* nrm;
    __device__ __forceinline__ bool any() const { return nrm != nullptr; }
    __device__ __forceinline__ double operator()(long long s) const {
        const long long j = link[s];
        const double* n = nrm + 3 * j;
        return plane_term((double)(src[3 * s] - dst[3 * j]), (double)(src[3 * s + 1] - dst[3 * j + 1]),
                          (double)(src[3 * s + 2] - dst[3 * j + 2]), n[0], n[1], n[2]);
    }
};
struct StoredTerm {
    const double* terms;
    __device__ __forceinline__ bool any() const { return terms != nullptr; }
    __device__ __forceinline__ double operator()(long long s) const { return terms[s]; }
};

// One direction over tally_blocks(ns) workgroups: out[block] = its share
template <class Term>
__global__ void __launch_bounds__(256) k_tally(long long ns, const long long* __restrict__ sqd, Term term, Partial* __restrict__ out) {
    __shared__ Partial sh[256];
    Partial acc = Partial::zero();
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (long long)gridDim.x * blockDim.x) {
        acc.distance((unsigned long long)sqd[s]);
        if (term.any()) acc.term(term(s));
    }
    const Partial sum = tree256(acc, sh, Merge());
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
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
    __shared__ Slots<Partial, 2> sh[256];
    Slots<Partial, 2> acc;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const Partial* p = side ? pba : pab;
        const int g = side ? gb : ga;
        acc.v[side] = Partial::zero();
        for (int b = threadIdx.x; b < g; b += 256) acc.v[side] = Merge()(acc.v[side], p[b]);
    }
    const Slots<Partial, 2> sum = tree256(acc, sh, EachSlot<Merge>());
    if (threadIdx.x == 0) {
        tally[0] = (double)nb;
        tally[1] = u128_to_double(sum.v[0].d1());
        tally[2] = u128_to_double(sum.v[1].d1());
        tally[3] = sum.v[0].d2;
        tally[4] = sum.v[1].d2;
        tally[5] = (double)sum.v[0].h1;
        tally[6] = (double)sum.v[1].h1;
        tally[7] = sum.v[0].h2;
        tally[8] = sum.v[1].h2;
    }
}

// ---- tie-averaged D2 (pcc_cloud_distortion_ties, tie_mode mean; DESIGN.md "Tie-averaged D2") --------------------------------------
// A -> B: k_tie_count counts every original point's tie set T_B(a), an exclusive scan places it, k_tie_emit writes its (b, a) pairs
// (a second search with the known smallest distance as its bound), the stable sort by b makes every decoded point's votes a segment
// in increasing a, k_bnormals averages them (or takes the orphan mean of k_tie_ba), k_terms_ab walks each point's own pairs.
// B -> A: one search, k_tie_ba, whose visitor accumulates the plane terms and the normals of T_A(b) as it meets them.
// The pair list is cloud_tally.h's: past the capacity every later kernel returns early and k_pair_nan turns the D2 / H2 slots into NaN
// (status tells the caller the capacity to come back with).

using TieCount = TieVisitor<>;        // the size of the tie set and its lowest row

struct TieEmit {                      // writes the rows at squared distance `target` (the smallest, known from k_tie_count)
    unsigned* out;
    unsigned long long target;
    unsigned cap, n = 0;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d == target && n < cap) out[n++] = r;
    }
    __device__ __forceinline__ unsigned long long bound() const { return target; }
};

struct PlaneSums {                    // over the tie set: sum of e(q - p_r, nrm[r]) and sum of nrm[r]
    const int32_t* pts;               // the indexed cloud in row order
    const double* nrm;                // its normals
    int q[3];
    double e = 0.0, s[3] = {0.0, 0.0, 0.0};
    __device__ __forceinline__ void reset() { e = 0.0; s[0] = s[1] = s[2] = 0.0; }
    __device__ __forceinline__ void add(unsigned r) {
#pragma clang fp contract(off)
        const long long j = r;
        const double* n = nrm + 3 * j;
        e += plane_term((double)(q[0] - pts[3 * j]), (double)(q[1] - pts[3 * j + 1]), (double)(q[2] - pts[3 * j + 2]), n[0], n[1], n[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += n[c];
    }
};
using TiePlane = TieVisitor<PlaneSums>;

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
        init.over.pts = pts;
        init.over.nrm = nrm;
        init.over.q[0] = q.x; init.over.q[1] = q.y; init.over.q[2] = q.z;
        const TiePlane ties = search(g, qc, 0, init);
        const long long row = q.w;
        const double c = (double)ties.count;
        nn[row] = (int32_t)ties.row;
        sqd[row] = (long long)ties.d2;
        terms[row] = ties.over.e / c;
#pragma unroll
        for (int k = 0; k < 3; ++k) orphan[3 * row + k] = ties.over.s[k] / c;
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
            const double* n = bn + 3 * j;
            e += plane_term((double)(q.x - bpts[3 * j]), (double)(q.y - bpts[3 * j + 1]), (double)(q.z - bpts[3 * j + 2]), n[0], n[1], n[2]);
        }
        terms[row] = e / (double)c;
    }
}

int key_bits(long long nb) {                    // bits of the largest decoded row, nb - 1 (at least 1)
    int bits = 1;
    while (bits < 31 && ((long long)1 << bits) < nb) ++bits;
    return bits;
}

// ---- workspace -----------------------------------------------------------------------------------------------------------------
// The default rule's buffers, and what the tie-averaged rule puts between them (cap > 0: its pair capacity, which then sizes the
// key / value arrays instead of na).
struct DistLayout {
    size_t nn_ab, d_ab, nn_ba, d_ba, keys0, vals0, keys1, vals1, seg_lo, seg_hi, bn, pab, pba, sort_tmp, sort_tmp_bytes, total;
};
struct TieLayout : DistLayout {
    size_t cnt, off, orphan, terms_a, terms_b, ctl, scan_tmp, scan_tmp_bytes;
};

TieLayout dist_layout(long long na, long long nb, long long cap = 0) {
    TieLayout l{};
    const bool mean = cap > 0;
    const size_t A = (size_t)na, B = (size_t)nb, P = mean ? (size_t)cap : A;
    Carver w;
    l.nn_ab = w.take(A * 4);
    l.d_ab = w.take(A * 8);
    l.nn_ba = w.take(B * 4);
    l.d_ba = w.take(B * 8);
    if (mean) { l.cnt = w.take(A * 8); l.off = w.take(A * 8); }
    l.keys0 = w.take(P * 4);
    l.vals0 = w.take(P * 4);
    l.keys1 = w.take(P * 4);
    l.vals1 = w.take(P * 4);
    l.seg_lo = w.take(B * 4);
    l.seg_hi = w.take(B * 4);
    l.bn = w.take(B * 24);
    if (mean) { l.orphan = w.take(B * 24); l.terms_a = w.take(A * 8); l.terms_b = w.take(B * 8); }
    l.pab = w.take(kTallyBlocks * sizeof(Partial));
    l.pba = w.take(kTallyBlocks * sizeof(Partial));
    if (mean) {
        l.ctl = w.take(sizeof(TieCtl));
        (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, l.scan_tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                               (int)na, (hipStream_t)0);
        l.scan_tmp = w.take(l.scan_tmp_bytes + 256);
    }
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, l.sort_tmp_bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)(mean ? cap : na > 0 ? na : 1), 0,
                                             key_bits(mean ? nb + 1 : nb), (hipStream_t)0);
    l.sort_tmp = w.take(l.sort_tmp_bytes + 256);
    l.total = w.o;
    return l;
}

// What both rules do around their own middle: the buffers of a call, and the tally of its two directions.
struct Call {
    hipStream_t st;
    IndexView A, B;
    TieLayout l;
    unsigned char* w;
    int32_t *nn_ab, *nn_ba;           // the caller's link arrays where it gave them
    long long *d_ab, *d_ba;
    unsigned *keys0, *vals0, *keys1, *vals1, *seg_lo, *seg_hi;
    double* bn;
    unsigned ga, gb;                  // workgroups of one lane per point of A / of B
};

Call open_call(const void* index_a, int64_t na, const void* index_b, int64_t nb, int64_t cap, int32_t* to_b, int32_t* to_a, void* workspace,
               void* stream) {
    Call c{(hipStream_t)stream, index_view(index_a, na), index_view(index_b, nb), dist_layout(na, nb, cap), (unsigned char*)workspace};
    const TieLayout& l = c.l;
    c.nn_ab = to_b ? to_b : (int32_t*)(c.w + l.nn_ab);
    c.nn_ba = to_a ? to_a : (int32_t*)(c.w + l.nn_ba);
    c.d_ab = (long long*)(c.w + l.d_ab); c.d_ba = (long long*)(c.w + l.d_ba);
    c.keys0 = (unsigned*)(c.w + l.keys0); c.vals0 = (unsigned*)(c.w + l.vals0);
    c.keys1 = (unsigned*)(c.w + l.keys1); c.vals1 = (unsigned*)(c.w + l.vals1);
    c.seg_lo = (unsigned*)(c.w + l.seg_lo); c.seg_hi = (unsigned*)(c.w + l.seg_hi);
    c.bn = (double*)(c.w + l.bn);
    c.ga = (unsigned)((na + 255) / 256); c.gb = (unsigned)((nb + 255) / 256);
    return c;
}

// the stable sort of the n pairs in keys0 / vals0 by decoded row, then every decoded point's segment
template <class Pairs>
int group_pairs(const Call& c, long long n, int bits, unsigned blocks, Pairs pairs) {
    const long long nb = c.B.n;
    size_t tmp = c.l.sort_tmp_bytes;                       // LSD radix sort: stable, so every segment stays in increasing original row
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(c.w + c.l.sort_tmp), tmp, (const unsigned*)c.keys0, c.keys1,
                                                     (const unsigned*)c.vals0, c.vals1, (int)n, 0, bits, c.st));
    PCC_CHECK_HIP(hipMemsetAsync(c.seg_lo, 0, (size_t)nb * 4, c.st));
    PCC_CHECK_HIP(hipMemsetAsync(c.seg_hi, 0, (size_t)nb * 4, c.st));
    hipLaunchKernelGGL(k_segments<Pairs>, dim3(blocks), dim3(256), 0, c.st, (const unsigned*)c.keys1, pairs, (unsigned)nb, c.seg_lo, c.seg_hi);
    return PCC_OK;
}

template <class Term>
void tally_call(const Call& c, Term ab, Term ba, double* tally) {
    Partial *pab = (Partial*)(c.w + c.l.pab), *pba = (Partial*)(c.w + c.l.pba);
    const int ta = tally_blocks(c.A.n), tb = tally_blocks(c.B.n);
    hipLaunchKernelGGL(k_tally<Term>, dim3(ta), dim3(256), 0, c.st, c.A.n, (const long long*)c.d_ab, ab, pab);
    hipLaunchKernelGGL(k_tally<Term>, dim3(tb), dim3(256), 0, c.st, c.B.n, (const long long*)c.d_ba, ba, pba);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(256), 0, c.st, (const Partial*)pab, ta, (const Partial*)pba, tb, c.B.n, tally);
}

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
    const Call c = open_call(index_a, na, index_b, nb, 0, to_b, to_a, workspace, stream);
    const IndexView &A = c.A, &B = c.B;
    // queries in the other index's Morton order
    hipLaunchKernelGGL(k_query<true>, dim3(c.ga), dim3(256), 0, c.st, B.hdr, B.codes, B.recs, B.n, A.recs, (const int32_t*)nullptr, A.n,
                       c.nn_ab, c.d_ab);
    hipLaunchKernelGGL(k_query<true>, dim3(c.gb), dim3(256), 0, c.st, A.hdr, A.codes, A.recs, A.n, B.recs, (const int32_t*)nullptr, B.n,
                       c.nn_ba, c.d_ba);
    const double* bn = nullptr;
    if (a_normals) {
        hipLaunchKernelGGL(k_link_keys, dim3(c.ga), dim3(256), 0, c.st, (const int32_t*)c.nn_ab, (long long)na, c.keys0, c.vals0);
        { const int rc = group_pairs(c, na, key_bits(nb), c.ga, AllLinks{(long long)na});
          if (rc != PCC_OK) return rc; }
        hipLaunchKernelGGL(k_bnormals<OrphanNearest>, dim3(c.gb), dim3(256), 0, c.st, (const unsigned*)c.seg_lo, (const unsigned*)c.seg_hi,
                           (const unsigned*)c.vals1, a_normals, OrphanNearest{a_normals, c.nn_ba}, (long long)nb, c.bn);
        bn = c.bn;
    }
    tally_call(c, LinkTerm{A.pts, B.pts, c.nn_ab, bn}, LinkTerm{B.pts, A.pts, c.nn_ba, a_normals}, tally);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_cloud_distortion_ties_workspace_bytes(int64_t na, int64_t nb, int32_t tie_mode, int64_t max_pairs) {
    if (!valid_n(na) || !valid_n(nb)) return 0;
    if (tie_mode == PCC_TIES_PICK) return dist_layout(na, nb).total;
    if (tie_mode != PCC_TIES_MEAN || !valid_n(max_pairs)) return 0;
    const size_t pick = dist_layout(na, nb).total, mean = dist_layout(na, nb, max_pairs).total;      // without normals mean runs pick's pass
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
    if (tie_mode == PCC_TIES_PICK || !a_normals) {      // the D1 / H1 slots do not depend on the rule: no pairs without normals
        PCC_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), (hipStream_t)stream));
        return pcc_cloud_distortion(ctx, index_a, na, index_b, nb, a_normals, tally, to_b, to_a, workspace, stream);
    }
    PCC_REQUIRE(valid_n(max_pairs), "pcc_cloud_distortion_ties: max_pairs = %lld outside [1, 2^31)", (long long)max_pairs);
    const Call c = open_call(index_a, na, index_b, nb, max_pairs, to_b, to_a, workspace, stream);
    const IndexView &A = c.A, &B = c.B;
    const TieLayout& l = c.l;
    unsigned char* w = c.w;
    hipStream_t st = c.st;
    unsigned long long *cnt = (unsigned long long*)(w + l.cnt), *off = (unsigned long long*)(w + l.off);
    double *orphan = (double*)(w + l.orphan), *terms_a = (double*)(w + l.terms_a), *terms_b = (double*)(w + l.terms_b);
    TieCtl* ctl = (TieCtl*)(w + l.ctl);
    const unsigned long long cap = (unsigned long long)max_pairs;
    const unsigned gp = (unsigned)((cap + 255) / 256);
    hipLaunchKernelGGL(k_tie_count, dim3(c.ga), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, A.n, c.nn_ab, c.d_ab, cnt);
    hipLaunchKernelGGL(k_tie_ba, dim3(c.gb), dim3(256), 0, st, A.hdr, A.codes, A.recs, A.n, A.pts, a_normals, B.recs, B.n, c.nn_ba, c.d_ba,
                       terms_b, orphan);
    size_t tmp = l.scan_tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum((void*)(w + l.scan_tmp), tmp, (const unsigned long long*)cnt, off, (int)na, st));
    hipLaunchKernelGGL(k_pair_total<false>, dim3(1), dim3(1), 0, st, (const unsigned long long*)cnt, (const unsigned long long*)off, (size_t)na,
                       cap, ctl, (long long*)status);
    hipLaunchKernelGGL(k_tie_emit, dim3(c.ga), dim3(256), 0, st, B.hdr, B.codes, B.recs, B.n, A.recs, A.n, (const long long*)c.d_ab,
                       (const unsigned long long*)cnt, (const unsigned long long*)off, (const TieCtl*)ctl, c.keys0, c.vals0);
    hipLaunchKernelGGL(k_pair_pad<unsigned>, dim3(gp), dim3(256), 0, st, (const TieCtl*)ctl, cap, (unsigned)nb, c.keys0, c.vals0);
    { const int rc = group_pairs(c, (long long)cap, key_bits(nb + 1), gp, TiePairs{ctl});
      if (rc != PCC_OK) return rc; }
    hipLaunchKernelGGL(k_bnormals<OrphanMean>, dim3(c.gb), dim3(256), 0, st, (const unsigned*)c.seg_lo, (const unsigned*)c.seg_hi,
                       (const unsigned*)c.vals1, a_normals, OrphanMean{orphan, ctl}, (long long)nb, c.bn);
    hipLaunchKernelGGL(k_terms_ab, dim3(c.ga), dim3(256), 0, st, A.recs, A.n, B.pts, (const double*)c.bn, (const unsigned*)c.keys0,
                       (const unsigned long long*)cnt, (const unsigned long long*)off, (const TieCtl*)ctl, terms_a);
    tally_call(c, StoredTerm{terms_a}, StoredTerm{terms_b}, tally);
    hipLaunchKernelGGL(k_pair_nan, dim3(1), dim3(256), 0, st, (const long long*)status, 2, tally + 3, tally + 7);      // D2_AB, D2_BA; H2_AB, H2_BA
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
