// Morton-sorted cell index over a voxelised cloud and its exact neighbour search (DESIGN.md §4.7 "Cell index"), shared by normals.hip
// (k nearest neighbours within one cloud) and cloud_metrics.hip (the nearest neighbour across two clouds).
//
// Build (index_build; one stream, no host synchronisation):
//   1. k_prepare: 63-bit Morton code of every point, a masked row-order copy of the points, the bounding box and the exact
//      coordinate sums (integer atomics, one set per workgroup);
//   2. hipCUB radix sort of (code, row); k_records gathers (x, y, z, row) in that order and histograms the highest differing Morton
//      bit of adjacent codes, which gives the number of occupied cells of edge 2^L for every L at once;
//   3. k_level picks the base cell level: the smallest L whose occupied cells hold twice_points_per_cell / 2 points or more on
//      average.  The cells of edge 2^L are contiguous ranges of the sorted codes, found by binary search.
// Search (search(), one lane per query; a wave's lanes should be neighbours in space): the cube of cells of Chebyshev radius `rad`
// around the query at the base level, growing to radius 2, then radius 2 at the next coarser levels, each stage skipping what the
// previous box covered, until the visitor's bound (its k-th best squared distance) is STRICTLY below the squared distance from the
// query to the outside of the visited box (on equality an equidistant point with a lower row could still be outside) or the box
// holds the cloud's bounding box.  At L = 21 one cell is the whole domain, so the search always ends.
#pragma once
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int kCoordMask = (1 << 21) - 1;
constexpr int kLevels = 22;           // cell edge 2^L, L = 0 .. 21 (L = 21: one cell holds the whole domain)

struct IndexHdr {
    int bmin[3], bmax[3];             // bounding box of the indexed cloud
    unsigned long long sum[3];        // exact coordinate sums
    unsigned hist[kLevels];           // adjacent sorted pairs by floor(highest differing Morton bit / 3)
    int level;                        // base cell level of the search
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

__device__ __forceinline__ long long lower_bound(const unsigned long long* __restrict__ codes, long long n, unsigned long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- build ---------------------------------------------------------------------------------------------------------------------

__global__ void k_init(IndexHdr* H) {
    for (int a = 0; a < 3; ++a) { H->bmin[a] = kCoordMask; H->bmax[a] = 0; H->sum[a] = 0; }
    for (int l = 0; l < kLevels; ++l) H->hist[l] = 0;
    H->level = 0;
}

// grid-stride over the points, one set of atomics per workgroup: thousands of same-address atomics serialise (a launch with one set
// per wave cost 1.4 ms at 1e6 points)
__global__ void __launch_bounds__(256) k_prepare(const int32_t* __restrict__ pts, long long n, unsigned long long* __restrict__ codes,
                                                 unsigned* __restrict__ rows, int32_t* __restrict__ copy, IndexHdr* H) {
    __shared__ int slo[4][3], shi[4][3];
    __shared__ unsigned long long ssum[4][3];
    int lo[3] = {kCoordMask, kCoordMask, kCoordMask}, hi[3] = {0, 0, 0};
    unsigned long long s[3] = {0, 0, 0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int3 p = load_pt(pts, i);
        codes[i] = morton(p.x, p.y, p.z);
        rows[i] = (unsigned)i;
        copy[3 * i] = p.x; copy[3 * i + 1] = p.y; copy[3 * i + 2] = p.z;
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
        atomicMin(&H->bmin[a], l);
        atomicMax(&H->bmax[a], h);
        atomicAdd(&H->sum[a], t);
    }
}

__global__ void __launch_bounds__(256) k_records(const int32_t* __restrict__ copy, long long n, const unsigned long long* __restrict__ codes,
                                                 const unsigned* __restrict__ rows, int4* __restrict__ recs, IndexHdr* H) {
    __shared__ unsigned h[kLevels];
    if (threadIdx.x < kLevels) h[threadIdx.x] = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const unsigned r = rows[t];
        recs[t] = make_int4(copy[3 * (long long)r], copy[3 * (long long)r + 1], copy[3 * (long long)r + 2], (int)r);
        if (t > 0) {
            const unsigned long long d = codes[t] ^ codes[t - 1];
            if (d) atomicAdd(&h[(63 - __clzll((long long)d)) / 3], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLevels && h[threadIdx.x]) atomicAdd(&H->hist[threadIdx.x], h[threadIdx.x]);
}

// base level: the smallest L with 2n >= twice_points_per_cell * (occupied cells of edge 2^L) (L = 21 always qualifies)
__global__ void k_level(long long n, int twice_points_per_cell, IndexHdr* H) {
    unsigned long long occ = 1;                 // occupied cells of edge 1: one more than the adjacent pairs that differ
    for (int l = 0; l < kLevels; ++l) occ += H->hist[l];
    int level = kLevels - 1;
    for (int l = 0; l < kLevels; ++l) {
        if (2ull * (unsigned long long)n >= (unsigned long long)twice_points_per_cell * occ) { level = l; break; }
        occ -= H->hist[l];                      // pairs that differ at level l but not above: merged one level up
    }
    H->level = level;
}

size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
bool valid_n(int64_t n) { return n > 0 && n < ((int64_t)1 << 31); }      // a point count an index (and an int-sized hipCUB call) takes

struct IndexLayout {
    size_t hdr, codes, recs, pts, codes0, rows0, rows1, sort_tmp, sort_tmp_bytes, total;
};

IndexLayout index_layout(long long n) {
    IndexLayout l;
    const size_t N = (size_t)n;
    size_t o = 0;
    l.hdr = o; o += al256(sizeof(IndexHdr));
    l.codes = o; o += al256(N * 8);
    l.recs = o; o += al256(N * 16);
    l.pts = o; o += al256(N * 12);
    l.codes0 = o; o += al256(N * 8);
    l.rows0 = o; o += al256(N * 4);
    l.rows1 = o; o += al256(N * 4);
    size_t tmp = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)(n > 0 ? n : 1), 0, 63, (hipStream_t)0);
    l.sort_tmp_bytes = tmp;
    l.sort_tmp = o; o += al256(tmp + 256);
    l.total = o;
    return l;
}

struct IndexView {                    // device pointers of a built index
    const IndexHdr* hdr;
    const unsigned long long* codes;  // sorted Morton codes
    const int4* recs;                 // (x, y, z, row) in code order
    const int32_t* pts;               // masked points in row order
    long long n;
};

IndexView index_view(const void* index, long long n) {
    const IndexLayout l = index_layout(n);
    const unsigned char* b = (const unsigned char*)index;
    return IndexView{(const IndexHdr*)(b + l.hdr), (const unsigned long long*)(b + l.codes), (const int4*)(b + l.recs),
                     (const int32_t*)(b + l.pts), n};
}

// builds the index of pts[0 .. n) into index_layout(n).total bytes at `index`
int index_build(const pcc_ctx* ctx, const int32_t* pts, long long n, void* index, int twice_points_per_cell, hipStream_t st) {
    const IndexLayout l = index_layout(n);
    unsigned char* w = (unsigned char*)index;
    IndexHdr* H = (IndexHdr*)(w + l.hdr);
    unsigned long long *codes0 = (unsigned long long*)(w + l.codes0), *codes = (unsigned long long*)(w + l.codes);
    unsigned *rows0 = (unsigned*)(w + l.rows0), *rows1 = (unsigned*)(w + l.rows1);
    int32_t* copy = (int32_t*)(w + l.pts);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const unsigned cus = (unsigned)(ctx->num_cu > 0 ? ctx->num_cu : 256);
    hipLaunchKernelGGL(k_init, dim3(1), dim3(1), 0, st, H);
    hipLaunchKernelGGL(k_prepare, dim3(blocks < cus ? blocks : cus), dim3(256), 0, st, pts, n, codes0, rows0, copy, H);
    size_t tmp = l.sort_tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.sort_tmp), tmp, (const unsigned long long*)codes0, codes,
                                                     (const unsigned*)rows0, rows1, (int)n, 0, 63, st));
    hipLaunchKernelGGL(k_records, dim3(blocks), dim3(256), 0, st, (const int32_t*)copy, n, (const unsigned long long*)codes,
                       (const unsigned*)rows1, (int4*)(w + l.recs), H);
    hipLaunchKernelGGL(k_level, dim3(1), dim3(1), 0, st, n, twice_points_per_cell, H);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

// ---- search --------------------------------------------------------------------------------------------------------------------

struct Cells {                        // what a search reads: the index arrays and its header fields, loaded once per lane
    const unsigned long long* codes;
    const int4* recs;
    long long n;
    int level, bmin[3], bmax[3];
};

__device__ __forceinline__ Cells cells(const IndexHdr* H, const unsigned long long* codes, const int4* recs, long long n) {
    Cells c{codes, recs, n, H->level, {}, {}};
#pragma unroll
    for (int a = 0; a < 3; ++a) { c.bmin[a] = H->bmin[a]; c.bmax[a] = H->bmax[a]; }
    return c;
}

// Feeds vis.consider(d2, row) the indexed points around qc, starting at Chebyshev radius `rad`, and returns vis once vis.bound(),
// its k-th best squared distance, is below the squared gap to every unvisited point: then every point at or below the bound has been
// considered.  The visitor travels by value: taken by reference, its key array stayed in memory longer and k_knn spilled more.
template <class Visitor>
__device__ __forceinline__ Visitor search(const Cells& g, const int (&qc)[3], int rad, Visitor vis) {
    int level = g.level;
    bool have_prev = false;
    int plo[3] = {0, 0, 0}, phi[3] = {0, 0, 0};
    for (;;) {
        const int e = 1 << level;
        int c[3], clo[3], chi[3], blo[3], bhi[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            c[ax] = qc[ax] >> level;
            clo[ax] = max(c[ax] - rad, g.bmin[ax] >> level);
            chi[ax] = min(c[ax] + rad, g.bmax[ax] >> level);
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
                    for (long long pos = lower_bound(g.codes, g.n, key0); pos < g.n; ++pos) {
                        const int4 r = g.recs[pos];
                        if ((r.x >> level) != cx || (r.y >> level) != cy || (r.z >> level) != cz) break;
                        if (have_prev && r.x >= plo[0] && r.x <= phi[0] && r.y >= plo[1] && r.y <= phi[1] && r.z >= plo[2] && r.z <= phi[2])
                            continue;
                        const long long dx = r.x - qc[0], dy = r.y - qc[1], dz = r.z - qc[2];
                        vis.consider((unsigned long long)(dx * dx + dy * dy + dz * dz), (unsigned)r.w);
                    }
                }
        // nearest possible unvisited point: just outside a face of the box; faces beyond the cloud's box hide nothing
        long long gap = -1;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (blo[ax] > g.bmin[ax]) { const long long d = qc[ax] - blo[ax] + 1; gap = gap < 0 || d < gap ? d : gap; }
            if (bhi[ax] < g.bmax[ax]) { const long long d = bhi[ax] + 1 - qc[ax]; gap = gap < 0 || d < gap ? d : gap; }
        }
        if (gap < 0 || vis.bound() < (unsigned long long)(gap * gap)) break;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { plo[ax] = blo[ax]; phi[ax] = bhi[ax]; }
        have_prev = true;
        if (rad < 2) ++rad; else ++level;
    }
    return vis;
}

}  // namespace
