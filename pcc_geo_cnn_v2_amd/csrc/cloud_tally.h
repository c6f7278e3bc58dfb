// What the whole-cloud tallies (cloud_metrics.hip, cloud_color.hip) and the D2 threshold searches (search_d2.hip) share, each stated
// once: the fixed-order sum of a 256-thread workgroup and the grid its partials come from, the point-to-plane term, the visitor of
// "every indexed point at the smallest distance so far", the control block of a device-counted pair list, and the workspace carver.
// Every number these files report is a sum whose order is fixed by the sizes alone; that order lives here.
#pragma once
#include "common.h"

namespace {

// ---- fixed-order sums ----------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads: thread t brings v; s[t] = op(s[t], s[t + w]) for w = 128, 64 .. 1.  Returns s[0] to every thread.
template <class V, class Op>
__device__ __forceinline__ V tree256(const V& v, V* s, Op op) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) s[t] = op(s[t], s[t + w]);
        __syncthreads();
    }
    return s[0];
}

struct Sum {
    template <class T>
    __device__ __forceinline__ T operator()(const T& a, const T& b) const { return a + b; }
};

template <class T, int K>
struct Slots { T v[K]; };             // K values that travel through one tree, combined slot by slot
template <class Op>
struct EachSlot {
    Op op;
    template <class T, int K>
    __device__ __forceinline__ Slots<T, K> operator()(Slots<T, K> a, const Slots<T, K>& b) const {
#pragma unroll
        for (int k = 0; k < K; ++k) a.v[k] = op(a.v[k], b.v[k]);
        return a;
    }
};

// The partials of a tally over n elements: a grid-stride loop over this many workgroups, then tree256 in each.  Fixed by n alone, so
// every per-thread sum visits the same elements in the same order on every call.
constexpr int kTallyBlocks = 1024;
inline int tally_blocks(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < kTallyBlocks ? b : kTallyBlocks);
}

// ((gx*nx + gy*ny) + gz*nz)^2 rounded after every operation: numpy's order, pc_metric.plane_terms
__device__ __forceinline__ double plane_term(double gx, double gy, double gz, double nx, double ny, double nz) {
#pragma clang fp contract(off)
    const double p = (gx * nx + gy * ny) + gz * nz;
    return p * p;
}

// ---- tie-set visitor of the cell-index search (cell_index.h search()) ----------------------------------------------------------
// Every indexed point at the smallest squared distance so far: their number, their lowest row, and what the payload gathers over
// them (reset() when a nearer point empties the set, add(row) for every member).
struct NoPayload {
    __device__ __forceinline__ void reset() {}
    __device__ __forceinline__ void add(unsigned) {}
};
template <class Payload = NoPayload>
struct TieVisitor {
    Payload over;
    unsigned long long d2 = ~0ull;
    unsigned count = 0, row = ~0u;
    __device__ __forceinline__ void consider(unsigned long long d, unsigned r) {
        if (d > d2) return;
        if (d < d2) { d2 = d; count = 0; row = ~0u; over.reset(); }
        ++count;
        row = r < row ? r : row;
        over.add(r);
    }
    __device__ __forceinline__ unsigned long long bound() const { return d2; }
};

// ---- pair lists whose length is only known on the device -----------------------------------------------------------------------
// Count per element, ExclusiveSum, k_pair_total against the caller's capacity, emit, k_pair_pad, stable SortPairs, group.  Past the
// capacity nothing below k_pair_total touches the pair arrays and k_pair_nan turns the sums made from them into NaN.
struct TieCtl {                       // written by k_pair_total
    unsigned long long pairs;         // sum of the counts
    int overflow;                     // pairs > capacity
};

// status = (pairs needed, overflowed).  KEEP_MAX: one call of several lists (the chunks of a search) keeps the largest and any overflow.
template <bool KEEP_MAX>
__global__ void k_pair_total(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off, size_t n,
                             unsigned long long cap, TieCtl* __restrict__ ctl, long long* __restrict__ status) {
    const unsigned long long pairs = off[n - 1] + cnt[n - 1];
    ctl->pairs = pairs;
    ctl->overflow = pairs > cap;
    if (KEEP_MAX) {
        if ((long long)pairs > status[0]) status[0] = (long long)pairs;
        if (pairs > cap) status[1] = 1;
    } else {
        status[0] = (long long)pairs;
        status[1] = pairs > cap;
    }
}

// the unused tail of the capacity sorts behind every pair (key `pad`)
template <class Key>
__global__ void __launch_bounds__(256) k_pair_pad(const TieCtl* __restrict__ ctl, unsigned long long cap, Key pad, Key* __restrict__ keys,
                                                  unsigned* __restrict__ vals) {
    if (ctl->overflow) return;
    for (unsigned long long p = ctl->pairs + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < cap;
         p += (unsigned long long)gridDim.x * blockDim.x) {
        keys[p] = pad;
        vals[p] = (unsigned)p;
    }
}

// a list met more pairs than the capacity: a[0 .. n) and b[0 .. n) say so instead of holding numbers made from unwritten pairs
__global__ void __launch_bounds__(256) k_pair_nan(const long long* __restrict__ status, int n, double* __restrict__ a, double* __restrict__ b) {
    if (!status[1]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = __longlong_as_double(0x7FF8000000000000ll); b[i] = __longlong_as_double(0x7FF8000000000000ll); }
}

// ---- workspace layouts ---------------------------------------------------------------------------------------------------------
struct Carver {                       // byte offsets of consecutive buffers, each on a 256-byte boundary
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

}  // namespace
