// Surface model of the surface anchor codec (include/pcc_geo.h "surface anchor"): everything of anchor_surface.py that
// is data parallel.  Integers only.  The entropy coder is sequential and stays on the host (anchor_coder.cpp); the set of leaves travels
// as an octree anchor stream (octree_anchor.hip).  The host reads a count back BETWEEN calls, never inside one.
//
// Encoder:
//   pcc_surface_leaves    k_pkeys (Morton key of every point), hipCUB radix sort + unique: the distinct points; their keys >> 3k are
//                         already ascending, a second unique gives the leaves.  Both counts stay in the device header.
//   pcc_surface_edges     k_edgekeys: 12 keys (morton(corner) << 2 | axis) per leaf, radix sort, unique: the edge list.
//   pcc_surface_vertices  k_pairs: every distinct point emits one (edge key, offset) pair per axis, or the key kNoEdge where it is not
//                         within 1 of a lattice line in both other axes; radix sort of the pairs by key; k_fit: one lane per edge of the
//                         list finds its run (lower_bound) and sums it: flag and t = (2 sum + n) / (2 n).  A run holds at most 9 W pairs.
// Decoder:
//   pcc_surface_count        k_raster<K, false>: per leaf the number of voxels it emits; exclusive scan; total in the header.
//   pcc_surface_reconstruct  k_raster<K, true> writes the Morton keys of the voxels at the scanned offsets; radix sort, unique,
//                            k_points de-interleaves them.
//
// k_raster: TPL lanes share a leaf (one wave for W <= 8, four above; a block holds 256 / TPL leaves).  Lanes 0 .. 11 look the
// leaf's edges up in the edge list, rank them by their index (= key order), and the flagged vertices go to LDS; every lane then reads
// them back (broadcast reads) for the centroid and the dominant axis, lanes 0 .. m - 1 rank themselves in the angular order by
// counting the vertices that come before them (the order is total, so the ranks are a permutation).  The m triangles x 3 axes x
// (W + 1)^2 samples are one flat index space the lanes stride over; a sample inside its triangle sets one bit of the leaf's
// (W + 1)^3 bit voxel map in LDS (34 KiB at W = 64).  An OR does not depend on the order of its operands: no result depends on atomic
// ordering.  The map is what both passes agree on: its population count is the count pass, its set bits in ascending order are
// the write pass, each lane owning a contiguous range of words behind a prefix sum over the lanes.
//
// Every index is checked against the count or the capacity it belongs to: wrong counts give wrong voxels, never an access outside
// the buffers.
#include <hipcub/hipcub.hpp>

#include "cell_index.h"

namespace {

constexpr int kBlock = 256;
constexpr int kEdgesPerLeaf = 12;
constexpr unsigned long long kNoEdge = 1ull << 62;      // above every edge key (morton of 20-bit corners << 2 | axis < 2^62)
constexpr unsigned long long kNoLeaf = ~0ull;

__device__ __forceinline__ int compact3(unsigned long long x) {           // inverse of spread3
    x &= 0x1249249249249249ull;
    x = (x | x >> 2) & 0x10c30c30c30c30c3ull;
    x = (x | x >> 4) & 0x100f00f00f00f00full;
    x = (x | x >> 8) & 0x1f0000ff0000ffull;
    x = (x | x >> 16) & 0x1f00000000ffffull;
    x = (x | x >> 32) & 0x1fffffull;
    return (int)x;
}

unsigned grid_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }
bool valid_count(int64_t n) { return n >= 1 && n < (1ll << 31); }
bool valid_k(int32_t k) { return k >= 2 && k <= 6; }

// ---- encoder ---------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) k_pkeys(const int32_t* __restrict__ pts, long long n, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int3 p = load_pt(pts, i);
    keys[i] = morton(p.x, p.y, p.z);
}

// leaf key of every distinct point; kNoLeaf behind the last one so that one unique over n entries serves any count
__global__ void __launch_bounds__(kBlock) k_leafkeys(const unsigned long long* __restrict__ pkeys, const long long* __restrict__ count, long long n,
                                                     int k, unsigned long long* __restrict__ lk) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long c = *count;
    c = c < n ? c : n;
    lk[i] = i < c ? pkeys[i] >> (3 * k) : kNoLeaf;
}

// the unique above counted the run of kNoLeaf as a leaf when there were duplicates
__global__ void k_leafcount(long long n, long long* hdr) {
    if (hdr[0] < n) hdr[1] -= 1;
}

// edge e of a leaf: axis a = e >> 2, corner = b + (e >> 1 & 1) e_u + (e & 1) e_v with (u, v) the other two axes, ascending
__global__ void __launch_bounds__(kBlock) k_edgekeys(const unsigned long long* __restrict__ leaves, long long nleaves,
                                                     unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nleaves * kEdgesPerLeaf) return;
    const unsigned long long lk = leaves[i / kEdgesPerLeaf];
    const int e = (int)(i % kEdgesPerLeaf), a = e >> 2;
    int c[3] = {compact3(lk >> 2), compact3(lk >> 1), compact3(lk)};
    c[a == 0 ? 1 : 0] += e >> 1 & 1;
    c[a == 2 ? 1 : 2] += e & 1;
    keys[i] = morton(c[0], c[1], c[2]) << 2 | (unsigned)a;
}

// lattice line within 1 of coordinate v, or -1: v = W c + {0, 1} or W c - 1
__device__ __forceinline__ int near_line(int v, int k) {
    const int w = 1 << k, r = v & (w - 1);
    return r <= 1 ? v >> k : r == w - 1 ? (v >> k) + 1 : -1;
}

__global__ void __launch_bounds__(kBlock) k_pairs(const unsigned long long* __restrict__ pkeys, long long n, int k,
                                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ offs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long pk = pkeys[i];
    const int p[3] = {compact3(pk >> 2), compact3(pk >> 1), compact3(pk)};
    const int l[3] = {near_line(p[0], k), near_line(p[1], k), near_line(p[2], k)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
        int c[3];
        c[a] = p[a] >> k; c[u] = l[u]; c[v] = l[v];
        keys[3 * i + a] = l[u] >= 0 && l[v] >= 0 ? morton(c[0], c[1], c[2]) << 2 | (unsigned)a : kNoEdge;
        offs[3 * i + a] = (unsigned)(p[a] & ((1 << k) - 1));
    }
}

__global__ void __launch_bounds__(kBlock) k_fit(const unsigned long long* __restrict__ edges, long long nedges,
                                                const unsigned long long* __restrict__ keys, const unsigned* __restrict__ offs, long long npairs,
                                                int k, uint8_t* __restrict__ flags, uint8_t* __restrict__ tt) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedges) return;
    const unsigned long long key = edges[e];
    long long sum = 0, cnt = 0;
    for (long long j = lower_bound(keys, npairs, key); j < npairs && keys[j] == key; ++j) {
        sum += offs[j];
        ++cnt;
    }
    long long t = cnt ? (2 * sum + cnt) / (2 * cnt) : 0;
    const long long w = 1ll << k;
    t = t < w ? t : w - 1;
    flags[e] = cnt > 0;
    tt[e] = (uint8_t)t;
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------

template <int K>
struct Geo {
    static constexpr int W = 1 << K, S = W + 1, S2 = S * S, BITS = S * S * S, WORDS = (BITS + 31) / 32;
    static constexpr int TPL = K <= 3 ? 64 : 256, LPB = kBlock / TPL, CHUNK = (WORDS + TPL - 1) / TPL;
};

__device__ __forceinline__ int cross2(int ax, int ay, int bx, int by) { return ax * by - ay * bx; }
__device__ __forceinline__ int half_of(int x, int y) { return y > 0 || (y == 0 && x > 0) ? 0 : y < 0 || (y == 0 && x < 0) ? 1 : 2; }

template <int K, bool WRITE>
__global__ void __launch_bounds__(kBlock) k_raster(const unsigned long long* __restrict__ leaves, long long nleaves,
                                                   const unsigned long long* __restrict__ edges, const uint8_t* __restrict__ flags,
                                                   const uint8_t* __restrict__ tt, long long nedges, int top,
                                                   unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ pos,
                                                   unsigned long long* __restrict__ out, long long cap) {
    using G = Geo<K>;
    constexpr int W = G::W, S = G::S, TPL = G::TPL;
    __shared__ unsigned bm[G::LPB][G::WORDS];
    __shared__ long long eidx[G::LPB][kEdgesPerLeaf];     // index in the edge list, -1: no vertex
    __shared__ int vr[G::LPB][kEdgesPerLeaf][3];          // the leaf's vertices relative to its origin, in edge order
    __shared__ int ord[G::LPB][kEdgesPerLeaf];            // angular order
    __shared__ int wtot[kBlock / 64];
    const int g = threadIdx.x / TPL, lane = threadIdx.x % TPL;
    const long long leaf = (long long)blockIdx.x * G::LPB + g;
    const bool live = leaf < nleaves;
    for (int w = lane; w < G::WORDS; w += TPL) bm[g][w] = 0;
    int o[3] = {0, 0, 0}, r[3] = {0, 0, 0};
    long long my = -1;
    if (live) {
        const unsigned long long lk = leaves[leaf];
        o[0] = compact3(lk >> 2); o[1] = compact3(lk >> 1); o[2] = compact3(lk);
    }
    if (lane < kEdgesPerLeaf) {
        if (live) {
            const int a = lane >> 2, u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
            int c[3] = {o[0], o[1], o[2]};
            c[u] += lane >> 1 & 1;
            c[v] += lane & 1;
            const unsigned long long key = morton(c[0], c[1], c[2]) << 2 | (unsigned)a;
            const long long p = lower_bound(edges, nedges, key);
            if (p < nedges && edges[p] == key && flags[p]) {
                my = p;
                const int t = tt[p];
                r[u] = (lane >> 1 & 1) * W; r[v] = (lane & 1) * W; r[a] = t < W ? t : W - 1;
            }
        }
        eidx[g][lane] = my;
    }
    __syncthreads();
    int m = 0;
#pragma unroll
    for (int j = 0; j < kEdgesPerLeaf; ++j) m += eidx[g][j] >= 0;
    if (my >= 0) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < kEdgesPerLeaf; ++j) rank += eidx[g][j] >= 0 && eidx[g][j] < my;
        vr[g][rank][0] = r[0]; vr[g][rank][1] = r[1]; vr[g][rank][2] = r[2];
    }
    __syncthreads();
    // centroid (G = sum), dominant axis, angular order
    int Gs[3] = {0, 0, 0};
    for (int i = 0; i < m; ++i) { Gs[0] += vr[g][i][0]; Gs[1] += vr[g][i][1]; Gs[2] += vr[g][i][2]; }
    if (live && m == 0 && lane == 0) {
        const int b = ((W / 2) * S + W / 2) * S + W / 2;
        atomicOr(&bm[g][b >> 5], 1u << (b & 31));
    }
    if (lane < m) {
        const int b = (vr[g][lane][0] * S + vr[g][lane][1]) * S + vr[g][lane][2];
        atomicOr(&bm[g][b >> 5], 1u << (b & 31));
    }
    if (m >= 3) {
        long long ss[3] = {0, 0, 0};
        for (int i = 0; i < m; ++i)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const long long d = m * vr[g][i][a] - Gs[a];
                ss[a] += d * d;
            }
        const int ad = ss[0] <= ss[1] && ss[0] <= ss[2] ? 0 : ss[1] <= ss[2] ? 1 : 2;
        const int pu = ad == 0 ? 1 : 0, pv = ad == 2 ? 1 : 2;
        if (lane < m) {
            const int xi = m * vr[g][lane][pu] - Gs[pu], yi = m * vr[g][lane][pv] - Gs[pv], hi = half_of(xi, yi);
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                if (j == lane) continue;
                const int xj = m * vr[g][j][pu] - Gs[pu], yj = m * vr[g][j][pv] - Gs[pv], hj = half_of(xj, yj);
                const int cr = cross2(xj, yj, xi, yi);             // > 0: j before lane
                const int nj = xj * xj + yj * yj, ni = xi * xi + yi * yi;
                const bool before = hj != hi ? hj < hi : cr != 0 ? cr > 0 : nj != ni ? nj < ni : j < lane;
                rank += before;
            }
            ord[g][rank] = lane;
        }
    }
    __syncthreads();
    if (m >= 3) {
        const int items = m * 3 * G::S2;
        for (int it = lane; it < items; it += TPL) {
            const int tq = it / G::S2, s = it - tq * G::S2, tri = tq / 3, q = tq - 3 * tri, i = s / S, j = s - i * S;
            const int u = q == 0 ? 1 : 0, v = q == 2 ? 1 : 2;
            const int ib = min((unsigned)ord[g][tri], 11u), ic = min((unsigned)ord[g][tri + 1 == m ? 0 : tri + 1], 11u);
            const int Au = Gs[u], Av = Gs[v], Aq = Gs[q];
            int Bu = m * vr[g][ib][u], Bv = m * vr[g][ib][v], Bq = m * vr[g][ib][q];
            int Cu = m * vr[g][ic][u], Cv = m * vr[g][ic][v], Cq = m * vr[g][ic][q];
            const int area2 = cross2(Bu - Au, Bv - Av, Cu - Au, Cv - Av);
            if (area2 == 0) continue;
            if (area2 < 0) {
                int x = Bu; Bu = Cu; Cu = x;
                x = Bv; Bv = Cv; Cv = x;
                x = Bq; Bq = Cq; Cq = x;
            }
            const int Pu = m * i, Pv = m * j;
            const long long la = cross2(Cu - Bu, Cv - Bv, Pu - Bu, Pv - Bv), lb = cross2(Au - Cu, Av - Cv, Pu - Cu, Pv - Cv),
                            lc = cross2(Bu - Au, Bv - Av, Pu - Au, Pv - Av);
            if (la < 0 || lb < 0 || lc < 0) continue;
            const long long lam = la + lb + lc;                     // = |area2| > 0
            long long h = (2 * (la * Aq + lb * Bq + lc * Cq) + m * lam) / (2 * m * lam);
            h = h < 0 ? 0 : h > W ? W : h;
            int x[3];
            x[q] = (int)h; x[u] = i; x[v] = j;
            const int b = (x[0] * S + x[1]) * S + x[2];
            atomicOr(&bm[g][b >> 5], 1u << (b & 31));
        }
    }
    __syncthreads();
    // set bits of this lane's words, and the lanes' prefix sum
    const int w0 = lane * G::CHUNK, w1 = w0 + G::CHUNK < G::WORDS ? w0 + G::CHUNK : G::WORDS;
    int c = 0;
    for (int w = w0; w < w1; ++w) c += __popc(bm[g][w]);
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if ((threadIdx.x & 63) >= d) inc += up;
    }
    if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    int before = inc - c, total;
    if (TPL == 64) {
        total = wtot[threadIdx.x >> 6];
    } else {
        total = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < (int)(threadIdx.x >> 6)) before += wtot[w];
            total += wtot[w];
        }
    }
    if (!live) return;
    if (!WRITE) {
        if (lane == 0) cnt[leaf] = (unsigned long long)total;
        return;
    }
    long long dst = (long long)pos[leaf] + before;
    for (int w = w0; w < w1; ++w) {
        unsigned bits = bm[g][w];
        while (bits) {
            const int b = w * 32 + __ffs(bits) - 1;
            bits &= bits - 1;
            const int x = b / G::S2, y = (b - x * G::S2) / S, z = b - x * G::S2 - y * S;
            const int px = min(o[0] * W + x, top), py = min(o[1] * W + y, top), pz = min(o[2] * W + z, top);
            if (dst >= 0 && dst < cap) out[dst] = morton(px, py, pz);
            ++dst;
        }
    }
}

__global__ void k_total(const unsigned long long* cnt, const unsigned long long* pos, long long n, long long* hdr) {
    hdr[0] = (long long)(pos[n - 1] + cnt[n - 1]);
}

__global__ void __launch_bounds__(kBlock) k_points(const unsigned long long* __restrict__ keys, const long long* __restrict__ count, long long cap,
                                                   int32_t* __restrict__ pts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long c = *count;
    c = c < cap ? c : cap;
    if (i >= c) return;
    const unsigned long long k = keys[i];
    pts[3 * i] = compact3(k >> 2); pts[3 * i + 1] = compact3(k >> 1); pts[3 * i + 2] = compact3(k);
}

template <int K, bool WRITE>
void launch_raster(hipStream_t st, const unsigned long long* leaves, long long nleaves, const unsigned long long* edges, const uint8_t* flags,
                   const uint8_t* tt, long long nedges, int top, unsigned long long* cnt, const unsigned long long* pos, unsigned long long* out,
                   long long cap) {
    const unsigned blocks = (unsigned)((nleaves + Geo<K>::LPB - 1) / Geo<K>::LPB);
    hipLaunchKernelGGL((k_raster<K, WRITE>), dim3(blocks), dim3(kBlock), 0, st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap);
}

template <bool WRITE>
void raster(int k, hipStream_t st, const unsigned long long* leaves, long long nleaves, const unsigned long long* edges, const uint8_t* flags,
            const uint8_t* tt, long long nedges, int top, unsigned long long* cnt, const unsigned long long* pos, unsigned long long* out, long long cap) {
    switch (k) {
        case 2: launch_raster<2, WRITE>(st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap); break;
        case 3: launch_raster<3, WRITE>(st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap); break;
        case 4: launch_raster<4, WRITE>(st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap); break;
        case 5: launch_raster<5, WRITE>(st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap); break;
        default: launch_raster<6, WRITE>(st, leaves, nleaves, edges, flags, tt, nedges, top, cnt, pos, out, cap); break;
    }
}

// ---- workspaces: two key buffers of n entries, optionally n values twice, and hipCUB's temporary storage
size_t sort_tmp_bytes(long long n, bool pairs) {
    size_t a = 0, b = 0, c = 0;
    if (pairs)
        (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                 (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, 0, 64, (hipStream_t)0);
    else
        (void)hipcub::DeviceRadixSort::SortKeys((void*)nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, 0, 64,
                                                (hipStream_t)0);
    (void)hipcub::DeviceSelect::Unique((void*)nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (long long*)nullptr, (int)n,
                                       (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, c, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, (hipStream_t)0);
    a = a > b ? a : b;
    return a > c ? a : c;
}

struct Layout { size_t keys0, keys1, vals0, vals1, tmp, tmp_bytes, total; };

Layout layout(long long n, bool pairs) {
    Layout l;
    const size_t N = (size_t)n;
    size_t o = 0;
    l.keys0 = o; o += al256(N * 8);
    l.keys1 = o; o += al256(N * 8);
    l.vals0 = o; o += pairs ? al256(N * 4) : 0;
    l.vals1 = o; o += pairs ? al256(N * 4) : 0;
    l.tmp_bytes = sort_tmp_bytes(n, pairs);
    l.tmp = o; o += al256(l.tmp_bytes + 256);
    l.total = o;
    return l;
}

}  // namespace

PCC_API size_t pcc_surface_leaves_workspace_bytes(int64_t npts) { return valid_count(npts) ? layout(npts, false).total : 0; }

PCC_API int pcc_surface_leaves(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t k, int64_t* hdr, uint64_t* pkeys, uint64_t* leaf_keys,
                               void* workspace, void* stream) {
    PCC_REQUIRE(ctx && pts && hdr && pkeys && leaf_keys && workspace, "pcc_surface_leaves: NULL argument");
    PCC_REQUIRE(valid_count(npts), "pcc_surface_leaves: npts = %lld outside [1, 2^31)", (long long)npts);
    PCC_REQUIRE(valid_k(k), "pcc_surface_leaves: node_log2 = %d outside [2, 6]", k);
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(npts, false);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *k0 = (unsigned long long*)(w + l.keys0), *k1 = (unsigned long long*)(w + l.keys1);
    void* tmp = (void*)(w + l.tmp);
    long long* H = (long long*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, 8 * PCC_SURFACE_HDR_WORDS, st));
    hipLaunchKernelGGL(k_pkeys, dim3(grid_for(npts)), dim3(kBlock), 0, st, pts, (long long)npts, k0);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, bytes, (const unsigned long long*)k0, k1, (int)npts, 0, 63, st));
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceSelect::Unique(tmp, bytes, (const unsigned long long*)k1, (unsigned long long*)pkeys, H, (int)npts, st));
    hipLaunchKernelGGL(k_leafkeys, dim3(grid_for(npts)), dim3(kBlock), 0, st, (const unsigned long long*)pkeys, (const long long*)H, (long long)npts,
                       (int)k, k0);
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceSelect::Unique(tmp, bytes, (const unsigned long long*)k0, (unsigned long long*)leaf_keys, H + 1, (int)npts, st));
    hipLaunchKernelGGL(k_leafcount, dim3(1), dim3(1), 0, st, (long long)npts, H);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_surface_edges_workspace_bytes(int64_t nleaves) {
    return valid_count(nleaves) && valid_count(kEdgesPerLeaf * nleaves) ? layout(kEdgesPerLeaf * nleaves, false).total : 0;
}

PCC_API int pcc_surface_edges(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, int64_t* hdr, uint64_t* edge_keys, void* workspace,
                              void* stream) {
    PCC_REQUIRE(ctx && leaf_keys && hdr && edge_keys && workspace, "pcc_surface_edges: NULL argument");
    PCC_REQUIRE(valid_count(nleaves) && valid_count(kEdgesPerLeaf * nleaves), "pcc_surface_edges: %lld leaves outside [1, 2^31 / 12)",
                (long long)nleaves);
    hipStream_t st = (hipStream_t)stream;
    const long long n = kEdgesPerLeaf * (long long)nleaves;
    const Layout l = layout(n, false);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *k0 = (unsigned long long*)(w + l.keys0), *k1 = (unsigned long long*)(w + l.keys1);
    void* tmp = (void*)(w + l.tmp);
    long long* H = (long long*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, 8 * PCC_SURFACE_HDR_WORDS, st));
    hipLaunchKernelGGL(k_edgekeys, dim3(grid_for(n)), dim3(kBlock), 0, st, (const unsigned long long*)leaf_keys, (long long)nleaves, k0);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, bytes, (const unsigned long long*)k0, k1, (int)n, 0, 63, st));
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceSelect::Unique(tmp, bytes, (const unsigned long long*)k1, (unsigned long long*)edge_keys, H, (int)n, st));
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_surface_vertices_workspace_bytes(int64_t npts) {
    return valid_count(npts) && valid_count(3 * npts) ? layout(3 * npts, true).total : 0;
}

PCC_API int pcc_surface_vertices(pcc_ctx* ctx, const uint64_t* pkeys, int64_t npts, int32_t k, const uint64_t* edge_keys, int64_t nedges,
                                 uint8_t* flags, uint8_t* t, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && pkeys && edge_keys && flags && t && workspace, "pcc_surface_vertices: NULL argument");
    PCC_REQUIRE(valid_count(npts) && valid_count(3 * npts), "pcc_surface_vertices: npts = %lld outside [1, 2^31 / 3)", (long long)npts);
    PCC_REQUIRE(valid_count(nedges), "pcc_surface_vertices: %lld edges outside [1, 2^31)", (long long)nedges);
    PCC_REQUIRE(valid_k(k), "pcc_surface_vertices: node_log2 = %d outside [2, 6]", k);
    hipStream_t st = (hipStream_t)stream;
    const long long n = 3 * (long long)npts;
    const Layout l = layout(n, true);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *k0 = (unsigned long long*)(w + l.keys0), *k1 = (unsigned long long*)(w + l.keys1);
    unsigned *v0 = (unsigned*)(w + l.vals0), *v1 = (unsigned*)(w + l.vals1);
    hipLaunchKernelGGL(k_pairs, dim3(grid_for(npts)), dim3(kBlock), 0, st, (const unsigned long long*)pkeys, (long long)npts, (int)k, k0, v0);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w + l.tmp), bytes, (const unsigned long long*)k0, k1, (const unsigned*)v0, v1, (int)n, 0,
                                                     63, st));
    hipLaunchKernelGGL(k_fit, dim3(grid_for(nedges)), dim3(kBlock), 0, st, (const unsigned long long*)edge_keys, (long long)nedges,
                       (const unsigned long long*)k1, (const unsigned*)v1, n, (int)k, flags, t);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_surface_count_workspace_bytes(int64_t nleaves) { return valid_count(nleaves) ? layout(nleaves, false).total : 0; }

PCC_API int pcc_surface_count(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, const uint64_t* edge_keys, const uint8_t* flags,
                              const uint8_t* t, int64_t nedges, int32_t k, uint64_t* pos, int64_t* hdr, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && leaf_keys && edge_keys && flags && t && pos && hdr && workspace, "pcc_surface_count: NULL argument");
    PCC_REQUIRE(valid_count(nleaves) && valid_count(nedges), "pcc_surface_count: %lld leaves, %lld edges", (long long)nleaves, (long long)nedges);
    PCC_REQUIRE(valid_k(k), "pcc_surface_count: node_log2 = %d outside [2, 6]", k);
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(nleaves, false);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long* cnt = (unsigned long long*)(w + l.keys0);
    long long* H = (long long*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, 8 * PCC_SURFACE_HDR_WORDS, st));
    raster<false>(k, st, (const unsigned long long*)leaf_keys, (long long)nleaves, (const unsigned long long*)edge_keys, flags, t, (long long)nedges, 0,
                  cnt, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ll);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum((void*)(w + l.tmp), bytes, (const unsigned long long*)cnt, (unsigned long long*)pos, (int)nleaves,
                                                   st));
    hipLaunchKernelGGL(k_total, dim3(1), dim3(1), 0, st, (const unsigned long long*)cnt, (const unsigned long long*)pos, (long long)nleaves, H);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API size_t pcc_surface_reconstruct_workspace_bytes(int64_t total) { return valid_count(total) ? layout(total, false).total : 0; }

PCC_API int pcc_surface_reconstruct(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, const uint64_t* edge_keys, const uint8_t* flags,
                                    const uint8_t* t, int64_t nedges, int32_t k, int32_t resolution, const uint64_t* pos, int64_t total,
                                    int32_t* pts, int64_t* hdr, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && leaf_keys && edge_keys && flags && t && pos && pts && hdr && workspace, "pcc_surface_reconstruct: NULL argument");
    PCC_REQUIRE(valid_count(nleaves) && valid_count(nedges) && valid_count(total), "pcc_surface_reconstruct: %lld leaves, %lld edges, %lld voxels",
                (long long)nleaves, (long long)nedges, (long long)total);
    PCC_REQUIRE(valid_k(k), "pcc_surface_reconstruct: node_log2 = %d outside [2, 6]", k);
    PCC_REQUIRE(resolution >= 1 && resolution <= (1 << 21), "pcc_surface_reconstruct: resolution = %d outside [1, 2^21]", resolution);
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(total, false);
    unsigned char* w = (unsigned char*)workspace;
    unsigned long long *k0 = (unsigned long long*)(w + l.keys0), *k1 = (unsigned long long*)(w + l.keys1);
    void* tmp = (void*)(w + l.tmp);
    long long* H = (long long*)hdr;
    PCC_CHECK_HIP(hipMemsetAsync(H, 0, 8 * PCC_SURFACE_HDR_WORDS, st));
    PCC_CHECK_HIP(hipMemsetAsync(k0, 0, (size_t)total * 8, st));          // a wrong `pos` leaves gaps: defined bytes, not stale ones
    raster<true>(k, st, (const unsigned long long*)leaf_keys, (long long)nleaves, (const unsigned long long*)edge_keys, flags, t, (long long)nedges,
                 (int)resolution - 1, (unsigned long long*)nullptr, (const unsigned long long*)pos, k0, (long long)total);
    size_t bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, bytes, (const unsigned long long*)k0, k1, (int)total, 0, 63, st));
    bytes = l.tmp_bytes;
    PCC_CHECK_HIP(hipcub::DeviceSelect::Unique(tmp, bytes, (const unsigned long long*)k1, k0, H, (int)total, st));
    hipLaunchKernelGGL(k_points, dim3(grid_for(total)), dim3(kBlock), 0, st, (const unsigned long long*)k0, (const long long*)H, (long long)total, pts);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
