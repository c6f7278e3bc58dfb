// D2 (point-to-plane) statistics on the GPU (round 4; src/utils/pc_metric.py:109-131 inside the search of src/model_opt.py:33-73).
//
// D2 needs WHICH point is nearest, not only how far it is: nearest-INDEX transforms replace the distance transforms.  Ties are
// the rule on a voxel grid and the reference's own numbers depend on the pick of scipy's KD-tree (pc_metric.py:114), so the rule
// here is stated and deterministic: among equidistant candidates the one with the LOWEST (x, y, z) in lexicographic order (= the
// lowest row-major voxel index, the order of np.argwhere).  Per pass of the separable transform that is "smaller coordinate
// wins a tie", which composes to the lexicographic rule (DESIGN_HISTORY.md 3.8).
//   B -> A (once per block): full-grid index transform of A -> a*(v); e(v) = ((v - a*) . n[a*])^2 in fp64;
//        D2_BA(t) = sum_{v : level(v) > t} e(v), one workgroup per (block, t), fixed summation order.
//   A -> B (per threshold):  z and y passes on the grid, x pass at the points of A -> b*(a, t);  the decoded point b* gets the MEAN
//        normal of the original points that chose it, summed in ascending point order like the reference's loop (pc_metric.py:16-18):
//        one stable radix sort of the (block, t, b*) keys of a whole chunk of thresholds groups them;
//        D2_AB(t) = sum_a ((a - b*) . mean_n(b*))^2, one workgroup per (block, t), fixed order.
// No float atomics anywhere: the results are bit-reproducible.
#include <hipcub/hipcub.hpp>

#include "cloud_tally.h"
#include "search_common.h"

namespace {

constexpr unsigned char kNo8 = 0xFF;
constexpr unsigned short kNo16 = 0xFFFF;

// The 64-bit key of both grouping sorts: block << 32 | slot << 24 | voxel, sorted on its low 48 bits.  voxel = the row-major index inside
// a block, < 2^21 (edges <= 128); slot = the threshold's place in the resident chunk, < 256 (chunks hold <= 64); block < B <= 65535 (D1
// call), so that block 0xFFFF does not exist and kPadKey sorts behind every key.
constexpr unsigned long long kPadKey = ~0ull;
__device__ __forceinline__ unsigned long long search_key(int block, int slot, unsigned voxel) {
    return ((unsigned long long)block << 32) | ((unsigned long long)slot << 24) | voxel;
}
struct SearchKey { unsigned slot, voxel; };
__device__ __forceinline__ SearchKey search_key_decode(unsigned long long key) { return {(unsigned)((key >> 24) & 0xFF), (unsigned)(key & 0xFFFFFFu)}; }

// nearest set voxel along z (level > t), ties -> the smaller z.  thread <-> (line (x,y), t); out: [b][tl][x][y][z] uint8
__global__ void __launch_bounds__(256) k_ft_z(const unsigned char* __restrict__ lev, const int* __restrict__ tcount, int tmax, int t0,
                                              int lines, int W, unsigned char* __restrict__ out) {
    const int b = blockIdx.z, tl = blockIdx.y, t = t0 + tl;
    if (t >= live_thresholds(tcount, b)) return;
    const int line = blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= lines) return;
    const unsigned char* l = lev + ((size_t)b * lines + line) * W;
    unsigned char* o = out + (((size_t)b * tmax + tl) * lines + line) * W;
    int last = -1;
    for (int z = 0; z < W; ++z) {
        if (l[z] > t) last = z;
        o[z] = last < 0 ? kNo8 : (unsigned char)last;
    }
    int nxt = -1;
    for (int z = W - 1; z >= 0; --z) {
        if (l[z] > t) nxt = z;
        const int prev = o[z] == kNo8 ? -1 : (int)o[z];
        if (nxt >= 0 && (prev < 0 || nxt - z < z - prev)) o[z] = (unsigned char)nxt;        // strictly nearer only: a tie keeps the smaller z
    }
}

// y pass: (y*, z*) minimising (y - y')^2 + (z - z*(x, y', z))^2, ties -> the smaller y'.  thread <-> output voxel
__global__ void __launch_bounds__(256) k_ft_y(const unsigned char* __restrict__ in, const int* __restrict__ tcount, int tmax, int t0,
                                              size_t nvox, int H, int W, unsigned short* __restrict__ out) {
    const int b = blockIdx.z, tl = blockIdx.y, t = t0 + tl;
    if (t >= live_thresholds(tcount, b)) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    const size_t base = ((size_t)b * tmax + tl) * nvox;
    const auto [x, y, z] = voxel_xyz(i, H, W);
    const unsigned char* c = in + base + i;
    unsigned best = 0xFFFFFFFFu, by = 0, bz = 0;
    if (c[0] != kNo8) { const int dz = z - c[0]; best = (unsigned)(dz * dz); by = (unsigned)y; bz = c[0]; }
    for (int d = 1; d < H; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd > best) break;                               // (>: a candidate at dd == best can still tie with a smaller y')
        if (y - d >= 0) {
            const unsigned char zs = c[-(ptrdiff_t)d * W];
            if (zs != kNo8) { const int dz = z - zs; const unsigned tot = dd + (unsigned)(dz * dz); if (tot <= best) { best = tot; by = (unsigned)(y - d); bz = zs; } }
        }
        if (y + d < H) {
            const unsigned char zs = c[(ptrdiff_t)d * W];
            if (zs != kNo8) { const int dz = z - zs; const unsigned tot = dd + (unsigned)(dz * dz); if (tot < best) { best = tot; by = (unsigned)(y + d); bz = zs; } }
        }
    }
    out[base + i] = best == 0xFFFFFFFFu ? kNo16 : (unsigned short)((by << 8) | bz);
}

// x pass over the full grid (index transform of A): out = x* << 16 | y* << 8 | z*, 0xFFFFFFFF = empty block
__global__ void __launch_bounds__(256) k_ft_x_full(const unsigned short* __restrict__ in, size_t nvox, int D, int H, int W,
                                                   unsigned* __restrict__ out) {
    const int b = blockIdx.z;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    const Voxel v = voxel_xyz(i, H, W);
    const int x = v.x, y = v.y, z = v.z;
    const size_t hw = (size_t)H * W;
    const unsigned short* c = in + (size_t)b * nvox + i;
    unsigned best = 0xFFFFFFFFu, arg = 0xFFFFFFFFu;
    auto cand = [&](int xs, unsigned dd, bool tie_wins) {
        const unsigned short e = c[((ptrdiff_t)xs - x) * (ptrdiff_t)hw];
        if (e == kNo16) return;
        const int dy = y - (e >> 8), dz = z - (e & 255);
        const unsigned tot = dd + (unsigned)(dy * dy + dz * dz);
        if (tot < best || (tie_wins && tot == best)) { best = tot; arg = ((unsigned)xs << 16) | e; }
    };
    cand(x, 0, false);
    for (int d = 1; d < D; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd > best) break;
        if (x - d >= 0) cand(x - d, dd, true);
        if (x + d < D) cand(x + d, dd, false);
    }
    out[(size_t)b * nvox + i] = arg;
}

// point index of every occupied voxel (lowest index when a voxel holds several points)
__global__ void __launch_bounds__(256) k_index_grid(const int* __restrict__ pts, const int* __restrict__ block_of, long long npts,
                                                    int D, int H, int W, int* __restrict__ grid) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const int x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (x < 0 || x >= D || y < 0 || y >= H || z < 0 || z >= W) return;
    atomicMin(&grid[(((size_t)block_of[i] * D + x) * H + y) * W + z], (int)i);
}

// e(v) = ((v - a*) . n[a*])^2 for the voxels that can be decoded at all (level >= 1)
__global__ void __launch_bounds__(256) k_plane_err_ba(const unsigned char* __restrict__ lev, const unsigned* __restrict__ fta,
                                                      const int* __restrict__ idxgrid, const float* __restrict__ normals,
                                                      size_t nvox, int D, int H, int W, double* __restrict__ e) {
    const int b = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    double val = 0.0;
    const unsigned a = fta[(size_t)b * nvox + i];
    if (lev[(size_t)b * nvox + i] && a != 0xFFFFFFFFu) {
        const int xs = (int)(a >> 16), ys = (int)((a >> 8) & 255), zs = (int)(a & 255);
        const auto [x, y, z] = voxel_xyz(i, H, W);
        const int pi = idxgrid[(size_t)b * nvox + voxel_index(xs, ys, zs, H, W)];
        const double proj = (double)(x - xs) * (double)normals[(size_t)pi * 3] + (double)(y - ys) * (double)normals[(size_t)pi * 3 + 1] +
                            (double)(z - zs) * (double)normals[(size_t)pi * 3 + 2];
        val = proj * proj;
    }
    e[(size_t)b * nvox + i] = val;
}

// D2_BA[b][t] = sum of e over the voxels with level > t.  One workgroup per (t, block); thread k adds voxels k, k + 256, ... in order
__global__ void __launch_bounds__(256) k_d2_ba(const unsigned char* __restrict__ lev, const double* __restrict__ e,
                                               const int* __restrict__ tcount, size_t nvox, double* __restrict__ d2_ba) {
    __shared__ double sh[256];
    const int t = blockIdx.x, b = blockIdx.y;
    if (t >= live_thresholds(tcount, b)) return;
    double s = 0.0;
    for (size_t i = threadIdx.x; i < nvox; i += 256)
        if (lev[(size_t)b * nvox + i] > t) s += e[(size_t)b * nvox + i];
    s = tree256(s, sh, Sum());
    if (threadIdx.x == 0) d2_ba[(size_t)b * kT + t] = s;
}

// x pass at the points of A: b*(a, t) (row-major voxel index) as the key (block, t, b*) of the grouping sort
__global__ void __launch_bounds__(256) k_ft_points(const unsigned short* __restrict__ g, const int* __restrict__ tcount, int tmax, int t0,
                                                   const int* __restrict__ pts, const int* __restrict__ block_of, long long npts,
                                                   int D, int H, int W, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int tl = blockIdx.y, t = t0 + tl;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = kPadKey;
    if (i < npts) {
        const int b = block_of[i];
        if (t < live_thresholds(tcount, b)) {
            const int xa = pts[i * 3], ya = pts[i * 3 + 1], za = pts[i * 3 + 2];
            const size_t hw = (size_t)H * W;
            const unsigned short* c = g + ((size_t)b * tmax + tl) * D * hw + (size_t)ya * W + za;
            unsigned best = 0xFFFFFFFFu, arg = 0;
            auto cand = [&](int xs, unsigned dd, bool tie_wins) {
                const unsigned short e = c[(size_t)xs * hw];
                if (e == kNo16) return;
                const int dy = ya - (e >> 8), dz = za - (e & 255);
                const unsigned tot = dd + (unsigned)(dy * dy + dz * dz);
                if (tot < best || (tie_wins && tot == best)) { best = tot; arg = (unsigned)voxel_index(xs, e >> 8, e & 255, H, W); }
            };
            cand(xa, 0, false);
            for (int d = 1; d < D; ++d) {
                const unsigned dd = (unsigned)(d * d);
                if (dd > best) break;
                if (xa - d >= 0) cand(xa - d, dd, true);
                if (xa + d < D) cand(xa + d, dd, false);
            }
            key = search_key(b, tl, arg);
        }
        keys[(size_t)tl * npts + i] = key;
        vals[(size_t)tl * npts + i] = (unsigned)i;
    }
}

// sorted (block, t, b*) groups: the head of a group sums the normals of its members in ascending point order (the stable sort kept
// it), every member gets ((a - b*) . mean)^2 written at its own (t, point) slot
__global__ void __launch_bounds__(256) k_group_plane_err(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                         size_t n, const int* __restrict__ pts, const float* __restrict__ normals,
                                                         long long npts, int H, int W, double* __restrict__ err) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned long long key = keys[j];
    if (key == kPadKey || (j > 0 && keys[j - 1] == key)) return;          // not a group head
    double sx = 0.0, sy = 0.0, sz = 0.0, cnt = 0.0;
    size_t end = j;
    for (; end < n && keys[end] == key; ++end) {
        const size_t pi = vals[end];
        sx += (double)normals[pi * 3]; sy += (double)normals[pi * 3 + 1]; sz += (double)normals[pi * 3 + 2]; cnt += 1.0;
    }
    sx /= cnt; sy /= cnt; sz /= cnt;
    const SearchKey k = search_key_decode(key);
    const auto [xs, ys, zs] = voxel_xyz(k.voxel, H, W);
    for (size_t m = j; m < end; ++m) {
        const size_t pi = vals[m];
        const double proj = (double)(pts[pi * 3] - xs) * sx + (double)(pts[pi * 3 + 1] - ys) * sy + (double)(pts[pi * 3 + 2] - zs) * sz;
        err[(size_t)k.slot * npts + pi] = proj * proj;
    }
}

struct Larger {
    __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
};

// D2_AB[b][t0 + tl] = sum over the points of block b of err[tl][.], fixed order
// HD (the Hausdorff entries): H2_AB[b][t0 + tl] = the largest of the same doubles beside it (a maximum has no order to fix; the terms are
// squares: finite, >= 0).  HD = false: the kernel of the plain entries.
template <bool HD>
__global__ void __launch_bounds__(256) k_d2_ab(const double* __restrict__ err, const int* __restrict__ block_start, const int* __restrict__ tcount,
                                               int t0, long long npts, double* __restrict__ d2_ab, double* __restrict__ h2_ab) {
    __shared__ double sh[256];
    __shared__ double shm[HD ? 256 : 1];
    const int tl = blockIdx.x, b = blockIdx.y, t = t0 + tl;
    if (t >= live_thresholds(tcount, b)) return;
    double s = 0.0;
    [[maybe_unused]] double m = 0.0;
    for (long long i = block_start[b] + threadIdx.x; i < block_start[b + 1]; i += 256) {
        const double e = err[(size_t)tl * npts + i];
        s += e;
        if constexpr (HD) m = Larger()(m, e);
    }
    s = tree256(s, sh, Sum());
    if (threadIdx.x == 0) d2_ab[(size_t)b * kT + t] = s;
    if constexpr (HD) {
        m = tree256(m, shm, Larger());
        if (threadIdx.x == 0) h2_ab[(size_t)b * kT + t] = m;
    }
}

// H2_BA by level: hmax[b][k] = the largest e(v) over the voxels of level k, the doubles k_d2_ba adds.  They are squares (finite, >= 0), so
// the order of their bit patterns as unsigned 64-bit integers is their order as numbers and an integer atomic maximum is exact, whatever
// order the voxels arrive in: a table of 256 maxima per workgroup in LDS, then one global atomic maximum per level met.  hmax is
// zero-filled by the caller (the bits of 0.0); H2_BA(t) = max_{k>t} hmax[b][k] is formed on the host like the suffix sums.
__global__ void __launch_bounds__(256) k_level_max(const unsigned char* __restrict__ lev, const double* __restrict__ e, size_t nvox,
                                                   unsigned long long* __restrict__ hmax) {
    __shared__ unsigned long long smax[kT];
    const int b = blockIdx.y;
    for (int j = threadIdx.x; j < kT; j += blockDim.x) smax[j] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (size_t)gridDim.x * blockDim.x) {
        const int k = lev[(size_t)b * nvox + i];
        if (k) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(e[(size_t)b * nvox + i]);
            if (bits) atomicMax(&smax[k], bits);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kT; j += blockDim.x)
        if (smax[j]) atomicMax(&hmax[(size_t)b * kT + j], smax[j]);
}

struct D2Layout {
    size_t ftz, fty, fta, idx, e, keys0, keys1, vals0, vals1, err, sort_tmp, sort_tmp_bytes, total;
    int TC;
};
D2Layout d2_layout(int32_t B, size_t nvox, int64_t npts) {
    D2Layout l;
    // thresholds resident at a time: 3 bytes per voxel of index grids, 32 bytes per point of sort / error buffers -> ~1 GiB
    size_t tc = ((size_t)1 << 30) / ((size_t)B * nvox * 3 + (size_t)npts * 32 + 1);
    l.TC = (int)(tc < 4 ? 4 : tc > 64 ? 64 : tc);
    Carver w;
    l.ftz = w.take((size_t)B * l.TC * nvox);
    l.fty = w.take((size_t)B * l.TC * nvox * 2);
    l.fta = w.take((size_t)B * nvox * 4);
    l.idx = w.take((size_t)B * nvox * 4);
    l.e = w.take((size_t)B * nvox * 8);
    const size_t pairs = (size_t)l.TC * (size_t)npts;
    l.keys0 = w.take(pairs * 8);
    l.keys1 = w.take(pairs * 8);
    l.vals0 = w.take(pairs * 4);
    l.vals1 = w.take(pairs * 4);
    l.err = w.take(pairs * 8);
    l.sort_tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, l.sort_tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)(pairs ? pairs : 1), 0, 48, (hipStream_t)0);
    l.sort_tmp = w.take(l.sort_tmp_bytes + 256);
    l.total = w.o + 4096;
    return l;
}

// =====================================================================================================================
// Tie-averaged D2 statistics (pcc_d12_threshold_stats_ties): DESIGN.md 4.8.1 ("Tie-averaged D2") applied per (block, threshold) with
// A = the block's rows and B = B_t.  Every equidistant nearest point counts: a decoded voxel takes the mean normal of ALL rows that
// have it in their tie set, a row's term is the mean plane error over its tie set, a voxel's term the mean over ALL rows at its
// smallest distance.  Nothing depends on which of several equidistant points an engine meets first, so the sums equal the host
// restatement (model_opt.host_threshold_stats(ties='mean')) up to float64 rounding.  The D1 outputs come from the same
// pcc_d1_threshold_stats call as pcc_d12_threshold_stats'.
//   B -> A (once per block): d^2(v) is the EDT of A the D1 call left in its workspace.  Every voxel of level >= 1 walks the block's
//        rows (staged through LDS, increasing row) and averages e over the rows at exactly that distance; k_d2_ba's per-threshold
//        sum over the level sets follows.
//   A -> B (per chunk of thresholds): z/y pass -> in-plane squared distance g[x'][y][z]; the x pass at a row gives d^2_t(a); the tie
//        set is then enumerated exactly: every plane x' with (x_a - x')^2 + g[x'][y_a][z_a] == d^2 holds the lattice points of the
//        circle of the remaining radius^2 around (y_a, z_a), of which those of level > t belong.  Count, exclusive scan, emit
//        (block, t, voxel) -> pair at offsets that increase with (t, row), stable radix sort by key: every group lists its rows in
//        increasing order; the head of a group sums their normals in that order and writes e of every member; each row averages e
//        over its own pairs; k_d2_ab's fixed-order sum per (block, t) follows.
// The pair count of a chunk is only known on the device (the pair list of cloud_tally.h): past the caller's capacity no pair is
// written, the chunk's later kernels return early, and k_pair_nan turns every D2 slot into NaN.  status = (largest pair count of a
// chunk, overflowed).  No float atomics, every sum in a fixed order, vector stores only.
// B -> A: ebar[b][v] = mean of e(v - a, n[a]) over ALL rows a of block b with |v - a|^2 == edt_a[v], for the voxels of level >= 1
// (0 elsewhere).  thread <-> voxel; the rows pass through LDS in tiles of 256, in increasing row.
__global__ void __launch_bounds__(256) k_tie_ba(const unsigned char* __restrict__ lev, const unsigned short* __restrict__ edt_a,
                                                const int* __restrict__ pts, const double* __restrict__ normals,
                                                const int* __restrict__ block_start, size_t nvox, int H, int W, double* __restrict__ ebar) {
    __shared__ int sp[256][3];
    __shared__ double sn[256][3];
    const int b = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < nvox && lev[(size_t)b * nvox + i] != 0;
    const int any = __syncthreads_or(live ? 1 : 0);
    if (!any) {
        if (i < nvox) ebar[(size_t)b * nvox + i] = 0.0;
        return;
    }
    const auto [x, y, z] = voxel_xyz(i, H, W);
    const int want = live ? (int)edt_a[(size_t)b * nvox + i] : -1;
    double acc = 0.0, cnt = 0.0;
    const int lo = block_start[b], hi = block_start[b + 1];
    for (int r0 = lo; r0 < hi; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        if (r < hi) {
            sp[threadIdx.x][0] = pts[(size_t)r * 3]; sp[threadIdx.x][1] = pts[(size_t)r * 3 + 1]; sp[threadIdx.x][2] = pts[(size_t)r * 3 + 2];
            sn[threadIdx.x][0] = normals[(size_t)r * 3]; sn[threadIdx.x][1] = normals[(size_t)r * 3 + 1]; sn[threadIdx.x][2] = normals[(size_t)r * 3 + 2];
        }
        __syncthreads();
        const int n = hi - r0 < 256 ? hi - r0 : 256;
        if (live) {
            for (int k = 0; k < n; ++k) {
                const int gx = x - sp[k][0], gy = y - sp[k][1], gz = z - sp[k][2];
                if (gx * gx + gy * gy + gz * gz == want) { acc += plane_term((double)gx, (double)gy, (double)gz, sn[k][0], sn[k][1], sn[k][2]); cnt += 1.0; }
            }
        }
        __syncthreads();
    }
    if (i < nvox) ebar[(size_t)b * nvox + i] = cnt > 0.0 ? acc / cnt : 0.0;
}

__device__ __forceinline__ int tie_isqrt(int v) {
    int s = (int)sqrtf((float)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// Every voxel of level > t at squared distance exactly d2 from (xa, ya, za), given that d2 is the smallest such distance: f(row-major
// voxel index), in a fixed order (x' ascending, then |dy| ascending, -dy before +dy, -dz before +dz).  l = the block's levels.
template <typename F>
__device__ __forceinline__ void tie_for_each(const unsigned short* __restrict__ c, const unsigned char* __restrict__ l, int t, int D, int H,
                                             int W, int xa, int ya, int za, unsigned d2, F f) {
    const size_t hw = (size_t)H * W;
    const int reach = tie_isqrt((int)d2);
    const int x_lo = xa - reach > 0 ? xa - reach : 0, x_hi = xa + reach < D - 1 ? xa + reach : D - 1;
    for (int xs = x_lo; xs <= x_hi; ++xs) {
        const int dx = xa - xs, r = (int)d2 - dx * dx;
        if (r < 0 || (int)c[(size_t)xs * hw] != r) continue;       // (kInf = 65535 > any r <= 3 * 127^2: an empty plane never matches)
        for (int dy = 0; dy * dy <= r; ++dy) {
            const int rem = r - dy * dy, dz = tie_isqrt(rem);
            if (dz * dz != rem) continue;
            for (int sy = (dy ? -1 : 1); sy <= 1; sy += 2) {
                const int y = ya + sy * dy;
                if (y < 0 || y >= H) continue;
                for (int sz = (dz ? -1 : 1); sz <= 1; sz += 2) {
                    const int z = za + sz * dz;
                    if (z < 0 || z >= W) continue;
                    const size_t v = voxel_index(xs, y, z, H, W);
                    if ((int)l[v] > t) f((unsigned)v);
                }
            }
        }
    }
}

// pass 1: |T_B(a)| and d^2_t(a) of every (slot, row); 0 pairs where t >= tcount[block]
__global__ void __launch_bounds__(256) k_tie_count(const unsigned short* __restrict__ g, const unsigned char* __restrict__ lev,
                                                   const int* __restrict__ tcount, int tmax, int t0, const int* __restrict__ pts,
                                                   const int* __restrict__ block_of, long long npts, int D, int H, int W,
                                                   unsigned long long* __restrict__ cnt, unsigned* __restrict__ dist) {
    const int tl = blockIdx.y, t = t0 + tl;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const int b = block_of[i];
    unsigned long long n = 0;
    unsigned d2 = 0;
    const int xa = pts[i * 3], ya = pts[i * 3 + 1], za = pts[i * 3 + 2];
    const bool inside = xa >= 0 && xa < D && ya >= 0 && ya < H && za >= 0 && za < W;      // (k_occupancy's rule: a row outside the grid takes no part)
    if (inside && t < live_thresholds(tcount, b)) {
        const size_t hw = (size_t)H * W, nvox = (size_t)D * hw;
        const unsigned short* c = g + ((size_t)b * tmax + tl) * nvox + (size_t)ya * W + za;
        d2 = edt_x_pass(c, hw, xa, D);
        tie_for_each(c, lev + (size_t)b * nvox, t, D, H, W, xa, ya, za, d2, [&](unsigned) { ++n; });
    }
    cnt[(size_t)tl * npts + i] = n;
    dist[(size_t)tl * npts + i] = d2;
}

// pass 2: the pairs of (slot, row) at [off, off + cnt): key (block, slot, voxel), value = the pair's own position; prow = its row
__global__ void __launch_bounds__(256) k_tie_emit(const unsigned short* __restrict__ g, const unsigned char* __restrict__ lev,
                                                  const int* __restrict__ tcount, int tmax, int t0, const int* __restrict__ pts,
                                                  const int* __restrict__ block_of, long long npts, int D, int H, int W,
                                                  const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                                  const unsigned* __restrict__ dist, const TieCtl* __restrict__ ctl, unsigned long long cap,
                                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ vals, unsigned* __restrict__ prow) {
    if (ctl->overflow) return;
    const int tl = blockIdx.y, t = t0 + tl;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const size_t slot = (size_t)tl * npts + i;
    const unsigned long long n = cnt[slot];
    if (n == 0) return;
    const int b = block_of[i];
    const int xa = pts[i * 3], ya = pts[i * 3 + 1], za = pts[i * 3 + 2];
    const size_t hw = (size_t)H * W, nvox = (size_t)D * hw;
    const unsigned short* c = g + ((size_t)b * tmax + tl) * nvox + (size_t)ya * W + za;
    unsigned long long p = off[slot];
    const unsigned long long end = p + n;
    const unsigned long long head = search_key(b, tl, 0);      // the voxel field is or-ed in per pair
    tie_for_each(c, lev + (size_t)b * nvox, t, D, H, W, xa, ya, za, dist[slot], [&](unsigned v) {
        if (p < end && p < cap) { keys[p] = head | v; vals[p] = (unsigned)p; prow[p] = (unsigned)i; }
        ++p;
    });
}

// sorted groups (block, slot, voxel): the head sums the normals of the group's rows in increasing row (the stable sort kept the
// emit order) and writes e(a - voxel, mean normal) of every member at the pair's own position
__global__ void __launch_bounds__(256) k_tie_groups(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                    const unsigned* __restrict__ prow, const TieCtl* __restrict__ ctl, unsigned long long cap,
                                                    const int* __restrict__ pts, const double* __restrict__ normals, int H, int W,
                                                    double* __restrict__ perr) {
    if (ctl->overflow) return;
    const unsigned long long n = ctl->pairs < cap ? ctl->pairs : cap;
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned long long key = keys[j];
    if (j > 0 && keys[j - 1] == key) return;            // not a group head
    double sx = 0.0, sy = 0.0, sz = 0.0, votes = 0.0;
    unsigned long long end = j;
    for (; end < n && keys[end] == key; ++end) {
        const size_t r = prow[vals[end]];
        sx += normals[r * 3]; sy += normals[r * 3 + 1]; sz += normals[r * 3 + 2]; votes += 1.0;
    }
    sx /= votes; sy /= votes; sz /= votes;
    const auto [xs, ys, zs] = voxel_xyz(search_key_decode(key).voxel, H, W);
    for (unsigned long long m = j; m < end; ++m) {
        const unsigned p = vals[m];
        const size_t r = prow[p];
        perr[p] = plane_term((double)(pts[r * 3] - xs), (double)(pts[r * 3 + 1] - ys), (double)(pts[r * 3 + 2] - zs), sx, sy, sz);
    }
}

// err[slot][row] = mean of perr over the row's own pairs (emit order)
__global__ void __launch_bounds__(256) k_tie_row_mean(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                                      const double* __restrict__ perr, const TieCtl* __restrict__ ctl, size_t n,
                                                      double* __restrict__ err) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double v = 0.0;
    if (!ctl->overflow && cnt[s]) {
        const unsigned long long o = off[s], c = cnt[s];
        double acc = 0.0;
        for (unsigned long long k = 0; k < c; ++k) acc += perr[o + k];
        v = acc / (double)c;
    }
    err[s] = v;
}

struct TieLayout {
    size_t g0, g1, ebar, cnt, off, dist, err, ctl, keys0, keys1, vals0, vals1, prow, perr, scan_tmp, scan_tmp_bytes, sort_tmp, sort_tmp_bytes, total;
    int TC;
};
int tie_chunk(int32_t B, size_t nvox) {
    const int tc = chunk_thresholds(B, nvox);
    return tc > 64 ? 64 : tc;
}
TieLayout tie_layout(int32_t B, size_t nvox, int64_t npts, int64_t max_pairs) {
    TieLayout l;
    l.TC = tie_chunk(B, nvox);
    const size_t slots = (size_t)l.TC * (size_t)npts, cap = (size_t)max_pairs;
    Carver w;
    l.g0 = w.take((size_t)B * l.TC * nvox * 2);
    l.g1 = w.take((size_t)B * l.TC * nvox * 2);
    l.ebar = w.take((size_t)B * nvox * 8);
    l.cnt = w.take(slots * 8);
    l.off = w.take(slots * 8);
    l.dist = w.take(slots * 4);
    l.err = w.take(slots * 8);
    l.ctl = w.take(sizeof(TieCtl));
    l.keys0 = w.take(cap * 8);
    l.keys1 = w.take(cap * 8);
    l.vals0 = w.take(cap * 4);
    l.vals1 = w.take(cap * 4);
    l.prow = w.take(cap * 4);
    l.perr = w.take(cap * 8);
    l.scan_tmp_bytes = l.sort_tmp_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum((void*)nullptr, l.scan_tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                           (int)(slots ? slots : 1), (hipStream_t)0);
    l.scan_tmp = w.take(l.scan_tmp_bytes + 256);
    (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, l.sort_tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                             (const unsigned*)nullptr, (unsigned*)nullptr, (int)(cap ? cap : 1), 0, 48, (hipStream_t)0);
    l.sort_tmp = w.take(l.sort_tmp_bytes + 256);
    l.total = w.o + 4096;
    return l;
}

}  // namespace

PCC_API size_t pcc_d12_search_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int64_t npts) {
    return d2_layout(B, (size_t)D * H * W, npts).total;
}

// As pcc_d1_threshold_stats (same D1 outputs, computed by the same kernels), plus the D2 sums of every threshold:
//   normals: (npts, 3) float32 (device), block_start: (B + 1,) int32 offsets of the blocks' points in pts (device),
//   workspace: pcc_d1_search_workspace_bytes, workspace2: pcc_d12_search_workspace_bytes,
//   d2_ab, d2_ba: (B, 256) float64 (device), entry [b][t] valid for t < tcount[b].
// The level grid comes from `src` (search_common.h): the D1 call builds it, everything here reads `lev` and `tcount` alone.
// hd1 / h2_ab / h2_max (the Hausdorff entries; NULL in the plain ones, which launch the kernels they always did): the D1 maxima of
// search_common.h's SearchHausdorff and, (B,256) float64, zero-filled here, h2_ab[b][t] = the largest term of d2_ab[b][t], h2_max[b][k] =
// the largest term of d2_ba among the voxels of level k.
static int d12_stats(pcc_ctx* ctx, const LevelSource& src, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* pts,
                     const int32_t* block_of, const int32_t* block_start, int64_t npts, const float* normals, void* workspace, void* workspace2,
                     uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, void* stream,
                     const SearchHausdorff& hd1 = {}, double* h2_ab = nullptr, double* h2_max = nullptr) {
    PCC_REQUIRE(normals && block_start && workspace2 && d2_ab && d2_ba && pts && npts > 0, "%s: NULL argument", src.who);
    PCC_REQUIRE((size_t)npts * 64 < ((size_t)1 << 31), "%s: too many points for one call", src.who);
    const bool HD = h2_ab != nullptr;
    PCC_REQUIRE(HD == (h2_max != nullptr) && HD == (hd1.h1_ab != nullptr), "%s: NULL argument", src.who);
    // D1 part (and the levels / tcount the D2 part builds on): unchanged kernels
    { const int rc = pcc_search_d1_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream, hd1);
      if (rc != PCC_OK) return rc; }
    const int nthr = src.levels();
    hipStream_t st = (hipStream_t)stream;
    const size_t nvox = (size_t)D * H * W;
    const D2Layout l = d2_layout(B, nvox, npts);
    unsigned char* w2 = (unsigned char*)workspace2;
    unsigned char* ftz = w2 + l.ftz;
    unsigned short* fty = (unsigned short*)(w2 + l.fty);
    unsigned* fta = (unsigned*)(w2 + l.fta);
    int* idx = (int*)(w2 + l.idx);
    double* e = (double*)(w2 + l.e);
    unsigned long long *keys0 = (unsigned long long*)(w2 + l.keys0), *keys1 = (unsigned long long*)(w2 + l.keys1);
    unsigned *vals0 = (unsigned*)(w2 + l.vals0), *vals1 = (unsigned*)(w2 + l.vals1);
    double* err = (double*)(w2 + l.err);
    // buffers of the D1 call that are still valid: levels, occupancy and its "one" counter
    const D1Layout l1 = d1_layout(B, nvox);
    unsigned char* w1 = (unsigned char*)workspace;
    unsigned char *lev = w1 + l1.lev, *occ = w1 + l1.occ;
    int* one = (int*)(w1 + l1.one);
    const int lines = D * H;
    const unsigned vox_blocks = (unsigned)((nvox + 255) / 256);
    const unsigned pblocks = (unsigned)((npts + 255) / 256);
    PCC_CHECK_HIP(hipMemsetAsync(d2_ab, 0, (size_t)B * kT * 8, st));
    PCC_CHECK_HIP(hipMemsetAsync(d2_ba, 0, (size_t)B * kT * 8, st));
    if (HD) {
        PCC_CHECK_HIP(hipMemsetAsync(h2_ab, 0, (size_t)B * kT * 8, st));
        PCC_CHECK_HIP(hipMemsetAsync(h2_max, 0, (size_t)B * kT * 8, st));
    }
    // ---- B -> A: index transform of the original points (occupancy as a one-threshold level set), plane error per voxel
    PCC_CHECK_HIP(hipMemsetAsync(idx, 0x7F, (size_t)B * nvox * 4, st));
    hipLaunchKernelGGL(k_index_grid, dim3(pblocks), dim3(256), 0, st, pts, block_of, (long long)npts, D, H, W, idx);
    hipLaunchKernelGGL(k_ft_z, dim3((lines + 255) / 256, 1, B), dim3(256), 0, st, occ, one, 1, 0, lines, W, ftz);
    hipLaunchKernelGGL(k_ft_y, dim3(vox_blocks, 1, B), dim3(256), 0, st, ftz, one, 1, 0, nvox, H, W, fty);
    hipLaunchKernelGGL(k_ft_x_full, dim3(vox_blocks, 1, B), dim3(256), 0, st, fty, nvox, D, H, W, fta);
    hipLaunchKernelGGL(k_plane_err_ba, dim3(vox_blocks, B), dim3(256), 0, st, lev, fta, idx, normals, nvox, D, H, W, e);
    hipLaunchKernelGGL(k_d2_ba, dim3(nthr, B), dim3(256), 0, st, lev, e, tcount, nvox, d2_ba);
    if (HD) hipLaunchKernelGGL(k_level_max, dim3(64, B), dim3(256), 0, st, lev, e, nvox, (unsigned long long*)h2_max);
    // ---- A -> B per chunk of thresholds (the D1 sums of this direction came from the D1 call above)
    for (int t0 = 0; t0 < nthr; t0 += l.TC) {
        const int nt = nthr - t0 < l.TC ? nthr - t0 : l.TC;
        const size_t pairs = (size_t)nt * (size_t)npts;
        hipLaunchKernelGGL(k_ft_z, dim3((lines + 255) / 256, nt, B), dim3(256), 0, st, lev, tcount, l.TC, t0, lines, W, ftz);
        hipLaunchKernelGGL(k_ft_y, dim3(vox_blocks, nt, B), dim3(256), 0, st, ftz, tcount, l.TC, t0, nvox, H, W, fty);
        hipLaunchKernelGGL(k_ft_points, dim3(pblocks, nt), dim3(256), 0, st, fty, tcount, l.TC, t0, pts, block_of, (long long)npts, D, H, W,
                           keys0, vals0);
        size_t tmp = l.sort_tmp_bytes;
        PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w2 + l.sort_tmp), tmp, keys0, keys1, vals0, vals1, (int)pairs, 0, 48, st));
        hipLaunchKernelGGL(k_group_plane_err, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, keys1, vals1, pairs, pts, normals,
                           (long long)npts, H, W, err);
        hipLaunchKernelGGL(HD ? k_d2_ab<true> : k_d2_ab<false>, dim3(nt, B), dim3(256), 0, st, err, block_start, tcount, t0, (long long)npts, d2_ab,
                           h2_ab);
    }
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_d12_threshold_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                                    int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of, const int32_t* block_start,
                                    int64_t npts, const float* normals, void* workspace, void* workspace2, uint64_t* s_ab, uint64_t* hsum,
                                    uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, void* stream) {
    const LevelSource src = {"pcc_d12_threshold_stats", thr, nthr, clip, nullptr, 0, nullptr, 0};
    return d12_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, block_start, npts, normals, workspace, workspace2, s_ab, hsum, hcnt, tcount, d2_ab,
                     d2_ba, stream);
}

// pcc_d12_threshold_stats for the top-counts[b][j] sets of every block (include/pcc_geo.h): only the source of the level grid differs
PCC_API int pcc_d12_count_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts, int32_t J,
                                const int32_t* pts, const int32_t* block_of, const int32_t* block_start, int64_t npts, const float* normals,
                                void* workspace, void* workspace2, void* rank_workspace, size_t rank_workspace_bytes, uint64_t* s_ab,
                                uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, void* stream) {
    PCC_REQUIRE(counts, "pcc_d12_count_stats: NULL argument");
    const LevelSource src = {"pcc_d12_count_stats", nullptr, 0, 0, counts, J, rank_workspace, rank_workspace_bytes};
    return d12_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, block_start, npts, normals, workspace, workspace2, s_ab, hsum, hcnt, tcount, d2_ab,
                     d2_ba, stream);
}

// pcc_d12_threshold_stats / pcc_d12_count_stats with the D1 and D2 Hausdorff terms beside the sums (include/pcc_geo.h "Hausdorff terms of
// the search"): the same kernels with their maxima switched on, so the shared outputs are the same bits
PCC_API int pcc_d12_threshold_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                                              int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of,
                                              const int32_t* block_start, int64_t npts, const float* normals, void* workspace, void* workspace2,
                                              uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba,
                                              uint32_t* h1_ab, uint32_t* h1_max, double* h2_ab, double* h2_max, void* stream) {
    PCC_REQUIRE(h1_ab && h1_max && h2_ab && h2_max, "pcc_d12_threshold_stats_hausdorff: NULL argument");
    const LevelSource src = {"pcc_d12_threshold_stats_hausdorff", thr, nthr, clip, nullptr, 0, nullptr, 0};
    return d12_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, block_start, npts, normals, workspace, workspace2, s_ab, hsum, hcnt, tcount, d2_ab,
                     d2_ba, stream, {h1_ab, h1_max}, h2_ab, h2_max);
}

PCC_API int pcc_d12_count_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts,
                                          int32_t J, const int32_t* pts, const int32_t* block_of, const int32_t* block_start, int64_t npts,
                                          const float* normals, void* workspace, void* workspace2, void* rank_workspace,
                                          size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount,
                                          double* d2_ab, double* d2_ba, uint32_t* h1_ab, uint32_t* h1_max, double* h2_ab, double* h2_max,
                                          void* stream) {
    PCC_REQUIRE(counts && h1_ab && h1_max && h2_ab && h2_max, "pcc_d12_count_stats_hausdorff: NULL argument");
    const LevelSource src = {"pcc_d12_count_stats_hausdorff", nullptr, 0, 0, counts, J, rank_workspace, rank_workspace_bytes};
    return d12_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, block_start, npts, normals, workspace, workspace2, s_ab, hsum, hcnt, tcount, d2_ab,
                     d2_ba, stream, {h1_ab, h1_max}, h2_ab, h2_max);
}

PCC_API int32_t pcc_d12_search_ties_chunk(int32_t B, int32_t D, int32_t H, int32_t W) {
    return tie_chunk(B, (size_t)D * H * W);
}

PCC_API size_t pcc_d12_search_ties_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int64_t npts, int64_t max_pairs) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || npts <= 0 || max_pairs < 1 || max_pairs > 0x7FFFFFFFll) return 0;
    return tie_layout(B, (size_t)D * H * W, npts, max_pairs).total;
}

// As pcc_d12_threshold_stats with float64 normals and the tie-averaged D2 definition (include/pcc_geo.h).  workspace:
// pcc_d1_search_workspace_bytes; workspace2: pcc_d12_search_ties_workspace_bytes(..., max_pairs); status: int64[2] (device).
PCC_API int pcc_d12_threshold_stats_ties(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                                         int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of,
                                         const int32_t* block_start, int64_t npts, const double* normals, int64_t max_pairs,
                                         int64_t* status, void* workspace, void* workspace2, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt,
                                         int32_t* tcount, double* d2_ab, double* d2_ba, void* stream) {
    PCC_REQUIRE(normals && block_start && workspace2 && d2_ab && d2_ba && pts && status && npts > 0, "pcc_d12_threshold_stats_ties: NULL argument");
    PCC_REQUIRE((size_t)npts * 64 < ((size_t)1 << 31), "pcc_d12_threshold_stats_ties: too many points for one call");
    PCC_REQUIRE(max_pairs >= 1 && max_pairs <= 0x7FFFFFFFll, "pcc_d12_threshold_stats_ties: max_pairs outside [1, 2^31)");
    { const int rc = pcc_d1_threshold_stats(ctx, x_hat, B, D, H, W, thr, nthr, clip, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream);
      if (rc != PCC_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    const size_t nvox = (size_t)D * H * W;
    const TieLayout l = tie_layout(B, nvox, npts, max_pairs);
    unsigned char* w2 = (unsigned char*)workspace2;
    unsigned short *g0 = (unsigned short*)(w2 + l.g0), *g1 = (unsigned short*)(w2 + l.g1);
    double *ebar = (double*)(w2 + l.ebar), *err = (double*)(w2 + l.err), *perr = (double*)(w2 + l.perr);
    unsigned long long *cnt = (unsigned long long*)(w2 + l.cnt), *off = (unsigned long long*)(w2 + l.off);
    unsigned* dist = (unsigned*)(w2 + l.dist);
    TieCtl* ctl = (TieCtl*)(w2 + l.ctl);
    unsigned long long *keys0 = (unsigned long long*)(w2 + l.keys0), *keys1 = (unsigned long long*)(w2 + l.keys1);
    unsigned *vals0 = (unsigned*)(w2 + l.vals0), *vals1 = (unsigned*)(w2 + l.vals1), *prow = (unsigned*)(w2 + l.prow);
    // buffers of the D1 call that are still valid: levels and the finished EDT of A
    const D1Layout l1 = d1_layout(B, nvox);
    unsigned char* w1 = (unsigned char*)workspace;
    unsigned char* lev = w1 + l1.lev;
    const unsigned short* edt_a = (const unsigned short*)(w1 + l1.ea0);
    const unsigned long long cap = (unsigned long long)max_pairs;
    const unsigned vox_blocks = (unsigned)((nvox + 255) / 256);
    const unsigned pblocks = (unsigned)((npts + 255) / 256);
    PCC_CHECK_HIP(hipMemsetAsync(d2_ab, 0, (size_t)B * kT * 8, st));
    PCC_CHECK_HIP(hipMemsetAsync(d2_ba, 0, (size_t)B * kT * 8, st));
    PCC_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st));
    // ---- B -> A
    hipLaunchKernelGGL(k_tie_ba, dim3(vox_blocks, B), dim3(256), 0, st, lev, edt_a, pts, normals, block_start, nvox, H, W, ebar);
    hipLaunchKernelGGL(k_d2_ba, dim3(nthr, B), dim3(256), 0, st, lev, ebar, tcount, nvox, d2_ba);
    // ---- A -> B per chunk of thresholds
    for (int t0 = 0; t0 < nthr; t0 += l.TC) {
        const int nt = nthr - t0 < l.TC ? nthr - t0 : l.TC;
        const size_t slots = (size_t)nt * (size_t)npts;
        pcc_search_edt_zy(st, lev, tcount, l.TC, t0, nt, B, D, H, W, g0, g1);
        hipLaunchKernelGGL(k_tie_count, dim3(pblocks, nt), dim3(256), 0, st, g1, lev, tcount, l.TC, t0, pts, block_of, (long long)npts, D, H, W,
                           cnt, dist);
        size_t tmp = l.scan_tmp_bytes;
        PCC_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum((void*)(w2 + l.scan_tmp), tmp, (const unsigned long long*)cnt, off, (int)slots, st));
        hipLaunchKernelGGL(k_pair_total<true>, dim3(1), dim3(1), 0, st, (const unsigned long long*)cnt, (const unsigned long long*)off, slots, cap, ctl,
                           (long long*)status);
        hipLaunchKernelGGL(k_tie_emit, dim3(pblocks, nt), dim3(256), 0, st, g1, lev, tcount, l.TC, t0, pts, block_of, (long long)npts, D, H, W,
                           cnt, off, dist, ctl, cap, keys0, vals0, prow);
        hipLaunchKernelGGL(k_pair_pad<unsigned long long>, dim3(256), dim3(256), 0, st, (const TieCtl*)ctl, cap, kPadKey, keys0, vals0);
        tmp = l.sort_tmp_bytes;
        PCC_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs((void*)(w2 + l.sort_tmp), tmp, keys0, keys1, vals0, vals1, (int)cap, 0, 48, st));
        hipLaunchKernelGGL(k_tie_groups, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, keys1, vals1, prow, ctl, cap, pts, normals, H, W,
                           perr);
        hipLaunchKernelGGL(k_tie_row_mean, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, cnt, off, perr, ctl, slots, err);
        hipLaunchKernelGGL(k_d2_ab<false>, dim3(nt, B), dim3(256), 0, st, err, block_start, tcount, t0, (long long)npts, d2_ab, (double*)nullptr);
    }
    hipLaunchKernelGGL(k_pair_nan, dim3((B * kT + 255) / 256), dim3(256), 0, st, (const long long*)status, B * kT, d2_ab, d2_ba);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
