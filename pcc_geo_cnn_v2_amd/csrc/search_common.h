// What the two sources of the per-block threshold search share: search_d1.hip (the D1 engine and its distance transforms) and
// search_d2.hip (the two D2 engines, which run after a D1 call on the same blocks and read what it left in its workspace).
#pragma once
#include "common.h"

constexpr unsigned short kInf = 0xFFFF;   // no set voxel on the line / plane seen so far
constexpr int kT = 256;

// Thresholds of block b that the engines compute.  Levels are stored as uint8, so a level of 256 (nthr == 256 and a voxel above thr[255])
// is held as 255 and the level set of t = 255 cannot be formed: tcount[b] == 256 reports it, t = 255 is then not computed and every
// output at [b][255] stays zero (include/pcc_geo.h).  tcount[b] <= 255 otherwise, and nothing changes.
__device__ __forceinline__ int live_thresholds(const int* __restrict__ tcount, int b) {
    const int n = tcount[b];
    return n < kT ? n : kT - 1;
}

// Thresholds resident at a time: the level-set EDTs are computed in chunks so that their two uint16 grids per
// (block, threshold) stay within ~1 GiB (32 blocks of 64^3 -> 32 thresholds per chunk; 8 blocks of 128^3 -> 16).
inline int chunk_thresholds(int32_t B, size_t nvox) {
    const size_t per_t = (size_t)B * nvox * 2 * 2;
    size_t tc = ((size_t)1 << 30) / (per_t ? per_t : 1);
    if (tc < 8) tc = 8;
    if (tc > (size_t)kT) tc = kT;
    return (int)tc;
}

// The workspace of pcc_d1_threshold_stats as byte offsets: levels + occupancy (u8), EDT of A ping/pong (u16), level-set EDT ping/pong
// (u16 x TC thresholds), the per-block "1 threshold" counter of the EDT of A (int) and a tail.  The D2 engines run after the D1 call
// and rely on what it leaves there: `occ` and `one` (pick), `lev` and `ea0` = the finished EDT of A (ties), `lev` (both).
struct D1Layout {
    size_t lev, occ, ea0, ea1, g0, g1, one, total;
    int TC;
};
inline D1Layout d1_layout(int32_t B, size_t nvox) {
    D1Layout l;
    l.TC = chunk_thresholds(B, nvox);
    const size_t grid = (size_t)B * nvox, chunk = grid * l.TC * 2;
    l.lev = 0;               l.occ = l.lev + grid;         // u8
    l.ea0 = l.occ + grid;    l.ea1 = l.ea0 + grid * 2;     // u16
    l.g0 = l.ea1 + grid * 2; l.g1 = l.g0 + chunk;          // u16 x TC
    l.one = l.g1 + chunk;
    l.total = l.one + (size_t)B * 64 + 4096;
    return l;
}

// Where the level grid of a search call comes from.  Thresholds (counts == nullptr): level(v) = #{t : x_hat[v] > thr[t]}, k_levels of
// search_d1.hip.  Candidate counts: level(v) = #{j : rank(v) < counts[b][j]}, pcc_rank_levels (rank_levels.hip) with its own workspace.
// Everything behind the grid reads `lev` and `tcount` alone, so both sources share it unchanged.
struct LevelSource {
    const char* who;                       // the public entry, for its messages
    const float* thr; int nthr, clip;
    const int32_t* counts; int J; void* rank_ws; size_t rank_ws_bytes;
    int levels() const { return counts ? J : nthr; }
};
// The D1 Hausdorff outputs of a search call, (B,256) uint32 each, caller-provided (no part of D1Layout); both NULL = the plain entries,
// which launch the kernels without the maxima.  h1_ab[b][t] per candidate, h1_max[b][k] per level (the host forms max_{k>t}).
struct SearchHausdorff {
    uint32_t* h1_ab = nullptr;
    uint32_t* h1_max = nullptr;
};
// pcc_d1_threshold_stats / pcc_d1_count_stats and their _hausdorff forms (search_d1.hip), and what the D2 entries run first
int pcc_search_d1_stats(pcc_ctx* ctx, const LevelSource& src, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* pts,
                        const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount,
                        void* stream, const SearchHausdorff& hd = {});

// Row-major voxel index <-> (x, y, z) on a grid of planes H x W; the divisions are done in the width of the caller's index type
struct Voxel { int x, y, z; };
__device__ __forceinline__ size_t voxel_index(int x, int y, int z, int H, int W) { return ((size_t)x * H + y) * W + z; }
template <typename I>
__device__ __forceinline__ Voxel voxel_xyz(I i, int H, int W) {
    const int z = (int)(i % W), y = (int)((i / W) % H), x = (int)(i / ((I)H * W));
    return {x, y, z};
}

// x pass of the distance transform at one row: d^2 = min_x' (xa - x')^2 + g[x'][ya][za]  (c = g at (x' = 0, ya, za) of the row's
// (block, slot), hw = the stride of a plane)
__device__ __forceinline__ unsigned edt_x_pass(const unsigned short* __restrict__ c, size_t hw, int xa, int D) {
    unsigned best = c[(size_t)xa * hw];
    for (int d = 1; d < D; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd >= best) break;
        if (xa - d >= 0) { const unsigned v = c[(size_t)(xa - d) * hw]; if (v != kInf && v + dd < best) best = v + dd; }
        if (xa + d < D) { const unsigned v = c[(size_t)(xa + d) * hw]; if (v != kInf && v + dd < best) best = v + dd; }
    }
    return best;
}

// z and y passes of the squared distance transform of the level sets {levels > t}, t in [t0, t0 + nt), of B blocks (search_d1.hip):
// g1[b][t - t0 of tmax][x][y][z] = min over (y', z') of the plane; g0: as large, scratch of the two-kernel form.  counts: the tcount
// of live_thresholds.
void pcc_search_edt_zy(hipStream_t st, const unsigned char* levels, const int* counts, int tmax, int t0, int nt, int B, int D, int H,
                       int W, unsigned short* g0, unsigned short* g1);
