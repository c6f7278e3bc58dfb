// Exact per-block D1 statistics for EVERY threshold at once (the search of src/model_opt.py:21-77, which the
// reference does on the CPU with up to 255 KD-tree builds + queries per block, src/utils/pc_metric.py:76-138).
//
// For block b with original points A and reconstruction x_hat, let level k(v) = #{t : x_hat[v] > thr[t]}, so
// that the decoded set at threshold t is B_t = {v : k(v) > t} (nested sets).  All point coordinates are integers,
// hence all squared distances are integers and the sums below are exact:
//     n_B(t)  = |B_t|
//     S_BA(t) = sum_{v in B_t} min_{a in A} |v - a|^2      (one EDT of A + a level histogram)
//     S_AB(t) = sum_{a in A}  min_{v in B_t} |a - v|^2     (EDT of every level set, evaluated at the points of A)
// Squared Euclidean distance transforms are separable: a 1-D two-sweep pass along z, then min-plus passes
// along y and x with early termination (a candidate at axis distance d cannot win once d^2 >= best).
// The host turns these integers into the reference's d1_* metrics and applies its selection logic unchanged.
#include "search_common.h"

namespace {

__global__ void __launch_bounds__(256) k_levels(const float* __restrict__ x, const float* __restrict__ thr, int nthr,
                                                int clip, size_t nvox, unsigned char* __restrict__ lev,
                                                int* __restrict__ maxlev) {
    __shared__ float tab[kT];
    __shared__ int smax;
    for (int j = threadIdx.x; j < nthr; j += blockDim.x) tab[j] = thr[j];
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    const int b = blockIdx.y;
    int m = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (size_t)gridDim.x * blockDim.x) {
        float v = x[(size_t)b * nvox + i];
        if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
        // thresholds are increasing: k = number of thresholds strictly below v (float32 compare, like the codec)
        int lo = 0, hi = nthr;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (v > tab[mid]) lo = mid + 1; else hi = mid; }
        lev[(size_t)b * nvox + i] = (unsigned char)min(lo, 255);
        m = max(m, lo);
    }
    atomicMax(&smax, m);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&maxlev[b], smax);
}

__global__ void __launch_bounds__(256) k_fill_int(int* p, int v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ void __launch_bounds__(256) k_occupancy(const int* __restrict__ pts, const int* __restrict__ block_of,
                                                   long long npts, int D, int H, int W, unsigned char* __restrict__ occ) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += (long long)gridDim.x * blockDim.x) {
        const int x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        if (x < 0 || x >= D || y < 0 || y >= H || z < 0 || z >= W) continue;
        occ[(((size_t)block_of[i] * D + x) * H + y) * W + z] = 1;
    }
}

// 1-D squared distance along z (the contiguous axis) to the nearest voxel with level > t.
// thread <-> (line (x,y), t); grid.z = block.  out: [b][t][x][y][z] uint16.
__global__ void __launch_bounds__(256) k_edt_z(const unsigned char* __restrict__ lev, const int* __restrict__ tcount,
                                               int tmax, int t0, int lines, int W, unsigned short* __restrict__ out) {
    const int b = blockIdx.z, tl = blockIdx.y, t = t0 + tl;      // tl: slot inside the resident chunk of `tmax` thresholds
    if (t >= live_thresholds(tcount, b)) return;
    const int line = blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= lines) return;
    const unsigned char* l = lev + ((size_t)b * lines + line) * W;
    unsigned short* o = out + (((size_t)b * tmax + tl) * lines + line) * W;
    int last = -100000;
    for (int z = 0; z < W; ++z) {           // forward sweep: distance to the previous set voxel
        if (l[z] > t) last = z;
        const int d = z - last;
        o[z] = d < 256 ? (unsigned short)(d * d) : kInf;
    }
    last = 100000;
    for (int z = W - 1; z >= 0; --z) {      // backward sweep
        if (l[z] > t) last = z;
        const int d = last - z;
        if (d < 256) { const unsigned short q = (unsigned short)(d * d); if (q < o[z]) o[z] = q; }
    }
}

// min-plus pass along an axis with stride `astride` (in elements) and length L:
//   out[p] = min_{q on the same line} (p - q)^2 + in[q]
// thread <-> one output element; innermost (contiguous) index fastest so that accesses stay coalesced.
__global__ void __launch_bounds__(256) k_edt_axis(const unsigned short* __restrict__ in, const int* __restrict__ tcount,
                                                  int tmax, int t0, size_t nvox, int L, int astride, unsigned short* __restrict__ out) {
    const int b = blockIdx.z, tl = blockIdx.y, t = t0 + tl;
    if (t >= live_thresholds(tcount, b)) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox) return;
    const size_t base = ((size_t)b * tmax + tl) * nvox;
    const int p = (int)((i / astride) % L);
    const unsigned short* c = in + base + i;
    unsigned best = c[0];
    for (int d = 1; d < L; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd >= best) break;                       // farther candidates cannot win any more
        if (p - d >= 0) { const unsigned v = c[-(ptrdiff_t)d * astride]; if (v != kInf && v + dd < best) best = v + dd; }
        if (p + d < L) { const unsigned v = c[(ptrdiff_t)d * astride]; if (v != kInf && v + dd < best) best = v + dd; }
    }
    out[base + i] = (unsigned short)min(best, (unsigned)kInf);
}

// ---- z and y passes in ONE kernel, linear time per line (round 6).  The two kernels above cost 0.51 of the 0.57 s a 190-block cloud spends in
// the adaptive search: k_edt_z walks its lines with a stride of one line between lanes (165 GB/s), k_edt_axis visits ~40 candidates per
// output element (its early exit needs best < d^2).  Here one wave owns the plane (b, t, x): (1) every line y of the plane becomes a bit
// mask of its set voxels (level > t) in LDS -- the 1-D distance along z is then two bit scans, f(y', z) = dz(mask[y'], z)^2, never stored;
// (2) lane z builds the lower envelope of the parabolas f(y', z) + (y - y')^2 over y' (Felzenszwalb & Huttenlocher's linear-time 1-D
// transform with the stack in LDS, [entry][lane]) and evaluates it at every y.  All comparisons are exact integer cross-multiplications
// (no intersection abscissa is ever divided out): the outputs are the same integers as k_edt_z + k_edt_axis, which stay as the fall-back
// for shapes this kernel does not take (W % 16 != 0 or an edge > 128) and for the x pass of the originals' transform.
constexpr int kBigDist = 1 << 20;
template <int NW>
__device__ __forceinline__ int zdist(const unsigned long long* m, int z) {
    if constexpr (NW == 1) {
        const unsigned long long lo = m[0] & (~0ull >> (63 - z)), hi = m[0] >> z;
        const int dl = lo ? z - (63 - __clzll((long long)lo)) : kBigDist, dr = hi ? __ffsll((long long)hi) - 1 : kBigDist;
        return dl < dr ? dl : dr;
    } else {
        const int w = z >> 6, bit = z & 63;
        const unsigned long long lo = m[w] & (~0ull >> (63 - bit)), hi = m[w] >> bit;
        int dl = kBigDist, dr = kBigDist;
        if (lo) dl = bit - (63 - __clzll((long long)lo));
        else if (w == 1 && m[0]) dl = z - (63 - __clzll((long long)m[0]));
        if (hi) dr = __ffsll((long long)hi) - 1;
        else if (w == 0 && m[1]) dr = 64 + __ffsll((long long)m[1]) - 1 - z;
        return dl < dr ? dl : dr;
    }
}
template <int NW, int HM>      // NW = 64-bit words per line (W <= 64 NW), HM = stack depth (H <= HM): 12.5 KB of LDS per wave at 64^3, 25 KB at 128^3
__global__ void __launch_bounds__(64) k_edt_zy(const unsigned char* __restrict__ lev, const int* __restrict__ tcount, int tmax, int t0,
                                               int D, int H, int W, unsigned short* __restrict__ out) {
    const int x = blockIdx.x, tl = blockIdx.y, b = blockIdx.z, t = t0 + tl;
    if (t >= live_thresholds(tcount, b)) return;
    __shared__ unsigned long long mask[HM][NW];
    __shared__ unsigned char sv[HM][64];         // envelope stack of lane z: positions y' ...
    __shared__ unsigned short sF[HM][64];        // ... and F = f + y'^2 (<= 2 * 127^2)
    const int lane = threadIdx.x;
    for (int y = lane; y < H; y += 64) {
        const unsigned char* l = lev + (((size_t)b * D + x) * H + y) * W;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            unsigned long long m = 0;
            for (int j = 0; j < 64 && w * 64 + j < W; j += 16) {
                const uint4 q = *reinterpret_cast<const uint4*>(l + w * 64 + j);
                const unsigned qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((int)((qs[u] >> (8 * c)) & 255u) > t) m |= 1ull << (j + 4 * u + c);
            }
            mask[y][w] = m;
        }
    }
    __syncthreads();
    for (int z = lane; z < W; z += 64) {
        int k = -1;
        for (int q = 0; q < H; ++q) {
            const int dz = zdist<NW>(mask[q], z);
            if (dz >= kBigDist) continue;                    // line q has no set voxel
            const int Fq = dz * dz + q * q;
            // the top entry leaves when its segment is empty: s(v[k-1], v[k]) >= s(v[k], q), cross-multiplied (all differences of positions > 0)
            while (k >= 1) {
                const int vk = sv[k][lane], Fk = sF[k][lane], vj = sv[k - 1][lane], Fj = sF[k - 1][lane];
                if ((Fk - Fj) * (q - vk) >= (Fq - Fk) * (vk - vj)) --k; else break;
            }
            ++k;
            sv[k][lane] = (unsigned char)q;
            sF[k][lane] = (unsigned short)Fq;
        }
        unsigned short* o = out + ((((size_t)b * tmax + tl) * D + x) * H) * W + z;
        if (k < 0) {
            for (int p = 0; p < H; ++p) o[(size_t)p * W] = kInf;
            continue;
        }
        int j = 0, vj = sv[0][lane], Fj = sF[0][lane];
        for (int p = 0; p < H; ++p) {
            while (j < k) {                                  // the next parabola takes over where it is at least as low
                const int vn = sv[j + 1][lane], Fn = sF[j + 1][lane];
                if (Fn - 2 * p * vn <= Fj - 2 * p * vj) { ++j; vj = vn; Fj = Fn; } else break;
            }
            const int val = Fj - 2 * p * vj + p * p;
            o[(size_t)p * W] = (unsigned short)(val < (int)kInf ? val : (int)kInf);
        }
    }
}
bool edt_zy_takes(int D, int H, int W) { return W % 16 == 0 && W <= 128 && H <= 128 && D >= 1; }

// last pass (along x = the slowest axis) evaluated only at the points of A: S_AB[b][t] += min_x' (x_a-x')^2 + g[x'][y_a][z_a]
// HD (the Hausdorff entries): the same value also goes through a maximum, H1_AB[b][t] = max_a of it -- integers, so the order of the
// atomics does not matter.  HD = false is the kernel of the plain entries, instruction for instruction (h_ab unused).
template <bool HD>
__global__ void __launch_bounds__(256) k_edt_points(const unsigned short* __restrict__ g, const int* __restrict__ tcount,
                                                    int tmax, int t0, const int* __restrict__ pts, const int* __restrict__ block_of,
                                                    long long npts, int D, int H, int W,
                                                    unsigned long long* __restrict__ s_ab, unsigned* __restrict__ h_ab) {
    const int tl = blockIdx.y, t = t0 + tl;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long val = 0;
    int b = -1;
    if (i < npts) {
        b = block_of[i];
        if (t < live_thresholds(tcount, b)) {
            const int xa = pts[i * 3], ya = pts[i * 3 + 1], za = pts[i * 3 + 2];
            const size_t hw = (size_t)H * W;
            const unsigned short* c = g + ((size_t)b * tmax + tl) * D * hw + (size_t)ya * W + za;
            val = edt_x_pass(c, hw, xa, D);   // level set t is non-empty for t < tcount[b], so the minimum is finite
        } else b = -1;
    }
    // points are grouped by block: reduce within the wave when the whole wave belongs to one block, else use atomics
    const int b0 = __shfl(b, 0, 64);
    const bool uniform = __all(b == b0 || b == -1) && b0 >= 0;
    [[maybe_unused]] unsigned far = (unsigned)val;      // (<= 3 * 127^2; 0 for the lanes that take no part)
    if (uniform) {
        for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
        if ((threadIdx.x & 63) == 0 && val) atomicAdd(&s_ab[(size_t)b0 * kT + t], val);
        if constexpr (HD) {
            for (int o = 32; o > 0; o >>= 1) far = max(far, (unsigned)__shfl_xor((int)far, o, 64));
            if ((threadIdx.x & 63) == 0 && far) atomicMax(&h_ab[(size_t)b0 * kT + t], far);
        }
    } else if (b >= 0 && val) {
        atomicAdd(&s_ab[(size_t)b * kT + t], val);
        if constexpr (HD) atomicMax(&h_ab[(size_t)b * kT + t], far);
    }
}

// S_BA / n_B histograms by level: hist[b][k] += edt_A[v] for every voxel of level k >= 1
// HD (the Hausdorff entries): hmax[b][k] = the largest edt_A[v] of level k beside them (a table of 256 maxima per workgroup in LDS, then
// one global atomic maximum per level met); H1_BA(t) = max_{k>t} hmax[b][k] is formed where the suffix sums are.  HD = false: as before.
template <bool HD>
__global__ void __launch_bounds__(256) k_level_hist(const unsigned char* __restrict__ lev, const unsigned short* __restrict__ edt_a,
                                                    size_t nvox, unsigned long long* __restrict__ hsum,
                                                    unsigned long long* __restrict__ hcnt, unsigned* __restrict__ hmax) {
    __shared__ unsigned long long ssum[kT];
    __shared__ unsigned int scnt[kT];
    __shared__ unsigned int smax[HD ? kT : 1];
    const int b = blockIdx.y;
    for (int j = threadIdx.x; j < kT; j += blockDim.x) {
        ssum[j] = 0; scnt[j] = 0;
        if constexpr (HD) smax[j] = 0;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (size_t)gridDim.x * blockDim.x) {
        const int k = lev[(size_t)b * nvox + i];
        if (k) {
            atomicAdd(&ssum[k], (unsigned long long)edt_a[(size_t)b * nvox + i]);
            atomicAdd(&scnt[k], 1u);
            if constexpr (HD) atomicMax(&smax[k], (unsigned)edt_a[(size_t)b * nvox + i]);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kT; j += blockDim.x) {
        if (scnt[j]) {
            atomicAdd(&hsum[(size_t)b * kT + j], ssum[j]); atomicAdd(&hcnt[(size_t)b * kT + j], (unsigned long long)scnt[j]);
            if constexpr (HD) { if (smax[j]) atomicMax(&hmax[(size_t)b * kT + j], smax[j]); }
        }
    }
}

}  // namespace

// The z/y passes of every caller (search_common.h): the fused kernel for the shapes it takes; else -- or with PCC_EDT_OLD set, the form the
// fused kernel is tested against -- k_edt_z into g0 and k_edt_axis along y into g1
void pcc_search_edt_zy(hipStream_t st, const unsigned char* levels, const int* counts, int tmax, int t0, int nt, int B, int D, int H,
                       int W, unsigned short* g0, unsigned short* g1) {
    if (edt_zy_takes(D, H, W) && !getenv("PCC_EDT_OLD")) {
        const auto zy = W <= 64 && H <= 64 ? k_edt_zy<1, 64> : W <= 64 ? k_edt_zy<1, 128> : k_edt_zy<2, 128>;
        hipLaunchKernelGGL(zy, dim3(D, nt, B), dim3(64), 0, st, levels, counts, tmax, t0, D, H, W, g1);
        return;
    }
    const int lines = D * H;
    const size_t nvox = (size_t)lines * W;
    hipLaunchKernelGGL(k_edt_z, dim3((lines + 255) / 256, nt, B), dim3(256), 0, st, levels, counts, tmax, t0, lines, W, g0);
    hipLaunchKernelGGL(k_edt_axis, dim3((unsigned)((nvox + 255) / 256), nt, B), dim3(256), 0, st, g0, counts, tmax, t0, nvox, H, W, g1);
}

PCC_API size_t pcc_d1_search_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W) {
    return d1_layout(B, (size_t)D * H * W).total;
}

// x_hat: (B,D,H,W) float32; thr: 256 float32 thresholds (device); pts: (npts,3) int32 local coordinates grouped by
// block, block_of: (npts,) int32.  Outputs (device, zero-filled by this call): s_ab, hsum, hcnt: (B,256) uint64;
// tcount: (B,) int32 = number of thresholds with a non-empty decoded set.  hsum/hcnt are per-level histograms:
// S_BA(t) = sum_{k>t} hsum[k], n_B(t) = sum_{k>t} hcnt[k].
// The level grid comes from `src` (search_common.h): thresholds or candidate counts; everything after it is the same code for both.
// hd (the Hausdorff entries; all NULL in the plain ones, which then launch the kernels they always did): h1_ab, h1_max (B,256) uint32,
// zero-filled by the call: h1_ab[b][t] = max_a min_{v in B_t} |a - v|^2, h1_max[b][k] = max over the voxels of level k of min_a |v - a|^2.
int pcc_search_d1_stats(pcc_ctx* ctx, const LevelSource& src, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* pts,
                        const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount,
                        void* stream, const SearchHausdorff& hd) {
    const int nthr = src.levels();
    const bool HD = hd.h1_ab != nullptr;
    PCC_REQUIRE((hd.h1_ab != nullptr) == (hd.h1_max != nullptr), "%s: NULL argument", src.who);
    PCC_REQUIRE(ctx && x_hat && (src.counts ? src.rank_ws != nullptr : src.thr != nullptr) && workspace && s_ab && hsum && hcnt && tcount,
                "%s: NULL argument", src.who);
    PCC_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && npts >= 0 && (pts || npts == 0), "%s: bad dimension", src.who);
    if (src.counts) PCC_REQUIRE(nthr >= 1 && nthr < kT, "%s: 1 to 255 candidate counts per block", src.who);
    else PCC_REQUIRE(nthr >= 1 && nthr <= kT, "%s: at most 256 thresholds", src.who);
    PCC_REQUIRE(D <= 128 && H <= 128 && W <= 128, "%s: blocks up to 128^3 (uint16 squared distances)", src.who);
    PCC_REQUIRE(B <= 65535, "%s: at most 65535 blocks per call", src.who);
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nvox = (size_t)D * H * W;
    const D1Layout l = d1_layout(B, nvox);
    unsigned char* w1 = (unsigned char*)workspace;
    unsigned char *lev = w1 + l.lev, *occ = w1 + l.occ;
    unsigned short *ea0 = (unsigned short*)(w1 + l.ea0), *ea1 = (unsigned short*)(w1 + l.ea1);
    unsigned short *g0 = (unsigned short*)(w1 + l.g0), *g1 = (unsigned short*)(w1 + l.g1);
    int* one = (int*)(w1 + l.one);   // per-block "1 threshold" counter for the EDT of A
    const int TC = l.TC;
    PCC_CHECK_HIP(hipMemsetAsync(occ, 0, (size_t)B * nvox, st));
    PCC_CHECK_HIP(hipMemsetAsync(tcount, 0, (size_t)B * sizeof(int), st));
    PCC_CHECK_HIP(hipMemsetAsync(s_ab, 0, (size_t)B * kT * 8, st));
    PCC_CHECK_HIP(hipMemsetAsync(hsum, 0, (size_t)B * kT * 8, st));
    PCC_CHECK_HIP(hipMemsetAsync(hcnt, 0, (size_t)B * kT * 8, st));
    if (HD) {
        PCC_CHECK_HIP(hipMemsetAsync(hd.h1_ab, 0, (size_t)B * kT * 4, st));
        PCC_CHECK_HIP(hipMemsetAsync(hd.h1_max, 0, (size_t)B * kT * 4, st));
    }
    const unsigned vox_blocks = (unsigned)((nvox + 255) / 256);
    if (src.counts) {       // (tcount and lev are written whole by the call; it runs behind the fills above on the same stream)
        const int rc = pcc_rank_levels(ctx, x_hat, (int64_t)nvox, B, (int64_t)nvox, src.counts, src.J, lev, tcount, src.rank_ws, src.rank_ws_bytes, stream);
        if (rc != PCC_OK) return rc;
    } else {
        hipLaunchKernelGGL(k_levels, dim3(256, B), dim3(256), 0, st, x_hat, src.thr, nthr, src.clip, nvox, lev, tcount);
    }
    // ---- EDT of the original points A (one "threshold": occupancy > 0)
    if (npts > 0) {
        unsigned pblocks = (unsigned)((npts + 255) / 256);
        if (pblocks > 65535u * 16u) pblocks = 65535u * 16u;
        hipLaunchKernelGGL(k_occupancy, dim3(pblocks), dim3(256), 0, st, pts, block_of, (long long)npts, D, H, W, occ);
    }
    hipLaunchKernelGGL(k_fill_int, dim3((B + 255) / 256), dim3(256), 0, st, one, 1, B);
    pcc_search_edt_zy(st, occ, one, 1, 0, 1, B, D, H, W, ea0, ea1);
    hipLaunchKernelGGL(k_edt_axis, dim3(vox_blocks, 1, B), dim3(256), 0, st, ea1, one, 1, 0, nvox, D, H * W, ea0);
    hipLaunchKernelGGL(HD ? k_level_hist<true> : k_level_hist<false>, dim3(64, B), dim3(256), 0, st, lev, ea0, nvox, (unsigned long long*)hsum,
                       (unsigned long long*)hcnt, hd.h1_max);
    // ---- EDT of every level set, evaluated at the points of A
    //      in chunks of TC thresholds (workspace bound); chunks beyond every block's tcount exit at once
    for (int t0 = 0; t0 < nthr; t0 += TC) {
        const int nt = nthr - t0 < TC ? nthr - t0 : TC;
        pcc_search_edt_zy(st, lev, tcount, TC, t0, nt, B, D, H, W, g0, g1);
        if (npts > 0) {
            const unsigned pblocks = (unsigned)((npts + 255) / 256);
            hipLaunchKernelGGL(HD ? k_edt_points<true> : k_edt_points<false>, dim3(pblocks, nt), dim3(256), 0, st, g1, tcount, TC, t0, pts,
                               block_of, (long long)npts, D, H, W, (unsigned long long*)s_ab, hd.h1_ab);
        }
    }
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_d1_threshold_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W,
                                   const float* thr, int32_t nthr, int32_t clip, const int32_t* pts,
                                   const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab,
                                   uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, void* stream) {
    const LevelSource src = {"pcc_d1_threshold_stats", thr, nthr, clip, nullptr, 0, nullptr, 0};
    return pcc_search_d1_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream);
}

// pcc_d1_threshold_stats with the D1 Hausdorff terms beside the sums (include/pcc_geo.h "Hausdorff terms of the search")
PCC_API int pcc_d1_threshold_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W,
                                             const float* thr, int32_t nthr, int32_t clip, const int32_t* pts,
                                             const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab,
                                             uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, uint32_t* h1_ab, uint32_t* h1_max, void* stream) {
    PCC_REQUIRE(h1_ab && h1_max, "pcc_d1_threshold_stats_hausdorff: NULL argument");
    const LevelSource src = {"pcc_d1_threshold_stats_hausdorff", thr, nthr, clip, nullptr, 0, nullptr, 0};
    return pcc_search_d1_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream, {h1_ab, h1_max});
}

// The same statistics for the top-counts[b][j] sets of every block (include/pcc_geo.h): only the source of the level grid differs
PCC_API int pcc_d1_count_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts, int32_t J,
                               const int32_t* pts, const int32_t* block_of, int64_t npts, void* workspace, void* rank_workspace,
                               size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, void* stream) {
    PCC_REQUIRE(counts, "pcc_d1_count_stats: NULL argument");
    const LevelSource src = {"pcc_d1_count_stats", nullptr, 0, 0, counts, J, rank_workspace, rank_workspace_bytes};
    return pcc_search_d1_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream);
}

PCC_API int pcc_d1_count_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts,
                                         int32_t J, const int32_t* pts, const int32_t* block_of, int64_t npts, void* workspace,
                                         void* rank_workspace, size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt,
                                         int32_t* tcount, uint32_t* h1_ab, uint32_t* h1_max, void* stream) {
    PCC_REQUIRE(counts && h1_ab && h1_max, "pcc_d1_count_stats_hausdorff: NULL argument");
    const LevelSource src = {"pcc_d1_count_stats_hausdorff", nullptr, 0, 0, counts, J, rank_workspace, rank_workspace_bytes};
    return pcc_search_d1_stats(ctx, src, x_hat, B, D, H, W, pts, block_of, npts, workspace, s_ab, hsum, hcnt, tcount, stream, {h1_ab, h1_max});
}
