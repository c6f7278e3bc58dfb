// conv_fwd_kernel / conv16_pers_kernel (conv_direct.h): Conv3D stride 1|2 (and Conv3DTranspose stride 1 through host-flipped weights),
// Cin, Cout multiples of 16; 16 input channels staged per pass.  Compiled once per instantiation group (-DPCC_INST_GROUP=n, Makefile)
// so that the heavily unrolled kernels build in parallel; group 0 holds the entry point pcc_conv_fwd.
#include "conv_direct.h"

#ifndef PCC_INST_GROUP
#define PCC_INST_GROUP 0
#endif

namespace pccmfma {

// =====================================================================================================
// forward conv (stride 1 or 2), Cin % 16 == 0, Cout % 16 == 0
//   tile = TZ x TY x TXT output voxels; a "row" = 16 voxels = RY(=16/TX) y-lines x TX voxels along x;
//   each wave owns R rows that are consecutive in y.
// =====================================================================================================
template <int CIN, int COUT, int KS, int S, int TX, int TZ, int TY, int TXT, int R, int CTW = COUT / 16>
struct FwdCfg {
    static constexpr int NG = CIN / 16, NCT = COUT / 16;
    static constexpr int RY = 16 / TX;
    static constexpr int NYB = TY / RY, NXB = TXT / TX;
    static constexpr int NCG = NCT / CTW;              // cout-tile groups: waves also split the output channels
    static constexpr int NW = TZ * (NYB / R) * NXB * NCG;
    static constexpr int NT = NW * 64;
    static constexpr int PL = (S == 1) ? (KS - 1) / 2 : (KS - 2) / 2;  // SAME pad_low (even input dims for S=2)
    static constexpr int LZ = (TZ - 1) * S + KS, LY = (TY - 1) * S + KS, LX = (TXT - 1) * S + KS;
    static constexpr int VS = 24;  // floats per voxel in LDS: 16 staged channels + 8 pad
    static constexpr int NV = LZ * LY * LX;
    static constexpr int LDS_BYTES = NV * VS * 4;
    static constexpr int ITEMS = (NV * 4 + NT - 1) / NT;
    static_assert(TY % RY == 0 && NYB % R == 0 && TXT % TX == 0, "bad tile");
};

template <int CIN, int COUT, int KS, int S, int TX, int TZ, int TY, int TXT, int R, int CTW = COUT / 16, bool F16 = false>
__global__ void __launch_bounds__((FwdCfg<CIN, COUT, KS, S, TX, TZ, TY, TXT, R, CTW>::NT))
conv_fwd_kernel(ConvArgs a) {
    using C = FwdCfg<CIN, COUT, KS, S, TX, TZ, TY, TXT, R, CTW>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;

    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % a.ntx; t /= a.ntx;
    const int ty = t % a.nty; t /= a.nty;
    const int tz = t % a.ntz;
    const int n = t / a.ntz;
    const int oz0 = tz * TZ, oy0 = ty * TY, ox0 = tx * TXT;          // output-tile origin
    const int iz0 = oz0 * S - C::PL, iy0 = oy0 * S - C::PL, ix0 = ox0 * S - C::PL;  // LDS-tile origin (input)

    // wave -> (z, y-block group, x-block)
    int wv = wave;
    const int ct0 = (wv % C::NCG) * CTW; wv /= C::NCG;   // first cout tile of this wave
    const int w_xb = wv % C::NXB; wv /= C::NXB;
    const int w_yg = wv % (C::NYB / R);
    const int w_z = wv / (C::NYB / R);
    const int ry = v / TX, rx = v % TX;
    const int ly0 = (w_yg * R * C::RY + ry), lx0 = (w_xb * TX + rx);  // local output coords of row 0
    const float* lbase = lds + ((w_z * S * C::LY + ly0 * S) * C::LX + lx0 * S) * C::VS + cq * 4;
    constexpr int ROW_OFF = C::RY * S * C::LX * C::VS;  // floats between consecutive rows of a wave

    f32x4 acc[R][CTW];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const float* inb = a.in + (size_t)n * a.D * a.H * a.W * CIN;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(inb, (unsigned)a.D * a.H * a.W * CIN * 4u);
    constexpr int NTAP = KS * KS * KS;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, (unsigned)(C::NG * NTAP * C::NCT) * 1024u);
    const unsigned wlane = lane * 16;
    // weights: RING-deep register prefetch ring over the linear (g, tap) sequence; the loads are pinned
    // RING - 1 taps ahead of their use so that L2 latency (500-900 cycles) never reaches the MFMA pipe.  A tap is R * CTW * 4 MFMAs:
    // two taps ahead are >= 1000 cycles for the big tiles, but only 256 for the R = CTW = 1 tiles of the 4^3 / 8^3 grids (round 3:
    // those layers were latency-bound on exactly this -- 64 -> 64 @4^3 26.5 us for 5 us of MFMAs), hence the deeper rings there.
    constexpr int RING = (KS == 3) ? (R * CTW == 1 ? (TX <= 4 ? 27 : 9) : (R * CTW == 2 ? 9 : 3)) : 5;      // (8-wide grids: 27 costs occupancy, 39.5 vs 36.4 us)
    constexpr int SLAB = (KS == 3) ? NTAP : KS * KS;   // taps unrolled per dynamic iteration
    static_assert(SLAB % RING == 0, "ring phase must be static");
    const int q_last = C::NG * NTAP - 1;
    auto tap_off = [](int kz, int ky, int kx) { return ((kz * C::LY + ky) * C::LX + kx) * C::VS; };

    // per-thread staging items: byte offset of channel group 0 inside the image, or kOOB (reads as zeros)
    unsigned soff[C::ITEMS];
#pragma unroll
    for (int it = 0; it < C::ITEMS; ++it) {
        const int item = it * C::NT + tid;
        const int u = item >> 2, q = item & 3;
        const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
        const int ly = rem / C::LX, lx = rem - ly * C::LX;
        const int gz = iz0 + lz, gy = iy0 + ly, gx = ix0 + lx;
        const bool ok = (item < C::NV * 4) & (gz >= 0) & (gz < a.D) & (gy >= 0) & (gy < a.H) & (gx >= 0) & (gx < a.W);
        soff[it] = ok ? (unsigned)(((gz * a.H + gy) * a.W + gx) * CIN + q * 4) * 4u : kOOB;
    }
    auto commit = [&](const f32x4 (&stg)[C::ITEMS]) {
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) {
            const int item = it * C::NT + tid;
            if (item < C::NV * 4) *reinterpret_cast<f32x4*>(lds + (item >> 2) * C::VS + (item & 3) * 4) = stg[it];
        }
    };

    if constexpr (KS == 3) {
        // ---- k3: software pipeline over the channel groups of the tile.  While group g is contracted (27 taps),
        //      the staging loads of group g+1 (one item per tap) and, in the last group, the residual rows are in
        //      flight; the weight ring runs continuously across groups.
        constexpr int NRES = R * CTW;                       // residual float4 per lane
        constexpr int RES0 = (27 - NRES) > 0 ? 27 - NRES : 0;
        static_assert(C::ITEMS <= 27 && NRES <= 27, "prefetch is spread over the tap sections");
        f32x4 stg[C::ITEMS];
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) stg[it] = buf_load4(rin, soff[it], 0);
        f32x4 wf[RING][CTW];
#pragma unroll
        for (int r = 0; r < RING - 1; ++r)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) wf[r][ct] = buf_load4(rw, wlane, (unsigned)(min(r, q_last) * C::NCT + ct0 + ct) * 1024u);
        commit(stg);
        __syncthreads();

        // residual rows of this wave (prefetched during the last group)
        const int gzo = oz0 + w_z;
        const bool has_res = (a.flags & PCC_CONV_ADD) != 0;
        const __amdgpu_buffer_rsrc_t rres = make_rsrc(has_res ? a.res + (size_t)n * a.OD * a.OH * a.OW * COUT : a.in,
                                                      has_res ? (unsigned)a.OD * a.OH * a.OW * COUT * 4u : 0u);
        f32x4 resv[R][CTW];

#pragma unroll 1
        for (int g = 0; g < C::NG; ++g) {
            const unsigned gnext = (unsigned)min(g + 1, C::NG - 1) * 64u;     // last group: harmless re-read
            const bool last = g == C::NG - 1;
            f32x4 bb[2][R];
#pragma unroll
            for (int i = 0; i < R; ++i) bb[0][i] = *reinterpret_cast<const f32x4*>(lbase + i * ROW_OFF);
#pragma unroll
            for (int ts = 0; ts < NTAP; ++ts) {
                {
                    const int q = min(g * NTAP + ts + RING - 1, q_last);
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        wf[(ts + RING - 1) % RING][ct] = buf_load4(rw, wlane, (unsigned)(q * C::NCT + ct0 + ct) * 1024u);
                    const int tn = (ts + 1 < NTAP) ? ts + 1 : ts;   // last tap: harmless re-read
                    const int toff = tap_off(tn / 9, (tn / 3) % 3, tn % 3);
#pragma unroll
                    for (int i = 0; i < R; ++i)
                        bb[(ts + 1) & 1][i] = *reinterpret_cast<const f32x4*>(lbase + toff + i * ROW_OFF);
                    if (ts < C::ITEMS) stg[ts] = buf_load4(rin, soff[ts], gnext);
                    if (ts >= RES0 && ts < RES0 + NRES) {
                        const int i = (ts - RES0) / CTW, ct = (ts - RES0) % CTW;
                        const int gy = oy0 + ly0 + i * C::RY, gx = ox0 + lx0;
                        const bool ok = last & has_res & (gzo < a.OD) & (gy < a.OH) & (gx < a.OW);
                        const unsigned off = (unsigned)(((gzo * a.OH + gy) * a.OW + gx) * COUT + (ct0 + ct) * 16 + cq * 4) * 4u;
                        resv[i][ct] = buf_load4(rres, ok ? off : kOOB, 0);
                    }
                }
                // k-slot quarter j outermost: consecutive MFMAs go to different accumulators (the 40-cycle
                // dependent-accumulator latency of v_mfma_f32_16x16x4_f32 never stalls the 32-cycle issue)
                if constexpr (F16) {
#pragma unroll
                    for (int i = 0; i < R; ++i)
#pragma unroll
                        for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = mfma16h(wf[ts % RING][ct], bb[ts & 1][i], acc[i][ct]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < R; ++i)
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct)
                                acc[i][ct] = mfma16(wf[ts % RING][ct][j], bb[ts & 1][i][j], acc[i][ct]);
                }
                PCC_PIN_MEM_MFMA();
            }
            if (!last) {
                __syncthreads();   // every wave finished reading group g
                commit(stg);
                __syncthreads();
            }
        }
        // ---- epilogue (residual already in registers)
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int gy = oy0 + ly0 + i * C::RY, gx = ox0 + lx0;
            if (gzo < a.OD && gy < a.OH && gx < a.OW) {
                const size_t vox = (((size_t)n * a.OD + gzo) * a.OH + gy) * a.OW + gx;
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    f32x4 o = acc[i][ct];
                    const int c0 = (ct0 + ct) * 16 + cq * 4;
                    if (a.flags & PCC_CONV_BIAS) o += *reinterpret_cast<const f32x4*>(a.bias + c0);
                    if (a.flags & PCC_CONV_RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                    if (has_res) o += resv[i][ct];
                    if (a.flags & PCC_CONV_CLIP01) {
                        o.x = fminf(fmaxf(o.x, 0.f), 1.f); o.y = fminf(fmaxf(o.y, 0.f), 1.f);
                        o.z = fminf(fmaxf(o.z, 0.f), 1.f); o.w = fminf(fmaxf(o.w, 0.f), 1.f);
                    }
                    if (a.flags & PCC_CONV_OUT16) {      // (wave-uniform) fp16 hand-over, as store_out
                        f16x4 h;
                        h[0] = (_Float16)o.x; h[1] = (_Float16)o.y; h[2] = (_Float16)o.z; h[3] = (_Float16)o.w;
                        *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.out) + vox * a.ocs + a.oco + c0) = h;
                    } else {
                        *reinterpret_cast<f32x4*>(a.out + vox * a.ocs + a.oco + c0) = o;
                    }
                }
            }
        }
    } else {
#pragma unroll 1
        for (int g = 0; g < C::NG; ++g) {
            f32x4 stg[C::ITEMS];
#pragma unroll
            for (int it = 0; it < C::ITEMS; ++it) stg[it] = buf_load4(rin, soff[it], (unsigned)g * 64u);
            f32x4 wf[RING][CTW];
#pragma unroll
            for (int r = 0; r < RING - 1; ++r) {
                const int q = min(g * NTAP + r, q_last);
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) wf[r][ct] = buf_load4(rw, wlane, (unsigned)(q * C::NCT + ct0 + ct) * 1024u);
            }
            if (g > 0) __syncthreads();  // all waves finished reading the previous group
            commit(stg);
            __syncthreads();
#pragma unroll 1
            for (int sl = 0; sl < NTAP / SLAB; ++sl) {
#pragma unroll
                for (int ts = 0; ts < SLAB; ++ts) {
                    const int t = sl * SLAB + ts;
                    const int q = min(g * NTAP + t + RING - 1, q_last);
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        wf[(ts + RING - 1) % RING][ct] = buf_load4(rw, wlane, (unsigned)(q * C::NCT + ct0 + ct) * 1024u);
                    PCC_PIN_VMEM();
                    const int toff = tap_off(sl, ts / KS, ts % KS);
                    f32x4 b[R];
#pragma unroll
                    for (int i = 0; i < R; ++i) b[i] = *reinterpret_cast<const f32x4*>(lbase + toff + i * ROW_OFF);
                    if constexpr (F16) {
#pragma unroll
                        for (int i = 0; i < R; ++i)
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = mfma16h(wf[ts % RING][ct], b[i], acc[i][ct]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int i = 0; i < R; ++i)
#pragma unroll
                                for (int ct = 0; ct < CTW; ++ct)
                                    acc[i][ct] = mfma16(wf[ts % RING][ct][j], b[i][j], acc[i][ct]);
                    }
                }
            }
        }
        // ---- epilogue
        const int gz = oz0 + w_z;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int gy = oy0 + ly0 + i * C::RY, gx = ox0 + lx0;
            if (gz < a.OD && gy < a.OH && gx < a.OW) {
                const size_t vox = (((size_t)n * a.OD + gz) * a.OH + gy) * a.OW + gx;
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) store_out(a, acc[i][ct], vox, (ct0 + ct) * 16 + cq * 4, COUT);
            }
        }
    }
}

// =====================================================================================================
// Persistent 16 -> 16, k3, stride 1 kernel (the dominant layer shape: Conv3DTranspose 16->16 @64^3 is 47 % of
// all c3p MACs).  One workgroup per CU walks tiles g, g+G, ...:
//   * all 27 weight fragments live in registers for the lifetime of the workgroup (108 VGPRs) -> no weight
//     traffic and no vmcnt coupling inside the tap loop;
//   * the haloed input tile is double-buffered in LDS: the global loads of tile i+1 (and the residual of
//     tile i) are issued BEFORE the 432 MFMAs of tile i and land under them;
//   * one barrier per tile.
// Accumulation order per output element is identical to conv_fwd_kernel (tap-major, 4 k-slots): results are
// bit-identical between the two kernels.
// =====================================================================================================
template <int TZ, int TY, int R, int VS_>
struct P16Cfg {
    static constexpr int CIN = 16, COUT = 16, KS = 3;
    static constexpr int NW = TZ * (TY / R);
    static constexpr int NT = NW * 64;
    static constexpr int LZ = TZ + 2, LY = TY + 2, LX = 18;
    static constexpr int VS = VS_;   // floats per voxel in LDS: 24 = conflict-free, 20 = smaller (some 2-way conflicts)
    static constexpr int NV = LZ * LY * LX;
    static constexpr int ITEMS = (NV * 4 + NT - 1) / NT;
    static constexpr int BUF = ITEMS * NT / 4 * VS;   // floats per LDS buffer (rounded up: no store guards)
    static constexpr int LDS_BYTES = 2 * BUF * 4;
    static_assert(ITEMS + R <= 27, "prefetch is spread over the 27 tap sections");
};

template <int TZ, int TY, int R, int VS_, int WGS_PER_CU>
__global__ void __launch_bounds__((P16Cfg<TZ, TY, R, VS_>::NT), (WGS_PER_CU * P16Cfg<TZ, TY, R, VS_>::NT / 256)) conv16_pers_kernel(ConvArgs a, int ntiles) {
    using C = P16Cfg<TZ, TY, R, VS_>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;
    const int G = gridDim.x;
    int tile = xcd_remap(blockIdx.x, G);
    if (tile >= ntiles) return;

    const int w_yg = wave % (TY / R), w_z = wave / (TY / R);
    const int ly0 = w_yg * R;
    const int lane_off = ((w_z * C::LY + ly0) * C::LX + v) * C::VS + cq * 4;
    constexpr int ROW_OFF = C::LX * C::VS;

    // ---- all weights -> registers
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, 27u * 1024u);
    f32x4 wreg[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) wreg[t] = buf_load4(rw, lane * 16, t * 1024u);

    // ---- per-thread staging items: fixed (lz,ly,lx,quarter) -> relative byte offset inside an image, LDS slot
    const unsigned img_bytes = (unsigned)a.D * a.H * a.W * 64u;     // 16 channels x 4 B per voxel, in == out size
    unsigned rel[C::ITEMS];      // byte offset relative to the tile's (z-1, y-1, x-1) corner voxel
    unsigned lyx[C::ITEMS];      // ly | lx << 8 (for the y/x range test; z is covered by the buffer range check)
#pragma unroll
    for (int it = 0; it < C::ITEMS; ++it) {
        const int item = it * C::NT + tid;
        const int u = item >> 2, q = item & 3;
        const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
        const int ly = rem / C::LX, lx = rem - ly * C::LX;
        rel[it] = (unsigned)(((lz * a.H + ly) * a.W + lx) * 16 + q * 4) * 4u;
        lyx[it] = (item < C::NV * 4) ? (unsigned)(ly | (lx << 8)) : 0xFFFFu;   // tail items: lx = 255 -> always out of range
    }

    // tile coordinates, advanced incrementally by G tiles per iteration (mixed radix, no divisions in the loop)
    int tx = tile % a.ntx, ty = (tile / a.ntx) % a.nty, tz = (tile / (a.ntx * a.nty)) % a.ntz, n = tile / (a.ntx * a.nty * a.ntz);
    const int gx_ = G % a.ntx, gy_ = (G / a.ntx) % a.nty, gz_ = (G / (a.ntx * a.nty)) % a.ntz, gn_ = G / (a.ntx * a.nty * a.ntz);

    struct Prefetch { __amdgpu_buffer_rsrc_t rin; unsigned base; int ylo, ny1, xlo, nx1; };
    auto setup = [&](int n_, int tz_, int ty_, int tx_) {
        Prefetch p;
        p.rin = make_rsrc(a.in + (size_t)n_ * a.D * a.H * a.W * 16, img_bytes);
        const int oz0 = tz_ * TZ, oy0 = ty_ * TY, ox0 = tx_ * 16;
        p.base = (unsigned)((((oz0 - 1) * a.H + (oy0 - 1)) * a.W + (ox0 - 1)) * 64);   // may wrap: unsigned arithmetic
        p.ylo = oy0 == 0 ? 1 : 0;                                   // valid local rows:    ylo <= ly <= ylo + ny1
        p.ny1 = min(C::LY, a.H - oy0 + 1) - p.ylo - 1;
        p.xlo = ox0 == 0 ? 1 : 0;                                   // valid local columns: xlo <= lx <= xlo + nx1
        p.nx1 = min(C::LX, a.W - ox0 + 1) - p.xlo - 1;
        return p;
    };
    auto load_item = [&](const Prefetch& p, int it) {
        // pure-VALU range test: a negative term sets the sign bit, and the sign bit IS the out-of-range offset.
        // z below 0 wraps to a huge offset, z >= D runs past the image: both hit the hardware range check.
        const int dy = (int)(lyx[it] & 0xFFu) - p.ylo, dx = (int)(lyx[it] >> 8) - p.xlo;
        const unsigned neg = (unsigned)(dy | (p.ny1 - dy) | dx | (p.nx1 - dx)) & kOOB;
        return buf_load4(p.rin, (p.base + rel[it]) | neg, 0);
    };
    auto commit = [&](float* buf, const f32x4 (&stg)[C::ITEMS]) {
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) {
            const int item = it * C::NT + tid;
            *reinterpret_cast<f32x4*>(buf + (item >> 2) * C::VS + (item & 3) * 4) = stg[it];
        }
    };

    f32x4 stg[C::ITEMS];
    {
        const Prefetch p = setup(n, tz, ty, tx);
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) stg[it] = load_item(p, it);
    }
    commit(lds, stg);
    __syncthreads();
    int cur = 0;
    const bool has_res = (a.flags & PCC_CONV_ADD) != 0;
    const unsigned out_img_bytes = (unsigned)a.OD * a.OH * a.OW * (unsigned)a.ocs * 4u;
    const f32x4 bias4 = (a.flags & PCC_CONV_BIAS) ? *reinterpret_cast<const f32x4*>(a.bias + cq * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wr_off = (tid >> 2) * C::VS + (tid & 3) * 4;      // LDS slot of this thread's staging item 0
    constexpr int WR_STRIDE = (C::NT / 4) * C::VS;               // floats between consecutive items
    constexpr int COMMIT_LAG = (C::ITEMS + 14 <= 27) ? 14 : 27 - C::ITEMS;                             // item k is loaded in tap k and written in tap k + LAG
    static_assert(C::ITEMS + COMMIT_LAG <= 27, "commit must fit in the tap loop");

    // deferred epilogue state of the PREVIOUS tile (its stores are issued inside this tile's tap loop)
    f32x4 pacc[R], pres[R];
    unsigned poff[R];                 // byte offset inside the output image, or kOOB (store dropped by hardware)
    __amdgpu_buffer_rsrc_t prout = make_rsrc(a.out, 0u);
#pragma unroll
    for (int i = 0; i < R; ++i) { pacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; pres[i] = pacc[i]; poff[i] = kOOB; }

    auto finish_row = [&](const f32x4& accv, const f32x4& resv_, unsigned off, __amdgpu_buffer_rsrc_t ro) {
        f32x4 o = accv + bias4;
        if (a.flags & PCC_CONV_RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        o += resv_;   // zeros when PCC_CONV_ADD is clear
        if (a.flags & PCC_CONV_CLIP01) {
            o.x = fminf(fmaxf(o.x, 0.f), 1.f); o.y = fminf(fmaxf(o.y, 0.f), 1.f);
            o.z = fminf(fmaxf(o.z, 0.f), 1.f); o.w = fminf(fmaxf(o.w, 0.f), 1.f);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, (int)off, 0, 0);
    };

    for (;;) {
        const int next = tile + G;
        const bool has_next = next < ntiles;
        int ntx_ = tx + gx_, nty_ = ty + gy_, ntz_ = tz + gz_, nn_ = n + gn_;
        if (ntx_ >= a.ntx) { ntx_ -= a.ntx; ++nty_; }
        if (nty_ >= a.nty) { nty_ -= a.nty; ++ntz_; }
        if (ntz_ >= a.ntz) { ntz_ -= a.ntz; ++nn_; }
        const Prefetch pn = has_next ? setup(nn_, ntz_, nty_, ntx_) : setup(n, tz, ty, tx);   // no next: harmless re-read
        const int oz0 = tz * TZ, oy0 = ty * TY, ox0 = tx * 16;
        const int gz = oz0 + w_z, gx = ox0 + v;
        const unsigned lvox0 = (unsigned)((gz * a.OH + oy0 + ly0) * a.OW + gx);
        const __amdgpu_buffer_rsrc_t rres = make_rsrc(has_res ? a.res + (size_t)n * a.OD * a.OH * a.OW * 16 : a.in, has_res ? img_bytes : 0u);
        const __amdgpu_buffer_rsrc_t rout = make_rsrc(a.out + (size_t)n * a.OD * a.OH * a.OW * a.ocs, out_img_bytes);
        const bool col_ok = gz < a.OD && gx < a.OW;
        f32x4 resv[R];

        const float* lbase = lds + cur * C::BUF + lane_off;
        float* wbase = lds + (cur ^ 1) * C::BUF + wr_off;
        f32x4 acc[R];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 bb[2][R];
#pragma unroll
        for (int i = 0; i < R; ++i) bb[0][i] = *reinterpret_cast<const f32x4*>(lbase + i * ROW_OFF);
#pragma unroll
        for (int ts = 0; ts < 27; ++ts) {
            // Everything that is not an MFMA is spread over the 27 tap sections and interleaved with the 16 MFMAs
            // of the section (sched_group_barrier below), so the matrix pipe never waits for the issue of:
            //   rows of tap ts+1 (4 ds_read) | staging load k of the NEXT tile (ts = k < ITEMS) and its LDS commit
            //   (ts = k + LAG) | residual load of THIS tile (ts = ITEMS..ITEMS+R-1) | the epilogue row of the PREVIOUS
            //   tile (ts = 27-R..26, branch-free buffer store).
            const int tn = (ts + 1 < 27) ? ts + 1 : ts;
            const int toff = (((tn / 9) * C::LY + (tn / 3) % 3) * C::LX + tn % 3) * C::VS;
#pragma unroll
            for (int i = 0; i < R; ++i)
                bb[(ts + 1) & 1][i] = *reinterpret_cast<const f32x4*>(lbase + toff + i * ROW_OFF);
            if (ts < C::ITEMS) stg[ts] = load_item(pn, ts);
            if (ts >= COMMIT_LAG && ts < C::ITEMS + COMMIT_LAG)
                *reinterpret_cast<f32x4*>(wbase + (ts - COMMIT_LAG) * WR_STRIDE) = stg[ts - COMMIT_LAG];
            if (ts >= C::ITEMS && ts < C::ITEMS + R) {
                const int i = ts - C::ITEMS;
                const bool ok = col_ok && (oy0 + ly0 + i) < a.OH && has_res;
                resv[i] = buf_load4(rres, ok ? ((lvox0 + (unsigned)(i * a.OW)) * 16 + cq * 4) * 4u : kOOB, 0);
            }
            if (ts >= 27 - R) finish_row(pacc[ts - (27 - R)], pres[ts - (27 - R)], poff[ts - (27 - R)], prout);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < R; ++i) acc[i] = mfma16(wreg[ts][j], bb[ts & 1][i][j], acc[i]);
            // issue order inside the section: 1 LDS read, 4 MFMA, ... (VMEM / LDS write / VALU wherever they fit)
#pragma unroll
            for (int k = 0; k < R; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 DS read
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // 4 MFMA
            }
            PCC_PIN_MEM_MFMA();
        }

        // hand the finished accumulators over to the deferred epilogue of the next iteration
#pragma unroll
        for (int i = 0; i < R; ++i) {
            pacc[i] = acc[i];
            pres[i] = resv[i];
            const bool ok = col_ok && (oy0 + ly0 + i) < a.OH;
            poff[i] = ok ? ((lvox0 + (unsigned)(i * a.OW)) * (unsigned)a.ocs + a.oco + cq * 4) * 4u : kOOB;
        }
        prout = rout;
        if (!has_next) break;
        __syncthreads();   // every wave's commits of the next tile are in LDS; nobody still reads `cur`
        cur ^= 1;
        tile = next; n = nn_; tz = ntz_; ty = nty_; tx = ntx_;
    }
    // epilogue of the last tile
#pragma unroll
    for (int i = 0; i < R; ++i) finish_row(pacc[i], pres[i], poff[i], prout);
}

template <int CIN, int COUT, int KS, int S>
int launch_fwd(const pcc_ctx* ctx, int tx, ConvArgs a, hipStream_t st) {
    // tile shapes per row width: (TX, TZ, TY, TXT, R)
#define PCC_FWD(TX, TZ, TY, TXT, R) PCC_FWDC(TX, TZ, TY, TXT, R, (COUT / 16))
#define PCC_FWDC(TX, TZ, TY, TXT, R, CTW)                                                               \
    {                                                                                                   \
        using C = FwdCfg<CIN, COUT, KS, S, TX, TZ, TY, TXT, R, CTW>;                                    \
        a.ntz = cdiv(a.OD, TZ); a.nty = cdiv(a.OH, TY); a.ntx = cdiv(a.OW, TXT);                        \
        if (a.flags & PCC_CONV_F16)                                                                     \
            return launch(conv_fwd_kernel<CIN, COUT, KS, S, TX, TZ, TY, TXT, R, CTW, true>, C::NT, C::LDS_BYTES, \
                          a.N * a.ntz * a.nty * a.ntx, a, st);                                          \
        return launch(conv_fwd_kernel<CIN, COUT, KS, S, TX, TZ, TY, TXT, R, CTW>, C::NT, C::LDS_BYTES,  \
                      a.N * a.ntz * a.nty * a.ntx, a, st);                                              \
    }
    if constexpr (S == 1) {
        if (tx == 16) {
            if constexpr (COUT >= 64) {
                // pick the tile whose workgroup count fills the CU slots best (avoids a mostly empty last round)
                const long vox = (long)a.N * a.OD * a.OH * a.OW;
                const long wg_small = vox / 128, wg_big = vox / 256;          // (2,4,16) vs (2,8,16)
                const double t_small = (double)((wg_small + 3 * ctx->num_cu - 1) / (3 * ctx->num_cu)) * 1.0;
                const double t_big = (double)((wg_big + 2 * ctx->num_cu - 1) / (2 * ctx->num_cu)) * 2.0;
                const bool big = t_big <= t_small;
                if (big) PCC_FWD(16, 2, 8, 16, 4)
                PCC_FWD(16, 2, 4, 16, 2)
            }
            else if (COUT == 16 && CIN == 16 && KS == 3 && !(a.flags & PCC_CONV_F16)) {
                // persistent kernel, 2 workgroups per CU (tile 2x4x16, 80-byte LDS voxel stride)
#define PCC_P16(TZ, TY, R, VS, WPC)                                                                     \
    {                                                                                                   \
        using P = P16Cfg<TZ, TY, R, VS>;                                                                \
        a.ntz = cdiv(a.OD, TZ); a.nty = cdiv(a.OH, TY); a.ntx = cdiv(a.OW, 16);                         \
        const int ntiles = a.N * a.ntz * a.nty * a.ntx;                                                 \
        const int grid = ntiles < ctx->num_cu * WPC ? ntiles : ctx->num_cu * WPC;                       \
        return launch(conv16_pers_kernel<TZ, TY, R, VS, WPC>, P::NT, P::LDS_BYTES, grid, a, st, ntiles); \
    }
                if (ctx->num(PCC_NUM_P16)) PCC_P16(2, 8, 2, 20, 1)     // one 8-wave workgroup per CU (same speed, fewer halo re-reads)
                PCC_P16(2, 4, 2, 20, 2)
#undef PCC_P16
            }
            else PCC_FWD(16, 2, 8, 16, 4)
        }
        // small grids: few voxels per workgroup and the cout tiles split over waves, so that every CU gets work
        if (tx == 8) {
            if constexpr (COUT >= 64) PCC_FWDC(8, 2, 4, 8, 1, 1)
            else PCC_FWD(8, 2, 8, 8, 2)
        }
        if constexpr (COUT >= 32) PCC_FWDC(4, 1, 4, 4, 1, 1)
        else PCC_FWD(4, 4, 4, 4, 1)
    } else if constexpr (KS == 3) {  // stride 2: the staged input tile is 2x larger per dim
        if (tx == 16) PCC_FWD(16, 2, 2, 16, 1)
        if (tx == 8) PCC_FWD(8, 2, 4, 8, 1)
        if constexpr (COUT >= 32) PCC_FWDC(4, 1, 4, 4, 1, 1)
        else PCC_FWD(4, 4, 4, 4, 1)
    } else {
        if (tx == 16) PCC_FWD(16, 1, 2, 16, 1)
        if (tx == 8) PCC_FWD(8, 1, 4, 8, 1)
        PCC_FWD(4, 4, 4, 4, 1)
    }
#undef PCC_FWD
#undef PCC_FWDC
}

// ---- instantiation groups (CIN, COUT, KS, S): one object each
#define PCC_FWD_G0(X) X(32, 32, 5, 2)
#define PCC_FWD_G1(X) X(16, 16, 3, 1) X(16, 32, 3, 2)
#define PCC_FWD_G2(X) X(32, 32, 3, 1) X(32, 32, 3, 2)
#define PCC_FWD_G3(X) X(64, 64, 3, 1) X(64, 64, 3, 2) X(32, 64, 3, 2)
#define PCC_INST_FWD(CI, CO, K, S) template int launch_fwd<CI, CO, K, S>(const pcc_ctx*, int, ConvArgs, hipStream_t);
#define PCC_EXT_FWD(CI, CO, K, S) extern template int launch_fwd<CI, CO, K, S>(const pcc_ctx*, int, ConvArgs, hipStream_t);
#if PCC_INST_GROUP == 0
PCC_FWD_G1(PCC_EXT_FWD) PCC_FWD_G2(PCC_EXT_FWD) PCC_FWD_G3(PCC_EXT_FWD)
#elif PCC_INST_GROUP == 1
PCC_FWD_G1(PCC_INST_FWD)
#elif PCC_INST_GROUP == 2
PCC_FWD_G2(PCC_INST_FWD)
#elif PCC_INST_GROUP == 3
PCC_FWD_G3(PCC_INST_FWD)
#endif

}  // namespace pccmfma

#if PCC_INST_GROUP == 0
using namespace pccmfma;

int pcc_conv_fwd(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                 float* out, int tx, hipStream_t st) {
    const ConvArgs a = conv_args(d, in, w_packed, bias, residual, out);
    const int ci = d->Cin, co = d->Cout, k = d->k, s = d->stride;
#define PCC_CASE_FWD(CI, CO, K, S) if (ci == CI && co == CO && k == K && s == S) return launch_fwd<CI, CO, K, S>(ctx, tx, a, st);
    PCC_FWD_G0(PCC_CASE_FWD) PCC_FWD_G1(PCC_CASE_FWD) PCC_FWD_G2(PCC_CASE_FWD) PCC_FWD_G3(PCC_CASE_FWD)
#undef PCC_CASE_FWD
    return no_instantiation(d);
}
#endif
