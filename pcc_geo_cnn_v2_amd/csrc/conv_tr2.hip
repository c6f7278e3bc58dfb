// conv_tr2_kernel / conv_tr2g_kernel (conv_direct.h): Conv3DTranspose stride 2 by output-parity decomposition (8 classes, each a
// small stride-1 gather conv on the input grid).  Compiled once per instantiation group (-DPCC_INST_GROUP=n, Makefile) so that the
// heavily unrolled kernels build in parallel; group 0 holds the entry point pcc_conv_tr2.
#include "conv_direct.h"

#ifndef PCC_INST_GROUP
#define PCC_INST_GROUP 0
#endif

namespace pccmfma {

template <int CIN, int COUT, int KS, int TX, int TZ, int TY, int TXT, int R, int CTW = COUT / 16>
struct Tr2Cfg {
    using G = Tr2Geo<KS>;
    static constexpr int NG = CIN / 16, NCT = COUT / 16;
    static constexpr int RY = 16 / TX;
    static constexpr int NYB = TY / RY, NXB = TXT / TX;
    static constexpr int NCG = NCT / CTW;
    static constexpr int NW = TZ * (NYB / R) * NXB * NCG;
    static constexpr int NT = NW * 64;
    static constexpr int LZ = TZ + G::HL + G::HH, LY = TY + G::HL + G::HH, LX = TXT + G::HL + G::HH;
    static constexpr int VS = CIN + 8;
    static constexpr int NV = LZ * LY * LX;
    static constexpr int LDS_BYTES = NV * VS * 4;
    static constexpr int Q = CIN / 4;  // float4 per voxel
    static constexpr int ITEMS = (NV * Q + NT - 1) / NT;
};

template <int CIN, int COUT, int KS, int TX, int TZ, int TY, int TXT, int R, int CTW = COUT / 16, bool F16 = false>
__global__ void __launch_bounds__((Tr2Cfg<CIN, COUT, KS, TX, TZ, TY, TXT, R, CTW>::NT))
conv_tr2_kernel(ConvArgs a) {
    using C = Tr2Cfg<CIN, COUT, KS, TX, TZ, TY, TXT, R, CTW>;
    using G = Tr2Geo<KS>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;

    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % a.ntx; t /= a.ntx;
    const int ty = t % a.nty; t /= a.nty;
    const int tz = t % a.ntz;
    const int n = t / a.ntz;
    const int bz0 = tz * TZ, by0 = ty * TY, bx0 = tx * TXT;  // base (input-grid) tile origin

    int wv = wave;
    const int ct0 = (wv % C::NCG) * CTW; wv /= C::NCG;
    const int w_xb = wv % C::NXB; wv /= C::NXB;
    const int w_yg = wv % (C::NYB / R);
    const int w_z = wv / (C::NYB / R);
    const int ry = v / TX, rx = v % TX;
    const int ly0 = w_yg * R * C::RY + ry, lx0 = w_xb * TX + rx;
    const float* lbase = lds + (((w_z + G::HL) * C::LY + ly0 + G::HL) * C::LX + lx0 + G::HL) * C::VS + cq * 4;
    constexpr int ROW_OFF = C::RY * C::LX * C::VS;

    // ---- stage the whole haloed tile, all channels (buffer loads: out-of-range voxels read as zeros)
    const float* inb = a.in + (size_t)n * a.D * a.H * a.W * CIN;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(inb, (unsigned)a.D * a.H * a.W * CIN * 4u);
#pragma unroll 1
    for (int it0 = 0; it0 < C::ITEMS; it0 += 8) {
        f32x4 stg[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int item = (it0 + k) * C::NT + tid;
            const int u = item / C::Q, q = item - u * C::Q;
            const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
            const int ly = rem / C::LX, lx = rem - ly * C::LX;
            const int gz = bz0 - G::HL + lz, gy = by0 - G::HL + ly, gx = bx0 - G::HL + lx;
            const bool ok = (item < C::NV * C::Q) && gz >= 0 && gz < a.D && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const unsigned off = (unsigned)(((gz * a.H + gy) * a.W + gx) * CIN + q * 4) * 4u;
            stg[k] = buf_load4(rin, ok ? off : kOOB, 0);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int item = (it0 + k) * C::NT + tid;
            const int u = item / C::Q, q = item - u * C::Q;
            if (item < C::NV * C::Q) *reinterpret_cast<f32x4*>(lds + u * C::VS + q * 4) = stg[k];
        }
    }

    // weights are packed in consumption order [class][tap in class][g][ct]
    constexpr int NSEQ = KS * KS * KS * C::NG;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, (unsigned)(NSEQ * C::NCT) * 1024u);
    const unsigned wlane = lane * 16;
    const int gzb = bz0 + w_z;
    // FULL: the whole (class, tap, g) sequence is unrolled so that a static 3-deep register ring prefetches two
    // units ahead.  For the widest shape (64 -> 64: 3456 MFMAs per wave) that would not fit the instruction
    // cache, so the cin-group loop stays dynamic there and the weights are loaded per (tap, group).
    // (round 3) the one-row, one-cout-tile configuration of the 4-wide grids is small enough to unroll whatever the width (432
    // MFMAs per wave) and needs a deep ring: a unit is 4 MFMAs = 128 cycles there, and loading per (tap, group) on demand left the
    // 64 -> 64 4^3 -> 8^3 layer at 53 us for 6 us of MFMAs.
    constexpr bool FULL = (C::NG * CTW < 16 && C::NG * C::NCT < 16) || R * CTW == 1;
    constexpr int RING = R * CTW == 1 ? 12 : 3;
    f32x4 wf[RING][CTW];
    if constexpr (FULL) {
#pragma unroll
        for (int r = 0; r < RING - 1; ++r)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) wf[r][ct] = buf_load4(rw, wlane, (unsigned)(r * C::NCT + ct0 + ct) * 1024u);
    }
    __syncthreads();

    int seq = 0;  // compile-time after unrolling
#pragma unroll
    for (int pz = 0; pz < 2; ++pz)
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                f32x4 acc[R][CTW];
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kz = (pz + G::PL) & 1; kz < KS; kz += 2)
#pragma unroll
                    for (int ky = (py + G::PL) & 1; ky < KS; ky += 2)
#pragma unroll
                        for (int kx = (px + G::PL) & 1; kx < KS; kx += 2) {
                            const int dz = (pz + G::PL - kz) / 2, dy = (py + G::PL - ky) / 2, dx = (px + G::PL - kx) / 2;
                            const int toff = ((dz * C::LY + dy) * C::LX + dx) * C::VS;
                            if constexpr (FULL) {
#pragma unroll
                                for (int g = 0; g < C::NG; ++g, ++seq) {
                                    {
                                        const int qn = (seq + RING - 1 < NSEQ) ? seq + RING - 1 : NSEQ - 1;
#pragma unroll
                                        for (int ct = 0; ct < CTW; ++ct)
                                            wf[(seq + RING - 1) % RING][ct] = buf_load4(rw, wlane, (unsigned)(qn * C::NCT + ct0 + ct) * 1024u);
                                        PCC_PIN_VMEM();
                                    }
                                    f32x4 b[R];
#pragma unroll
                                    for (int i = 0; i < R; ++i)
                                        b[i] = *reinterpret_cast<const f32x4*>(lbase + toff + i * ROW_OFF + g * 16);
                                    if constexpr (F16) {
#pragma unroll
                                        for (int i = 0; i < R; ++i)
#pragma unroll
                                            for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = mfma16h(wf[seq % RING][ct], b[i], acc[i][ct]);
                                    } else {
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
#pragma unroll
                                        for (int i = 0; i < R; ++i)
#pragma unroll
                                            for (int ct = 0; ct < CTW; ++ct)
                                                acc[i][ct] = mfma16(wf[seq % RING][ct][j], b[i][j], acc[i][ct]);
                                    }
                                }
                            } else {
                                const int seq0 = seq;
                                seq += C::NG;
#pragma unroll 1
                                for (int g = 0; g < C::NG; ++g) {
                                    f32x4 w1[CTW];
#pragma unroll
                                    for (int ct = 0; ct < CTW; ++ct)
                                        w1[ct] = buf_load4(rw, wlane, (unsigned)((seq0 + g) * C::NCT + ct0 + ct) * 1024u);
                                    f32x4 b[R];
#pragma unroll
                                    for (int i = 0; i < R; ++i)
                                        b[i] = *reinterpret_cast<const f32x4*>(lbase + toff + i * ROW_OFF + g * 16);
                                    if constexpr (F16) {
#pragma unroll
                                        for (int i = 0; i < R; ++i)
#pragma unroll
                                            for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = mfma16h(w1[ct], b[i], acc[i][ct]);
                                    } else {
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
#pragma unroll
                                        for (int i = 0; i < R; ++i)
#pragma unroll
                                            for (int ct = 0; ct < CTW; ++ct)
                                                acc[i][ct] = mfma16(w1[ct][j], b[i][j], acc[i][ct]);
                                    }
                                }
                            }
                        }
                // epilogue of this parity class
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int gyb = by0 + ly0 + i * C::RY, gxb = bx0 + lx0;
                    if (gzb < a.D && gyb < a.H && gxb < a.W) {
                        const size_t vox = (((size_t)n * a.OD + 2 * gzb + pz) * a.OH + 2 * gyb + py) * a.OW + 2 * gxb + px;
#pragma unroll
                        for (int ct = 0; ct < CTW; ++ct) store_out(a, acc[i][ct], vox, (ct0 + ct) * 16 + cq * 4, COUT);
                    }
                }
            }
}

// =====================================================================================================
// transposed conv, stride 2, k = 3: channel-group pipelined variant (conv_tr2g_kernel).
//   Same parity decomposition, but the loop nest is  cin group (16 ch) -> parity class -> tap:
//   * one 16-channel group of the haloed input tile is staged at a time, global -> LDS directly
//     (buffer_load ... lds: no staging registers, no ds_write, no per-item index math in the loop) into a double
//     buffer; group g+1 is in flight while group g feeds the MFMAs;
//   * the accumulators of ALL 8 parity classes stay live across the groups (8 x R x CTW float4);
//   * the epilogue uses per-row offsets computed once and one buffer descriptor per parity class.
// =====================================================================================================
template <int CIN, int COUT, int TX, int TZ, int TY, int TXT, int R, int CTW>
struct Tr2gCfg {
    static constexpr int NG = CIN / 16, NCT = COUT / 16;
    static constexpr int RY = 16 / TX;
    static constexpr int NYB = TY / RY, NXB = TXT / TX;
    static constexpr int NCG = NCT / CTW;
    static constexpr int NW = TZ * (NYB / R) * NXB * NCG;
    static constexpr int NT = NW * 64;
    static constexpr int LZ = TZ + 1, LY = TY + 1, LX = TXT + 1;     // k3: taps reach b-1 only
    static constexpr int VSQ = 5;                                     // 16-byte slots per voxel: 4 data + 1 pad (80 B stride)
    static constexpr int VS = VSQ * 4;
    static constexpr int NV = LZ * LY * LX;
    static constexpr int CHUNKS = (NV * VSQ + 63) / 64;               // 1 KB wave-sized chunks of one group image
    static constexpr int ITEMS = (CHUNKS + NW - 1) / NW;              // chunks per wave
    static constexpr int BUF_BYTES = ITEMS * NW * 1024;
    static constexpr int LDS_BYTES = 2 * BUF_BYTES;
};

// tap seq (0..26) of the parity-class order [class (pz,py,px)][kz][ky][kx]: its class, input offsets (0 / -1 per dim), and
// whether it is the first / last tap of its class.  Evaluated at compile time (seq is a constant of the unrolled loops).
struct Tr2gTap { int cls, dz, dy, dx; bool first, last; };
__host__ __device__ constexpr Tr2gTap tr2g_tap(int want) {
    int seq = 0;
    for (int cls = 0; cls < 8; ++cls) {
        const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
        const int ntap = (pz ? 1 : 2) * (py ? 1 : 2) * (px ? 1 : 2);      // even outputs take taps 0 and 2, odd ones tap 1
        int t = 0;
        for (int kz = pz; kz < 3; kz += 2)
            for (int ky = py; ky < 3; ky += 2)
                for (int kx = px; kx < 3; kx += 2, ++seq, ++t)
                    if (seq == want) return Tr2gTap{cls, (pz - kz) / 2, (py - ky) / 2, (px - kx) / 2, t == 0, t == ntap - 1};
    }
    return Tr2gTap{0, 0, 0, 0, false, false};
}

// EPI: the epilogue is compiled for the layer's flags (the per-store flag tests of a generic epilogue cost this kernel more
// scalar registers and branches than it has to spare): 0 = bias / ReLU, fp32 store (every stride-2 transposed layer of the c*
// graphs); 1 = bias / ReLU, fp16 store (PCC_CONV_OUT16, the fp16 mode); 2 = any flags (residual, clip), tested at run time.
enum { TR2G_EPI_F32 = 0, TR2G_EPI_F16 = 1, TR2G_EPI_ANY = 2 };

template <int CIN, int COUT, int TX, int TZ, int TY, int TXT, int R, int CTW, bool F16 = false, int EPI = TR2G_EPI_F32>
__global__ void __launch_bounds__((Tr2gCfg<CIN, COUT, TX, TZ, TY, TXT, R, CTW>::NT), 2)   // two waves per SIMD: <= 256 registers
conv_tr2g_kernel(ConvArgs a, int ntiles) {
    using C = Tr2gCfg<CIN, COUT, TX, TZ, TY, TXT, R, CTW>;
    static_assert(C::NG % 2 == 0, "the LDS double buffer alternates per cin group across tiles");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;
    const int G = gridDim.x;
    int tile = xcd_remap(blockIdx.x, G);
    if (tile >= ntiles) return;

    int wv = wave;
    const int ct0 = (wv % C::NCG) * CTW; wv /= C::NCG;
    const int w_xb = wv % C::NXB; wv /= C::NXB;
    const int w_yg = wv % (C::NYB / R);
    const int w_z = wv / (C::NYB / R);
    const int ry = v / TX, rx = v % TX;
    const int ly0 = w_yg * R * C::RY + ry, lx0 = w_xb * TX + rx;
    // B operand base: voxel (w_z+1, ly0+1, lx0+1) of the haloed tile, channel quad cq
    const int lane_off = (((w_z + 1) * C::LY + ly0 + 1) * C::LX + lx0 + 1) * C::VS + cq * 4;
    constexpr int ROW_OFF = C::RY * C::LX * C::VS;

    // ---- staging items of this lane (fixed for the life of the workgroup): the tile-local voxel packed in 10-bit fields
    //      (lz | ly << 10 | lx << 20; pad slots carry an lz that fails every range test) and its byte offset relative to the
    //      tile's first haloed voxel.  Per tile the range test of all three dims is two packed adds: with a bias of 512 per
    //      field, bit 9 of (p + lo) says g >= 0 and bit 9 of (hi - p) says g <= dim - 1 (fields neither carry nor borrow:
    //      coordinates and dims stay below 256 -- the launcher checks).
    unsigned pk[C::ITEMS], rel[C::ITEMS];
    {
        const int HWc = a.H * a.W * CIN * 4, Wc = a.W * CIN * 4;
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) {
            const int slot = (wave * C::ITEMS + it) * 64 + lane;
            const int u = slot / C::VSQ, q = slot - u * C::VSQ;
            const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
            const int ly = rem / C::LX, lx = rem - ly * C::LX;
            const bool data = u < C::NV && q < 4;
            pk[it] = data ? (unsigned)(lz | (ly << 10) | (lx << 20)) : 511u;
            rel[it] = data ? (unsigned)(lz * HWc + ly * Wc + lx * (CIN * 4) + q * 16) : 0u;
        }
    }
    constexpr unsigned kBit9 = (1u << 9) | (1u << 19) | (1u << 29);
    const unsigned in_bytes = (unsigned)a.D * a.H * a.W * CIN * 4u;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    // global -> LDS of cin group g of tile (n, bz0, by0, bx0): zeros land in LDS for SAME padding, tile overhang, pad slots
    auto stage_group = [&](int n_, int bz0, int by0, int bx0, int g, int buf) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.in + (size_t)n_ * a.D * a.H * a.W * CIN + g * 16, in_bytes - (unsigned)g * 64u);
        const int HWc = a.H * a.W * CIN * 4, Wc = a.W * CIN * 4;
        const unsigned lo = (unsigned)((bz0 - 1 + 512) | ((by0 - 1 + 512) << 10) | ((bx0 - 1 + 512) << 20));
        const unsigned hi = (unsigned)((a.D - bz0 + 512) | ((a.H - by0 + 512) << 10) | ((a.W - bx0 + 512) << 20));
        const unsigned base = (unsigned)((bz0 - 1) * HWc + (by0 - 1) * Wc + (bx0 - 1) * (CIN * 4));     // (may wrap below 0: rel brings it back)
#pragma unroll
        for (int it = 0; it < C::ITEMS; ++it) {
            const bool ok = (((pk[it] + lo) & (hi - pk[it])) & kBit9) == kBit9;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (lds_ptr)((char*)lds + buf * C::BUF_BYTES + (wave * C::ITEMS + it) * 1024), 16,
                                                     (int)(ok ? base + rel[it] : kOOB), 0, 0, 0);
        }
    };
    auto decode = [&](int t, int& n_, int& bz0, int& by0, int& bx0) {
        const int tx = t % a.ntx; t /= a.ntx;
        const int ty = t % a.nty; t /= a.nty;
        bz0 = (t % a.ntz) * TZ; by0 = ty * TY; bx0 = tx * TXT; n_ = t / a.ntz;
    };

    int n, bz0, by0, bx0;
    decode(tile, n, bz0, by0, bx0);
    stage_group(n, bz0, by0, bx0, 0, 0);

    // weights packed in consumption order [g][class][tap in class][ct]
    constexpr int NSEQ = 27;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, (unsigned)(NSEQ * C::NG * C::NCT) * 1024u);
    const unsigned wlane = lane * 16;
    // vmcnt retires in order: a weight load issued AFTER the staging loads of the next group cannot be consumed before
    // those have landed (HBM latency).  A deep ring (8 taps ahead = ~4500 cycles) keeps that wait out of the tap loop.
    constexpr int RING = (CTW == 1) ? 9 : 3;
    static_assert(NSEQ % RING == 0, "the weight ring position must repeat per group");
    f32x4 wf[RING][CTW];
    const size_t ovox_n = (size_t)a.OD * a.OH * a.OW;
    const bool any_res = EPI == TR2G_EPI_ANY && (a.flags & PCC_CONV_ADD) != 0;
    const bool any_out16 = EPI == TR2G_EPI_ANY && (a.flags & PCC_CONV_OUT16) != 0;
    const bool out16 = EPI == TR2G_EPI_F16 || any_out16;
    const float relu_lo = (a.flags & PCC_CONV_RELU) ? 0.f : -__builtin_inff();
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 bias4[CTW];
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct)
        bias4[ct] = (a.flags & PCC_CONV_BIAS) ? *reinterpret_cast<const f32x4*>(a.bias + (ct0 + ct) * 16 + cq * 4) : zero4;

    // The weight stream wraps around: the last group of a tile prefetches the first RING - 1 taps of the NEXT tile (same
    // weights).  Restarting it at the top of a tile would put those loads behind the tile's last stores, and the in-order
    // vmcnt wait at the first barrier would then wait for the store acknowledgements.
#pragma unroll
    for (int r = 0; r < RING - 1; ++r)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) wf[r][ct] = buf_load4(rw, wlane, (unsigned)(r * C::NCT + ct0 + ct) * 1024u);
    f32x4 acc[8][R][CTW];
#pragma unroll 1
    for (;;) {
        const int next = tile + G;
        const bool has_next = next < ntiles;
        int nn = n, nbz0 = bz0, nby0 = by0, nbx0 = bx0;
        if (has_next) decode(next, nn, nbz0, nby0, nbx0);
        // per-row output BYTE offsets of this tile for class (0,0,0) (the epilogue of a parity class runs inside the last
        // group, right after the class's taps: the 8 x R x CTW stores of a tile are spread over that group instead of bursting
        // at its end).  One descriptor per tile (image n); the class adds a wave-uniform offset.  kOOB plus those offsets
        // stays beyond the descriptor's range (the launcher admits images below 2^31 bytes only).
        const int gzb = bz0 + w_z, gxb = bx0 + lx0;
        const unsigned esz = out16 ? 2u : 4u;
        unsigned ooff[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int gyb = by0 + ly0 + i * C::RY;
            const bool ok = gzb < a.D && gyb < a.H && gxb < a.W;
            const unsigned vox = (unsigned)((2 * gzb * a.OH + 2 * gyb) * a.OW + 2 * gxb);
            ooff[i] = ok ? (vox * (unsigned)a.ocs + (unsigned)a.oco + cq * 4) * esz : kOOB;
        }
        const __amdgpu_buffer_rsrc_t rout = make_rsrc((const char*)a.out + (size_t)n * ovox_n * a.ocs * esz, (unsigned)(ovox_n * a.ocs * esz));
        // residual (EPI_ANY only; no layer of the c* graphs adds one to a stride-2 transposed conv): offsets computed on demand
        const __amdgpu_buffer_rsrc_t rres = make_rsrc(any_res ? a.res + (size_t)n * ovox_n * COUT : a.in, any_res ? (unsigned)(ovox_n * COUT * 4) : 0u);
        auto roff_of = [&](int i) -> unsigned {
            const int gyb = by0 + ly0 + i * C::RY;
            const bool ok = gzb < a.D && gyb < a.H && gxb < a.W;
            return ok ? ((unsigned)((2 * gzb * a.OH + 2 * gyb) * a.OW + 2 * gxb) * (unsigned)COUT + cq * 4) * 4u : kOOB;
        };

        // one cin group of the tile.  FIRST: the accumulators start from 0 (srcC = inline 0, no zero-init pass);
        // LAST: each parity class is finished and stored right after its taps.
        auto group = [&](auto first_tag, auto last_tag, int g) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
            // group g has landed in LDS (this wave's loads: vmcnt; the other waves': barrier); nobody reads the other buffer any more
            __builtin_amdgcn_s_waitcnt(0x0F70 | ((RING - 1) * CTW));    // vmcnt(weights still in flight) expcnt(7) lgkmcnt(15)
            __syncthreads();
            if (!LAST) stage_group(n, bz0, by0, bx0, g + 1, (g + 1) & 1);
            else if (has_next) stage_group(nn, nbz0, nby0, nbx0, 0, 0);          // next tile's first group under this tile's last
            const float* lbase = lds + (g & 1) * (C::BUF_BYTES / 4) + lane_off;
            const unsigned wg_off = (unsigned)(g * NSEQ * C::NCT) * 1024u;
            // B operands are read one tap ahead (double buffer): the LDS latency of tap t + 1 runs under the MFMAs of tap t
            f32x4 b[2][R];
#pragma unroll
            for (int i = 0; i < R; ++i) b[0][i] = *reinterpret_cast<const f32x4*>(lbase + i * ROW_OFF);       // tap 0: class (0,0,0), no offset
            static_for(std::make_integer_sequence<int, NSEQ>{}, [&](auto seq_tag) __attribute__((always_inline)) {
                constexpr int seq = decltype(seq_tag)::value;
                constexpr Tr2gTap T = tr2g_tap(seq);
                constexpr Tr2gTap Tn = tr2g_tap(seq + 1 < NSEQ ? seq + 1 : seq);
                constexpr int next_off = ((Tn.dz * C::LY + Tn.dy) * C::LX + Tn.dx) * C::VS;
                constexpr int cls = T.cls;
                // weights RING - 1 taps ahead: runs into the next group's first taps, and from the last group into the next tile's
                constexpr bool wrap = LAST && seq + RING - 1 >= NSEQ;
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct)
                    wf[(seq + RING - 1) % RING][ct] = buf_load4(rw, wlane, (wrap ? 0u : wg_off) + (unsigned)((seq + RING - 1 - (wrap ? NSEQ : 0)) * C::NCT + ct0 + ct) * 1024u);
                if constexpr (seq + 1 < NSEQ) {
#pragma unroll
                    for (int i = 0; i < R; ++i) b[(seq + 1) & 1][i] = *reinterpret_cast<const f32x4*>(lbase + next_off + i * ROW_OFF);
                }
                PCC_PIN_MEM_MFMA();
                constexpr bool open = FIRST && T.first;  // first tap of the class in the first group: start from the bias
                if constexpr (F16) {
#pragma unroll
                    for (int i = 0; i < R; ++i)
#pragma unroll
                        for (int ct = 0; ct < CTW; ++ct) acc[cls][i][ct] = mfma16h(wf[seq % RING][ct], b[seq & 1][i], open ? bias4[ct] : acc[cls][i][ct]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < R; ++i)
#pragma unroll
                            for (int ct = 0; ct < CTW; ++ct)
                                acc[cls][i][ct] = mfma16(wf[seq % RING][ct][j], b[seq & 1][i][j], (open && j == 0) ? bias4[ct] : acc[cls][i][ct]);
                }
                if constexpr (LAST && T.last) {      // this class is complete: ReLU (/ residual / clip), stores (the bias is already in)
                    constexpr int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
                    const unsigned coff = (unsigned)(((pz * a.OH + py) * a.OW + px) * a.ocs) * esz;  // (wave-uniform) bytes
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                        for (int i = 0; i < R; ++i) {
                            f32x4 o = acc[cls][i][ct];
                            // one v_maximum3_f32 per element (fmaxf on a raw MFMA result costs a second v_max that quiets NaNs)
                            o = __builtin_elementwise_maximum(o, (f32x4){relu_lo, relu_lo, relu_lo, relu_lo});
                            if constexpr (EPI == TR2G_EPI_ANY) {
                                if (any_res) o += buf_load4(rres, roff_of(i), (unsigned)((((pz * a.OH + py) * a.OW + px) * COUT + (ct0 + ct) * 16) * 4));
                                if (a.flags & PCC_CONV_CLIP01) {
#pragma unroll
                                    for (int c = 0; c < 4; ++c) o[c] = fminf(fmaxf(o[c], 0.f), 1.f);
                                }
                            }
                            const unsigned boff = ooff[i] + coff + (unsigned)((ct0 + ct) * 16) * esz;
                            if (EPI == TR2G_EPI_F16 || (EPI == TR2G_EPI_ANY && any_out16)) {
                                f16x4 oh;
#pragma unroll
                                for (int c = 0; c < 4; ++c) oh[c] = (_Float16)o[c];
                                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, oh), rout, (int)boff, 0, 0);
                            } else {
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rout, (int)boff, 0, 0);
                            }
                        }
                }
            });
        };
        group(std::true_type{}, std::false_type{}, 0);
#pragma unroll 1
        for (int g = 1; g < C::NG - 1; ++g) group(std::false_type{}, std::false_type{}, g);
        group(std::false_type{}, std::true_type{}, C::NG - 1);

        if (!has_next) break;
        tile = next; n = nn; bz0 = nbz0; by0 = nby0; bx0 = nbx0;
    }
}

template <int CIN, int COUT, int KS>
int launch_tr2(const pcc_ctx* ctx, int tx, ConvArgs a, hipStream_t st) {
#define PCC_TR2(TX, TZ, TY, TXT, R) PCC_TR2C(TX, TZ, TY, TXT, R, (COUT / 16))
#define PCC_TR2C(TX, TZ, TY, TXT, R, CTW)                                                               \
    {                                                                                                   \
        using C = Tr2Cfg<CIN, COUT, KS, TX, TZ, TY, TXT, R, CTW>;                                       \
        a.ntz = cdiv(a.D, TZ); a.nty = cdiv(a.H, TY); a.ntx = cdiv(a.W, TXT);                           \
        if (a.flags & PCC_CONV_F16)                                                                     \
            return launch(conv_tr2_kernel<CIN, COUT, KS, TX, TZ, TY, TXT, R, CTW, true>, C::NT, C::LDS_BYTES, \
                          a.N * a.ntz * a.nty * a.ntx, a, st);                                          \
        return launch(conv_tr2_kernel<CIN, COUT, KS, TX, TZ, TY, TXT, R, CTW>, C::NT, C::LDS_BYTES,     \
                      a.N * a.ntz * a.nty * a.ntx, a, st);                                              \
    }
#define PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, F16, EPI)                                                  \
    return launch(conv_tr2g_kernel<CIN, COUT, TX, TZ, TY, TXT, R, CTW, F16, EPI>, C::NT, C::LDS_BYTES,       \
                  ntiles < slots ? ntiles : slots, a, st, ntiles);
#define PCC_TR2G(TX, TZ, TY, TXT, R, CTW)                                                               \
    if ((double)a.OD * a.OH * a.OW * a.ocs * 4.0 < 2147483648.0 && a.D < 512 && a.H < 512 && a.W < 512) { \
        using C = Tr2gCfg<CIN, COUT, TX, TZ, TY, TXT, R, CTW>;                                          \
        a.w += 27 * CIN * COUT;                                                                         \
        a.ntz = cdiv(a.D, TZ); a.nty = cdiv(a.H, TY); a.ntx = cdiv(a.W, TXT);                           \
        const int ntiles = a.N * a.ntz * a.nty * a.ntx;                                                 \
        const int slots = ctx->num_cu * (C::NT > 256 ? 1 : 2);                                          \
        const bool plain = !(a.flags & (PCC_CONV_ADD | PCC_CONV_CLIP01));                               \
        if (a.flags & PCC_CONV_F16) {                                                                   \
            if (plain && (a.flags & PCC_CONV_OUT16)) PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, true, TR2G_EPI_F16) \
            if (plain) PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, true, TR2G_EPI_F32)                        \
            PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, true, TR2G_EPI_ANY)                                   \
        }                                                                                               \
        if (plain) PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, false, TR2G_EPI_F32)                           \
        PCC_TR2G_EPI(TX, TZ, TY, TXT, R, CTW, false, TR2G_EPI_ANY)                                      \
    }
    const bool tr2_old = ctx->num(PCC_NUM_TR2_OLD);
    if (tx == 16) {
        if constexpr (KS == 3) { if (!tr2_old) { if constexpr (CIN >= 64) { PCC_TR2G(16, 2, 4, 16, 2, 2) } else { PCC_TR2G(16, 2, 8, 16, 4, 1) } } }
        if constexpr (CIN >= 64) PCC_TR2(16, 2, 4, 16, 2)
        else PCC_TR2(16, 2, 8, 16, 4)
    }
    if (tx == 8) {
        if constexpr (KS == 3) { if (!tr2_old) { if constexpr (COUT >= 64) { PCC_TR2G(8, 2, 4, 8, 1, 1) } else { PCC_TR2G(8, 2, 8, 8, 2, 1) } } }
        if constexpr (COUT >= 64 && KS == 3) PCC_TR2C(8, 2, 4, 8, 1, 1)
        else PCC_TR2(8, 2, 8, 8, 2)
    }
#undef PCC_TR2G
#undef PCC_TR2G_EPI
    if constexpr (COUT >= 32 && KS == 3) PCC_TR2C(4, 1, 4, 4, 1, 1)
    else PCC_TR2(4, 4, 4, 4, 1)
#undef PCC_TR2
#undef PCC_TR2C
}

// ---- instantiation groups (CIN, COUT, KS): one object each
#define PCC_TR2_G0(X) X(32, 32, 5)
#define PCC_TR2_G1(X) X(64, 64, 3) X(64, 32, 3)
#define PCC_TR2_G2(X) X(32, 16, 3) X(32, 32, 3)
#define PCC_INST_TR2(CI, CO, K) template int launch_tr2<CI, CO, K>(const pcc_ctx*, int, ConvArgs, hipStream_t);
#define PCC_EXT_TR2(CI, CO, K) extern template int launch_tr2<CI, CO, K>(const pcc_ctx*, int, ConvArgs, hipStream_t);
#if PCC_INST_GROUP == 0
PCC_TR2_G1(PCC_EXT_TR2) PCC_TR2_G2(PCC_EXT_TR2)
#elif PCC_INST_GROUP == 1
PCC_TR2_G1(PCC_INST_TR2)
#elif PCC_INST_GROUP == 2
PCC_TR2_G2(PCC_INST_TR2)
#endif

}  // namespace pccmfma

#if PCC_INST_GROUP == 0
using namespace pccmfma;

int pcc_conv_tr2(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                 float* out, int tx, hipStream_t st) {
    const ConvArgs a = conv_args(d, in, w_packed, bias, residual, out);
    const int ci = d->Cin, co = d->Cout, k = d->k;
#define PCC_CASE_TR2(CI, CO, K) if (ci == CI && co == CO && k == K) return launch_tr2<CI, CO, K>(ctx, tx, a, st);
    PCC_TR2_G0(PCC_CASE_TR2) PCC_TR2_G1(PCC_CASE_TR2) PCC_TR2_G2(PCC_CASE_TR2)
#undef PCC_CASE_TR2
    return no_instantiation(d);
}
#endif
