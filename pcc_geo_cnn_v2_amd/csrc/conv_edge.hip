// The first and last layers of the transforms on the direct MFMA path (conv_direct.h):
//   conv_cin1_kernel      : Conv3D with Cin = 1 (first layer): k-slots of the MFMA are kernel taps along x.
//   conv_cout1_kernel     : Conv3DTranspose with Cout = 1 (last layer): VALU dot products from an LDS tile.
//   conv_cout1_mfma_kernel: Conv3DTranspose 16 -> 1, k3, stride 1 on the matrix cores, optionally with the occupancy bits.
#include "conv_direct.h"

namespace pccmfma {

// =====================================================================================================
// forward conv with Cin = 1, stride 2 (first layer of every analysis transform).
//   k-slots of each MFMA = 4 consecutive taps along x (x taps padded to a multiple of 4 with zero
//   weights), so the B operand is one ds_read_b32 with an immediate offset.
//   tile = TZ x TY x 16 output voxels; wave owns R rows consecutive in y.
// =====================================================================================================
template <int COUT, int KS, int TZ, int TY, int R>
struct Cin1Cfg {
    static constexpr int S = 2;
    static constexpr int NCT = COUT / 16;
    static constexpr int KXG = (KS + 3) / 4;  // groups of 4 x-taps
    static constexpr int NW = TZ * (TY / R);
    static constexpr int NT = NW * 64;
    static constexpr int PL = (KS - 2) / 2;
    static constexpr int LZ = (TZ - 1) * S + KS, LY = (TY - 1) * S + KS;
    static constexpr int LXU = 15 * S + KXG * 4;             // x extent actually addressed
    static constexpr int LX = (LXU | 1);                     // odd row stride: fewer bank conflicts
    static constexpr int NV = LZ * LY * LX;
    static constexpr int LDS_BYTES = NV * 4;
    static constexpr int ITEMS = (NV + NT - 1) / NT;
};

template <int COUT, int KS, int TZ, int TY, int R>
__global__ void __launch_bounds__((Cin1Cfg<COUT, KS, TZ, TY, R>::NT)) conv_cin1_kernel(ConvArgs a) {
    using C = Cin1Cfg<COUT, KS, TZ, TY, R>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, kq = lane >> 4;

    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % a.ntx; t /= a.ntx;
    const int ty = t % a.nty; t /= a.nty;
    const int tz = t % a.ntz;
    const int n = t / a.ntz;
    const int oz0 = tz * TZ, oy0 = ty * TY, ox0 = tx * 16;
    const int iz0 = oz0 * 2 - C::PL, iy0 = oy0 * 2 - C::PL, ix0 = ox0 * 2 - C::PL;

    const float* inb = a.in + (size_t)n * a.D * a.H * a.W;
    if constexpr (KS == 3) {
        // k3: no low-side halo (PL = 0) and ix0 = 32 tx, so a row of the tile is 9 aligned float4 of one image row: all loads of a
        // thread are in flight together (the scalar loop below spent ~50 VALU instructions per element on index arithmetic: the
        // kernel was VALU-bound at 0.14 of the MFMA peak with its matrix pipe 4 % busy)
        constexpr int Q = (C::LXU + 3) / 4, ROWS = C::LZ * C::LY, NITEM = ROWS * Q, PER = (NITEM + C::NT - 1) / C::NT;
        const size_t img = (size_t)a.D * a.H * a.W;
        const __amdgpu_buffer_rsrc_t rin = make_rsrc(inb, (unsigned)(img * 4));       // (the planner admits < 2 GiB per image)
        f32x4 v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int it = i * C::NT + tid, row = it / Q, q = it - row * Q;
            const int lz = row / C::LY, ly = row - lz * C::LY;
            const int gz = iz0 + lz, gy = iy0 + ly, gx = ix0 + 4 * q;
            const bool ok = it < NITEM && gz < a.D && gy < a.H && gx < a.W;
            v[i] = buf_load4(rin, ok ? (unsigned)((((size_t)gz * a.H + gy) * a.W + gx) * 4) : kOOB, 0);
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int it = i * C::NT + tid, row = it / Q, q = it - row * Q;
            if (it < NITEM) {
                float* lp = lds + row * C::LX + 4 * q;
                const int gx = ix0 + 4 * q;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < C::LX) lp[e] = (gx + e < a.W) ? v[i][e] : 0.f;       // beyond the image row: SAME padding
            }
        }
    } else {
#pragma unroll 1
    for (int it = 0; it < C::ITEMS; ++it) {
        const int u = it * C::NT + tid;
        const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
        const int ly = rem / C::LX, lx = rem - ly * C::LX;
        const int gz = iz0 + lz, gy = iy0 + ly, gx = ix0 + lx;
        if (u < C::NV) {
            const bool ok = gz >= 0 && gz < a.D && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            lds[u] = ok ? inb[((size_t)gz * a.H + gy) * a.W + gx] : 0.f;
        }
    }
    }
    __syncthreads();

    const int w_yg = wave % (TY / R), w_z = wave / (TY / R);
    const float* lbase = lds + ((w_z * 2) * C::LY + (w_yg * R) * 2) * C::LX + v * 2 + kq;
    constexpr int ROW_OFF = 2 * C::LX;

    f32x4 acc[R][C::NCT];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int ct = 0; ct < C::NCT; ++ct) acc[i][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const float* wp = a.w + lane;  // packed [kz][ky][kxg][ct][lane]
#pragma unroll 1
    for (int kz = 0; kz < KS; ++kz) {
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
            for (int kg = 0; kg < C::KXG; ++kg) {
                float wf[C::NCT];
#pragma unroll
                for (int ct = 0; ct < C::NCT; ++ct) wf[ct] = wp[(size_t)((((kz * KS + ky) * C::KXG + kg) * C::NCT) + ct) * 64];
                const float* lp = lbase + (kz * C::LY + ky) * C::LX + kg * 4;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const float b = lp[i * ROW_OFF];
#pragma unroll
                    for (int ct = 0; ct < C::NCT; ++ct) acc[i][ct] = mfma16(wf[ct], b, acc[i][ct]);
                }
            }
        }
    }

    const int gz = oz0 + w_z;
    float mx = 0.f;      // max |stored value| of this lane (NaNs skipped: fmaxf returns the other operand)
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gy = oy0 + w_yg * R + i, gx = ox0 + v;
        if (gz < a.OD && gy < a.OH && gx < a.OW) {
            const size_t vox = (((size_t)n * a.OD + gz) * a.OH + gy) * a.OW + gx;
#pragma unroll
            for (int ct = 0; ct < C::NCT; ++ct) {
                const f32x4 o = store_out(a, acc[i][ct], vox, ct * 16 + kq * 4, COUT);
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
            }
        }
    }
    // the fp16-split layer behind this one scales block n by its max |x| (conv_wino_f16s.hip): order-independent atomicMax of bit patterns
    if (a.amax_out != nullptr) pcc_amax_record(a.amax_out + (size_t)n * PCC_AMAX_SLOTS, mx, (int)blockIdx.x + wave);
}

// =====================================================================================================
// transposed conv with Cout = 1 (last synthesis layer): VALU.  One thread = one output voxel... each
// thread accumulates CIN x taps FMAs reading float4 channel quads from an LDS tile; weights are read
// through the scalar cache (uniform addresses).
//   S = 1: gather conv with (host-)flipped weights, pad (KS-1)/2.
//   S = 2: parity decomposition; a thread produces the 8 outputs of one base voxel.
// Accumulation order: taps (kz,ky,kx) outer, channels inner, fp32 FMA chain -> deterministic.
// =====================================================================================================
template <int CIN, int KS, int S, int TZ, int TY, int TXT>
struct Cout1Cfg {
    static constexpr int NT = TZ * TY * TXT;  // one thread per base voxel
    static constexpr int PLO = (S == 1) ? (KS - 1) / 2 : Tr2Geo<KS>::HL;
    static constexpr int PHI = (S == 1) ? (KS - 1) / 2 : Tr2Geo<KS>::HH;
    static constexpr int LZ = TZ + PLO + PHI, LY = TY + PLO + PHI, LX = TXT + PLO + PHI;
    static constexpr int VS = CIN + 4;  // +4: consecutive voxels land on different bank slots
    static constexpr int NV = LZ * LY * LX;
    static constexpr int LDS_BYTES = NV * VS * 4;
    static constexpr int Q = CIN / 4;
};

template <int CIN, int KS, int S, int TZ, int TY, int TXT>
__global__ void __launch_bounds__((Cout1Cfg<CIN, KS, S, TZ, TY, TXT>::NT)) conv_cout1_kernel(ConvArgs a) {
    using C = Cout1Cfg<CIN, KS, S, TZ, TY, TXT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % a.ntx; t /= a.ntx;
    const int ty = t % a.nty; t /= a.nty;
    const int tz = t % a.ntz;
    const int n = t / a.ntz;
    const int bz0 = tz * TZ, by0 = ty * TY, bx0 = tx * TXT;

    const float* inb = a.in + (size_t)n * a.D * a.H * a.W * CIN;
#pragma unroll 1
    for (int item = tid; item < C::NV * C::Q; item += C::NT) {
        const int u = item / C::Q, q = item - u * C::Q;
        const int lz = u / (C::LY * C::LX), rem = u - lz * (C::LY * C::LX);
        const int ly = rem / C::LX, lx = rem - ly * C::LX;
        const int gz = bz0 - C::PLO + lz, gy = by0 - C::PLO + ly, gx = bx0 - C::PLO + lx;
        const bool ok = gz >= 0 && gz < a.D && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        f32x4 val = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ok) val = *reinterpret_cast<const f32x4*>(inb + (((size_t)gz * a.H + gy) * a.W + gx) * CIN + q * 4);
        *reinterpret_cast<f32x4*>(lds + u * C::VS + q * 4) = val;
    }
    __syncthreads();

    const int lx = tid % TXT, ly = (tid / TXT) % TY, lz = tid / (TXT * TY);
    const float* lbase = lds + (((lz + C::PLO) * C::LY + ly + C::PLO) * C::LX + lx + C::PLO) * C::VS;
    const int gz = bz0 + lz, gy = by0 + ly, gx = bx0 + lx;
    const bool inb_ok = gz < a.D && gy < a.H && gx < a.W;
    const float bias = (a.flags & PCC_CONV_BIAS) ? a.bias[0] : 0.f;
    const f32x4* wq = reinterpret_cast<const f32x4*>(a.w);  // packed [tap][CIN/4] float4 (S=1: already flipped)

    auto finish = [&](float s, size_t vox) {
        s += bias;
        if (a.flags & PCC_CONV_RELU) s = fmaxf(s, 0.f);
        if (a.flags & PCC_CONV_ADD) s += a.res[vox];
        if (a.flags & PCC_CONV_CLIP01) s = fminf(fmaxf(s, 0.f), 1.f);
        a.out[vox * a.ocs + a.oco] = s;
    };

    if constexpr (S == 1) {
        float s = 0.f;
#pragma unroll 1
        for (int kz = 0; kz < KS; ++kz)
#pragma unroll
            for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const float* lp = lbase + (((kz - C::PLO) * C::LY + (ky - C::PLO)) * C::LX + (kx - C::PLO)) * C::VS;
                    const f32x4* wt = wq + (size_t)((kz * KS + ky) * KS + kx) * C::Q;
#pragma unroll
                    for (int q = 0; q < C::Q; ++q) {
                        const f32x4 x = *reinterpret_cast<const f32x4*>(lp + q * 4);
                        const f32x4 w = wt[q];
                        s = fmaf(x.x, w.x, s); s = fmaf(x.y, w.y, s); s = fmaf(x.z, w.z, s); s = fmaf(x.w, w.w, s);
                    }
                }
        if (inb_ok) finish(s, (((size_t)n * a.OD + gz) * a.OH + gy) * a.OW + gx);
    } else {
        using G = Tr2Geo<KS>;
#pragma unroll 1
        for (int pz = 0; pz < 2; ++pz)
#pragma unroll 1
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    float s = 0.f;
                    for (int kz = (pz + G::PL) & 1; kz < KS; kz += 2)
                        for (int ky = (py + G::PL) & 1; ky < KS; ky += 2)
#pragma unroll
                            for (int kx = (px + G::PL) & 1; kx < KS; kx += 2) {
                                const int dz = (pz + G::PL - kz) / 2, dy = (py + G::PL - ky) / 2, dx = (px + G::PL - kx) / 2;
                                const float* lp = lbase + ((dz * C::LY + dy) * C::LX + dx) * C::VS;
                                const f32x4* wt = wq + (size_t)((kz * KS + ky) * KS + kx) * C::Q;
#pragma unroll
                                for (int q = 0; q < C::Q; ++q) {
                                    const f32x4 x = *reinterpret_cast<const f32x4*>(lp + q * 4);
                                    const f32x4 w = wt[q];
                                    s = fmaf(x.x, w.x, s); s = fmaf(x.y, w.y, s); s = fmaf(x.z, w.z, s); s = fmaf(x.w, w.w, s);
                                }
                            }
                    if (inb_ok) finish(s, (((size_t)n * a.OD + 2 * gz + pz) * a.OH + 2 * gy + py) * a.OW + 2 * gx + px);
                }
    }
}

// =====================================================================================================
// Conv3DTranspose 16 -> 1, k3, stride 1 (last layer of the V2 synthesis transforms) on the matrix cores.
//   A GEMV-shaped layer has no N dimension for an implicit GEMM, so the contraction is split:
//     (1) P[tap][voxel] = sum_c w[tap][c] * in[voxel][c]      -- MFMA: M = 27 taps (2 tiles), N = 16 voxels,
//         K = 16 channels; every input voxel is read ONCE from global memory (coalesced 1 KiB per wave load);
//     (2) out[z,y,x] = sum_tap P[tap][voxel + offset(tap)]      -- 27 LDS reads + adds per output voxel.
//   A workgroup owns a T x T (y,x) column block of one image (and, with a z split, a slab of it) and marches along z: input
//   plane p feeds the three output planes p-1, p, p+1 through rolling accumulators.  T = 32 (round 3, when the grid still fills
//   the CUs): the haloed plane is 34^2 = 1156 voxels for 1024 outputs instead of 18^2 = 324 for 256 -- 13 % halo instead of 27 %
//   in both the MFMA work (which costs this layer as much time as its HBM floor) and the input reads.
//   Summation order per output: channels (MFMA chain) -> (ky,kx) -> kz, fixed => deterministic.
// =====================================================================================================
template <int T>
struct Cout1M {
    static constexpr int TYX = T, NT = T * T, NW = NT / 64;   // T = 16: 4 waves, 2-3 workgroups per CU; T = 32: 16 waves, one workgroup per CU
    static constexpr int LYX = TYX + 2;                 // haloed plane edge
    static constexpr int NTILE = (LYX * LYX + 15) / 16; // N-tiles of 16 voxels: 21 (324 voxels) / 73 (1156)
    static constexpr int NU = NTILE * 16;
    static constexpr int RS = NU + 20;                  // row pitch of P in floats: 4 * RS = 16 (mod 32) -> the four channel quads of a
                                                        // ds_write_b32 fall on two bank halves (2 cycles, the minimum for 64 lanes) instead of one;
                                                        // columns [NU + 4, NU + 20) of a row take the writes of the N-tiles past the plane (the last,
                                                        // partial round of tiles): every wave writes every round, no branch in the MFMA stream
    static_assert((4 * RS) % 32 == 16, "row pitch");
    static constexpr int LDS_BYTES = 32 * RS * 4;       // 32 tap rows: 27 + the zero rows of the second M tile (45.5 KB / 148.5 KB)
    static constexpr int PER_WAVE = (NTILE + NW - 1) / NW;    // N-tiles per wave (6,5,5,5 / 5 x9, 4 x7)
};

// IN16 (fp16 mode, PCC_CONV_IN16): the input is fp16 NDHWC; a lane's 4 channels are one 8-byte load and feed ONE
// v_mfma_f32_16x16x16_f16 per tap tile instead of four fp32 MFMAs.
// THR (pcc_thr_fuse, fixed-threshold extraction): the epilogue also decides occupancy -- (clipped) x_hat > thr[n], the float32
// compare of model_types.py:202,209 / :232-234 -- and stores it as one bit per voxel in (z,y,x) order: a wave's ballot is T-bit
// pieces of 64 / T output rows, each written once by its row's first lane.  The compaction pass then reads 32 KB per 64^3 block
// instead of x_hat twice.
template <bool IN16, int T, bool THR>
__global__ void __launch_bounds__((Cout1M<T>::NT)) conv_cout1_mfma_kernel(ConvArgs a) {
    using C = Cout1M<T>;
    extern __shared__ __attribute__((aligned(16))) float P[];   // [32][RS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % a.ntx; t /= a.ntx;
    const int ty = t % a.nty; t /= a.nty;
    const int zs = t % a.ntz;                          // z slab [zb, ze) of output planes
    const int n = t / a.ntz;
    const int y0 = ty * C::TYX, x0 = tx * C::TYX;
    const int zlen = (a.D + a.ntz - 1) / a.ntz, zb = zs * zlen, ze = min(zb + zlen, a.D);
    const int p0 = max(zb - 1, 0), p1 = min(ze, a.D - 1);     // input planes of this slab

    // A operand: w[tap = 16*mt + (lane & 15)][channel 4*(lane>>4) + j], taps >= 27 are zero rows
    const f32x4 wA0 = *reinterpret_cast<const f32x4*>(a.w + (0 * 64 + lane) * 4);
    const f32x4 wA1 = *reinterpret_cast<const f32x4*>(a.w + (1 * 64 + lane) * 4);

    // this lane's voxels (one per N-tile it serves): byte offset inside a plane, sign bit set when outside H x W
    unsigned voff[C::PER_WAVE];
    int uidx[C::PER_WAVE];
#pragma unroll
    for (int k = 0; k < C::PER_WAVE; ++k) {
        const int nt = wave + C::NW * k;
        const int u = nt * 16 + v;
        const int ly = u / C::LYX, lx = u - ly * C::LYX;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        const bool ok = nt < C::NTILE && u < C::LYX * C::LYX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        voff[k] = ok ? (unsigned)((gy * a.W + gx) * 16 + cq * 4) * (IN16 ? 2u : 4u) : kOOB;
        uidx[k] = nt < C::NTILE ? u : C::NU + 4 + v;
    }
    const unsigned plane_bytes = (unsigned)a.H * a.W * (IN16 ? 32u : 64u);
    const unsigned char* inb = (const unsigned char*)a.in + (size_t)n * a.D * plane_bytes;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(inb, (unsigned)a.D * plane_bytes);
    // fp16 input arrives as 4 halfs in the low half of the float4 slot (bit pattern), converted weights beside it
    const f16x4 wA0h = __builtin_convertvector(wA0, f16x4), wA1h = __builtin_convertvector(wA1, f16x4);
    auto load_in = [&](unsigned voff_, unsigned soff) -> f32x4 {
        if constexpr (IN16) {
            const u32x2 r = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rin, (int)voff_, (int)soff, 0));
            return __builtin_bit_cast(f32x4, (u32x4){r[0], r[1], 0u, 0u});
        } else {
            return buf_load4(rin, voff_, soff);
        }
    };

    // gather side: thread -> output column (y, x)
    const int oy = tid / C::TYX, ox = tid % C::TYX;
    const bool col_ok = (y0 + oy) < a.OH && (x0 + ox) < a.OW;
    const float* pcol = P + oy * C::LYX + ox;
    const float bias = (a.flags & PCC_CONV_BIAS) ? a.bias[0] : 0.f;
    const size_t out_plane = (size_t)a.OH * a.OW;
    float* ob = a.out + ((size_t)n * a.OD * out_plane + (size_t)(y0 + oy) * a.OW + x0 + ox) * a.ocs + a.oco;
    // (a column past H x W has no residual either: on the last plane of the last image its row would lie behind the end of the tensor)
    const float* rb = ((a.flags & PCC_CONV_ADD) && col_ok) ? a.res + (size_t)n * a.OD * out_plane + (size_t)(y0 + oy) * a.OW + x0 + ox : nullptr;

    float thr_n = 0.f;
    unsigned short* mrow = nullptr;        // this lane's row of the bit mask (meaningful on the first lane of each T-lane group)
    if constexpr (THR) {
        thr_n = a.thr[n];
        mrow = a.mask + ((size_t)n * a.OD * out_plane + (size_t)(y0 + oy) * a.OW + x0) / 16;
    }

    auto finish = [&](float s, int z) {
        s += bias;
        if (a.flags & PCC_CONV_RELU) s = fmaxf(s, 0.f);
        if (rb) s += rb[(size_t)z * out_plane];
        if (a.flags & PCC_CONV_CLIP01) s = fminf(fmaxf(s, 0.f), 1.f);
        if (col_ok) ob[(size_t)z * out_plane * a.ocs] = s;
        if constexpr (THR) {
            const float v = a.thr_clip ? fminf(fmaxf(s, 0.f), 1.f) : s;
            const unsigned long long hits = __ballot(col_ok && v > thr_n);
            if ((lane & (T - 1)) == 0 && (y0 + oy) < a.OH) {
                const unsigned piece = (unsigned)(hits >> (lane & 63 & ~(T - 1)));
                unsigned short* mp = mrow + (size_t)z * out_plane / 16;
                if constexpr (T == 32) *reinterpret_cast<unsigned*>(mp) = piece;
                else *mp = (unsigned short)piece;
            }
        }
    };

#ifndef PCC_C1_PROBE
#define PCC_C1_PROBE 0      // timing probes (tools/build_variant.sh): 1 no P writes, 2 no gather reads, 4 no MFMA, 8 no barriers, 16 no plane loads
#endif
    // ---- (1) P[tap][voxel] = W x in, one N-tile (16 voxels) at a time: d0 = taps 0..15, d1 = taps 16..31 of tile k
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};      // first k-slot starts from the inline constant 0: no zero-init pass (VALU costs MFMA time)
    f32x4 x[C::PER_WAVE], d0[C::PER_WAVE], d1[C::PER_WAVE];
    auto taps = [&](auto k0_tag, auto k1_tag) __attribute__((always_inline)) {      // tiles [K0, K1)
        constexpr int K0 = decltype(k0_tag)::value, K1 = decltype(k1_tag)::value;
        if constexpr ((PCC_C1_PROBE & 4) != 0) {
#pragma unroll
            for (int k = K0; k < K1; ++k) { d0[k] = x[k]; d1[k] = x[k] * wA1; }
        } else if constexpr (IN16) {
#pragma unroll
            for (int k = K0; k < K1; ++k) {
                const u32x4 cb = __builtin_bit_cast(u32x4, x[k]);
                const f16x4 bh = __builtin_bit_cast(f16x4, (u32x2){cb[0], cb[1]});
                d0[k] = __builtin_amdgcn_mfma_f32_16x16x16f16(wA0h, bh, zero4, 0, 0, 0);
                d1[k] = __builtin_amdgcn_mfma_f32_16x16x16f16(wA1h, bh, zero4, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = K0; k < K1; ++k) {
                    d0[k] = mfma16(wA0[j], x[k][j], j == 0 ? zero4 : d0[k]);
                    d1[k] = mfma16(wA1[j], x[k][j], j == 0 ? zero4 : d1[k]);
                }
        }
    };
    auto fetch = [&](auto k0_tag, auto k1_tag, int plane) __attribute__((always_inline)) {
        constexpr int K0 = decltype(k0_tag)::value, K1 = decltype(k1_tag)::value;
        const unsigned soff = (unsigned)(((PCC_C1_PROBE & 16) != 0) ? p0 : min(plane, p1)) * plane_bytes;     // (clamped: a plane past the slab is loaded, never used)
#pragma unroll
        for (int k = K0; k < K1; ++k) x[k] = load_in(voff[k], soff);
    };
    // all 32 tap rows are written (rows 27..31 are never read), tiles past the plane go to the pad columns: no branch around the ds_writes
    auto store = [&](auto k0_tag, auto k1_tag) __attribute__((always_inline)) {
        constexpr int K0 = decltype(k0_tag)::value, K1 = decltype(k1_tag)::value;
#pragma unroll
        for (int k = K0; k < K1; ++k) {
            if constexpr ((PCC_C1_PROBE & 1) != 0) { if (d0[k][0] == 1.2345f && d1[k][1] == 5.4321f) P[uidx[k]] = d0[k][2]; continue; }
            float* pw = P + uidx[k] + 4 * cq * C::RS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pw[r * C::RS] = d0[k][r];
                pw[(16 + r) * C::RS] = d1[k][r];
            }
        }
    };
    // ---- (2) gather: the plane in P is tap kz = 0 of output p+1, kz = 1 of output p, kz = 2 of output p-1
    float accA = 0.f, accB = 0.f, accC = 0.f;   // outputs z = p+1, p, p-1
    auto gather = [&]() __attribute__((always_inline)) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float* q = pcol + ky * C::LYX + kx;
                if constexpr ((PCC_C1_PROBE & 2) != 0) { if (ky + kx > 0) continue; }
                s0 += q[(0 * 9 + ky * 3 + kx) * C::RS];
                s1 += q[(1 * 9 + ky * 3 + kx) * C::RS];
                s2 += q[(2 * 9 + ky * 3 + kx) * C::RS];
            }
        accA += s0; accB += s1; accC += s2;
    };
    auto sync = [&]() __attribute__((always_inline)) { if constexpr ((PCC_C1_PROBE & 8) == 0) __syncthreads(); };

    // Software pipeline (round 3; round 2 ran load -> MFMA -> LDS write -> barrier -> gather -> barrier strictly in turn, with the
    // matrix pipe idle 45 % of the time).  The N-tiles of a wave are split into a front group [0, KB) and a back group [KB, PER_WAVE).
    // At the top of iteration q:  P = tap planes of plane q;  d[front] = tap planes of plane q+1 (in flight);  d[back] = stale
    // (plane q, already in P);  x[back] = inputs of plane q+1;  x[front] = inputs of plane q+2 (loads in flight).
    //   phase A:  back-group MFMAs of plane q+1  ||  the 27 LDS reads of the gather of plane q;  finish(q-1);  refill x[back]
    //   barrier   (every wave has read P)
    //   phase B:  per front tile: write its plane-(q+1) rows, then its MFMAs of plane q+2 into the same registers;  refill x[front];
    //             the back group's rows are written between those MFMAs
    //   barrier   (P = plane q+1)
    // so the matrix pipe always has work while LDS is read or written, and every input tile is loaded one iteration before use.
    constexpr int KB = C::PER_WAVE - 2;
    using I0 = std::integral_constant<int, 0>;
    using IB = std::integral_constant<int, KB>;
    using IE = std::integral_constant<int, C::PER_WAVE>;
    fetch(I0{}, IE{}, p0);
    taps(I0{}, IE{});
    store(I0{}, IE{});
    fetch(I0{}, IB{}, p0 + 1);
    sync();
    taps(I0{}, IB{});
    fetch(I0{}, IB{}, p0 + 2);
    fetch(IB{}, IE{}, p0 + 1);
#pragma unroll 1
    for (int q = p0; q < p1; ++q) {
        // ---- phase A
        taps(IB{}, IE{});
        gather();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // 2 DS reads
        }
        fetch(IB{}, IE{}, q + 2);
        if (q - 1 >= zb) finish(accC, q - 1);          // (q - 1 < ze always: q <= ze)
        accC = accB; accB = accA; accA = 0.f;
        sync();
        // ---- phase B
        store(I0{}, IB{});
        taps(I0{}, IB{});
        store(IB{}, IE{});
        if constexpr (!IN16 && (PCC_C1_PROBE & 5) == 0) {
            // a front tile's 8 row writes go out before its first MFMA pair overwrites the registers; the remaining MFMAs carry the back rows
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x200, 8, 0);  // 8 DS writes
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMA (j = 0 of tile k)
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            }
        }
        fetch(I0{}, IB{}, q + 3);
        sync();
    }
    gather();                                          // plane p1
    if (p1 - 1 >= zb) finish(accC, p1 - 1);
    accC = accB; accB = accA; accA = 0.f;
    if (ze == a.D) finish(accC, a.D - 1);              // the last plane of the volume has no plane behind it
}

}  // namespace pccmfma

using namespace pccmfma;

int pcc_conv_cin1(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                  float* out, pcc_conv_ext* ext, hipStream_t st) {
    ConvArgs a = conv_args(d, in, w_packed, bias, residual, out);
    const int co = d->Cout, k = d->k;
#define PCC_CIN1(CO, K, TZ, TY, R)                                                                      \
    if (co == CO && k == K) {                                                                           \
        using C = Cin1Cfg<CO, K, TZ, TY, R>;                                                            \
        if (ext && ext->out_amax && !(d->flags & PCC_CONV_OUT16)) { a.amax_out = ext->out_amax; ext->out_recorded = true; } \
        a.ntz = cdiv(a.OD, TZ); a.nty = cdiv(a.OH, TY); a.ntx = cdiv(a.OW, 16);                         \
        return launch(conv_cin1_kernel<CO, K, TZ, TY, R>, C::NT, C::LDS_BYTES, a.N * a.ntz * a.nty * a.ntx, a, st); \
    }
    PCC_CIN1(16, 3, 2, 8, 4) PCC_CIN1(32, 3, 2, 8, 4) PCC_CIN1(16, 9, 2, 8, 4) PCC_CIN1(32, 9, 2, 8, 4)
#undef PCC_CIN1
    return no_instantiation(d);
}

int pcc_conv_cout1_mfma(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias,
                        const float* residual, float* out, const pcc_thr_fuse* fuse, bool* fused, hipStream_t st) {
    ConvArgs a = conv_args(d, in, w_packed, bias, residual, out);
    // 32 x 32 columns (one 16-wave workgroup per CU) when H, W allow it and the grid, z-split into slabs of >= 16 planes, still
    // gives every CU a workgroup; else 16 x 16 columns, whole z range.  PCC_COUT1_T16=1 forces the latter (A/B runs).
    const bool t16 = ctx->num(PCC_NUM_COUT1_T16);
    typedef void (*kern_t)(ConvArgs);
    const bool in16 = (d->flags & PCC_CONV_IN16) != 0;
    // the kernel reads `residual` as fp32 whatever the input type, and pcc_conv3d lets an fp16-input layer have an fp16 residual only
    PCC_REQUIRE(!(in16 && (d->flags & PCC_CONV_ADD)), "pcc_conv3d: the 16 -> 1 layer with fp16 input (PCC_CONV_IN16) takes no residual");
    // the occupancy bits ride along when the caller asked for them and whole T-voxel rows map to whole mask pieces
    const bool thr = fuse != nullptr && a.ocs == 1 && a.oco == 0 && a.W % 16 == 0 && ((size_t)a.H * a.W) % 32 == 0;
    if (thr) { a.thr = fuse->thr; a.mask = (unsigned short*)fuse->mask; a.thr_clip = fuse->clip; }
    if (fused) *fused = thr;
    if (!t16 && a.H % 32 == 0 && a.W % 32 == 0) {
        const int base = a.N * (a.H / 32) * (a.W / 32);
        int zsp = 1;
        while (base * zsp < ctx->num_cu && a.D / (zsp * 2) >= 16) zsp *= 2;
        if (base * zsp >= ctx->num_cu) {
            using C = Cout1M<32>;
            a.ntz = zsp; a.nty = a.H / 32; a.ntx = a.W / 32;
            static const kern_t k32[4] = {conv_cout1_mfma_kernel<false, 32, false>, conv_cout1_mfma_kernel<true, 32, false>,
                                          conv_cout1_mfma_kernel<false, 32, true>, conv_cout1_mfma_kernel<true, 32, true>};
            return launch(k32[(in16 ? 1 : 0) + (thr ? 2 : 0)], C::NT, C::LDS_BYTES, base * zsp, a, st);
        }
    }
    using C = Cout1M<16>;
    a.ntz = 1; a.nty = cdiv(a.H, C::TYX); a.ntx = cdiv(a.W, C::TYX);
    static const kern_t k16[4] = {conv_cout1_mfma_kernel<false, 16, false>, conv_cout1_mfma_kernel<true, 16, false>,
                                  conv_cout1_mfma_kernel<false, 16, true>, conv_cout1_mfma_kernel<true, 16, true>};
    return launch(k16[(in16 ? 1 : 0) + (thr ? 2 : 0)], C::NT, C::LDS_BYTES, a.N * a.nty * a.ntx, a, st);
}

int pcc_conv_cout1(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                   float* out, hipStream_t st) {
    ConvArgs a = conv_args(d, in, w_packed, bias, residual, out);
    const int ci = d->Cin, k = d->k, s = d->stride;
#define PCC_COUT1(CI, K, S, TZ, TY, TXT)                                                                \
    if (ci == CI && k == K && s == S) {                                                                 \
        using C = Cout1Cfg<CI, K, S, TZ, TY, TXT>;                                                      \
        a.ntz = cdiv(a.D, TZ); a.nty = cdiv(a.H, TY); a.ntx = cdiv(a.W, TXT);                           \
        return launch(conv_cout1_kernel<CI, K, S, TZ, TY, TXT>, C::NT, C::LDS_BYTES, a.N * a.ntz * a.nty * a.ntx, a, st); \
    }
    PCC_COUT1(16, 3, 1, 4, 8, 8) PCC_COUT1(32, 3, 1, 4, 8, 8) PCC_COUT1(32, 9, 2, 2, 8, 8)
#undef PCC_COUT1
    return no_instantiation(d);
}
