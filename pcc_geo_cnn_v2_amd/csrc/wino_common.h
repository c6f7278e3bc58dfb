// Shared pieces of the Winograd F(2x2,3x3)+z kernels (conv_wino.hip: exact-fp32 MFMA; conv_wino_bf16.hip: split-bf16 MFMA;
// conv_wino_f16s.hip: two-piece fp16 MFMA): the LDS plane geometry, the launch arguments, the fp32 input / output transforms and
// the micro-step modes of the z march.
#pragma once
#include <cstdlib>

#include "common.h"
#include "kernel_common.h"

namespace pccwino {

using namespace pcck;

constexpr int NT = 256;
constexpr int PLANE_VOX = 18 * 18;
constexpr int PLANE_ITEMS = PLANE_VOX * 4;             // float4 slots per plane (1296)
constexpr int CHUNKS = (PLANE_ITEMS + 63) / 64;        // 21 wave-sized (1 KB) chunks; the last one is padding beyond slot 1295
constexpr int PLANE_BYTES = CHUNKS * 1024;             // 21504: three planes end below 64 KB -> every plane offset is a DS immediate
constexpr int U_BASE = 3 * PLANE_BYTES;
constexpr int U_BYTES = 48 * 1024;                     // 3 z taps x 16 points x 64 lanes x float4
constexpr int LDS_BYTES = U_BASE + U_BYTES;            // 113664
constexpr int LDS_BYTES_CIN = U_BASE + 2 * U_BYTES;    // 162816 <= 160 KB (conv16_wino_cin_kernel): tile ring + two U buffers
constexpr int ITEMS = 6;                               // chunks per wave: wave w stages chunks 5w .. 5w+5 (5, 10, 15 twice: same data)

struct WinoArgs {
    const float* in;
    const float* u;     // packed transformed weights of this cin group: [cout group][48][64][4]
    const float* bias;
    const float* res;
    float* out;
    int N, D, H, W;
    int nty, ntx, zsplit, zlen;
    int nco;            // cout groups of 16 handled by this launch (grid dimension)
    int flags, ocs, oco;
    int ics, ico;       // input channel stride / offset of this launch's 16-channel cin group
    int rcs;            // residual channel stride (its channel offset follows the cout group)
    int ncig;           // cin groups processed by one launch of conv16_wino_cin_kernel (u: [cin group][cout group][48][64][4])
    // fp16-split kernels (conv_wino_f16s.hip): per-block max |x| of the input (fp32 bit patterns, one per block n) that fixes the block's
    // power-of-two pre-scale; where to record the same for the output (nullptr: not recorded); the weight image's scale (device, 1 float)
    const unsigned* amax_in = nullptr;
    unsigned* amax_out = nullptr;
    const float* utail = nullptr;
    int ig0 = 0;        // first cin group this launch marches (the 64-channel layers run as two launches of two groups)
};

// Measured on MI355X (tools/ubench/mfma_valu.hip): a wave's VALU instructions do NOT overlap with its own fp32 MFMAs
// (v_mfma_f32_16x16x4_f32 runs at the packed-FMA rate of the same SIMD): every VALU op costs ~5 cycles of MFMA time,
// v_mov / v_accvgpr_read ~8.  Hence: packed adds everywhere (the compiler turns a-b into two scalar v_sub), no
// register copies, no per-lane address arithmetic in the loop.
__device__ __forceinline__ f32x4 sub4(const f32x4& a, const f32x4& b) {
    f32x2 lo, hi;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(__builtin_shufflevector(a, a, 0, 1)), "v"(__builtin_shufflevector(b, b, 0, 1)));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(__builtin_shufflevector(a, a, 2, 3)), "v"(__builtin_shufflevector(b, b, 2, 3)));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
__device__ __forceinline__ f32x4 add4(const f32x4& a, const f32x4& b) {
    f32x2 lo, hi;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(__builtin_shufflevector(a, a, 0, 1)), "v"(__builtin_shufflevector(b, b, 0, 1)));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(__builtin_shufflevector(a, a, 2, 3)), "v"(__builtin_shufflevector(b, b, 2, 3)));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

// B^T along x, in place, on a 4x4 array of float4 (4 input channels each)
__device__ __forceinline__ void transform_x_rows(f32x4 (&P)[16], int y0, int y1) {
#pragma unroll
    for (int y = y0; y < y1; ++y) {
        const f32x4 d0 = P[y * 4 + 0], d1 = P[y * 4 + 1], d2 = P[y * 4 + 2], d3 = P[y * 4 + 3];
        P[y * 4 + 0] = sub4(d0, d2); P[y * 4 + 1] = add4(d1, d2); P[y * 4 + 2] = sub4(d2, d1); P[y * 4 + 3] = sub4(d1, d3);
    }
}
// B^T along y, one output row: V[r][x] from the x-transformed patch
__device__ __forceinline__ void transform_y_row(f32x4 (&V)[16], const f32x4 (&P)[16], int r) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        if (r == 0) V[x] = sub4(P[x], P[8 + x]);
        else if (r == 1) V[4 + x] = add4(P[4 + x], P[8 + x]);
        else if (r == 2) V[8 + x] = sub4(P[8 + x], P[4 + x]);
        else V[12 + x] = sub4(P[4 + x], P[12 + x]);
    }
}

// Micro-step modes of the z march: which of the 12 MFMA rows (dz = 2, 1, 0 x 4 point rows) a step runs.
//   M_ALL  every interior step
//   M_S0   step 0 (plane zb - 1 of a slab inside the volume): only its dz = 0 rows feed an output plane of this slab
//   M_S1   step 1 behind M_S0: its dz = 2 rows would finish output plane zb - 1, which belongs to the slab below
//   M_S1O  step 1 of a slab that starts at z = 0 (step 0 skipped): as M_S1, and its dz = 1 rows OPEN their accumulators
//   M_FIN  last step of a slab that ends at z = D: no matrix work, only the reduction + store of output plane D - 1
enum { M_ALL = 0, M_S0 = 1, M_S1 = 2, M_S1O = 3, M_FIN = 4 };
__host__ __device__ constexpr bool row_active(int mode, int dz) {
    return mode == M_ALL || (mode == M_S0 && dz == 0) || ((mode == M_S1 || mode == M_S1O) && dz <= 1);
}
__host__ __device__ constexpr int next_mode(int mode) { return mode == M_S0 ? M_S1 : M_ALL; }
// Slots q = 0..11 in py-major order (py = q / 3, dz = 2 - q % 3; conv_wino_bf16.hip, conv_wino_f16s.hip): the first active slot q' > q
// of this step, or 12 + the first active slot of the next step
__host__ __device__ constexpr int next_slot(int mode, int q) {
    for (int n = q + 1; n < 12; ++n)
        if (row_active(mode, 2 - n % 3)) return n;
    for (int n = 0; n < 12; ++n)
        if (row_active(next_mode(mode), 2 - n % 3)) return 12 + n;
    return 12;
}
__host__ __device__ constexpr int first_slot(int mode) {
    for (int n = 0; n < 12; ++n)
        if (row_active(mode, 2 - n % 3)) return n;
    return 0;
}

}  // namespace pccwino
