// Shared skeleton of the Winograd F(2x2,3x3)+z kernels (conv_wino.hip: exact-fp32 MFMA, one cin group per march and the cin groups
// inside the march; conv_wino_bf16.hip: split-bf16 MFMA; conv_wino_f16s.hip: two-piece fp16 MFMA): the LDS plane geometry, the launch
// arguments and their host fill, the z split, the launch, the workgroup's place in the grid, the fp32 input / output transforms, the
// epilogue of an output voxel and the micro-step modes of the z march with their tags.  Each kernel keeps what is its own: the MFMA
// schedule, the operand split, its LDS reads and its U layout.
//
// WHERE A FUNCTION BOUNDARY MAY FALL.  As in tr2m_common.h: these kernels hold 192 AccVGPRs live and the register allocation follows
// the order of allocas and basic blocks that inlining leaves behind.  Every device piece here was lifted on its own and the gfx950
// instruction stream compared with the copies it replaced: identical in all 25 kernels of the three sources
// (profiles/wino_skeleton_isa.md).  The probe macros of the split kernels (PCC_WB_PROBE, PCC_WH_PROBE) gate at the call site; nothing
// here takes one.  What did NOT come out identical stays written out in each kernel on purpose:
//   * the THREE-PHASE DRIVER (head planes, loop over s mod 3, M_FIN dispatch) as a function template over the step callable, by
//     reference or by value: conv16_wino_bf16_kernel spills 26 VGPRs / 108 B scratch in all four instantiations instead of 4 - 16 /
//     20 - 68 B; conv16_wino_kernel 208 -> 204 AccVGPRs, +10 .. +17 instructions; conv16_wino_f16s_kernel<., ., 1> 76 -> 77 SGPRs,
//     +5 .. +7 instructions (its G = 2 instantiations came out identical);
//   * the STAGING INDICES rel[] of both plane layouts as a function: register counts equal, +17 .. +24 instructions per kernel (the
//     blocks of the inlined bounds test land elsewhere relative to the U copy in front of them);
//   * the EPILOGUE ADDRESSES (ovo / rvo, ovo0 / rvo0 / oso / rso) and the PATCH ADDRESSES (ra[16], pa0) as functions: register counts
//     equal, -2 .. +2 instructions and 100 - 19 000 lines of another register assignment per file (cin <false, 4>: -27 instructions);
//   * in conv16_wino_kernel only, reduce_at_row and keep_store_data: its <., false, false> instantiations take another scalar register
//     assignment (counts equal, -1 instruction in one), so that kernel keeps both written out; the other three kernels call them.
// None of these was timed; the test of this header is the identical stream.  Do not "finish the job" without comparing the streams again.
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

// One layout for all four kernels (the kernarg offsets are part of the recorded instruction streams).
struct WinoArgs {
    const float* in;
    // the packed weight image, per kernel:
    //   conv16_wino_kernel       fp32 U of THIS launch's cin group: [cout group][48 rows (dz, py, px)][64 lanes][4]
    //   conv16_wino_cin_kernel   fp32 U of the layer: [cin group][cout group][48][64][4]
    //   conv16_wino_bf16_kernel  three bf16 pieces: [cout group][slot q][px][operand [Uh | Um], [Ul | Uh]][64 lanes][8 bf16]
    //   conv16_wino_f16s_kernel  two fp16 pieces, lane-contiguous: [cout group][cin group][64 lanes][776 B]; its scale: utail
    const float* u;
    const float* bias;
    const float* res;
    float* out;
    int N, D, H, W;
    int nty, ntx, zsplit, zlen;
    int nco;            // cout groups of 16 handled by this launch (grid dimension)
    int flags, ocs, oco;
    int ics, ico;       // input channel stride / offset of the first 16-channel cin group this launch reads
    int rcs;            // residual channel stride (its channel offset follows the cout group)
    // cin groups: conv16_wino_cin_kernel: marched by this launch (its template G); conv16_wino_f16s_kernel: of the LAYER (the stride of
    // its image; the launch marches its template G of them from ig0 on); the one-group kernels do not read it (1)
    int ncig;
    // fp16-split kernels (conv_wino_f16s.hip): per-block max |x| of the input (fp32 bit patterns, one per block n) that fixes the block's
    // power-of-two pre-scale; where to record the same for the output (nullptr: not recorded); the weight image's scale (device, 1 float)
    const unsigned* amax_in = nullptr;
    unsigned* amax_out = nullptr;
    const float* utail = nullptr;
    int ig0 = 0;        // conv16_wino_f16s_kernel: first cin group this launch marches (the 64-channel layers run as two launches of two)
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

// The workgroup's place in the grid: cout group fastest (neighbours in the grid share their input planes in L2), then x tile, y tile,
// z slab, block.
struct WinoTile { int cog, n, X0, Y0, zb; };
__device__ __forceinline__ WinoTile wino_tile(const WinoArgs& a, int nwg) {
    int wg = xcd_remap(blockIdx.x, nwg);
    const int cog = wg % a.nco; wg /= a.nco;
    const int tx = wg % a.ntx; wg /= a.ntx;
    const int ty = wg % a.nty; wg /= a.nty;
    const int zs = wg % a.zsplit;
    return WinoTile{cog, wg / a.zsplit, tx * 16, ty * 16, zs * a.zlen};
}

// Padded plane layout (conv_wino_bf16.hip, conv_wino_f16s.hip, which describe it): byte offset of patch voxel (dy, dx) from the
// lane's patch (0, 0) -- compile-time constants that fold into the DS offset field
__host__ __device__ constexpr int patch_off_padded(int dy, int dx) { return 64 * (18 * dy + 9 * (dx & 1) + (dx >> 1)) + (dy >= 2 ? 32 : 0); }

// compile-time tags of the schedules: V / patch row, split stage, accumulator phase (s mod 3)
using R0 = std::integral_constant<int, 0>;
using R1 = std::integral_constant<int, 1>;
using R2 = std::integral_constant<int, 2>;
using R3 = std::integral_constant<int, 3>;
using ST0 = std::integral_constant<int, 0>;
using ST1 = std::integral_constant<int, 1>;
using ST2 = std::integral_constant<int, 2>;
using PH0 = std::integral_constant<int, 0>;
using PH1 = std::integral_constant<int, 1>;
using PH2 = std::integral_constant<int, 2>;

// B^T along x, in place, on a 4x4 array of float4 (4 input channels each)
__device__ __forceinline__ void transform_x_rows(f32x4 (&P)[16], int y0, int y1) {
#pragma unroll
    for (int y = y0; y < y1; ++y) {
        const f32x4 d0 = P[y * 4 + 0], d1 = P[y * 4 + 1], d2 = P[y * 4 + 2], d3 = P[y * 4 + 3];
        P[y * 4 + 0] = sub4(d0, d2); P[y * 4 + 1] = add4(d1, d2); P[y * 4 + 2] = sub4(d2, d1); P[y * 4 + 3] = sub4(d1, d3);
    }
}
// the same on one patch row (4 voxels x 4 channels)
__device__ __forceinline__ void transform_x_row(f32x4 (&P)[4]) {
    const f32x4 d0 = P[0], d1 = P[1], d2 = P[2], d3 = P[3];
    P[0] = sub4(d0, d2); P[1] = add4(d1, d2); P[2] = sub4(d2, d1); P[3] = sub4(d1, d3);
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
// the same from four separate patch rows into the fp32 row Y on its way through the operand split: (point x, channel c) at 4x + c
template <int r>
__device__ __forceinline__ void transform_y_row_split(float (&Y)[16], const f32x4 (&P0)[4], const f32x4 (&P1)[4], const f32x4 (&P2)[4], const f32x4 (&P3)[4]) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const f32x4 y = r == 0 ? sub4(P0[x], P2[x]) : r == 1 ? add4(P1[x], P2[x]) : r == 2 ? sub4(P2[x], P1[x]) : sub4(P1[x], P3[x]);
        Y[4 * x + 0] = y[0]; Y[4 * x + 1] = y[1]; Y[4 * x + 2] = y[2]; Y[4 * x + 3] = y[3];
    }
}

// A^T along x on row r of the finished plane (its four points m0..m3), accumulated along y into the 2 x 2 outputs S
__device__ __forceinline__ void reduce_at_row(f32x4 (&S)[2][2], int r, const f32x4& m0, const f32x4& m1, const f32x4& m2, const f32x4& m3) {
    const f32x4 r0 = add4(add4(m0, m1), m2), r1 = sub4(sub4(m1, m2), m3);
    if (r == 0) { S[0][0] = r0; S[0][1] = r1; }
    else if (r == 1) { S[0][0] = add4(S[0][0], r0); S[0][1] = add4(S[0][1], r1); S[1][0] = r0; S[1][1] = r1; }
    else if (r == 2) { S[0][0] = add4(S[0][0], r0); S[0][1] = add4(S[0][1], r1); S[1][0] = sub4(S[1][0], r0); S[1][1] = sub4(S[1][1], r1); }
    else { S[1][0] = sub4(S[1][0], r0); S[1][1] = sub4(S[1][1], r1); }
}

// Epilogue of one output voxel: (PRE: + the partial sums `prev` of the cin groups an earlier launch marched,) ReLU, residual, clip;
// the bias is already inside (it rides in the accumulator of point (1,1)).  addu(o, x) = o + x, un-scaling o where the kernel
// computes under a scale (conv_wino_f16s.hip: one packed fma); it is applied once, to the first thing added.  `resv` holds zeros without
// PCC_CONV_ADD (zero-sized buffer).
template <bool RELU, bool CLIP, bool PRE, class ADDU>
__device__ __forceinline__ f32x4 epilogue_voxel(f32x4 o, const f32x4& prev, const f32x4& resv, ADDU&& addu) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (PRE) o = addu(o, prev);
    // one v_maximum3_f32 per element: fmaxf on the result of the inline-asm packed add costs a second v_max (NaN quieting)
    if (RELU) o = __builtin_elementwise_maximum(o, zero4);
    o = PRE ? add4(o, resv) : addu(o, resv);
    if (CLIP) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = fminf(fmaxf(o[c], 0.f), 1.f);
    }
    return o;
}
template <bool RELU, bool CLIP, bool PRE>
__device__ __forceinline__ f32x4 epilogue_voxel(const f32x4& o, const f32x4& prev, const f32x4& resv) {
    return epilogue_voxel<RELU, CLIP, PRE>(o, prev, resv, [](const f32x4& x, const f32x4& y) __attribute__((always_inline)) { return add4(x, y); });
}
// gfx950: a buffer_store_dwordx4 reads its data registers late; a VALU write to them in the next issue slots corrupts the last dword
// of the last lanes (seen as out[q].w <- out[q+1].w).  The compiler only guards the immediate-soffset form with one wait state, so the
// data registers of output row oy are kept live (and therefore unwritten) for one more slot: called in the slot behind its stores.
__device__ __forceinline__ void keep_store_data(const f32x4 (&ost)[4], int oy) {
    asm volatile("" ::"v"(ost[2 * oy]));
    asm volatile("" ::"v"(ost[2 * oy + 1]));
}

// Micro-step modes of the z march: which of the 12 MFMA rows (dz = 2, 1, 0 x 4 point rows) a step runs.
//   M_ALL  every interior step
//   M_S0   step 0 (plane zb - 1 of a slab inside the volume): only its dz = 0 rows feed an output plane of this slab
//   M_S1   step 1 behind M_S0: its dz = 2 rows would finish output plane zb - 1, which belongs to the slab below
//   M_S1O  step 1 of a slab that starts at z = 0 (step 0 skipped): as M_S1, and its dz = 1 rows OPEN their accumulators
//   M_FIN  last step of a slab that ends at z = D: no matrix work, only the reduction + store of output plane D - 1
//   M_TAIL last step of a slab that ends inside the volume (plane zb + zlen), where a kernel peels it (conv16_wino_cin_kernel): only
//          its dz = 2 rows feed this slab (output plane zb + zlen - 1); the other kernels run that step as M_ALL
enum { M_ALL = 0, M_S0 = 1, M_S1 = 2, M_S1O = 3, M_FIN = 4, M_TAIL = 5 };
using MAll = std::integral_constant<int, M_ALL>;
using MS0 = std::integral_constant<int, M_S0>;
using MS1 = std::integral_constant<int, M_S1>;
using MS1O = std::integral_constant<int, M_S1O>;
using MFin = std::integral_constant<int, M_FIN>;
using MTail = std::integral_constant<int, M_TAIL>;
__host__ __device__ constexpr bool row_active(int mode, int dz) {
    return mode == M_ALL || (mode == M_S0 && dz == 0) || ((mode == M_S1 || mode == M_S1O) && dz <= 1) || (mode == M_TAIL && dz == 2);
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
// Rows j = 0..11 in dz-major order (dz = 2 - j / 4, py = j % 4; conv_wino.hip): the first active row of a step
__host__ __device__ constexpr int first_row(int mode) { return 4 * (first_slot(mode) % 3); }

// ---- host

// The fp32 image's row (dz, py, px) = 16 dz + 4 py + px -> its place in the slot order of the split kernels' images: 4 q + px,
// q = 3 py + 2 - dz
constexpr int wino_row_slot(int row) { return (3 * ((row / 4) % 4) + 2 - row / 16) * 4 + row % 4; }

// z split: halve the slabs until every CU has a workgroup (`base` = workgroups of an unsplit launch), down to min_zlen planes per
// slab -- each split pays the U load and two halo planes
__host__ constexpr int wino_zsplit(int base, int D, int min_zlen, int num_cu) {
    int zs = 1;
    while (base * zs < num_cu && D % (zs * 2) == 0 && D / (zs * 2) >= min_zlen) zs *= 2;
    return zs;
}
// 256 CUs.  The bench launches (32 blocks): 64^3 x 16 ch, 32^3 x 32 ch: already 512 / 256 workgroups; 16^3 x 64 ch: 128 -> 256
static_assert(wino_zsplit(32 * 4 * 4 * 1, 64, 8, 256) == 1 && wino_zsplit(32 * 2 * 2 * 2, 32, 4, 256) == 1 && wino_zsplit(32 * 1 * 1 * 4, 16, 4, 256) == 2, "");
// 32 -> 32 @16^3 x 32: 256 workgroups of 4 planes (41 us; 128 of 8: 69 us); one block of 16^3: down to the shortest slab allowed
static_assert(wino_zsplit(32 * 1 * 1 * 2, 16, 4, 256) == 4 && wino_zsplit(1, 16, 8, 256) == 2 && wino_zsplit(2, 8, 4, 256) == 2 && wino_zsplit(1, 5, 4, 256) == 1, "");
// D not a power of two: 24 stops at 4 slabs of 6 planes, 12 at 2 of 6 (or not at all under min_zlen 8), 20 at 4 of 5
static_assert(wino_zsplit(1, 24, 4, 256) == 4 && wino_zsplit(1, 12, 4, 256) == 2 && wino_zsplit(1, 12, 8, 256) == 1 && wino_zsplit(1, 20, 4, 256) == 4, "");

// The arguments every launch shares, for a layer of NG = Cin / 16 cin groups whose launches each cover all NG cout groups; sets the z
// split (slabs of at least 8 planes, 4 for the multi-group layers: the 32 -> 32 case above).  Left to the launcher: u, and whatever of
// flags / ico / ncig / ig0 and the amax fields differs per launch.
inline WinoArgs wino_fill_args(const pcc_ctx* ctx, const pcc_conv_desc* d, int NG, const float* in, const float* bias, const float* residual, float* out) {
    WinoArgs a;
    a.in = in; a.bias = bias; a.res = residual; a.out = out;
    a.N = d->N; a.D = d->D; a.H = d->H; a.W = d->W;
    a.nty = d->H / 16; a.ntx = d->W / 16;
    a.ocs = d->out_cstride ? d->out_cstride : d->Cout;
    a.oco = d->out_coffset;
    a.nco = NG; a.ics = d->Cin; a.rcs = d->Cout; a.ico = 0; a.ncig = 1;
    a.flags = d->flags;
    a.zsplit = wino_zsplit(d->N * a.nty * a.ntx * NG, d->D, NG >= 2 ? 4 : 8, ctx->num_cu);
    a.zlen = d->D / a.zsplit;
    return a;
}
inline int wino_num_wg(const WinoArgs& a) { return a.N * a.nty * a.ntx * a.nco * a.zsplit; }
inline int wino_launch(void (*kern)(WinoArgs, int), int lds, int nwg, hipStream_t st, const WinoArgs& a) {
    { const int rc = pcc_enable_big_lds((const void*)kern, lds); if (rc != PCC_OK) return rc; }
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(NT), lds, st, a, nwg);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

}  // namespace pccwino
