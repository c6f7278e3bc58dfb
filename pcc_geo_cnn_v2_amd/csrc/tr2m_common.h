// Shared skeleton of the z-marching Conv3DTranspose k3 stride-2 kernels (conv_tr2m.hip: fp32; conv_tr2m_bf16.hip: split bf16;
// conv_tr2m_f16s.hip: two-piece fp16; conv_tr2m_f16.hip: the fp16 mode): the tile geometry, the tap order of a micro-step, the launch
// grid (struct, host fill, z split, launch), the workgroup's place in it, the address of the next tile to fetch, the epilogue schedule
// under the first taps, the drain and the shape rule.
//
// WHERE A FUNCTION BOUNDARY MAY FALL.  These kernels hold 192 AccVGPRs live, and what the register allocator and the scheduler make of
// them follows the order of allocas and basic blocks that inlining leaves behind.  Every device piece here was lifted on its own and the
// gfx950 instruction stream compared with the copies it replaced: identical in all 14 instantiations (profiles/tr2m_skeleton_isa.md).
// What did NOT come out identical stays in each kernel on purpose (fp32 kernels <2,f> / <2,t> / <4,f> / <4,t> unless said otherwise):
//   * the PLANE LOOP (halo plane, then pairs of compile-time parity) as a function template, lambdas by reference or by value:
//     388 / 392 / 440 / 436 VGPRs became 352 / 360 / 368 / 376 and 2 760 AccVGPR moves 2 080;
//   * the DRAIN with its `if (nsteps & 1)` inside the helper: <4,t> 436 -> 432 VGPRs, some 4 800 lines of assembly changed.  The branch
//     and keep[32] stay in the kernel; tr2m_drain<PH> is one side of it;
//   * the PREAMBLE (nsteps, HWI, in_n, OW, ob, PLANE_O, out_n, bias_l) as a function returning a struct the lambdas read: <4,f> 440 ->
//     428 VGPRs, 6 510 -> 6 497 instructions, 700 -> 688 AccVGPR moves.  In two halves at the two places of the original: the same.  Taken
//     apart by structured bindings: 432 / 432 for <4,.>.  Copied into the kernel's old locals: counts equal, 2 580 lines of another
//     register assignment (and no line saved).  A struct of just {nsteps, HWI} in place of the two locals: <4,f> 432;
//   * the STAGING INDICES (gperm, rel[], cw) of the register-staged variants as a function, whichever way tile, rel and cw travel:
//     register counts equal, +7 (bf16 <2,f>), +20..25 (f16s), +12 (f16) instructions and 2 300 - 4 200 changed lines per file: the
//     blocks of the inlined && chain land elsewhere relative to the weight-copy loop in front of them;
//   * tr2m_next_tile in conv_tr2m.hip (which bumps the address first and wraps second): -4 instructions, 94 / 96 -> 88 / 92 SGPRs.
// None of these was timed; the test of this header is the identical stream.  Do not "finish the job" without comparing the streams again.
#pragma once
#include "common.h"
#include "kernel_common.h"

namespace pcctr2 {

constexpr int NT = 256;
constexpr int LXY = 17;                                 // tile edge incl. the low-side halo (taps reach b - 1 only)
constexpr int TILE_SLOTS = LXY * LXY * 4;               // (voxel, channel quad) slots of one (plane, cin group) tile: 1156
constexpr int ITEMS = 5;                                // staged slots per thread: 5 x 256 = 1280 >= 1156

// tap t = 0..26 of a micro-step, kz-major; within a kz the (ky, kx) order keeps equal input offsets together and lets the
// first four taps open the four parity classes
struct Tap { int kz, ky, kx, cls, dyi, dxi, sq; bool opens; };
__host__ __device__ constexpr int tr2g_seq(int kz, int ky, int kx) {      // position in the packed (class-major) weight order
    int seq = 0;
    for (int cls = 0; cls < 8; ++cls) {
        const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
        for (int z = pz; z < 3; z += 2)
            for (int y = py; y < 3; y += 2)
                for (int x = px; x < 3; x += 2, ++seq)
                    if (z == kz && y == ky && x == kx) return seq;
    }
    return -1;
}
__host__ __device__ constexpr Tap tap_of(int t) {
    constexpr int KY[9] = {0, 0, 1, 1, 0, 1, 2, 2, 2}, KX[9] = {0, 1, 0, 1, 2, 2, 0, 1, 2};
    const int kz = t / 9, r = t % 9, ky = KY[r], kx = KX[r];
    return Tap{kz, ky, kx, (ky & 1) * 2 + (kx & 1), ky == 2 ? 1 : 0, kx == 2 ? 1 : 0, tr2g_seq(kz, ky, kx), r < 4};
}

// The launch grid: one member of every variant's argument struct, behind its pointers.
struct Tr2mGrid {
    int N, D, H, W;      // input dims (output = 2x)
    int nty, ntx, zsplit, zlen, nct;
    int flags, ocs, oco;
};

// The workgroup's place in the grid: cout tile fastest (neighbours in the grid share their input tiles in L2), then x tile, y tile,
// z slab, block.
struct Tr2mTile { int ct, n, X0, Y0, zb; };
__device__ __forceinline__ Tr2mTile tr2m_tile(const Tr2mGrid& a, int nwg) {
    int wg = pcck::xcd_remap(blockIdx.x, nwg);
    const int ct = wg % a.nct; wg /= a.nct;
    const int tx = wg % a.ntx; wg /= a.ntx;
    const int ty = wg % a.nty; wg /= a.nty;
    const int zs = wg % a.zsplit;
    return Tr2mTile{ct, wg / a.zsplit, tx * 16, ty * 16, zs * a.zlen};
}

// (s2, c2, tile_pl): input plane step / cin group / address of the next tile to fetch (wave-uniform); GB bytes per voxel and cin group
template <int NG, int GB>
__device__ __forceinline__ void tr2m_next_tile(int& s2, int& c2, unsigned long long& tile_pl, unsigned HWI) {
    if (++c2 == NG) { c2 = 0; ++s2; tile_pl += HWI - GB * (NG - 1); } else tile_pl += GB;
}

// The epilogue schedule: the planes finished by the previous input plane leave under the first taps of a plane's first micro-step.  Its
// kz = 0 taps only touch even_cur, so the odd set (items 0..15 of `finish`) goes under taps 0..7, two per tap, and the old even_cur
// (items 16..31) under taps 0..15, before taps 9 / 18 re-open those registers.  The store data registers ost[t & 1][] stay untouched
// for one more tap (late read, see conv_wino.hip).  Called behind tap t of a FIRST, non-halo micro-step.
template <int t, class F, class PH, class V>
__device__ __forceinline__ void tr2m_finish_under_tap(F& finish, PH ph_tag, const __amdgpu_buffer_rsrc_t& rout, V (&ost)[2][3]) {
    if constexpr (t < 8) {
        finish(ph_tag, std::integral_constant<int, 2 * t>{}, rout, ost[t & 1][0]);
        finish(ph_tag, std::integral_constant<int, 2 * t + 1>{}, rout, ost[t & 1][1]);
    }
    if constexpr (t < 16) finish(ph_tag, std::integral_constant<int, 16 + t>{}, rout, ost[t & 1][2]);
    if constexpr (t >= 1 && t < 17) {
        asm volatile("" ::"v"(ost[(t - 1) & 1][2]));
        if constexpr (t < 9) { asm volatile("" ::"v"(ost[(t - 1) & 1][0])); asm volatile("" ::"v"(ost[(t - 1) & 1][1])); }
    }
}
// The drain: the 32 items of the planes finished by the last input plane.  Its parity decides which even set is complete: a last plane
// of PH = 0 left its even_cur in E[0] = "E[PH ^ 1]" of a PH = 1 epilogue, so the kernel calls tr2m_drain<1> when nsteps is odd.  The
// branch and keep[] (pinned behind it, as ost[] above) stay in the kernel: see the note at the top.
template <int PH, class F, class V>
__device__ __forceinline__ void tr2m_drain(F& finish, const __amdgpu_buffer_rsrc_t& rout, V (&keep)[32]) {
    pcck::static_for(std::make_integer_sequence<int, 32>{}, [&](auto e_tag) __attribute__((always_inline)) {
        finish(std::integral_constant<int, PH>{}, e_tag, rout, keep[decltype(e_tag)::value]); });
}

// z split: every CU gets a workgroup; every split pays one extra (halo) input plane of 9 taps
inline int tr2m_zsplit(const pcc_ctx* ctx, const pcc_conv_desc* d) {
    const int base = d->N * (d->H / 16) * (d->W / 16) * (d->Cout / 16);
    int zs = 1;
    while (base * zs < ctx->num_cu && d->D % (zs * 2) == 0 && d->D / (zs * 2) >= 4) zs *= 2;
    return zs;
}

// The host side of the grid: fills g from the layer (output channel stride defaults to Cout; z split above) and returns the number
// of workgroups
inline int tr2m_grid(const pcc_ctx* ctx, const pcc_conv_desc* d, Tr2mGrid& g) {
    g.N = d->N; g.D = d->D; g.H = d->H; g.W = d->W;
    g.nty = d->H / 16; g.ntx = d->W / 16; g.nct = d->Cout / 16;
    g.flags = d->flags;
    g.ocs = d->out_cstride ? d->out_cstride : d->Cout;
    g.oco = d->out_coffset;
    g.zsplit = tr2m_zsplit(ctx, d); g.zlen = d->D / g.zsplit;
    return d->N * g.nty * g.ntx * g.nct * g.zsplit;
}
template <class A>
inline int tr2m_launch(void (*kern)(A, int), int lds, int nwg, const A& a, hipStream_t st) {
    { const int rc = pcc_enable_big_lds((const void*)kern, lds); if (rc != PCC_OK) return rc; }
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(NT), lds, st, a, nwg);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

// The shapes a z-marching kernel covers: k3 stride-2 transposed, (Cin, Cout) in {(32, 16), (64, 32)}, H and W multiples of 16, and
// offsets that keep one input plane and two output planes (out_bytes per element) inside one buffer descriptor.  Flags are the
// caller's to check.
inline bool tr2m_shape_ok(const pcc_conv_desc* d, int out_bytes) {
    if (!d->transposed || d->k != 3 || d->stride != 2) return false;
    if (!((d->Cin == 32 && d->Cout == 16) || (d->Cin == 64 && d->Cout == 32))) return false;
    if (d->H % 16 || d->W % 16) return false;
    const int ocs = d->out_cstride ? d->out_cstride : d->Cout;
    if (ocs % 4 || d->out_coffset % 4) return false;
    if ((double)d->H * d->W * d->Cin * 4.0 >= 2147483648.0) return false;                       // one input plane per descriptor
    if (2.0 * (2.0 * d->H) * (2.0 * d->W) * ocs * out_bytes >= 2147483648.0) return false;      // two output planes per descriptor
    return true;
}

}  // namespace pcctr2
