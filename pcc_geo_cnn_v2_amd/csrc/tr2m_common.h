// Shared pieces of the z-marching Conv3DTranspose k3 stride-2 kernels (conv_tr2m.hip: fp32; conv_tr2m_bf16.hip: split bf16;
// conv_tr2m_f16s.hip: two-piece fp16; conv_tr2m_f16.hip: the fp16 mode): the tile geometry, the tap order of a micro-step, the
// workgroup's place in the grid, the z split of the launch and the shape rule.
#pragma once
#include "common.h"
#include "kernel_common.h"

namespace pcctr2 {

constexpr int NT = 256;
constexpr int LXY = 17;                                 // tile edge incl. the low-side halo (taps reach b - 1 only)
constexpr int TILE_SLOTS = LXY * LXY * 4;               // (voxel, channel quad) slots of one (plane, cin group) tile: 1156

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

// The workgroup's place in the grid: cout tile fastest (neighbours in the grid share their input tiles in L2), then x tile, y tile,
// z slab, block.  A: the launch arguments of the variant.
struct Tr2mTile { int ct, n, X0, Y0, zb; };
template <class A>
__device__ __forceinline__ Tr2mTile tr2m_tile(const A& a, int nwg) {
    int wg = pcck::xcd_remap(blockIdx.x, nwg);
    const int ct = wg % a.nct; wg /= a.nct;
    const int tx = wg % a.ntx; wg /= a.ntx;
    const int ty = wg % a.nty; wg /= a.nty;
    const int zs = wg % a.zsplit;
    return Tr2mTile{ct, wg / a.zsplit, tx * 16, ty * 16, zs * a.zlen};
}

// z split: every CU gets a workgroup; every split pays one extra (halo) input plane of 9 taps
inline int tr2m_zsplit(const pcc_ctx* ctx, const pcc_conv_desc* d) {
    const int base = d->N * (d->H / 16) * (d->W / 16) * (d->Cout / 16);
    int zs = 1;
    while (base * zs < ctx->num_cu && d->D % (zs * 2) == 0 && d->D / (zs * 2) >= 4) zs *= 2;
    return zs;
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
