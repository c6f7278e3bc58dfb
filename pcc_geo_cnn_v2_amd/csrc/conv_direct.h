// Shared by the direct MFMA implicit-GEMM conv families (conv_fwd.hip, conv_tr2.hip, conv_edge.hip), fp32.
//
// GEMM view:  D[cout][voxel] = sum_k  Wt[cout][k] * In[k][voxel],   k = (tap, cin)
//   * MFMA: v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered FMA chain -> bit-deterministic results that do
//     not depend on tile position, batch size or launch geometry; SURVEY.md §5 determinism requirement).
//   * A operand = weights, pre-packed on the host in fragment order (one float4 per lane covers 4 MFMAs;
//     conv_route.hip, pcc_conv_pack_weights); B operand = a 16-voxel row of the NDHWC input tile staged in LDS
//     (one ds_read_b128 per lane covers the 4 MFMAs of a 16-channel group: MFMA j contracts channels {j, 4+j, 8+j, 12+j}).
//   * D layout: lane holds 4 consecutive output channels of one voxel -> float4 epilogue loads/stores
//     (bias, ReLU, residual add, clip fused).
//   * LDS voxel stride = staged channels + 8 floats: the +8 makes every ds_read_b128 lane group hit 16
//     distinct 16-byte bank slots (stride = 2 mod 4 slots), so tap offsets stay immediates.
#pragma once
#include "common.h"
#include "kernel_common.h"

namespace pccmfma {

using namespace pcck;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// PCC_CONV_F16 (BASELINE.json configs[4]): the same fragments -- a lane's float4 holds k-slots 4*(lane>>4)..+3 of a
// 16-channel group, exactly the k layout of v_mfma_f32_16x16x16_f16 -- are rounded to fp16 (v_cvt_pk_f16_f32, RTN) and
// contracted by ONE matrix instruction instead of four; accumulation, bias, activations in HBM and LDS stay fp32.
__device__ __forceinline__ f32x4 mfma16h(const f32x4& a, const f32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_convertvector(a, f16x4), __builtin_convertvector(b, f16x4), c, 0, 0, 0);
}

// sched_barrier mask: VALU, SALU, DS and transcendental ops may cross; vector-memory ops and MFMAs may not ->
// a prefetch load stays in front of the MFMAs of the tap it was written in (two taps before its use).
// (The stricter PCC_PIN_MEM_MFMA is in kernel_common.h.)
#define PCC_PIN_VMEM() __builtin_amdgcn_sched_barrier(0x786)

struct ConvArgs {
    const float* in;
    const float* w;  // packed
    const float* bias;
    const float* res;
    float* out;
    int N, D, H, W;     // input dims
    int OD, OH, OW;     // output dims
    int ntz, nty, ntx;  // tiles per dim (base grid)
    int flags, ocs, oco;
    // 16 -> 1 last layer with the occupancy decision folded into its epilogue (pcc_thr_fuse): bit (z,y,x) of `mask` = x_hat > thr[n]
    const float* thr = nullptr;
    unsigned short* mask = nullptr;
    int thr_clip = 0;
    // per-block max |out| for the fp16-split layer that consumes `out` (common.h, pcc_conv_ext); filled by conv_cin1_kernel
    unsigned* amax_out = nullptr;
};

__device__ __forceinline__ f32x4 store_out(const ConvArgs& a, f32x4 v, size_t vox, int c0, int COUT) {
    // v = 4 consecutive output channels c0..c0+3 of voxel `vox`; returns what was stored (fp32 path)
    if (a.flags & PCC_CONV_BIAS) v += *reinterpret_cast<const f32x4*>(a.bias + c0);
    if (a.flags & PCC_CONV_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if (a.flags & PCC_CONV_ADD) v += *reinterpret_cast<const f32x4*>(a.res + vox * COUT + c0);
    if (a.flags & PCC_CONV_CLIP01) {
        v.x = fminf(fmaxf(v.x, 0.f), 1.f); v.y = fminf(fmaxf(v.y, 0.f), 1.f);
        v.z = fminf(fmaxf(v.z, 0.f), 1.f); v.w = fminf(fmaxf(v.w, 0.f), 1.f);
    }
    if (a.flags & PCC_CONV_OUT16) {      // fp16 hand-over to conv_f16.hip (fp16 mode): 8 bytes per lane
        f16x4 h;
        h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
        *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.out) + vox * a.ocs + a.oco + c0) = h;
    } else {
        *reinterpret_cast<f32x4*>(a.out + vox * a.ocs + a.oco + c0) = v;
    }
    return v;
}

// =====================================================================================================
// transposed conv, stride 2: parity decomposition on the INPUT (base) grid.
//   out[2b + p] = sum over taps kappa = (p + PL) mod 2 (step 2) of W[kappa] * in[b + (p + PL - kappa)/2]
//   PL = SAME pad_low of the adjoint forward conv = (KS-2)/2.
// =====================================================================================================
template <int KS>
struct Tr2Geo {
    static constexpr int PL = (KS - 2) / 2;
    // delta range over both parities: kappa in [0,KS): delta = (p + PL - kappa)/2
    static constexpr int HL = (KS - 1 - PL) / 2;      // max(-delta)  (kappa = KS-1 or KS-2)
    static constexpr int HH = (1 + PL) / 2;           // max(+delta)  (p = 1, kappa = 0 or 1)
};

template <typename KernelT, typename... Extra>
int launch(KernelT kern, int nt, int lds_bytes, int tiles, const ConvArgs& a, hipStream_t st, Extra... extra) {
    { const int rc = pcc_enable_big_lds((const void*)kern, lds_bytes); if (rc != PCC_OK) return rc; }
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(nt), lds_bytes, st, a, extra...);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// the kernel arguments of layer `d`; the launcher sets the tile counts
inline ConvArgs conv_args(const pcc_conv_desc* d, const float* in, const float* w, const float* bias, const float* res, float* out) {
    ConvArgs a;
    a.in = in; a.w = w; a.bias = bias; a.res = res; a.out = out;
    a.N = d->N; a.D = d->D; a.H = d->H; a.W = d->W;
    pcc_conv_out_dims(d, &a.OD, &a.OH, &a.OW);
    a.flags = d->flags; a.ocs = d->out_cstride ? d->out_cstride : d->Cout; a.oco = d->out_coffset;
    a.ntz = a.nty = a.ntx = 0;
    return a;
}

inline int no_instantiation(const pcc_conv_desc* d) {
    pcc_set_error("pcc_conv3d_mfma: no instantiation for Cin=%d Cout=%d k=%d s=%d transposed=%d", d->Cin, d->Cout, d->k, d->stride,
                  d->transposed);
    return PCC_ERR_ARG;
}

}  // namespace pccmfma
