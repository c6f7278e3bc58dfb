// Weight and bias gradients of the conv layers (training, pcc_conv3d_wgrad).
//
// Every layer is taken in its FORWARD view: a Conv3D (Cin -> Cout, k, s) is itself; a Conv3DTranspose is the adjoint of the SAME
// Conv3D on its larger grid (oracle/torch_oracle.py), whose Keras kernel (k,k,k,Cout_T,Cin_T) has the memory layout of the forward
// kernel of that view.  So with u = the large-grid tensor (forward: the input; transposed: the output gradient) and dz = the
// small-grid tensor (forward: the output gradient; transposed: the input):
//
//     dW[tap, cu, cz] = sum_{n, o} u[n, s*o + tap - padlo, cu] * dz[n, o, cz]        (zeros outside the grid)
//
// a GEMM with M = Cu, N = Cz and a reduction over every voxel of the small grid.  The reduction is split into S fixed voxel slices
// (S a function of the layer's geometry only); each workgroup sums its slice into a [S][k^3 Cu Cz] partial buffer with one k-ordered
// fp32 chain per element, and wgrad_reduce adds the S partials in slice order.  No float atomics: the result is the same bits run to
// run.
//
// Cu, Cz multiples of 16 (every layer of c1..c3p but the Cin = 1 / Cout = 1 ends): exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), A = the
// haloed u patch of a voxel tile staged in LDS (each u element feeds k^3 taps), B = the tile's dz.  Other shapes: one thread per
// weight element, the same slices, fp32 FMA in voxel order.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kPartialFloats = size_t(1) << 25;     // cap of S * k^3 Cu Cz (128 MiB of partials)
constexpr int kMaxSlices = 1024;
constexpr int kBiasSlices = 1024;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct WGeo {
    int N, D, H, W;          // u grid
    int OD, OH, OW;          // dz grid
    int pd, ph, pw;          // SAME low padding on the u grid
    int ntz, nty, ntx;       // voxel tiles of the dz grid per axis (MFMA path)
    int ntiles, slices;
    int cu, cz, k, s;
};

// forward view of a layer: u / dz grids and channels
WGeo view_of(const pcc_conv_desc* d) {
    WGeo g = {};
    int od, oh, ow;
    pcc_conv_out_dims(d, &od, &oh, &ow);
    if (!d->transposed) {
        g.N = d->N; g.D = d->D; g.H = d->H; g.W = d->W; g.OD = od; g.OH = oh; g.OW = ow;
        g.cu = d->Cin; g.cz = d->Cout;
    } else {
        g.N = d->N; g.D = od; g.H = oh; g.W = ow; g.OD = d->D; g.OH = d->H; g.OW = d->W;
        g.cu = d->Cout; g.cz = d->Cin;
    }
    g.k = d->k; g.s = d->stride;
    g.pd = pcc_same_pad_low(g.D, g.k, g.s);
    g.ph = pcc_same_pad_low(g.H, g.k, g.s);
    g.pw = pcc_same_pad_low(g.W, g.k, g.s);
    return g;
}

// ---- MFMA kernel ----------------------------------------------------------------------------------------------------------------
// Template: channels (CU, CZ), kernel (K, S), voxel tile TZ x TY x TX of the dz grid, RW taps per wave.  Grid (slices, chunks): a
// chunk is one 16-channel group `cig` of u and 4 * RW consecutive taps of it (wave w: taps row0 + w*RW .. + RW - 1), all CZ columns.
template <int CU, int CZ, int K, int S, int TZ, int TY, int TX, int RW>
struct WgCfg {
    static constexpr int NCZ = CZ / 16, TAPS = K * K * K, TV = TZ * TY * TX;
    static constexpr int PZ = S * (TZ - 1) + K, PY = S * (TY - 1) + K, PX = S * (TX - 1) + K;
    static constexpr int CHUNKS_PER_CIG = (TAPS + 4 * RW - 1) / (4 * RW);
    static constexpr int CHUNKS = (CU / 16) * CHUNKS_PER_CIG;
    static constexpr int U_FLOATS = PZ * PY * PX * 16;
    static constexpr int LDS_BYTES = (U_FLOATS + TV * CZ) * 4;
    static_assert(TV % 4 == 0 && RW * NCZ <= 16, "tile");
};

template <int CU, int CZ, int K, int S, int TZ, int TY, int TX, int RW>
__global__ void __launch_bounds__(kThreads) wgrad_mfma_kernel(WGeo g, const float* __restrict__ u, const float* __restrict__ dz,
                                                              float* __restrict__ partial) {
    using C = WgCfg<CU, CZ, K, S, TZ, TY, TX, RW>;
    extern __shared__ float lds[];
    float* lu = lds;                     // [PZ][PY][PX][16]
    float* lz = lds + C::U_FLOATS;       // [TV][CZ]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, chunk = blockIdx.y;
    const int cig = chunk / C::CHUNKS_PER_CIG;
    const int tap0 = (chunk % C::CHUNKS_PER_CIG) * 4 * RW + wave * RW;
    int toff[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int t = tap0 + r < C::TAPS ? tap0 + r : 0;
        toff[r] = (((t / (K * K)) * C::PY + (t / K) % K) * C::PX + t % K) * 16;
    }
    f32x4 acc[RW][C::NCZ];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < C::NCZ; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int t_begin = (int)((long long)slice * g.ntiles / g.slices);
    const int t_end = (int)((long long)(slice + 1) * g.ntiles / g.slices);
    for (int tile = t_begin; tile < t_end; ++tile) {
        int t = tile;
        const int tx = t % g.ntx; t /= g.ntx;
        const int ty = t % g.nty; t /= g.nty;
        const int tz = t % g.ntz;
        const int n = t / g.ntz;
        const int oz0 = tz * TZ, oy0 = ty * TY, ox0 = tx * TX;
        const int uz0 = oz0 * S - g.pd, uy0 = oy0 * S - g.ph, ux0 = ox0 * S - g.pw;
        __syncthreads();                 // the previous tile's reads are done
        for (int i = threadIdx.x; i < C::PZ * C::PY * C::PX * 4; i += kThreads) {
            const int c4 = i & 3, p = i >> 2;
            const int px = p % C::PX, py = (p / C::PX) % C::PY, pz = p / (C::PX * C::PY);
            const int z = uz0 + pz, y = uy0 + py, x = ux0 + px;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (z >= 0 && z < g.D && y >= 0 && y < g.H && x >= 0 && x < g.W)
                v = *(const float4*)(u + ((((size_t)n * g.D + z) * g.H + y) * g.W + x) * CU + cig * 16 + c4 * 4);
            *(float4*)(lu + p * 16 + c4 * 4) = v;
        }
        for (int i = threadIdx.x; i < C::TV * CZ / 4; i += kThreads) {
            const int c4 = i % (CZ / 4), v = i / (CZ / 4);
            const int vx = v % TX, vy = (v / TX) % TY, vz = v / (TX * TY);
            const int z = oz0 + vz, y = oy0 + vy, x = ox0 + vx;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (z < g.OD && y < g.OH && x < g.OW)
                val = *(const float4*)(dz + ((((size_t)n * g.OD + z) * g.OH + y) * g.OW + x) * CZ + c4 * 4);
            *(float4*)(lz + v * CZ + c4 * 4) = val;
        }
        __syncthreads();
        if (tap0 < C::TAPS) {
#pragma unroll 2
            for (int k0 = 0; k0 < C::TV; k0 += 4) {
                const int v = k0 + (lane >> 4);
                const int vx = v % TX, vy = (v / TX) % TY, vz = v / (TX * TY);
                const int ub = (((S * vz) * C::PY + S * vy) * C::PX + S * vx) * 16 + (lane & 15);
                float b[C::NCZ];
#pragma unroll
                for (int c = 0; c < C::NCZ; ++c) b[c] = lz[v * CZ + c * 16 + (lane & 15)];
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    if (tap0 + r >= C::TAPS) break;                      // wave-uniform
                    const float a = lu[ub + toff[r]];
#pragma unroll
                    for (int c = 0; c < C::NCZ; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[c], acc[r][c], 0, 0, 0);
                }
            }
        }
    }
    // D[i = cu][j = cz]: column j = lane & 15, row i = 4 * (lane >> 4) + e
    const size_t P = (size_t)C::TAPS * CU * CZ;
    float* out = partial + (size_t)slice * P;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int tap = tap0 + r;
        if (tap >= C::TAPS) break;
#pragma unroll
        for (int c = 0; c < C::NCZ; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cu = cig * 16 + 4 * (lane >> 4) + e, cz = c * 16 + (lane & 15);
                out[((size_t)tap * CU + cu) * CZ + cz] = acc[r][c][e];
            }
    }
}

// ---- VALU kernel: any Cu / Cz (the Cin = 1 first layers and the Cout = 1 last layers) --------------------------------------------
// Thread = one weight element (tap, cu, cz) of one slice; the slice is a contiguous range of dz voxels, summed in voxel order.
__global__ void __launch_bounds__(kThreads) wgrad_valu_kernel(WGeo g, const float* __restrict__ u, const float* __restrict__ dz,
                                                              float* __restrict__ partial) {
    const size_t P = (size_t)g.k * g.k * g.k * g.cu * g.cz;
    const size_t e = (size_t)blockIdx.y * kThreads + threadIdx.x;
    if (e >= P) return;
    const int cz = (int)(e % g.cz), cu = (int)((e / g.cz) % g.cu), tap = (int)(e / ((size_t)g.cz * g.cu));
    const int kz = tap / (g.k * g.k), ky = (tap / g.k) % g.k, kx = tap % g.k;
    const long long nvox = (long long)g.N * g.OD * g.OH * g.OW;
    const long long v0 = (long long)blockIdx.x * nvox / g.slices, v1 = (long long)(blockIdx.x + 1) * nvox / g.slices;
    float acc = 0.f;
    for (long long v = v0; v < v1; ++v) {
        long long t = v;
        const int ox = (int)(t % g.OW); t /= g.OW;
        const int oy = (int)(t % g.OH); t /= g.OH;
        const int oz = (int)(t % g.OD);
        const int n = (int)(t / g.OD);
        const int z = oz * g.s + kz - g.pd, y = oy * g.s + ky - g.ph, x = ox * g.s + kx - g.pw;
        if (z < 0 || z >= g.D || y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
        acc = fmaf(u[((((size_t)n * g.D + z) * g.H + y) * g.W + x) * g.cu + cu], dz[(size_t)v * g.cz + cz], acc);
    }
    partial[(size_t)blockIdx.x * P + e] = acc;
}

// ---- bias: per-channel sums of the output-space gradient over fixed voxel slices -------------------------------------------------
__global__ void __launch_bounds__(kThreads) bias_partial_kernel(const float* __restrict__ g, long long nvox, int C, int slices,
                                                                float* __restrict__ partial) {
    __shared__ float lds[kThreads];
    const int lanes = kThreads / C;                     // voxel lanes per channel (C <= 256)
    const int lv = threadIdx.x / C, c = threadIdx.x % C;
    const long long v0 = (long long)blockIdx.x * nvox / slices, v1 = (long long)(blockIdx.x + 1) * nvox / slices;
    float acc = 0.f;
    if (lv < lanes)
        for (long long v = v0 + lv; v < v1; v += lanes) acc += g[(size_t)v * C + c];
    lds[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < C) {
        float s = 0.f;
        for (int l = 0; l < lanes; ++l) s += lds[l * C + threadIdx.x];
        partial[(size_t)blockIdx.x * C + threadIdx.x] = s;
    }
}

// out[i] = sum over s = 0 .. S-1, in that order, of partial[s][i]
__global__ void __launch_bounds__(kThreads) wgrad_reduce_kernel(const float* __restrict__ partial, int S, size_t P,
                                                                float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    float s = 0.f;
    for (int j = 0; j < S; ++j) s += partial[(size_t)j * P + i];
    out[i] = s;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------------------
typedef void (*wgrad_kern_t)(WGeo, const float*, const float*, float*);
struct MfmaEntry {
    int cu, cz, k, s, tz, ty, tx, chunks, lds;
    wgrad_kern_t kern;
};
#define PCC_WG(CU, CZ, K, S, TZ, TY, TX, RW)                                                                               \
    {CU, CZ, K, S, TZ, TY, TX, WgCfg<CU, CZ, K, S, TZ, TY, TX, RW>::CHUNKS, WgCfg<CU, CZ, K, S, TZ, TY, TX, RW>::LDS_BYTES, \
     wgrad_mfma_kernel<CU, CZ, K, S, TZ, TY, TX, RW>}
// every MFMA-shaped forward view of c1, c2, c3 and c3p
const MfmaEntry kMfma[] = {
    PCC_WG(16, 16, 3, 1, 2, 4, 16, 7), PCC_WG(32, 32, 3, 1, 2, 4, 16, 7), PCC_WG(64, 64, 3, 1, 2, 4, 16, 4),
    PCC_WG(16, 32, 3, 2, 2, 4, 8, 7),  PCC_WG(32, 32, 3, 2, 2, 4, 8, 7),  PCC_WG(32, 64, 3, 2, 2, 4, 8, 4),
    PCC_WG(64, 64, 3, 2, 2, 4, 8, 4),  PCC_WG(32, 32, 5, 2, 1, 4, 8, 8),
};
#undef PCC_WG

const MfmaEntry* find_mfma(const WGeo& g) {
    for (const auto& e : kMfma)
        if (e.cu == g.cu && e.cz == g.cz && e.k == g.k && e.s == g.s) return &e;
    return nullptr;
}

int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// geometry and slice counts: functions of the descriptor only, so that the reduction order never depends on the device
WGeo plan(const pcc_conv_desc* d, const MfmaEntry** mf) {
    WGeo g = view_of(d);
    const MfmaEntry* e = find_mfma(g);
    *mf = e;
    const size_t P = (size_t)g.k * g.k * g.k * g.cu * g.cz;
    long long units;
    if (e) {
        g.ntz = cdiv(g.OD, e->tz); g.nty = cdiv(g.OH, e->ty); g.ntx = cdiv(g.OW, e->tx);
        g.ntiles = g.N * g.ntz * g.nty * g.ntx;
        units = g.ntiles;
    } else {
        units = (long long)g.N * g.OD * g.OH * g.OW;
    }
    long long s = (long long)(kPartialFloats / P);
    if (s > kMaxSlices) s = kMaxSlices;
    if (s > units) s = units;
    g.slices = (int)(s < 1 ? 1 : s);
    return g;
}

}  // namespace

PCC_API size_t pcc_conv_wgrad_workspace_bytes(const pcc_conv_desc* d) {
    if (!d || d->N <= 0 || d->k <= 0 || d->Cin <= 0 || d->Cout <= 0 || (d->stride != 1 && d->stride != 2)) return 0;
    const MfmaEntry* mf;
    const WGeo g = plan(d, &mf);
    const size_t P = (size_t)g.k * g.k * g.k * g.cu * g.cz;
    return ((size_t)g.slices * P + (size_t)kBiasSlices * d->Cout) * sizeof(float);
}

PCC_API int pcc_conv_wgrad_slices(const pcc_conv_desc* d, int32_t* slices, int64_t* slice_terms) {
    PCC_REQUIRE(d && slices && slice_terms, "pcc_conv_wgrad_slices: NULL argument");
    PCC_REQUIRE(d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->k >= 1 &&
                (d->stride == 1 || d->stride == 2), "pcc_conv_wgrad_slices: bad descriptor");
    const MfmaEntry* mf;
    const WGeo g = plan(d, &mf);
    *slices = g.slices;
    if (mf) *slice_terms = (int64_t)cdiv(g.ntiles, g.slices) * mf->tz * mf->ty * mf->tx;
    else *slice_terms = cdiv((long long)g.N * g.OD * g.OH * g.OW, g.slices);
    return PCC_OK;
}

PCC_API int pcc_conv3d_wgrad(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* dout, float* dw, float* db,
                             void* workspace, size_t ws_bytes, void* stream) {
    PCC_REQUIRE(ctx && d && in && dout && dw && workspace, "pcc_conv3d_wgrad: NULL argument");
    PCC_REQUIRE(d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->k >= 1 &&
                (d->stride == 1 || d->stride == 2), "pcc_conv3d_wgrad: bad descriptor");
    PCC_REQUIRE(d->out_cstride == 0 && d->out_coffset == 0, "pcc_conv3d_wgrad: the output gradient is a whole tensor");
    PCC_REQUIRE(d->Cout <= kThreads, "pcc_conv3d_wgrad: more than %d output channels", kThreads);
    PCC_REQUIRE(ws_bytes >= pcc_conv_wgrad_workspace_bytes(d), "pcc_conv3d_wgrad: workspace smaller than pcc_conv_wgrad_workspace_bytes");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const MfmaEntry* mf;
    const WGeo g = plan(d, &mf);
    const size_t P = (size_t)g.k * g.k * g.k * g.cu * g.cz;
    float* wpart = (float*)workspace;
    float* bpart = wpart + (size_t)g.slices * P;
    const float* u = d->transposed ? dout : in;
    const float* z = d->transposed ? in : dout;
    if (mf) {
        PCC_REQUIRE(((uintptr_t)u | (uintptr_t)z) % 16 == 0, "pcc_conv3d_wgrad: tensors must be 16-byte aligned");
        { const int rc = pcc_enable_big_lds((const void*)mf->kern, mf->lds); if (rc != PCC_OK) return rc; }
        hipLaunchKernelGGL(mf->kern, dim3(g.slices, mf->chunks), dim3(kThreads), mf->lds, st, g, u, z, wpart);
    } else {
        hipLaunchKernelGGL(wgrad_valu_kernel, dim3(g.slices, cdiv((long long)P, kThreads)), dim3(kThreads), 0, st, g, u, z, wpart);
    }
    PCC_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long long)P, kThreads)), dim3(kThreads), 0, st, wpart, g.slices, P, dw);
    PCC_CHECK_HIP(hipGetLastError());
    if (db) {
        // the layer's output-space gradient is dout in both views
        int od, oh, ow;
        pcc_conv_out_dims(d, &od, &oh, &ow);
        const long long nvox = (long long)d->N * od * oh * ow;
        const int sb = (int)(nvox < kBiasSlices ? nvox : kBiasSlices);
        hipLaunchKernelGGL(bias_partial_kernel, dim3(sb), dim3(kThreads), 0, st, dout, nvox, d->Cout, sb, bpart);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(d->Cout, kThreads)), dim3(kThreads), 0, st, bpart, sb, (size_t)d->Cout, db);
        PCC_CHECK_HIP(hipGetLastError());
    }
    return PCC_OK;
}
