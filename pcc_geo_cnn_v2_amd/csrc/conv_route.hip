// Host-side policy of the conv layers, every kernel family: the plan of a layer (make_plan), its family (pcc_conv_route), the
// layout and packing of its weight image, and the dispatch to the family's entry point (common.h).  No device code.
#include <cstdlib>

#include "common.h"

namespace {

enum Kind { K_NONE = 0, K_FWD, K_TR2, K_CIN1, K_COUT1, K_COUT1M };

struct Plan {
    Kind kind = K_NONE;
    int tx = 0;           // 16 / 8 / 4: voxels of a row along x
    bool flip = false;    // transposed stride-1 -> forward with flipped taps
};

inline int base_w(const pcc_conv_desc* d) {  // x extent of the grid the rows live on
    if (d->transposed) return d->W;          // TR2: input grid; TR s1: same
    return pcc_same_out(d->W, d->stride);
}

static Plan make_plan(const pcc_conv_desc* d) {
    Plan p;
    if ((double)d->D * d->H * d->W * d->Cin * 4.0 >= 2147483648.0) return p;
    const bool out_vec_ok = d->out_cstride == 0 || (d->out_cstride % 4 == 0 && d->out_coffset % 4 == 0);
    const int k = d->k, s = d->stride;
    const bool even = (d->D % 2 == 0) && (d->H % 2 == 0) && (d->W % 2 == 0);
    if (!d->transposed && d->Cin == 1) {
        if (out_vec_ok && s == 2 && even && (k == 3 || k == 9) && (d->Cout == 16 || d->Cout == 32) && base_w(d) % 16 == 0) p.kind = K_CIN1;
        return p;
    }
    if (d->transposed && d->Cout == 1) {
        if (s == 1 && k == 3 && d->Cin == 16) { p.kind = K_COUT1M; p.flip = true; }
        else if (s == 1 && k == 3 && d->Cin == 32 && d->W % 8 == 0) { p.kind = K_COUT1; p.flip = true; }
        else if (s == 2 && k == 9 && d->Cin == 32 && d->W % 8 == 0) p.kind = K_COUT1;
        return p;
    }
    if (!out_vec_ok) return p;
    if (d->Cin % 16 || d->Cout % 16 || d->Cin > 64 || d->Cout > 64 || d->Cin == 48 || d->Cout == 48) return p;
    const int bw = base_w(d);
    const int tx = bw % 16 == 0 ? 16 : (bw == 8 ? 8 : (bw == 4 ? 4 : 0));
    if (!tx) return p;
    if (!d->transposed) {
        if (s == 1 && k == 3) p.kind = K_FWD;
        else if (s == 2 && even && (k == 3 || k == 5)) p.kind = K_FWD;
    } else {
        if (s == 1 && k == 3) { p.kind = K_FWD; p.flip = true; }
        else if (s == 2 && (k == 3 || k == 5)) p.kind = K_TR2;
    }
    if (p.kind == K_FWD && k == 5 && !(d->Cin == 32 && d->Cout == 32)) p.kind = K_NONE;
    if (p.kind == K_TR2 && k == 5 && !(d->Cin == 32 && d->Cout == 32)) p.kind = K_NONE;
    p.tx = tx;
    return p;
}

// The packed image of a layer: the Keras-order taps at 0, then the images of the kernels that can compute the layer, each at its
// offset in floats (0: the layer carries no such image).  A function of the layer's kind and (Cin, Cout, k, stride) only, never of
// its grid: pcc_weights_pack lays a network's blob out once.
struct Packed {
    size_t wino_u = 0;      // Winograd-transformed weights U (conv_wino.hip): 16 / 32 / 64-channel k3 stride-1 layers
    size_t f16 = 0;         // fp16 fragments (conv_f16.hip)
    size_t wino_ub = 0;     // U as three bf16 pieces (conv_wino_bf16.hip)
    size_t split = 0;       // split-bf16 taps of the direct kernel (conv_split.hip), 32 / 64 channels
    size_t wino_uh = 0;     // U as two fp16 pieces (conv_wino_f16s.hip)
    size_t tr2g = 0;        // k3 stride-2 transposed layers: the taps in the order of conv_tr2g_kernel and the z marches
    size_t tr2_split = 0;   // its split-bf16 image (conv_tr2m_bf16.hip, conv_tr2_split_kernel): 32 -> 16, 64 -> 32, 64 -> 64
    size_t tr2_f16s = 0;    // its two-piece fp16 image (conv_tr2m_f16s.hip): 32 -> 16, 64 -> 32
    size_t total = 0;
};
static Packed packed_layout(const pcc_conv_desc* d, Kind kind) {
    Packed L;
    const int ci = d->Cin, co = d->Cout, k = d->k;
    const size_t groups = (size_t)(ci / 16) * (co / 16);
    size_t end = (size_t)k * k * k * ci * co;
    auto put = [&end](size_t& at, size_t floats) { at = end; end += floats; };
    if (kind == K_FWD && pcc_wino_channels(ci, co) && k == 3 && d->stride == 1) {
        put(L.wino_u, groups * PCC_WINO_U_FLOATS);
        put(L.f16, pcc_f16_packed_bytes(ci) / 4);
        put(L.wino_ub, groups * PCC_WINO_UB_FLOATS);
        if (ci >= 32) put(L.split, pcc_split_packed_floats(ci));
        put(L.wino_uh, groups * PCC_WINO_UH_FLOATS + PCC_WINO_UH_TAIL);
    } else if (kind == K_TR2 && k == 3) {
        put(L.tr2g, (size_t)27 * ci * co);
        if ((ci == 32 && co == 16) || (ci == 64 && (co == 32 || co == 64))) put(L.tr2_split, pcc_tr2m_bf16_packed_floats(ci, co));
        if ((ci == 32 && co == 16) || (ci == 64 && co == 32)) put(L.tr2_f16s, pcc_tr2m_f16s_packed_floats(ci, co));
    } else if (kind == K_CIN1) {
        end = (size_t)k * k * ((k + 3) / 4) * 4 * co;
    } else if (kind == K_COUT1M) {
        end = 2 * 64 * 4;
    } else if (kind == K_NONE) {
        end = 0;
    }
    L.total = end;
    return L;
}

// logical forward-style weight W(tap, ci, co) of the gather formulation, from the Keras layouts: forward (k,k,k,Cin,Cout); transposed
// (k,k,k,Cout,Cin), taps flipped for the transposed stride-1 layers
struct Taps {
    const pcc_conv_desc* d;
    const float* w;
    bool flip;
    float operator()(int kz, int ky, int kx, int ci, int co) const {
        const int k = d->k;
        if (!d->transposed) return w[((((size_t)kz * k + ky) * k + kx) * d->Cin + ci) * d->Cout + co];
        if (flip) { kz = k - 1 - kz; ky = k - 1 - ky; kx = k - 1 - kx; }
        return w[((((size_t)kz * k + ky) * k + kx) * d->Cout + co) * d->Cin + ci];
    }
};

// conv_fwd_kernel, then (k3 stride 1, Cin = Cout in {16, 32, 64}) the Winograd U and the images built from U and from the taps
static int pack_fwd(const pcc_conv_desc* d, const Taps& Wf, const Packed& L, float* pk) {
    const int k = d->k, Cin = d->Cin, Cout = d->Cout;
    const int NG = Cin / 16, NCT = Cout / 16;
    // [g][tap][ct][lane][j] : cin = g*16 + 4*(lane>>4) + j, cout = ct*16 + (lane&15)
    for (int g = 0; g < NG; ++g)
        for (int kz = 0; kz < k; ++kz) for (int ky = 0; ky < k; ++ky) for (int kx = 0; kx < k; ++kx) {
            const int tap = (kz * k + ky) * k + kx;
            for (int ct = 0; ct < NCT; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        pk[((((size_t)g * k * k * k + tap) * NCT + ct) * 64 + lane) * 4 + j] =
                            Wf(kz, ky, kx, g * 16 + 4 * (lane >> 4) + j, ct * 16 + (lane & 15));
        }
    if (!L.wino_u) return PCC_OK;
    // [cin group][cout group] U[dz][py][px][lane][kk] = (G (x) G) g_dz  for cin = 16 cig + 4*(lane>>4) + kk,
    // cout = 16 cog + (lane & 15); double precision
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    float* u = pk + L.wino_u;
    for (int cig = 0; cig < NG; ++cig) for (int cog = 0; cog < NCT; ++cog)
        for (int kz = 0; kz < 3; ++kz) for (int py = 0; py < 4; ++py) for (int px = 0; px < 4; ++px)
            for (int lane = 0; lane < 64; ++lane)
                for (int kk = 0; kk < 4; ++kk) {
                    double s = 0;
                    for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx)
                        s += G[py][ky] * G[px][kx] * (double)Wf(kz, ky, kx, 16 * cig + 4 * (lane >> 4) + kk, 16 * cog + (lane & 15));
                    u[(((size_t)(cig * NCT + cog) * 48 + (kz * 4 + py) * 4 + px) * 64 + lane) * 4 + kk] = (float)s;
                }
    // the images built from U and from the logical taps
    float* wlog = (float*)malloc((size_t)27 * Cin * Cout * sizeof(float));
    PCC_REQUIRE(wlog != nullptr, "pcc_conv_pack_weights: out of memory");
    for (int kz = 0; kz < 3; ++kz) for (int ky = 0; ky < 3; ++ky) for (int kx = 0; kx < 3; ++kx)
        for (int ci = 0; ci < Cin; ++ci) for (int co = 0; co < Cout; ++co)
            wlog[((((size_t)kz * 3 + ky) * 3 + kx) * Cin + ci) * Cout + co] = Wf(kz, ky, kx, ci, co);
    pcc_f16_pack(Cin, wlog, (unsigned short*)(pk + L.f16));
    pcc_wino_bf16_pack(NG, u, pk + L.wino_ub);
    if (L.split) pcc_split_pack(Cin, wlog, pk + L.split);
    pcc_wino_f16s_pack(NG, u, pk + L.wino_uh);
    free(wlog);
    return PCC_OK;
}

// conv_tr2_kernel, then (k3) conv_tr2g_kernel's image and the piece images built from it
static void pack_tr2(const pcc_conv_desc* d, const Taps& Wf, const Packed& L, float* pk) {
    const int k = d->k, Cin = d->Cin, Cout = d->Cout;
    const int NG = Cin / 16, NCT = Cout / 16;
    // consumption order of conv_tr2_kernel: [parity class (pz,py,px)][taps of the class (kz,ky,kx)][g][ct][lane][j]
    const int PL = (k - 2) / 2;
    size_t seq = 0;
    for (int pz = 0; pz < 2; ++pz) for (int py = 0; py < 2; ++py) for (int px = 0; px < 2; ++px)
        for (int kz = (pz + PL) & 1; kz < k; kz += 2) for (int ky = (py + PL) & 1; ky < k; ky += 2)
            for (int kx = (px + PL) & 1; kx < k; kx += 2)
                for (int g = 0; g < NG; ++g, ++seq)
                    for (int ct = 0; ct < NCT; ++ct)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j)
                                pk[(((seq * NCT) + ct) * 64 + lane) * 4 + j] =
                                    Wf(kz, ky, kx, g * 16 + 4 * (lane >> 4) + j, ct * 16 + (lane & 15));
    if (!L.tr2g) return;
    // conv_tr2g_kernel: [g][parity class][taps of the class][ct][lane][j]
    float* pg = pk + L.tr2g;
    for (int g = 0; g < NG; ++g) {
        size_t sq = 0;
        for (int pz = 0; pz < 2; ++pz) for (int py = 0; py < 2; ++py) for (int px = 0; px < 2; ++px)
            for (int kz = pz; kz < 3; kz += 2) for (int ky = py; ky < 3; ky += 2) for (int kx = px; kx < 3; kx += 2, ++sq)
                for (int ct = 0; ct < NCT; ++ct)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j)
                            pg[((((size_t)g * 27 + sq) * NCT + ct) * 64 + lane) * 4 + j] =
                                Wf(kz, ky, kx, g * 16 + 4 * (lane >> 4) + j, ct * 16 + (lane & 15));
    }
    if (L.tr2_split) pcc_tr2m_bf16_pack(Cin, Cout, pg, pk + L.tr2_split);
    if (L.tr2_f16s) pcc_tr2m_f16s_pack(Cin, Cout, pg, pk + L.tr2_f16s);
}

// conv_cin1_kernel: [kz][ky][kxg][ct][lane] : kx = kxg*4 + (lane>>4) (zero beyond k), cout = ct*16 + (lane&15)
static void pack_cin1(const pcc_conv_desc* d, const Taps& Wf, float* pk) {
    const int k = d->k, NCT = d->Cout / 16;
    const int KXG = (k + 3) / 4;
    for (int kz = 0; kz < k; ++kz) for (int ky = 0; ky < k; ++ky) for (int kg = 0; kg < KXG; ++kg)
        for (int ct = 0; ct < NCT; ++ct)
            for (int lane = 0; lane < 64; ++lane) {
                const int kx = kg * 4 + (lane >> 4);
                pk[((((size_t)(kz * k + ky) * KXG + kg) * NCT) + ct) * 64 + lane] =
                    kx < k ? Wf(kz, ky, kx, 0, ct * 16 + (lane & 15)) : 0.f;
            }
}

// conv_cout1_mfma_kernel: [mt][lane][j]: tap = 16*mt + (lane & 15) (zero rows beyond 27), channel = 4*(lane>>4) + j
static void pack_cout1m(const Taps& Wf, float* pk) {
    for (int mt = 0; mt < 2; ++mt)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) {
                const int tap = 16 * mt + (lane & 15);
                pk[(mt * 64 + lane) * 4 + j] = tap < 27 ? Wf(tap / 9, (tap / 3) % 3, tap % 3, 4 * (lane >> 4) + j, 0) : 0.f;
            }
}

// conv_cout1_kernel: [tap][ci]
static void pack_cout1(const pcc_conv_desc* d, const Taps& Wf, float* pk) {
    const int k = d->k, Cin = d->Cin;
    for (int kz = 0; kz < k; ++kz) for (int ky = 0; ky < k; ++ky) for (int kx = 0; kx < k; ++kx)
        for (int ci = 0; ci < Cin; ++ci)
            pk[((size_t)((kz * k + ky) * k + kx)) * Cin + ci] = Wf(kz, ky, kx, ci, 0);
}

}  // namespace

PCC_API int pcc_conv_mfma_supported(const pcc_conv_desc* d) {
    if (!d) return 0;
    return make_plan(d).kind != K_NONE ? 1 : 0;
}

PCC_API size_t pcc_conv_packed_floats(const pcc_conv_desc* d) { return d ? packed_layout(d, make_plan(d).kind).total : 0; }

PCC_API int pcc_conv_pack_weights(const pcc_conv_desc* d, const float* w, float* pk) {
    PCC_REQUIRE(d && w && pk, "pcc_conv_pack_weights: NULL argument");
    const Plan p = make_plan(d);
    PCC_REQUIRE(p.kind != K_NONE, "pcc_conv_pack_weights: shape not covered by the MFMA path");
    const Packed L = packed_layout(d, p.kind);
    const Taps Wf{d, w, p.flip};
    switch (p.kind) {
        case K_FWD: return pack_fwd(d, Wf, L, pk);
        case K_TR2: pack_tr2(d, Wf, L, pk); break;
        case K_CIN1: pack_cin1(d, Wf, pk); break;
        case K_COUT1M: pack_cout1m(Wf, pk); break;
        default: pack_cout1(d, Wf, pk);
    }
    return PCC_OK;
}

// The kernel family that computes a layer: a function of the layer (shape, flags, impl) and the context's numerics word only, never
// of the batch -- encoder and decoder run with different batch sizes, and the family is part of the stream's identity (DESIGN.md
// section 5).  Everything that depends on the choice reads it here: the dispatch below, pcc_conv_kernel_family, the block-maximum rows
// of pcc_network_plan (pcc_conv_wants_amax) and the generic / MFMA decision of pcc_conv3d.
pcc_conv_family pcc_conv_route(const pcc_conv_desc* d, uint32_t numerics) {
    auto num = [numerics](uint32_t bits) { return (numerics & bits) != 0; };
    const Plan p = make_plan(d);
    const int ci = d->Cin, fl = d->flags, impl = d->impl;
    const bool autoi = impl == PCC_IMPL_AUTO;
    if (p.kind == K_NONE || !(autoi || impl == PCC_IMPL_MFMA || impl == PCC_IMPL_WINOGRAD || impl == PCC_IMPL_SPLIT)) return PCC_FAM_GENERIC;
    if ((fl & (PCC_CONV_IN16 | PCC_CONV_RES16)) && p.kind != K_COUT1M) return PCC_FAM_F16;
    if (p.kind == K_CIN1) return PCC_FAM_CIN1;
    if (p.kind == K_COUT1M) return PCC_FAM_COUT1M;
    if (p.kind == K_COUT1) return PCC_FAM_COUT1;
    const bool plain = !(fl & (PCC_CONV_F16 | PCC_CONV_OUT16));
    if (p.kind == K_TR2) {
        // k3 stride 2: fp16-mode march | two-piece fp16 march (32 -> 16, 64 -> 32 on grids of 16-multiples) | parity-class tiles, bf16 x 3
        // (64 -> 32 / 64 -> 64) | bf16 x 3 march (32 -> 16) | exact-fp32 march | the tiled exact-fp32 kernels (also every k5 layer)
        if (d->k != 3) return PCC_FAM_TR2;
        if (autoi && !num(PCC_NUM_NO_TR2M) && pcc_tr2m_f16_covers(d)) return PCC_FAM_TR2M_F16;
        const bool f16s = plain && !num(PCC_NUM_NO_TR2M | PCC_NUM_NO_SPLIT | PCC_NUM_NO_SPLIT_TR2 | PCC_NUM_NO_F16S) && pcc_tr2m_eligible(d);
        if (autoi && f16s) return PCC_FAM_TR2M_F16S;
        if (autoi && plain && pcc_tr2_split_covers(d) && !num(PCC_NUM_NO_SPLIT | PCC_NUM_NO_SPLIT_TR2)) return PCC_FAM_TR2_SPLIT;
        // The march (PCC_IMPL_MFMA callers, PCC_TR2M=1: wherever eligible): 32 -> 16 always; 64 -> 32 from 32 input planes up (16^3 x 32
        // blocks gives 4-plane slabs: the 9-tap halo plane and the 108 KB weight prologue per workgroup make the tiled conv_tr2g_kernel
        // faster there: 127 vs 135 us).  The two sum in different orders (DESIGN_HISTORY.md section 4).
        if (num(PCC_NUM_NO_TR2M) || !pcc_tr2m_eligible(d) || !(num(PCC_NUM_TR2M) || ci == 32 || d->D >= 32)) return PCC_FAM_TR2;
        if (f16s) return PCC_FAM_TR2M_F16S;
        return pcc_tr2m_bf16_covers(d) && !num(PCC_NUM_NO_SPLIT | PCC_NUM_NO_SPLIT_TR2) ? PCC_FAM_TR2M_BF16 : PCC_FAM_TR2M;
    }
    const pcc_conv_family fwd = (fl & PCC_CONV_F16) ? PCC_FAM_FWD_F16 : PCC_FAM_FWD;
    if (!(pcc_wino_channels(ci, d->Cout) && d->k == 3 && d->stride == 1)) return fwd;
    // k3 stride 1, Cin = Cout in {16, 32, 64}.  The direct split-bf16 kernel (conv_split.hip) in its 16x16x32 or 32x32x16 MFMA
    // formulation, measured at batch 32 (tools/bench_one.py): 64 -> 64 @16^3 128 us (16x16x32, tile 2 x 4 x 16) / 134 - 148 (32x32x16);
    // 32 -> 32 @16^3 41 / 38.5 us, @32^3 332 / 373 us.  The 32x32 tiles need W % 32 == 0 or W == 16.  PCC_SPLIT_MFMA=16 | 32 overrides (A/B).
    const bool mfma32 = !num(PCC_NUM_SPLIT_MFMA16) && (num(PCC_NUM_SPLIT_MFMA32) || ci == 32) && (d->W % 32 == 0 || d->W == 16);
    const pcc_conv_family split = mfma32 ? PCC_FAM_SPLIT32 : PCC_FAM_SPLIT16;
    if (impl == PCC_IMPL_SPLIT) return split;
    // 64 channels on grids of 16-multiples: the two-piece fp16 Winograd kernel as two launches of two cin groups (conv_wino_f16s.hip)
    // ahead of the direct split kernel; PCC_NO_F16S=1 / PCC_NO_WINOGRAD64=1: the direct kernel (A/B)
    if (autoi && ci == 64 && !(fl & (PCC_CONV_F16 | PCC_CONV_OUT16 | PCC_CONV_CLIP01)) &&
        !num(PCC_NUM_NO_SPLIT | PCC_NUM_NO_F16S | PCC_NUM_NO_WINOGRAD | PCC_NUM_NO_WINOGRAD64) && pcc_wino_eligible(d))
        return PCC_FAM_WINO_F16S;
    // The direct split kernel where it beats the fp32-MFMA Winograd kernel: 64 channels (128 us against 138 - 146 @16^3 x 32); 32 channels
    // on the small grids only (38.5 against 45 us @16^3; at 32^3 the Winograd kernel's 241 us stand against 332: every tile of the
    // direct kernel pays its staging, split and epilogue un-overlapped, DESIGN_HISTORY.md 3.0d).  PCC_NO_SPLIT_DIRECT=1: off (A/B)
    if (autoi && plain && !num(PCC_NUM_NO_SPLIT | PCC_NUM_NO_SPLIT_DIRECT) && pcc_split_covers(d) &&
        (ci == 64 || (ci == 32 && d->D <= 16 && (d->W % 32 == 0 || d->W == 16))))
        return split;
    const bool want = impl == PCC_IMPL_WINOGRAD || (autoi && !(fl & PCC_CONV_F16) && !num(PCC_NUM_NO_WINOGRAD) &&
                                                    !(ci == 32 && (num(PCC_NUM_NO_WINOGRAD32) || d->D < 16)) && !(ci == 64 && num(PCC_NUM_NO_WINOGRAD64)));
    if (!(want && pcc_wino_eligible(d))) return fwd;
    // two fp16 pieces under a per-block power-of-two pre-scale (conv_wino_f16s.hip); PCC_NO_F16S=1: three bf16 pieces (16 channels) /
    // exact fp32; PCC_NO_SPLIT=1: exact-fp32 MFMA everywhere (A/B)
    if (!num(PCC_NUM_NO_SPLIT | PCC_NUM_NO_F16S) && (ci == 16 || !(fl & PCC_CONV_CLIP01)) && !(ci == 64 && (fl & PCC_CONV_F16))) return PCC_FAM_WINO_F16S;
    if (!num(PCC_NUM_NO_SPLIT) && ci == 16) return PCC_FAM_WINO_BF16;
    return PCC_FAM_WINO;
}

// What bench.py prints beside every layer's time, and what a maintainer asks when two builds disagree in the last bits.
PCC_API int pcc_conv_kernel_family(pcc_ctx* ctx, const pcc_conv_desc* d, char* buf, int32_t cap) {
    PCC_REQUIRE(ctx && d && buf && cap > 0, "pcc_conv_kernel_family: NULL argument");
    static const char* const names[PCC_FAM_COUNT] = {
        "generic (reference-order fp32 FMA chain)", "conv_f16 (fp16 storage, f16 MFMA)", "conv_fwd (exact fp32 MFMA)", "conv_fwd (f16 MFMA)",
        "conv_k3s1_split (direct, bf16 x 3, 16x16x32 MFMA)", "conv_k3s1_split32 (direct, bf16 x 3, 32x32x16 MFMA)",
        "conv16_wino (Winograd, exact fp32 MFMA)", "conv16_wino_bf16 (Winograd, bf16 x 3)", "conv16_wino_f16s (Winograd, fp16 x 2 under a per-block pre-scale)",
        "conv_tr2 (exact fp32 MFMA)", "conv_tr2m_f16 (z march, f16 MFMA)", "conv_tr2m_f16s (z march, fp16 x 2 under a per-block pre-scale)",
        "conv_tr2_split (parity classes, bf16 x 3)", "conv_tr2m_bf16 (z march, bf16 x 3)", "conv_tr2m (z march, exact fp32 MFMA)",
        "conv_cin1 (exact fp32 MFMA)", "conv_cout1_mfma (exact fp32 MFMA)", "conv_cout1 (fp32 VALU)"};
    snprintf(buf, (size_t)cap, "%s", names[pcc_conv_route(d, ctx->numerics)]);
    return PCC_OK;
}

int pcc_conv3d_mfma_thr(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_packed, const float* bias,
                        const float* residual, float* out, const pcc_thr_fuse* fuse, bool* fused, pcc_conv_ext* ext, hipStream_t st) {
    if (fused) *fused = false;
    if (ext) ext->out_recorded = false;
    const Plan p = make_plan(d);
    const pcc_conv_family fam = pcc_conv_route(d, ctx->numerics);
    PCC_REQUIRE(fam != PCC_FAM_GENERIC, "pcc_conv3d_mfma: shape not covered");
    const Packed L = packed_layout(d, p.kind);
    PCC_REQUIRE(!(d->flags & PCC_CONV_OUT16) || p.kind == K_FWD || p.kind == K_TR2 || p.kind == K_CIN1,
                "pcc_conv3d: PCC_CONV_OUT16 needs a layer with Cout a multiple of 16");
    PCC_REQUIRE(!(d->flags & PCC_CONV_OUT16) || d->impl != PCC_IMPL_WINOGRAD, "pcc_conv3d: PCC_CONV_OUT16 is not implemented by the Winograd kernel (fp32)");
    switch (fam) {
        case PCC_FAM_F16:      // fp16 input (and residual), fp16 or fp32 output
            PCC_REQUIRE(p.kind == K_FWD && (d->flags & PCC_CONV_IN16) && pcc_f16_eligible(d),
                        "pcc_conv3d: PCC_CONV_IN16 covers k3 stride-1 layers with Cin = Cout in {16, 32, 64} (H, W multiples of 16) and the 16 -> 1 transposed layer");
            return pcc_conv_f16(ctx, d, in, w_packed + L.f16, bias, residual, out, !(d->flags & PCC_CONV_OUT16), st);
        case PCC_FAM_SPLIT16:
        case PCC_FAM_SPLIT32:
            PCC_REQUIRE(d->Cin >= 32 && pcc_split_covers(d) && !(d->flags & (PCC_CONV_F16 | PCC_CONV_OUT16)), "pcc_conv3d: PCC_IMPL_SPLIT covers fp32 k3 stride-1 layers with Cin = Cout in {32, 64}, W % 16 == 0");
            return pcc_conv_split(ctx, d, fam == PCC_FAM_SPLIT32, in, w_packed + L.split, bias, residual, out, st);
        case PCC_FAM_WINO_F16S: return pcc_conv_wino_f16s(ctx, d, in, w_packed + L.wino_uh, bias, residual, out, ext, st);
        case PCC_FAM_WINO_BF16: return pcc_conv_wino_bf16(ctx, d, in, w_packed + L.wino_ub, bias, residual, out, st);
        case PCC_FAM_WINO: return pcc_conv_wino(ctx, d, in, w_packed + L.wino_u, bias, residual, out, st);
        case PCC_FAM_FWD:
        case PCC_FAM_FWD_F16:
            PCC_REQUIRE(d->impl != PCC_IMPL_WINOGRAD, "%s", L.wino_u ? "pcc_conv3d: PCC_IMPL_WINOGRAD needs W and H multiples of 16"
                                                                     : "pcc_conv3d: PCC_IMPL_WINOGRAD covers Cin = Cout in {16,32,64} k3 stride-1 layers only");
            return pcc_conv_fwd(ctx, d, in, w_packed, bias, residual, out, p.tx, st);
        case PCC_FAM_TR2M_F16: return pcc_conv_tr2m_f16(ctx, d, in, w_packed + L.tr2g, bias, out, st);
        case PCC_FAM_TR2M_F16S: return pcc_conv_tr2m_f16s(ctx, d, in, w_packed + L.tr2_f16s, bias, out, ext, st);
        case PCC_FAM_TR2_SPLIT: return pcc_conv_tr2_split(ctx, d, in, w_packed + L.tr2_split, bias, out, ext, st);
        case PCC_FAM_TR2M_BF16: return pcc_conv_tr2m_bf16(ctx, d, in, w_packed + L.tr2_split, bias, out, ext, st);
        case PCC_FAM_TR2M: return pcc_conv_tr2m(ctx, d, in, w_packed + L.tr2g, bias, out, st);
        case PCC_FAM_TR2: return pcc_conv_tr2(ctx, d, in, w_packed, bias, residual, out, p.tx, st);
        case PCC_FAM_CIN1: return pcc_conv_cin1(ctx, d, in, w_packed, bias, residual, out, ext, st);
        case PCC_FAM_COUT1M: return pcc_conv_cout1_mfma(ctx, d, in, w_packed, bias, residual, out, fuse, fused, st);
        case PCC_FAM_COUT1: return pcc_conv_cout1(ctx, d, in, w_packed, bias, residual, out, st);
        default: break;
    }
    pcc_set_error("pcc_conv3d_mfma: no kernel for family %d", (int)fam);
    return PCC_ERR_ARG;
}

// Gather map of the packed image for pcc_conv_repack_weights_device (train.hip): the segments that are pure reorders of the Keras taps
// -- the base image of every kind (conv_fwd, conv_tr2, conv_cin1, conv_cout1_mfma, conv_cout1) and the tr2g image of the k3 stride-2
// transposed layers -- found by packing an iota kernel (indices + 1 as floats: exact below 2^24; 0 = a zero the packer wrote).
// Every other segment (Winograd U and the bf16 / fp16 piece images) is marked -2: the training context turns those families off.
PCC_API int pcc_conv_repack_map(const pcc_conv_desc* d, int32_t* map) {
    PCC_REQUIRE(d && map, "pcc_conv_repack_map: NULL argument");
    const Plan p = make_plan(d);
    PCC_REQUIRE(p.kind != K_NONE, "pcc_conv_repack_map: shape not covered by the MFMA path");
    const Packed L = packed_layout(d, p.kind);
    const size_t taps = (size_t)d->k * d->k * d->k * d->Cin * d->Cout;
    PCC_REQUIRE(taps < (size_t(1) << 24), "pcc_conv_repack_map: kernel too large for an fp32 iota");
    size_t base_end = L.total;
    for (size_t off : {L.wino_u, L.f16, L.wino_ub, L.split, L.wino_uh, L.tr2g, L.tr2_split, L.tr2_f16s})
        if (off && off < base_end) base_end = off;
    float* iota = (float*)malloc(taps * sizeof(float));
    float* pk = (float*)malloc(L.total * sizeof(float));
    if (!iota || !pk) { free(iota); free(pk); PCC_REQUIRE(false, "pcc_conv_repack_map: out of memory"); }
    for (size_t i = 0; i < taps; ++i) iota[i] = (float)(i + 1);
    const int rc = pcc_conv_pack_weights(d, iota, pk);
    if (rc == PCC_OK)
        for (size_t i = 0; i < L.total; ++i) {
            const bool gathered = i < base_end || (L.tr2g && i >= L.tr2g && i < L.tr2g + (size_t)27 * d->Cin * d->Cout);
            map[i] = gathered ? (int32_t)pk[i] - 1 : -2;
        }
    free(iota);
    free(pk);
    return rc;
}
