// Conv3DTranspose, k = 3, stride 2, 32 -> 16, marching along z, on the bf16 MFMA pipe with fp32-EQUIVALENT operands (round 4).
//
// conv_tr2m_kernel<2> (conv_tr2m.hip) ran the first layer of the last SynthesisBlock (/root/reference/src/model_transforms.py:78:
// 32 -> 16 @32^3 -> 64^3) at 0.67 of the fp32-MFMA peak: 432 fp32 MFMAs per micro-step behind 16 B-operand vectors that are read
// from LDS once.  That structure is what the operand split wants: the 16 operand vectors of a micro-step feed 27 taps x 4 rows x 3 =
// 324 v_mfma_f32_16x16x32_bf16 of 16 cycles instead of 432 x 32: 5.2 k instead of 13.8 k MFMA cycles per micro-step.  The split itself
// happens ONCE PER TILE ELEMENT (late round 4): the tile of the next micro-step travels global -> registers -> split -> LDS in operand
// form (160 bytes per voxel as in conv_split.hip: [dh | dm] x 4 channel quads, [dl | dh] x 4, pad), 5 items per thread, and the 16
// vectors of a lane are 32 plain ds_read_b128.  (First version: the fp32 tile by LDS-direct loads and 8 split blocks per lane and
// micro-step on the 16 vectors -- the same voxel split up to four times, for its two x and two y offsets; 203 -> 173 us of that launch
// were the split, a probe build showed.)  x = h + m + l (three bf16 pieces), terms hh hm mh hl mm lh, fp32
// accumulation in a fixed order, as conv_wino_bf16.hip / conv_split.hip:
//     acc += [Wh | Wm] . [dh | dm];   acc += [Wh | Wm] . [dl | dh];   acc += [Wl | Wh] . [dh | dm]
// The split weights of the cout tile (2 x 27 fragments of 2 KB = 108 KB) stay LDS-resident beside the two-tile ring (40 KB); NG = 4
// (64 -> 32: 216 KB) does not fit and keeps the fp32 kernel / conv_tr2g_kernel.  Everything else -- parity decomposition, three
// accumulator sets, epilogue under the first taps of the next plane, compile-time plane parity -- is conv_tr2m_kernel's (conv_tr2m.hip);
// the code the variants share -- grid, launch, next tile, epilogue schedule, drain -- is in tr2m_common.h.
#include <cstdlib>

#include "tr2m_common.h"

namespace pcctr2mb {

using namespace pcck;
using namespace pcctr2;

constexpr int VSB = 160;                                // bytes per voxel of the operand-form tile: B1 x 4 quads, B2 x 4 quads, 32 pad (10 bank quads:
                                                        // the 8 voxels x 2 quads of a ds_read_b128 lane group fall on 16 different ones)
constexpr int TILE_BYTES = ITEMS * 64 * VSB;            // 51200: 320 voxel slots (289 used; the items past the tile write zeros into the rest)
constexpr int W_BASE = TILE_BYTES;                      // one tile, then the weights
constexpr int ROWB = LXY * VSB;                         // bytes per tile row

struct Tr2mArgs {
    const float* in;
    const float* w;      // split image in conv_tr2g order: [cin group][27 taps, class-major][cout tile][operand][64 lanes][8 bf16]
    const float* bias;
    float* out;
    Tr2mGrid g;
    unsigned* amax_out = nullptr;      // per-block max |out| for the fp16-split layer behind this one (common.h, pcc_conv_ext)
};

template <int NG, bool RELU>
__global__ void __launch_bounds__(NT, 1) conv_tr2m_bf16_kernel(Tr2mArgs a, int nwg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = lane & 15, cq = lane >> 4;
    auto ldsu = [&](unsigned off) -> u32x4 { return *reinterpret_cast<const u32x4*>(smem + off); };
    typedef __attribute__((address_space(3))) void* lds_ptr;

    const Tr2mTile tile = tr2m_tile(a.g, nwg);
    const int ct = tile.ct, n = tile.n, X0 = tile.X0, Y0 = tile.Y0, zb = tile.zb;
    const int nsteps = a.g.zlen + 1;                   // input planes zb-1 .. zb+zlen-1 (the first one only opens output plane 2 zb)
    constexpr int CIN = NG * 16;
    const size_t HW = (size_t)a.g.H * a.g.W;
    const unsigned HWI = (unsigned)(HW * CIN * 4);
    const float* in_n = a.in + (size_t)n * a.g.D * HW * CIN;

    // ---- split weights of this cout tile -> LDS (resident): NG x 27 fragments of 2 KB ([Wh | Wm] then [Wl | Wh]), fragment (g, sq) at
    //      W_BASE + (g * 27 + sq) * 2 KB
    {
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, (unsigned)(NG * 27 * a.g.nct) * 2048u);
        for (int p = wave; p < NG * 27 * 2; p += 4)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(smem + W_BASE + p * 1024), 16, lane * 16, ((p >> 1) * a.g.nct + ct) * 2048 + (p & 1) * 1024, 0, 0);
    }
    // ---- tile staging: global -> registers (one micro-step ahead) -> split -> LDS.  Item it of thread tid = (voxel u, channel quad q) =
    //      ((it * 256 + tid) >> 2, tid & 3); its operands go to u * 160 + q * 16 (B1) and + 64 (B2).  OOB items read zeros.
    // (round 5) the four voxels of 16 consecutive lanes are taken in the order 0, 2, 1, 3: a ds_write_b128 is served in groups of 8 lanes on 32
    // banks, and two voxels 160 B apart overlap in 8 of them (2-way conflicts on every staging write: the 0.10 - 0.18 of the PMC rows) -- 320 B apart
    // they use the other 16 banks
    const int gperm = ((tid >> 2) & ~3) | (((tid >> 2) & 1) << 1) | (((tid >> 2) >> 1) & 1);
    unsigned rel[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = it * NT + tid;
        const int u = it * 64 + gperm, q = item & 3, ly = u / LXY, lx = u - ly * LXY;
        const int y = Y0 - 1 + ly, x = X0 - 1 + lx;
        const bool ok = item < TILE_SLOTS && y >= 0 && y < a.g.H && x >= 0 && x < a.g.W;
        rel[it] = ok ? (unsigned)(((y * a.g.W + x) * CIN + q * 4) * 4) : kOOB;
    }
    const unsigned cw = (unsigned)(gperm * VSB + (tid & 3) * 16);       // item it: cw + it * 64 * VSB
    f32x4 stg[ITEMS];
    // tile of (step sp, cin group cg): `addr` = address of channel 16 cg of input plane zb - 1 + sp (kept incrementally)
    auto fetch_tile = [&](int sp, int cg, unsigned long long addr) __attribute__((always_inline)) {
        const bool ok = (unsigned)(zb - 1 + sp) < (unsigned)a.g.D && sp < nsteps;
        const __amdgpu_buffer_rsrc_t rp = make_rsrc((const void*)(ok ? addr : (unsigned long long)in_n), ok ? HWI - (unsigned)(64 * cg) : 0u);
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) stg[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rp, (int)rel[it], 0, 0));
    };
    // items j, j + 1 (j = 0, 2) or the single item 4: split and written
    auto commit2 = [&](auto j_tag) __attribute__((always_inline)) {
        constexpr int j = decltype(j_tag)::value, j1 = j + 1 < ITEMS ? j + 1 : j;
        u32x4 p1, p2, q1, q2;
        split_items2(p1, p2, q1, q2, stg[j], stg[j1]);
        *reinterpret_cast<u32x4*>(smem + cw + (unsigned)(j * 64 * VSB)) = p1;
        *reinterpret_cast<u32x4*>(smem + cw + (unsigned)(j * 64 * VSB + 64)) = p2;
        if constexpr (j1 != j) {
            *reinterpret_cast<u32x4*>(smem + cw + (unsigned)(j1 * 64 * VSB)) = q1;
            *reinterpret_cast<u32x4*>(smem + cw + (unsigned)(j1 * 64 * VSB + 64)) = q2;
        }
    };

    // ---- B operand addresses: lane (v, cq) reads voxel (row, lx = v + 1 - dx) of the tile, its channel quad cq; one base per x offset,
    //      rows / y offsets and the operand (B2 = + 64) are immediates.  ba[dxi] points at tile row 4 * wave.
    unsigned ba[2];
#pragma unroll
    for (int dxi = 0; dxi < 2; ++dxi) ba[dxi] = (unsigned)((4 * wave * LXY + v + 1 - dxi) * VSB + cq * 16);
    unsigned wa = (unsigned)(W_BASE + lane * 16);      // + cin group * 54 KB (per micro-step), + tap * 2 KB (immediate)

    // ---- epilogue addressing: lane writes couts 4 cq .. 4 cq + 3 (of this cout tile) of output voxel (2 z + pz, 2 y + py, 2 x + px)
    const int OH = 2 * a.g.H, OW = 2 * a.g.W;
    const unsigned ob = (unsigned)((((2 * (Y0 + 4 * wave)) * OW + 2 * (X0 + v)) * a.g.ocs + a.g.oco + 16 * ct + 4 * cq) * 4);
    const unsigned PLANE_O = (unsigned)((size_t)OH * OW * a.g.ocs * 4);          // bytes per output plane (launcher: two planes < 2^31)
    float* out_n = a.out + (size_t)n * (2 * a.g.D) * OH * OW * a.g.ocs;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bias_l = (a.g.flags & PCC_CONV_BIAS) ? *reinterpret_cast<const f32x4*>(a.bias + 16 * ct + 4 * cq) : zero4;

    // ---- prologue
    // (s2, c2, tile_pl): input plane step / cin group / address of the next tile to fetch (wave-uniform)
    int s2 = 0, c2 = 0;
    unsigned long long tile_pl = (unsigned long long)in_n + (unsigned long long)(long long)(zb - 1) * HWI;     // tile of micro-step 0
    auto fetch_next = [&]() __attribute__((always_inline)) {
        fetch_tile(s2, c2, tile_pl);
        tr2m_next_tile<NG, 64>(s2, c2, tile_pl, HWI);
    };
    fetch_next();
    commit2(std::integral_constant<int, 0>{}); commit2(std::integral_constant<int, 2>{}); commit2(std::integral_constant<int, 4>{});
    fetch_next();                                     // raw tile of micro-step 1 waits in registers
    __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0): the weights' LDS-direct loads
    __syncthreads();

    f32x4 E[2][4][4], O[4][4];                        // accumulators [set][class py * 2 + px][row]
    u32x4 b1[2][2][4], b2[2][2][4];                   // split B operands [dyi][dxi][row] of the current micro-step: [dh | dm], [dl | dh]
    u32x4 wf1[3], wf2[3];                             // weight fragment ring, two taps ahead (a tap is 12 MFMAs = 192 cycles: one tap does not cover an LDS read): [Wh | Wm], [Wl | Wh]
    // the 16 operand vectors of the micro-step: 32 plain LDS reads
    auto load_b = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int dyi = 0; dyi < 2; ++dyi)
#pragma unroll
            for (int dxi = 0; dxi < 2; ++dxi)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b1[dyi][dxi][i] = ldsu(ba[dxi] + (unsigned)((i + 1 - dyi) * ROWB));
                    b2[dyi][dxi][i] = ldsu(ba[dxi] + (unsigned)((i + 1 - dyi) * ROWB + 64));
                }
    };
    auto load_w = [&](int slot, int sq) __attribute__((always_inline)) {
        wf1[slot] = ldsu(wa + (unsigned)(sq * 2048));
        wf2[slot] = ldsu(wa + (unsigned)(sq * 2048 + 1024));
    };
    load_b();
    load_w(0, tap_of(18).sq); load_w(1, tap_of(19).sq);      // step 0 is the halo plane: its first tap is 18 (ring slot = (t - T0) % 3)

    // wave-uniform march state
    int s = 0, c = 0;                                 // input plane step / cin group of the current micro-step
    unsigned long long out_pl = (unsigned long long)out_n + (unsigned long long)(long long)(2 * (zb - 2)) * PLANE_O;   // planes 2 (z - 1), 2 (z - 1) + 1 of step s = 0

    float mx = 0.f, mxt = 0.f;      // max |stored value|: all planes so far / the plane pair in flight (dropped with its stores when s < 2)
    // epilogue item e of a finished plane pair: e < 16: odd set (pz = 1), class e >> 2, row e & 3; else the old even_cur (pz = 0)
    auto finish = [&](auto ph_tag, auto e_tag, const __amdgpu_buffer_rsrc_t& rout, f32x4& keep) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph_tag)::value, e = decltype(e_tag)::value;
        constexpr int pz = e < 16 ? 1 : 0, cls = (e >> 2) & 3, i = e & 3, py = cls >> 1, px = cls & 1;
        f32x4 o = acc_read(pz ? O[cls][i] : E[PH ^ 1][cls][i]);
        if (RELU) o = __builtin_elementwise_maximum(o, zero4);
        keep = o;
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(mxt) : "v"(o[0]), "v"(o[1]));
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(mxt) : "v"(o[2]), "v"(o[3]));
        const unsigned soff = (unsigned)pz * PLANE_O + (unsigned)(((2 * i + py) * OW + px) * a.g.ocs * 4);
        buf_store4(rout, keep, ob, soff);
    };

    // HALO: the slab's first input plane (zb - 1) only contributes its kz = 2 taps (to output plane 2 zb): 9 taps instead of 27
    auto micro = [&](auto ph_tag, auto first_tag, auto halo_tag) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value, HALO = decltype(halo_tag)::value;
        constexpr int T0 = HALO ? 18 : 0;
        // FIRST: the planes finished by the previous input plane leave under the first taps (zero-sized: stores dropped, s < 2)
        const bool prev_ok = s >= 2;
        const __amdgpu_buffer_rsrc_t rout = make_rsrc((const void*)(prev_ok ? out_pl : (unsigned long long)out_n), FIRST && prev_ok ? 2u * PLANE_O : 0u);
        f32x4 ost[2][3];
        static_for(std::make_integer_sequence<int, 27 - T0>{}, [&](auto t_tag) __attribute__((always_inline)) {
            constexpr int t = decltype(t_tag)::value + T0;
            constexpr Tap T = tap_of(t);
            // weight fragment of the next tap (wraps to tap 0 of the next micro-step: loaded after the barrier instead)
            if constexpr (t + 2 < 27) load_w((t + 2 - T0) % 3, tap_of(t + 2).sq);
            constexpr bool open = FIRST && T.opens && T.kz != 0;     // first tap of a class of the odd / even_next set in this plane
            // three MFMAs per row, term outermost: a dependent MFMA is four issue slots away
#pragma unroll
            for (int tm = 0; tm < 3; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f32x4& acc = T.kz == 0 ? E[PH][T.cls][i] : T.kz == 1 ? O[T.cls][i] : E[PH ^ 1][T.cls][i];
                    acc = mfma_bf16(tm == 2 ? wf2[(t - T0) % 3] : wf1[(t - T0) % 3], tm == 1 ? b2[T.dyi][T.dxi][i] : b1[T.dyi][T.dxi][i], (open && tm == 0) ? bias_l : acc);
                }
#ifndef PCC_TR2MB_INTERLEAVE
            __builtin_amdgcn_sched_barrier(0);
#endif
            // the tile of the NEXT micro-step (raw, in registers since the previous micro-step) replaces this one in LDS.  Every wave read
            // its 16 vectors before tap T0: the barrier behind that tap -- where the waves are still close together -- orders the
            // overwrite behind those reads; split + writes + the request for the tile after next run behind the last tap.  (Measured,
            // min of bench_one on one box: this placement 182 - 185 us, barrier and blocks all behind the last tap 187 - 190, the three
            // split blocks spread over taps T0 + 3 .. 5 220 - 228 -- their LDS writes sit between the weight-fragment reads of the
            // ring, which return in order -- against 202 - 206 for the version that split the 16 vectors per micro-step.)
            if constexpr (t == T0) __syncthreads();
            if constexpr (t == 26) {
                commit2(std::integral_constant<int, 0>{}); commit2(std::integral_constant<int, 2>{}); commit2(std::integral_constant<int, 4>{});
                fetch_next();
            }
            if constexpr (FIRST && !HALO) tr2m_finish_under_tap<t>(finish, ph_tag, rout, ost);
            __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (FIRST && !HALO) { mx = fmaxf(mx, prev_ok ? mxt : 0.f); mxt = 0.f; }
        // the operand-form tile of the next micro-step is complete in LDS (this wave's ds_writes: lgkmcnt; the others': barrier)
        __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0); vmcnt / expcnt untouched (stores and the raw loads stay in flight)
        __syncthreads();
        // ---- advance (wave-uniform) and fetch the operands of the next micro-step
        if (++c == NG) { c = 0; ++s; out_pl += 2ull * PLANE_O; wa -= (unsigned)((NG - 1) * 27 * 2048); } else wa += 27u * 2048u;
        load_b();
        // first weight fragment of the next micro-step (buffer parity follows its first tap: 0, or 18 inside the halo plane)
        if (s == 0) { load_w(0, tap_of(18).sq); load_w(1, tap_of(19).sq); }
        else { load_w(0, tap_of(0).sq); load_w(1, tap_of(1).sq); }
    };
    // one input plane = NG micro-steps, unrolled (a run-time loop over the middle ones made the register allocator shuttle the
    // accumulators between AccVGPRs and VGPRs at the loop boundary)
    auto plane = [&](auto ph_tag, auto halo_tag) __attribute__((always_inline)) {
        micro(ph_tag, std::true_type{}, halo_tag);
#pragma unroll
        for (int k = 1; k < NG; ++k) micro(ph_tag, std::false_type{}, halo_tag);
    };
    // the plane loop is written out in every variant: as a shared function template it compiles to other code (note in tr2m_common.h)
    plane(std::integral_constant<int, 0>{}, std::true_type{});          // step 0: the halo plane
#pragma nounroll
    for (int sp = 1; sp < nsteps; sp += 2) {
        plane(std::integral_constant<int, 1>{}, std::false_type{});
        if (sp + 1 < nsteps) plane(std::integral_constant<int, 0>{}, std::false_type{});
    }
    // ---- drain: the planes finished by the last input plane (s == nsteps here; tr2m_common.h on the parity, the branch and keep[])
    {
        const __amdgpu_buffer_rsrc_t rout = make_rsrc((const void*)out_pl, nsteps >= 2 ? 2u * PLANE_O : 0u);
        f32x4 keep[32];
        if (nsteps & 1) tr2m_drain<1>(finish, rout, keep);
        else tr2m_drain<0>(finish, rout, keep);
#pragma unroll
        for (int e = 0; e < 32; ++e) asm volatile("" ::"v"(keep[e]));
        mx = fmaxf(mx, nsteps >= 2 ? mxt : 0.f);
    }
    // ---- max |out| of block n for the fp16-split layer behind this one (conv_wino_f16s.hip): atomicMax of non-negative fp32 bit patterns
    if (a.amax_out != nullptr) pcc_amax_record(a.amax_out + (size_t)n * PCC_AMAX_SLOTS, mx, (int)blockIdx.x * 4 + wave);
}

}  // namespace pcctr2mb

using namespace pcctr2mb;

// ---- host: split image of the class-major weights.  w_tr2g: [cin group][27][cout tile][64 lanes][4 floats] (conv_tr2g order, fp32)
//      -> out: [cin group][27][cout tile][operand][64 lanes][8 bf16]; operand 0 = [Wh | Wm], 1 = [Wl | Wh]
size_t pcc_tr2m_bf16_packed_floats(int Cin, int Cout) { return (size_t)(Cin / 16) * 27 * (Cout / 16) * 2 * 64 * 4; }
void pcc_tr2m_bf16_pack(int Cin, int Cout, const float* w_tr2g, float* out) {
    unsigned short* o = reinterpret_cast<unsigned short*>(out);
    const size_t nfrag = (size_t)(Cin / 16) * 27 * (Cout / 16);
    for (size_t f = 0; f < nfrag; ++f)
        for (int lane = 0; lane < 64; ++lane) {
            unsigned short h[4], m[4], l[4];
            for (int c = 0; c < 4; ++c) {
                const float x = w_tr2g[(f * 64 + lane) * 4 + c];
                bf16_split3(x, h[c], m[c], l[c]);
            }
            unsigned short* a1 = o + ((f * 2 + 0) * 64 + lane) * 8;
            unsigned short* a2 = o + ((f * 2 + 1) * 64 + lane) * 8;
            for (int c = 0; c < 4; ++c) { a1[c] = h[c]; a1[4 + c] = m[c]; a2[c] = l[c]; a2[4 + c] = h[c]; }
        }
}

// the split kernel covers the 32 -> 16 layer (its 108 KB of split weights fit LDS beside the tile ring); shape-only rule
bool pcc_tr2m_bf16_covers(const pcc_conv_desc* d) { return pcc_tr2m_eligible(d) && d->Cin == 32 && d->Cout == 16; }

int pcc_conv_tr2m_bf16(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w_split, const float* bias, float* out,
                       pcc_conv_ext* ext, hipStream_t st) {
    PCC_REQUIRE(pcc_tr2m_bf16_covers(d), "pcc_conv_tr2m_bf16: shape not covered");
    Tr2mArgs a;
    a.in = in; a.w = w_split; a.bias = bias; a.out = out;
    if (ext && ext->out_amax) { a.amax_out = ext->out_amax; ext->out_recorded = true; }
    const int nwg = tr2m_grid(ctx, d, a.g);
    const int lds = W_BASE + 2 * 27 * 2048;
    typedef void (*kern_t)(Tr2mArgs, int);
    const kern_t kern = (d->flags & PCC_CONV_RELU) ? (kern_t)conv_tr2m_bf16_kernel<2, true> : (kern_t)conv_tr2m_bf16_kernel<2, false>;
    return tr2m_launch(kern, lds, nwg, a, st);
}
