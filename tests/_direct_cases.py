"""The table of the direct exact-fp32 conv kernels, their fp16-MFMA twins and the fp16-storage kernels (tests/test_direct_cases_cpu.py,
tests/test_direct_exact_gpu.py): one row per kernel instantiation that launch_fwd, launch_tr2, pcc_conv_cin1, pcc_conv_cout1_mfma (fp32
and fp16 input), pcc_conv_cout1, pcc_conv_tr2m, pcc_conv_f16, pcc_conv_tr2m_f16 and the generic kernel can select, on the smallest grid
that gives the instantiation a partial tile or, for the kernels that march whole columns along z, its edges in z (SAME padding, slab
seams); the launchers' choices restated as plain Python (`select`); integer inputs on which every fp32 summation order gives the
float64 value bit for bit; and the references.  The four instantiations of conv_cout1_mfma_kernel with the threshold-fusing epilogue
are listed here (INSTANCES, `select` with flags['thr']) and launched through the codec graph by tests/test_thr_fuse_gpu.py on the cases
of tests/_thr_ref.py: pcc_thr_fuse has no export of its own.

Exactness.  Set A (fp32 rows): x integers of [-3, 3], w and bias integers of [-2, 2] times 2^e per OUTPUT channel (e in [-6, 6]),
residual integers of [-3, 3].  Every term of one output carries the same power of two, so each product and partial sum is an integer
multiple of 2^min(e, 0) and, while the sum of |terms| in those units stays below 2^24, a float32.  Set B (fp16-MFMA and fp16-storage
rows): x in {0, 1}, w and bias in {-1, 0, 1}, residual integers of [-2, 2]: exact in fp16, the products accumulate in fp32; with an
fp16 output the results must stay within +-2048, where fp16 holds every integer (at most 27 x 64 + 1 + 2 = 1731), and so must the raw
fp16 partial sums that the first launch of a 64-channel conv_f16 layer leaves for the second (at most 27 x 32 = 864).
tests/test_direct_cases_cpu.py asserts all of these per row.

Importing this module needs numpy only.
"""
import functools
import zlib

import numpy as np

import _family_cases as FC

# ---- the instantiations, one block per launcher, spelled with every template argument (csrc/conv_fwd.hip, conv_tr2.hip, conv_edge.hip,
# conv_tr2m.hip, conv_generic.hip).  conv_fwd_kernel<CIN,COUT,KS,S,TX,TZ,TY,TXT,R,CTW>, conv16_pers_kernel<TZ,TY,R,VS,WGS_PER_CU>,
# conv_tr2_kernel<CIN,COUT,KS,TX,TZ,TY,TXT,R,CTW>, conv_tr2g_kernel<CIN,COUT,TX,TZ,TY,TXT,R,CTW,F16,EPI>.
_FWD = """
conv16_pers_kernel<2,4,2,20,2> conv16_pers_kernel<2,8,2,20,1>
conv_fwd_kernel<16,16,3,1,8,2,8,8,2,1> conv_fwd_kernel<16,16,3,1,4,4,4,4,1,1>
conv_fwd_kernel<32,32,3,1,16,2,8,16,4,2> conv_fwd_kernel<32,32,3,1,8,2,8,8,2,2> conv_fwd_kernel<32,32,3,1,4,1,4,4,1,1>
conv_fwd_kernel<64,64,3,1,16,2,8,16,4,4> conv_fwd_kernel<64,64,3,1,16,2,4,16,2,4> conv_fwd_kernel<64,64,3,1,8,2,4,8,1,1>
conv_fwd_kernel<64,64,3,1,4,1,4,4,1,1>
conv_fwd_kernel<16,32,3,2,16,2,2,16,1,2> conv_fwd_kernel<16,32,3,2,8,2,4,8,1,2> conv_fwd_kernel<16,32,3,2,4,1,4,4,1,1>
conv_fwd_kernel<32,32,3,2,16,2,2,16,1,2> conv_fwd_kernel<32,32,3,2,8,2,4,8,1,2> conv_fwd_kernel<32,32,3,2,4,1,4,4,1,1>
conv_fwd_kernel<32,64,3,2,16,2,2,16,1,4> conv_fwd_kernel<32,64,3,2,8,2,4,8,1,4> conv_fwd_kernel<32,64,3,2,4,1,4,4,1,1>
conv_fwd_kernel<64,64,3,2,16,2,2,16,1,4> conv_fwd_kernel<64,64,3,2,8,2,4,8,1,4> conv_fwd_kernel<64,64,3,2,4,1,4,4,1,1>
conv_fwd_kernel<32,32,5,2,16,1,2,16,1,2> conv_fwd_kernel<32,32,5,2,8,1,4,8,1,2> conv_fwd_kernel<32,32,5,2,4,4,4,4,1,2>
"""
# the fp16-MFMA twin of 16 -> 16 at row width 16 has no fp32 launch: the persistent kernel takes the fp32 layer
_FWD_F16_ONLY = 'conv_fwd_kernel<16,16,3,1,16,2,8,16,4,1,true>'
_TR2 = """
conv_tr2_kernel<64,64,3,4,1,4,4,1,1> conv_tr2_kernel<64,32,3,4,1,4,4,1,1> conv_tr2_kernel<32,16,3,4,4,4,4,1,1>
conv_tr2_kernel<32,32,3,4,1,4,4,1,1>
conv_tr2_kernel<64,64,3,16,2,4,16,2,4> conv_tr2_kernel<64,32,3,16,2,4,16,2,2> conv_tr2_kernel<32,16,3,16,2,8,16,4,1>
conv_tr2_kernel<32,32,3,16,2,8,16,4,2>
conv_tr2_kernel<64,64,3,8,2,4,8,1,1> conv_tr2_kernel<64,32,3,8,2,8,8,2,2> conv_tr2_kernel<32,16,3,8,2,8,8,2,1>
conv_tr2_kernel<32,32,3,8,2,8,8,2,2>
conv_tr2_kernel<32,32,5,16,2,8,16,4,2> conv_tr2_kernel<32,32,5,8,2,8,8,2,2> conv_tr2_kernel<32,32,5,4,4,4,4,1,2>
"""
_TR2G = """
conv_tr2g_kernel<64,64,16,2,4,16,2,2,false,TR2G_EPI_F32> conv_tr2g_kernel<64,64,16,2,4,16,2,2,false,TR2G_EPI_ANY>
conv_tr2g_kernel<64,32,16,2,4,16,2,2,false,TR2G_EPI_F32> conv_tr2g_kernel<64,32,16,2,4,16,2,2,false,TR2G_EPI_ANY>
conv_tr2g_kernel<32,16,16,2,8,16,4,1,false,TR2G_EPI_F32> conv_tr2g_kernel<32,16,16,2,8,16,4,1,false,TR2G_EPI_ANY>
conv_tr2g_kernel<32,32,16,2,8,16,4,1,false,TR2G_EPI_F32> conv_tr2g_kernel<32,32,16,2,8,16,4,1,false,TR2G_EPI_ANY>
conv_tr2g_kernel<64,64,8,2,4,8,1,1,false,TR2G_EPI_F32> conv_tr2g_kernel<64,64,8,2,4,8,1,1,false,TR2G_EPI_ANY>
conv_tr2g_kernel<64,32,8,2,8,8,2,1,false,TR2G_EPI_F32> conv_tr2g_kernel<64,32,8,2,8,8,2,1,false,TR2G_EPI_ANY>
conv_tr2g_kernel<32,16,8,2,8,8,2,1,false,TR2G_EPI_F32> conv_tr2g_kernel<32,16,8,2,8,8,2,1,false,TR2G_EPI_ANY>
conv_tr2g_kernel<32,32,8,2,8,8,2,1,false,TR2G_EPI_F32> conv_tr2g_kernel<32,32,8,2,8,8,2,1,false,TR2G_EPI_ANY>
"""
_TR2M = 'conv_tr2m_kernel<2,false> conv_tr2m_kernel<2,true> conv_tr2m_kernel<4,false> conv_tr2m_kernel<4,true>'
_CIN1 = 'conv_cin1_kernel<16,3,2,8,4> conv_cin1_kernel<32,3,2,8,4> conv_cin1_kernel<16,9,2,8,4> conv_cin1_kernel<32,9,2,8,4>'
_COUT1M = 'conv_cout1_mfma_kernel<false,16,false> conv_cout1_mfma_kernel<false,32,false>'
# conv_cout1_kernel<16,3,1,4,8,8> is compiled and unreachable: make_plan sends Cin = 16 to conv_cout1_mfma_kernel
_COUT1 = 'conv_cout1_kernel<32,3,1,4,8,8> conv_cout1_kernel<32,9,2,2,8,8>'
_GENERIC = 'conv_fwd_generic conv_tr_generic'
# ---- fp16 storage (csrc/conv_f16.hip, conv_tr2m_f16.hip) and the IN16 / THR variants of the 16 -> 1 layer (conv_edge.hip).
# conv_f16_kernel<C,OUT32,SUB>: <32,.,true> is the 64-channel layer, two launches with raw fp16 partial sums in between;
# conv_tr2m_f16_kernel<NG,RELU>; conv_cout1_mfma_kernel<IN16,T,THR>
_F16 = """
conv_f16_kernel<16,false,false> conv_f16_kernel<16,true,false> conv_f16_kernel<32,false,false> conv_f16_kernel<32,true,false>
conv_f16_kernel<32,false,true> conv_f16_kernel<32,true,true>
"""
_TR2M_F16 = 'conv_tr2m_f16_kernel<1,true> conv_tr2m_f16_kernel<1,false> conv_tr2m_f16_kernel<2,true> conv_tr2m_f16_kernel<2,false>'
_COUT1M_IN16 = 'conv_cout1_mfma_kernel<true,16,false> conv_cout1_mfma_kernel<true,32,false>'
# the threshold-fusing epilogue exists inside the codec graph only (pcc_thr_fuse has no export): its rows are the cases of
# tests/_thr_ref.py, launched by tests/test_thr_fuse_gpu.py through ops.codec_encode / ops.codec_decode_main
_COUT1M_THR = """
conv_cout1_mfma_kernel<false,16,true> conv_cout1_mfma_kernel<false,32,true> conv_cout1_mfma_kernel<true,16,true>
conv_cout1_mfma_kernel<true,32,true>
"""


def _twin(name):
    """The fp16-MFMA twin (template argument F16 = true) of a conv_fwd_kernel / conv_tr2_kernel / conv_tr2g_kernel name."""
    if name.startswith('conv_tr2g_kernel'):
        return name.replace(',false,', ',true,')
    return name[:-1] + ',true>'


INSTANCES = {
    'launch_fwd': _FWD.split(),
    'launch_fwd (PCC_CONV_F16)': [_twin(n) for n in _FWD.split() if n.startswith('conv_fwd_kernel')] + [_FWD_F16_ONLY],
    'launch_tr2': _TR2.split() + _TR2G.split(),
    'launch_tr2 (PCC_CONV_F16)': [_twin(n) for n in _TR2.split() + _TR2G.split()] +
                                 [_twin(n).replace('TR2G_EPI_F32', 'TR2G_EPI_F16') for n in _TR2G.split() if 'EPI_F32' in n],
    'pcc_conv_tr2m': _TR2M.split(),
    'pcc_conv_cin1': _CIN1.split(),
    'pcc_conv_cout1_mfma': _COUT1M.split(),
    'pcc_conv_cout1': _COUT1.split(),
    'pcc_conv3d_generic': _GENERIC.split(),
    'pcc_conv_f16': _F16.split(),
    'pcc_conv_tr2m_f16': _TR2M_F16.split(),
    'pcc_conv_cout1_mfma (PCC_CONV_IN16)': _COUT1M_IN16.split(),
    'pcc_conv_cout1_mfma (pcc_thr_fuse)': _COUT1M_THR.split(),
}
GRAPH_ONLY = INSTANCES['pcc_conv_cout1_mfma (pcc_thr_fuse)']      # no row here: the cases of tests/_thr_ref.py
UNREACHABLE = ['conv_cout1_kernel<16,3,1,4,8,8>']
ALL_INSTANCES = [n for block in INSTANCES.values() for n in block]
assert len(set(ALL_INSTANCES)) == len(ALL_INSTANCES)
assert [len(v) for v in INSTANCES.values()] == [26, 25, 31, 39, 4, 4, 2, 2, 2, 6, 4, 2, 4] and len(ALL_INSTANCES) == 135 + 16

CPU_NUM_CU = 256          # what the CPU tests restate the launchers for: the MI355X


# ---- the launchers' choices, restated -----------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def flags_of(row):
    m = row['mode']
    return dict(f16=m != 'fp32', in16=m.startswith('in16'), out16=m in ('out16', 'in16-out16'), res=bool(row['res']),
                clip=bool(row.get('clip')), thr=bool(row.get('thr')))


def out_dims(geo):
    N, D, H, W, cin, cout, k, s, tr = geo
    return tuple(n * s for n in (D, H, W)) if tr else tuple(_cdiv(n, s) for n in (D, H, W))


def base_dims(geo):
    """The grid the 16-voxel rows live on: the input grid of a transposed layer, the output grid of a forward one."""
    return tuple(geo[1:4]) if geo[8] else out_dims(geo)


def _sel(kernel, tile=None, ntiles=None, slots=None, **more):
    """tile: (TZ, TY, TXT) voxels of the base grid per workgroup (None: no tile); ntiles / slots: of a persistent kernel."""
    return dict(kernel=kernel, tile=tile, ntiles=ntiles, slots=slots, **more)


def _fwd_name(cin, cout, k, s, t, f16):
    return 'conv_fwd_kernel<%d,%d,%d,%d,%s%s>' % (cin, cout, k, s, ','.join(map(str, t)), ',true' if f16 else '')


def _tr2_name(cin, cout, k, t, f16):
    return 'conv_tr2_kernel<%d,%d,%d,%s%s>' % (cin, cout, k, ','.join(map(str, t)), ',true' if f16 else '')


def select(desc, flags, switches, num_cu):
    """The kernel instantiation pcc_conv3d launches for a row (desc: anything with 'geo' and 'impl'; flags: flags_of; switches: the
    numerics switches set), its voxel tile and, for a persistent kernel, its tile count and workgroup slots."""
    N, D, H, W, cin, cout, k, s, tr = desc['geo']
    sw = lambda name: bool(switches.get(name))
    f16, out16 = flags['f16'], flags['out16']
    plain = not (flags['res'] or flags['clip'])
    od, oh, ow = out_dims(desc['geo'])
    if desc['impl'] == 'GENERIC':                                      # conv_generic.hip:127 (d->transposed)
        return _sel('conv_tr_generic' if tr else 'conv_fwd_generic')
    if not tr and cin == 1:                                            # conv_route.hip:28 make_plan -> K_CIN1; conv_edge.hip:503
        assert s == 2 and k in (3, 9) and cout in (16, 32) and ow % 16 == 0 and not (D % 2 or H % 2 or W % 2)
        return _sel('conv_cin1_kernel<%d,%d,2,8,4>' % (cout, k), (2, 8, 16))
    in16 = bool(flags.get('in16'))
    if tr and cout == 1:
        if s == 1 and k == 3 and cin == 16:                            # conv_route.hip:33 -> K_COUT1M (:252: also with fp16 input)
            t16 = sw('cout1_t16')                                      # conv_edge.hip:513
            # conv_edge.hip:515-517: fp16 input; the occupancy bits ride along when the caller asked for them (pcc_thr_fuse), the
            # output is dense and whole 16-voxel rows map to whole mask pieces
            thr = bool(flags.get('thr')) and not desc.get('ocs') and W % 16 == 0 and (H * W) % 32 == 0
            name = 'conv_cout1_mfma_kernel<%s,%%d,%s>' % ('true' if in16 else 'false', 'true' if thr else 'false')
            if not t16 and H % 32 == 0 and W % 32 == 0:                # conv_edge.hip:520
                base, zsp = N * (H // 32) * (W // 32), 1
                while base * zsp < num_cu and D // (zsp * 2) >= 16:    # conv_edge.hip:523
                    zsp *= 2
                if base * zsp >= num_cu:                               # conv_edge.hip:524
                    return _sel(name % 32, (D, 32, 32), zsp=zsp, fused=thr)                 # conv_edge.hip:527-529
            return _sel(name % 16, (D, 16, 16), zsp=1, fused=thr)                           # conv_edge.hip:532-536
        assert not in16, 'conv_route.hip:252: fp16 input on a 32 -> 1 layer goes to pcc_conv_f16, which refuses it'
        assert cin == 32 and W % 8 == 0 and (k, s) in ((3, 1), (9, 2))          # conv_route.hip:34-35 -> K_COUT1
        return _sel('conv_cout1_kernel<32,%d,%d,%s>' % (k, s, '4,8,8' if s == 1 else '2,8,8'), (4, 8, 8) if s == 1 else (2, 8, 8))
    bw = W if tr else ow                                               # conv_route.hip:17 base_w
    assert bw % 16 == 0 or bw in (8, 4)
    tx = 16 if bw % 16 == 0 else bw                                    # conv_route.hip:41
    nct = cout // 16
    if in16:
        # conv_route.hip:252 -> PCC_FAM_F16, :328 and pcc_f16_eligible (conv_f16.hip:287-294): k3 stride 1 (a transposed layer through
        # flipped taps), Cin = Cout in {16, 32, 64}, H and W multiples of 16, a dense output; pcc_conv3d admits fp16 storage under AUTO only
        assert desc['impl'] == 'AUTO' and s == 1 and k == 3 and cin == cout and cin in (16, 32, 64) and H % 16 == 0 and W % 16 == 0
        assert not desc.get('ocs') and not desc.get('oco')
        sub = cin == 64                                                # conv_f16.hip:335: two launches of the 32-channel kernel
        C = 32 if sub else cin                                         # conv_f16.hip:355-366
        ty = 16 if cin == 16 else 8                                    # conv_f16.hip:339
        base, zs = N * (H // ty) * (W // 16) * (2 if sub else 1), 1    # conv_f16.hip:342
        while base * zs < num_cu and D % (zs * 2) == 0 and D // (zs * 2) >= 4:              # conv_f16.hip:346
            zs *= 2
        while base * zs < 2 * num_cu and D % (zs * 2) == 0 and D // (zs * 2) >= 8:          # conv_f16.hip:347
            zs *= 2
        return _sel('conv_f16_kernel<%d,%s,%s>' % (C, 'false' if out16 else 'true', 'true' if sub else 'false'), (D // zs, ty, 16),
                    zsplit=zs, zlen=D // zs, nwg=base * zs, launches=2 if sub else 1)       # conv_f16.hip:348-349
    if tr and s == 2:
        # conv_route.hip:260-261 and pcc_tr2m_f16_covers (conv_tr2m_f16.hip:237-241, tr2m_shape_ok of tr2m_common.h:134-143): under AUTO
        # the fp16 mode with fp16 hand-over marches along z unless no_tr2m is set; bias / ReLU only, offsets in multiples of 4
        if (k == 3 and desc['impl'] == 'AUTO' and not sw('no_tr2m') and f16 and out16 and plain and (cin, cout) in ((32, 16), (64, 32))
                and H % 16 == 0 and W % 16 == 0 and (desc.get('ocs') or cout) % 4 == 0 and (desc.get('oco') or 0) % 4 == 0):
            base, zs = N * (H // 16) * (W // 16) * nct, 1              # tr2m_common.h:105-110
            while base * zs < num_cu and D % (zs * 2) == 0 and D // (zs * 2) >= 4:
                zs *= 2
            return _sel('conv_tr2m_f16_kernel<%d,%s>' % (cin // 32, 'true' if desc['relu'] else 'false'), (D // zs, 16, 16),
                        zsplit=zs, zlen=D // zs)                       # conv_tr2m_f16.hip:249-254
        # conv_route.hip:257-270: the z march where it is eligible and wanted, else the tiled kernels
        march = (k == 3 and not sw('no_tr2m') and not f16 and plain and (cin, cout) in ((32, 16), (64, 32)) and H % 16 == 0
                 and W % 16 == 0 and (sw('tr2m') or cin == 32 or D >= 32))
        if march:
            assert sw('no_split'), 'without no_split the march is a split family: outside this table'
            return _sel('conv_tr2m_kernel<%d,%s>' % (cin // 16, 'true' if desc['relu'] else 'false'), (D, 16, 16))  # conv_tr2m.hip:234
        if tx == 16:
            t = (16, 2, 4, 16, 2) if cin >= 64 else (16, 2, 8, 16, 4)                        # conv_tr2.hip:489-491
            g_ctw = 2 if cin >= 64 else 1
        elif tx == 8:
            t = (8, 2, 4, 8, 1) if cout >= 64 and k == 3 else (8, 2, 8, 8, 2)                # conv_tr2.hip:494-496
            g_ctw = 1
        if tx in (16, 8) and k == 3 and not sw('tr2_old'):             # conv_tr2.hip:487-489, :494: conv_tr2g_kernel
            assert od * oh * ow * (desc.get('ocs') or cout) * 4 < 2 ** 31 and max(D, H, W) < 512         # conv_tr2.hip:472
            if f16:                                                    # conv_tr2.hip:479-482
                epi = 'TR2G_EPI_F16' if plain and out16 else ('TR2G_EPI_F32' if plain else 'TR2G_EPI_ANY')
            else:                                                      # conv_tr2.hip:484-485
                epi = 'TR2G_EPI_F32' if plain else 'TR2G_EPI_ANY'
            TX, TZ, TY, TXT, R = t
            waves = TZ * ((TY // (16 // TX)) // R) * (TXT // TX) * (nct // g_ctw)            # Tr2gCfg::NW
            return _sel('conv_tr2g_kernel<%d,%d,%s,%d,%s,%s>' % (cin, cout, ','.join(map(str, t)), g_ctw, 'true' if f16 else 'false', epi),
                        (TZ, TY, TXT), N * _cdiv(D, TZ) * _cdiv(H, TY) * _cdiv(W, TXT), num_cu * (1 if waves * 64 > 256 else 2))  # :477
        if tx in (16, 8):
            ctw = 1 if (tx == 8 and cout >= 64 and k == 3) else nct    # conv_tr2.hip:495: PCC_TR2C(8, 2, 4, 8, 1, 1)
        elif cout >= 32 and k == 3:                                    # conv_tr2.hip:500
            t, ctw = (4, 1, 4, 4, 1), 1
        else:                                                          # conv_tr2.hip:501
            t, ctw = (4, 4, 4, 4, 1), nct
        return _sel(_tr2_name(cin, cout, k, t + (ctw,), f16), t[1:4])
    # ---- launch_fwd (conv_fwd.hip:470): forward, and transposed stride 1 through flipped weights
    if s == 1:
        if tx == 16:
            if cout >= 64:                                             # conv_fwd.hip:486-494: the tile that fills the CU slots best
                vox = N * od * oh * ow
                wg_small, wg_big = vox // 128, vox // 256
                t_small = (wg_small + 3 * num_cu - 1) // (3 * num_cu) * 1.0
                t_big = (wg_big + 2 * num_cu - 1) // (2 * num_cu) * 2.0
                big = t_big <= t_small
                t, ctw = ((16, 2, 8, 16, 4) if big else (16, 2, 4, 16, 2)), nct
            elif cout == 16 and cin == 16 and k == 3 and not f16:      # conv_fwd.hip:496-507: the persistent kernel
                TZ, TY, wpc = (2, 8, 1) if sw('p16') else (2, 4, 2)
                return _sel('conv16_pers_kernel<%d,%d,2,20,%d>' % (TZ, TY, wpc), (TZ, TY, 16),
                            N * _cdiv(od, TZ) * _cdiv(oh, TY) * _cdiv(ow, 16), num_cu * wpc)
            else:                                                      # conv_fwd.hip:510
                t, ctw = (16, 2, 8, 16, 4), nct
        elif tx == 8:                                                  # conv_fwd.hip:513-516
            t, ctw = ((8, 2, 4, 8, 1), 1) if cout >= 64 else ((8, 2, 8, 8, 2), nct)
        else:                                                          # conv_fwd.hip:517-518
            t, ctw = ((4, 1, 4, 4, 1), 1) if cout >= 32 else ((4, 4, 4, 4, 1), nct)
    elif k == 3:                                                       # conv_fwd.hip:519-523
        if tx == 16:
            t, ctw = (16, 2, 2, 16, 1), nct
        elif tx == 8:
            t, ctw = (8, 2, 4, 8, 1), nct
        else:
            t, ctw = ((4, 1, 4, 4, 1), 1) if cout >= 32 else ((4, 4, 4, 4, 1), nct)
    else:                                                              # conv_fwd.hip:524-528 (k5)
        t, ctw = {16: (16, 1, 2, 16, 1), 8: (8, 1, 4, 8, 1), 4: (4, 4, 4, 4, 1)}[tx], nct
    return _sel(_fwd_name(cin, cout, k, s, t + (ctw,), f16), t[1:4])


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
BASE = {16: (3, 9, 32), 8: (3, 9, 8), 4: (5, 6, 4)}       # base grids per row width: partial tiles in z and y, rows across the y edge
N_BASE = 2
BARE = dict(bias=False, relu=False, res=False, clip=False)
NORES = dict(bias=True, relu=True, res=False, clip=False)
FULL = dict(bias=True, relu=True, res=True, clip=False)
FULLCLIP = dict(bias=True, relu=True, res=True, clip=True)
NORESCLIP = dict(bias=True, relu=True, res=False, clip=True)


def _row(rid, fam, kernel, geo, impl, switches, mode, epi, off, group='base', oco=8):
    cout = geo[5]
    r = FC._case(rid, fam, geo, impl, switches, mode, tol=0.0, ocs=cout + 8 if off else 0, oco=oco if off else 0, **epi)
    r.update(kernel=kernel, group=group, set='A' if mode == 'fp32' else 'B')
    return r


def _geo(cin, cout, k, s, tr, base, n=N_BASE):
    dims = base if (tr or s == 1) else tuple(2 * b for b in base)     # a forward stride-2 layer takes twice the base grid
    return (n,) + tuple(dims) + (cin, cout, k, s, int(tr))


# (cin, cout, k, stride) -> {row width: (TX, TZ, TY, TXT, R, CTW) | 'pers'} as the launcher's comments and macros give them
_FWD_TILES = {
    (16, 16, 3, 1): {16: 'pers', 8: (8, 2, 8, 8, 2, 1), 4: (4, 4, 4, 4, 1, 1)},
    (32, 32, 3, 1): {16: (16, 2, 8, 16, 4, 2), 8: (8, 2, 8, 8, 2, 2), 4: (4, 1, 4, 4, 1, 1)},
    (64, 64, 3, 1): {16: (16, 2, 4, 16, 2, 4), 8: (8, 2, 4, 8, 1, 1), 4: (4, 1, 4, 4, 1, 1)},
    (16, 32, 3, 2): {16: (16, 2, 2, 16, 1, 2), 8: (8, 2, 4, 8, 1, 2), 4: (4, 1, 4, 4, 1, 1)},
    (32, 32, 3, 2): {16: (16, 2, 2, 16, 1, 2), 8: (8, 2, 4, 8, 1, 2), 4: (4, 1, 4, 4, 1, 1)},
    (32, 64, 3, 2): {16: (16, 2, 2, 16, 1, 4), 8: (8, 2, 4, 8, 1, 4), 4: (4, 1, 4, 4, 1, 1)},
    (64, 64, 3, 2): {16: (16, 2, 2, 16, 1, 4), 8: (8, 2, 4, 8, 1, 4), 4: (4, 1, 4, 4, 1, 1)},
    (32, 32, 5, 2): {16: (16, 1, 2, 16, 1, 2), 8: (8, 1, 4, 8, 1, 2), 4: (4, 4, 4, 4, 1, 2)},
}
# (cin, cout, k) -> {row width: conv_tr2_kernel's (TX, TZ, TY, TXT, R, CTW)}; widths 16 and 8 of k3 only under tr2_old
_TR2_TILES = {
    (64, 64, 3): {16: (16, 2, 4, 16, 2, 4), 8: (8, 2, 4, 8, 1, 1), 4: (4, 1, 4, 4, 1, 1)},
    (64, 32, 3): {16: (16, 2, 4, 16, 2, 2), 8: (8, 2, 8, 8, 2, 2), 4: (4, 1, 4, 4, 1, 1)},
    (32, 16, 3): {16: (16, 2, 8, 16, 4, 1), 8: (8, 2, 8, 8, 2, 1), 4: (4, 4, 4, 4, 1, 1)},
    (32, 32, 3): {16: (16, 2, 8, 16, 4, 2), 8: (8, 2, 8, 8, 2, 2), 4: (4, 1, 4, 4, 1, 1)},
    (32, 32, 5): {16: (16, 2, 8, 16, 4, 2), 8: (8, 2, 8, 8, 2, 2), 4: (4, 4, 4, 4, 1, 2)},
}
# (cin, cout) -> {row width: conv_tr2g_kernel's (TX, TZ, TY, TXT, R, CTW)}
_TR2G_TILES = {
    (64, 64): {16: (16, 2, 4, 16, 2, 2), 8: (8, 2, 4, 8, 1, 1)}, (64, 32): {16: (16, 2, 4, 16, 2, 2), 8: (8, 2, 8, 8, 2, 1)},
    (32, 16): {16: (16, 2, 8, 16, 4, 1), 8: (8, 2, 8, 8, 2, 1)}, (32, 32): {16: (16, 2, 8, 16, 4, 1), 8: (8, 2, 8, 8, 2, 1)},
}


def _cycle(i):
    """Row i of a family: (transposed-flipped?, epilogue, channel-offset output?) -- all eight combinations within eight rows."""
    epi = (FULLCLIP if i % 4 == 3 else FULL) if i % 2 else BARE
    return (i // 2) % 2 == 1, epi, i % 4 in (1, 2)


def _base_rows():
    rows = []
    # ---- launch_fwd
    for f16 in (False, True):
        fam, tag = ('conv_fwd_f16', '-f16') if f16 else ('conv_fwd', '')
        i = 0
        for (cin, cout, k, s), tiles in _FWD_TILES.items():
            for width, t in tiles.items():
                tr, epi, off = _cycle(i)
                tr = tr and s == 1
                # fp16 twins: every other one hands its output over as fp16 (PCC_CONV_OUT16, which pcc_conv3d admits under AUTO only)
                mode = ('out16' if i % 2 == 0 else 'f16') if f16 else 'fp32'
                impl = 'AUTO' if f16 else 'MFMA'
                rid = f'fwd-{cin}-{cout}-k{k}s{s}{"T" if tr else ""}-w{width}{tag}'
                geo = _geo(cin, cout, k, s, tr, BASE[width])
                if t == 'pers' and not f16:
                    rows.append(_row(rid, fam, 'conv16_pers_kernel<2,4,2,20,2>', geo, impl, {}, mode, epi, off))
                    tr2, epi2, off2 = _cycle(i + 3)
                    rows.append(_row(rid + '-p16', fam, 'conv16_pers_kernel<2,8,2,20,1>', _geo(cin, cout, k, s, tr2, BASE[width]), impl,
                                     {'p16': True}, mode, epi2, off2))
                else:
                    t = (16, 2, 8, 16, 4, 1) if t == 'pers' else t
                    rows.append(_row(rid, fam, _fwd_name(cin, cout, k, s, t, f16), geo, impl, {}, mode, epi, off))
                i += 1
    # ---- launch_tr2: conv_tr2g_kernel (k3, widths 16 and 8), conv_tr2_kernel (width 4, k5, and under tr2_old)
    i = 0
    for (cin, cout), tiles in _TR2G_TILES.items():
        for width, t in tiles.items():
            geo = _geo(cin, cout, 3, 2, True, BASE[width])
            rid = f'tr2g-{cin}-{cout}-w{width}'
            targs = ','.join(map(str, t))
            for epi_name, mode, epi in (('TR2G_EPI_F32', 'fp32', NORES if i % 2 else BARE), ('TR2G_EPI_ANY', 'fp32', FULLCLIP if i % 2 else FULL),
                                        ('TR2G_EPI_F32', 'f16', BARE if i % 2 else NORES), ('TR2G_EPI_ANY', 'f16', FULL if i % 2 else FULLCLIP),
                                        ('TR2G_EPI_F16', 'out16', NORES)):
                f16 = mode != 'fp32'
                name = f'conv_tr2g_kernel<{cin},{cout},{targs},{"true" if f16 else "false"},{epi_name}>'
                rows.append(_row(f'{rid}-{epi_name[9:].lower()}{"-f16" if f16 else ""}', 'tr2', name, geo, 'AUTO' if f16 else 'MFMA',
                                 {'no_tr2m': True}, mode, epi, (i + (epi_name == 'TR2G_EPI_ANY')) % 2 == 1))
            i += 1
    i = 0
    for f16 in (False, True):
        for (cin, cout, k), tiles in _TR2_TILES.items():
            for width, t in tiles.items():
                old = k == 3 and width != 4
                _, epi, off = _cycle(i)
                mode = ('out16' if i % 2 == 0 else 'f16') if f16 else 'fp32'
                rid = f'tr2-{cin}-{cout}-k{k}-w{width}{"-f16" if f16 else ""}{"-tr2old" if old else ""}'
                sws = {'no_tr2m': True, 'tr2_old': True} if old else {'no_tr2m': True}
                rows.append(_row(rid, 'tr2', _tr2_name(cin, cout, k, t, f16), _geo(cin, cout, k, 2, True, BASE[width]),
                                 'AUTO' if f16 else 'MFMA', sws, mode, epi, off))
                i += 1
    # ---- pcc_conv_tr2m: the grids of TR2M_CASES (tests/test_conv_gpu.py) with D = 1, 5, 9 and 32; bias / ReLU epilogues only
    for j, (geo, relu) in enumerate((((1, 1, 16, 16, 32, 16, 3, 2, 1), True), ((2, 5, 16, 32, 64, 32, 3, 2, 1), False),
                                     ((1, 9, 32, 16, 64, 32, 3, 2, 1), True), ((2, 32, 16, 16, 32, 16, 3, 2, 1), False))):
        name = 'conv_tr2m_kernel<%d,%s>' % (geo[4] // 16, 'true' if relu else 'false')
        rows.append(_row(f'tr2m-{geo[4]}-{geo[5]}-d{geo[1]}', 'tr2m', name, geo, 'MFMA', {'no_split': True, 'tr2m': True}, 'fp32',
                         dict(bias=j != 3, relu=relu, res=False, clip=False), j % 2 == 1))
    # ---- pcc_conv_cin1: input (6, 18, 32); with k = 9 the halo is larger than the grid
    for j, (cout, k) in enumerate(((16, 3), (32, 3), (16, 9), (32, 9))):
        _, epi, off = _cycle(j)
        rows.append(_row(f'cin1-{cout}-k{k}', 'cin1', 'conv_cin1_kernel<%d,%d,2,8,4>' % (cout, k), (N_BASE, 6, 18, 32, 1, cout, k, 2, 0),
                         'AUTO', {}, 'fp32', epi, off))
    # ---- pcc_conv_cout1_mfma, T = 16: W no multiple of 16; pcc_conv_cout1
    rows.append(_row('cout1m-t16-w24', 'cout1_mfma', 'conv_cout1_mfma_kernel<false,16,false>', (N_BASE, 5, 10, 24, 16, 1, 3, 1, 1), 'AUTO', {},
                     'fp32', BARE, False))
    rows.append(_row('cout1m-t16-w5', 'cout1_mfma', 'conv_cout1_mfma_kernel<false,16,false>', (N_BASE, 4, 6, 5, 16, 1, 3, 1, 1), 'AUTO', {},
                     'fp32', FULLCLIP, True, oco=3))
    rows.append(_row('cout1-k3s1', 'cout1', 'conv_cout1_kernel<32,3,1,4,8,8>', (N_BASE, 5, 10, 8, 32, 1, 3, 1, 1), 'AUTO', {}, 'fp32', FULL, True,
                     oco=3))
    rows.append(_row('cout1-k9s2', 'cout1', 'conv_cout1_kernel<32,9,2,2,8,8>', (N_BASE, 5, 10, 8, 32, 1, 9, 2, 1), 'AUTO', {}, 'fp32', BARE, False))
    # ---- pcc_conv_cout1_mfma with fp16 input, T = 16: the same two shapes; the layer takes no fp16 residual (it reads `residual` as fp32)
    rows.append(_row('cout1m-t16-w24-in16', 'cout1_mfma', 'conv_cout1_mfma_kernel<true,16,false>', (N_BASE, 5, 10, 24, 16, 1, 3, 1, 1), 'AUTO', {},
                     'in16-out32', BARE, False))
    rows.append(_row('cout1m-t16-w5-in16', 'cout1_mfma', 'conv_cout1_mfma_kernel<true,16,false>', (N_BASE, 4, 6, 5, 16, 1, 3, 1, 1), 'AUTO', {},
                     'in16-out32', NORESCLIP, True, oco=3))
    # ---- pcc_conv_f16: H and W are multiples of 16 and the tiles (16 x 16 at C = 16, 8 x 16 at C = 32 / 64) divide them, so the edges
    # are in z: SAME padding and the slab seams.  Every instantiation at D = 5 (odd: one slab) and at D = 16, where N = 2 leaves so few
    # workgroups that the first loop of the launcher ends at its smallest slab of 4 planes; two tiles in x (C = 16) or y (C = 32 / 64).
    # No channel offset: pcc_f16_eligible refuses one.
    i = 0
    for C in (16, 32, 64):
        for out32 in (False, True):
            for D, zsplit in ((5, 1), (16, 4)):
                epi = (BARE, NORES, FULL)[i % 3]
                tr = i % 4 in (1, 2)
                name = 'conv_f16_kernel<%d,%s,%s>' % (min(C, 32), 'true' if out32 else 'false', 'true' if C == 64 else 'false')
                geo = (N_BASE, D, 16, 32 if C == 16 else 16, C, C, 3, 1, int(tr))
                r = _row(f'f16-{C}-{"out32" if out32 else "out16"}{"T" if tr else ""}-d{D}', 'conv_f16', name, geo, 'AUTO', {},
                         'in16-out32' if out32 else 'in16-out16', epi, False)
                r['zsplit'] = zsplit
                rows.append(r)
                i += 1
    # ---- pcc_conv_tr2m_f16: the four grids of the pcc_conv_tr2m rows above, fp16 hand-over; bias / ReLU epilogues only
    for j, (geo, relu) in enumerate((((1, 1, 16, 16, 32, 16, 3, 2, 1), True), ((2, 5, 16, 32, 64, 32, 3, 2, 1), False),
                                     ((1, 9, 32, 16, 64, 32, 3, 2, 1), True), ((2, 32, 16, 16, 32, 16, 3, 2, 1), False))):
        name = 'conv_tr2m_f16_kernel<%d,%s>' % (geo[4] // 32, 'true' if relu else 'false')
        rows.append(_row(f'tr2mf16-{geo[4]}-{geo[5]}-d{geo[1]}', 'tr2m_f16', name, geo, 'AUTO', {}, 'out16',
                         dict(bias=j != 3, relu=relu, res=False, clip=False), j % 2 == 1))
    # ---- the generic kernels: the odd shapes of GENERIC_CASES (tests/test_conv_gpu.py)
    rows.append(_row('generic-fwd', 'generic', 'conv_fwd_generic', (N_BASE, 7, 9, 6, 3, 5, 3, 2, 0), 'GENERIC', {}, 'fp32', FULLCLIP, True, oco=3))
    rows.append(_row('generic-tr', 'generic', 'conv_tr_generic', (N_BASE, 5, 4, 6, 4, 3, 3, 2, 1), 'GENERIC', {}, 'fp32', BARE, False))
    return rows


ROWS = _base_rows()
BY_ID = {r['id']: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def _window_n(per_image, slots):
    """The smallest batch whose tile count exceeds the slots and is no multiple of them."""
    n = slots // per_image + 1
    while (n * per_image) % slots == 0:
        n += 1
    return n


def windowed_rows(num_cu):
    """The rows whose kernel or loop depends on the voxel count against the CU count; N follows num_cu.  Groups: 'big' (the 2 x 8 x 16
    tile of 64 -> 64), 'pers' and 'tr2g' (persistent loops: more tiles than slots, no multiple of them, partial tiles in z and y),
    'cout1' (32 x 32 columns with one, two, four and eight z slabs, each with fp32 and with fp16 input, and the one-slab layer under
    cout1_t16; every row carries the slab count it means as 'zsp')."""
    rows = []
    def big(n):        # conv_fwd.hip:486-494
        row = dict(geo=(n, 15, 20, 32, 64, 64, 3, 1, 0), impl='MFMA')
        return select(row, dict(f16=False, out16=False, res=True, clip=False), {}, num_cu)['kernel'].endswith('16,2,8,16,4,4>')
    n = next(i for i in range(1, 4096) if big(i))
    while big(n + 1):      # the last batch of the first window in which the big tile wins (13 at 256 CUs: 975 small workgroups on 768 slots)
        n += 1
    g = (n, 15, 20, 32, 64, 64, 3, 1, 0)
    rows.append(_row('big-64-64', 'conv_fwd', 'conv_fwd_kernel<64,64,3,1,16,2,8,16,4,4>', g, 'MFMA', {}, 'fp32', FULL, False, 'big'))
    rows.append(_row('big-64-64-f16', 'conv_fwd_f16', 'conv_fwd_kernel<64,64,3,1,16,2,8,16,4,4,true>', g[:8] + (1,), 'AUTO', {}, 'f16', NORES, True,
                     'big'))
    grid = (17, 22, 32)
    for p16 in (False, True):
        TZ, TY, wpc = (2, 8, 1) if p16 else (2, 4, 2)
        one = select(dict(geo=(1,) + grid + (16, 16, 3, 1, int(p16)), impl='MFMA'), dict(f16=False, out16=False, res=True, clip=False),
                     {'p16': p16}, num_cu)
        g = (_window_n(one['ntiles'], one['slots']),) + grid + (16, 16, 3, 1, int(p16))
        rows.append(_row('pers-loop' + ('-p16' if p16 else ''), 'conv_fwd', 'conv16_pers_kernel<%d,%d,2,20,%d>' % (TZ, TY, wpc), g, 'MFMA',
                         {'p16': True} if p16 else {}, 'fp32', FULL, p16, 'pers'))
    for (cin, cout, width, grid, epi) in ((32, 16, 16, (9, 20, 32), NORES), (64, 32, 16, (9, 22, 32), FULL), (64, 64, 8, (7, 9, 8), NORES)):
        TX, TZ, TY, TXT, R, ctw = _TR2G_TILES[(cin, cout)][width]
        one = select(dict(geo=(1,) + grid + (cin, cout, 3, 2, 1), impl='MFMA'), dict(f16=False, out16=False, res=epi['res'], clip=False),
                     {'no_tr2m': True}, num_cu)
        g = (_window_n(one['ntiles'], one['slots']),) + grid + (cin, cout, 3, 2, 1)
        name = 'conv_tr2g_kernel<%d,%d,%s,false,%s>' % (cin, cout, ','.join(map(str, (TX, TZ, TY, TXT, R, ctw))), 'TR2G_EPI_ANY' if epi['res'] else 'TR2G_EPI_F32')
        rows.append(_row(f'tr2g-loop-{cin}-{cout}-w{width}', 'tr2', name, g, 'MFMA', {'no_tr2m': True}, 'fp32', epi, epi['res'], 'tr2g'))
    for rid, g, sws, name in (('cout1m-t32-zsp1', (num_cu, 3, 32, 32, 16, 1, 3, 1, 1), {}, 'conv_cout1_mfma_kernel<false,32,false>'),
                              ('cout1m-t32-zsp2', (num_cu // 2, 33, 32, 32, 16, 1, 3, 1, 1), {}, 'conv_cout1_mfma_kernel<false,32,false>'),
                              ('cout1m-t16-forced', (num_cu, 3, 32, 32, 16, 1, 3, 1, 1), {'cout1_t16': True}, 'conv_cout1_mfma_kernel<false,16,false>')):
        rows.append(_row(rid, 'cout1_mfma', name, g, 'AUTO', sws, 'fp32', FULL, False, 'cout1'))
    # four and eight slabs of 16 planes (the 64^3 and 128^3 batches of the benchmark): every seam has 16 planes on either side.  The
    # launcher splits only while a slab keeps 16 planes and only until every CU has a workgroup, so N x D cannot be smaller than
    # 16 planes per CU: these rows have the voxel count of cout1m-t32-zsp2.  Then every slab count again with fp16 input (no residual).
    for zsp, D in ((4, 64), (8, 128)):
        rows.append(_row(f'cout1m-t32-zsp{zsp}', 'cout1_mfma', 'conv_cout1_mfma_kernel<false,32,false>', (num_cu // zsp, D, 32, 32, 16, 1, 3, 1, 1),
                         'AUTO', {}, 'fp32', FULL, False, 'cout1'))
    for r in [r for r in rows if r['group'] == 'cout1' and not r['switches']]:
        rows.append(_row(r['id'] + '-in16', 'cout1_mfma', 'conv_cout1_mfma_kernel<true,32,false>', r['geo'], 'AUTO', {}, 'in16-out32', NORES, False,
                         'cout1'))
    for r in rows:
        if r['group'] == 'cout1':
            r['zsp'] = 1 if r['switches'] else int(r['id'].split('zsp')[1].split('-')[0])
    return rows


# ---- inputs and references ----------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=8)
def _arrays(geo, which):
    """(x, w, bias, residual, e) of a geometry in set `which`: float32, shared between rows (do not write to them); e: the exponent of every output channel's scale."""
    N, D, H, W, cin, cout, k, s, tr = geo
    rng = _rng('direct', geo, which)
    oshape = (N,) + out_dims(geo) + (cout,)
    wshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
    if which == 'A':
        if cin == 1:
            x = (rng.random((N, D, H, W, cin)) < 0.3).astype(np.float32)           # the first layer reads 0 / 1 occupancy
        else:
            x = (rng.integers(-3, 4, (N, D, H, W, cin)) * (rng.random((N, D, H, W, cin)) < 0.6)).astype(np.float32)
        e = rng.integers(-6, 7, cout)
        scale = np.exp2(e).astype(np.float32)
        w = rng.integers(-2, 3, wshape).astype(np.float32) * (scale[:, None] if tr else scale)
        b = rng.integers(-2, 3, cout).astype(np.float32) * scale
        r = rng.integers(-3, 4, oshape).astype(np.float32)
    else:
        x = (rng.random((N, D, H, W, cin)) < 0.3).astype(np.float32)
        e = np.zeros(cout, np.int64)
        w = rng.integers(-1, 2, wshape).astype(np.float32)
        b = rng.integers(-1, 2, cout).astype(np.float32)
        r = rng.integers(-2, 3, oshape).astype(np.float32)
    return x, w, b, r, e


def inputs(row):
    """(x, w, b or None, r or None) as tests/_family_cases.py::run takes them; rows that share a geometry and a set share the arrays."""
    x, w, b, r, _ = _arrays(row['geo'], row['set'])
    return x, w, (b if row['bias'] else None), (r if row['res'] else None)


def exponents(row):
    return _arrays(row['geo'], row['set'])[4]


def epilogue(y, row, r):
    """What follows bias and ReLU, in the kernels' order: residual, then clip.  float64."""
    y = np.asarray(y, np.float64)
    if row['res']:
        y = y + r
    if row.get('clip'):
        y = np.clip(y, 0.0, 1.0)
    return y


@functools.lru_cache(maxsize=4)
def _conv_ref(geo, which, bias, relu, absolute, use_torch):
    x, w, b, r, _ = _arrays(geo, which)
    f = np.abs if absolute else (lambda a: a)
    if use_torch:
        from oracle import torch_oracle as T
        conv = lambda *a: (T.conv3d_transpose if geo[8] else T.conv3d)(*a).numpy()
    else:
        from oracle import oracle as O
        conv = O.conv3d_transpose if geo[8] else O.conv3d
    return conv(f(x), f(w), f(b) if bias else None, geo[7], bool(relu))


def reference(row, absolute=False, use_torch=None):
    """The float64 reference of a row: the float64-accumulating C loops (oracle/pcc_oracle.c) for the base-grid rows, the oneDNN
    restatement (oracle/torch_oracle.py: exact in fp32 on these operands, pinned to the C loops by the GPU test) for the windowed
    ones.  absolute: on |x|, |w|, |bias|, |residual| without the clip -- the sum of |terms| of every output."""
    if use_torch is None:
        use_torch = row['group'] != 'base'
    y = _conv_ref(row['geo'], row['set'], bool(row['bias']), bool(row['relu']), absolute, use_torch)
    r = _arrays(row['geo'], row['set'])[3]
    if absolute:
        return np.asarray(y, np.float64) + (np.abs(r) if row['res'] else 0.0)
    return epilogue(y, row, r)


def magnitude_bound(row):
    """An upper bound of the sum of |terms| of any output of a Set A or B row, in units of the smallest power of two the terms of its
    channel carry (2^min(e, 0)): taps x channels x max |x| x max |w| + |bias| + |residual|, times 2^6 in set A (e = 6 scales the
    conv terms by it, e = -6 the residual)."""
    N, D, H, W, cin, cout, k, s, tr = row['geo']
    if row['set'] == 'A':
        return (k ** 3 * cin * 3 * 2 + 2 + 3) * 64
    return k ** 3 * cin + 1 + 2


def is_sub(row):
    """The 64-channel layer of conv_f16.hip: two launches of conv_f16_kernel<32,.,true> with raw fp16 partial sums in between."""
    return row['kernel'].startswith('conv_f16_kernel') and row['kernel'].endswith(',true>')


def partial_bound(row):
    """An upper bound of |raw partial sum| that the launch of input half 0 of a SUB row leaves in fp16: taps x 32 channels x max |x| x
    max |w|; no bias, no residual (conv_f16.hip:150-159: `raw`)."""
    assert is_sub(row) and row['set'] == 'B'
    return row['geo'][6] ** 3 * 32


def partial_reference(row, absolute=False):
    """float64: the partial sums of input channels 0 .. 31 of a SUB row (a.ico = 0, the cig = 0 images of pcc_f16_pack), bare."""
    from oracle import oracle as O
    assert is_sub(row)
    x, w, _, _, _ = _arrays(row['geo'], row['set'])
    f = np.abs if absolute else (lambda a: a)
    x0 = np.ascontiguousarray(f(x[..., :32]))
    w0 = np.ascontiguousarray(f(w[..., :32] if row['geo'][8] else w[:, :, :, :32, :]))
    return np.asarray((O.conv3d_transpose if row['geo'][8] else O.conv3d)(x0, w0, None, row['geo'][7], False), np.float64)


def explain(row, got, want, tile, limit=5):
    """The count of wrong outputs and the first few with got / want and their place under the row's voxel tile."""
    bad = np.argwhere(got != want)
    s = row['geo'][7]
    lines = [f'{row["id"]} ({row["kernel"]}): {len(bad)} of {got.size} outputs differ']
    for idx in bad[:limit]:
        n, z, y, x, c = (int(v) for v in idx)
        where = ''
        if tile is not None:
            bz, by, bx = ((z // s, y // s, x // s) if row['geo'][8] and s == 2 else (z, y, x))       # base-grid voxel of the output
            where = ' tile (%d,%d,%d) + (%d,%d,%d)' % (bz // tile[0], by // tile[1], bx // tile[2], bz % tile[0], by % tile[1], bx % tile[2])
        lines.append(f'  [n={n} z={z} y={y} x={x} c={c}]{where}: got {got[tuple(idx)]!r} want {want[tuple(idx)]!r}')
    return '\n'.join(lines)
