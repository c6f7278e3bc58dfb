"""GPU: the latent step.  The three stepped kernels and the rate ladder (csrc/latent_step.hip) against the numpy restatement
tests/_latent_step_ref.py, bit for bit, and against their un-stepped twins at q = 16; the stepped stream through the model, the rate target
and the CLIs.  All kernel inputs are normal floats: subnormal quotients are outside the contract (include/pcc_geo.h)."""
import functools
import gzip
import io
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax as MS
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType

import _latent_step_ref as R
import _pack_ref as P
from test_pack_fused_gpu import Guarded, bits, dev, stream_shape

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_NP = {1: np.uint8, 2: np.int16, 4: np.int32}

# (N, vox, C): every block its own step; 65 x 65 crosses the 64 x 64 pack tile both ways; 8 voxels are fewer than a tile; one whole tile
SHAPES = [(3, 65, 65), (3, 8, 64), (3, 64, 64)]
QS = (16, 0, 37)
IDS = ['x'.join(map(str, s)) for s in SHAPES]
TABLE = P.scale_tables()['ref64']


def steps_of(q):
    return np.array([R.latent_step(v) for v in q], F32)


def stream(sym, cf, dtype):
    """(N, vox, C) int32 -> stream order, narrowed by the C cast (two's-complement wrap, also to uint8)"""
    return (np.ascontiguousarray(np.moveaxis(sym, -1, 1)) if cf else sym).astype(dtype)


@functools.lru_cache(maxsize=None)
def quant_values(shape, q):
    """N(0, 3) x step with, at the head of every block: the exact ties (k + 1/2) x step for k in -32..31 and their two float32 neighbours
    (quotients within one ulp of a tie: a reciprocal multiply gets some of them wrong), +-0, +-40000.3 x step (symbols beyond int16) and
    one value of its own magnitude per block (so that a tile maximum stored at another block's entry shows)."""
    rng = np.random.default_rng([31] + list(shape))
    step = steps_of(q)
    v = (rng.standard_normal(shape) * 3).astype(F32) * step[:, None, None]
    flat = v.reshape(shape[0], -1)
    for n in range(shape[0]):
        ties = ((np.arange(-32, 32) + 0.5) * np.float64(step[n])).astype(F32)
        assert np.array_equal(ties.astype(np.float64) / np.float64(step[n]), np.arange(-32, 32) + 0.5)        # exact in float32
        planted = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)), np.array([0.0, -0.0], F32),
                                  (np.array([40000.3, -40000.3, 50000 + 1000 * n], F32) * step[n]).astype(F32)])
        where = rng.permutation(flat.shape[1])[:planted.size]
        flat[n, where] = planted
    assert np.all((v == 0) | (np.abs(v) >= np.finfo(F32).tiny))
    return v


@functools.lru_cache(maxsize=None)
def sigma_values(shape, q):
    """log-uniform over [0.01, 600] x step with, in every block, table entries x step and their float32 neighbours (quotients on, just
    below and just above the entries), the entries themselves, and values below table[0] and above the last entry"""
    rng = np.random.default_rng([32] + list(shape))
    step = steps_of(q)
    s = np.exp(rng.uniform(np.log(0.01), np.log(600), shape)).astype(F32) * step[:, None, None]
    flat = s.reshape(shape[0], -1)
    for n in range(shape[0]):
        on = (TABLE * step[n]).astype(F32)
        planted = np.concatenate([on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf)), TABLE,
                                  (np.array([0.05, 0.1099, 256.5, 900.0], F32) * step[n]).astype(F32)])
        where = rng.permutation(flat.shape[1])[:planted.size]
        flat[n, where] = planted
    return s


def stream_values(shape, dtype):
    """symbols as the host coder hands them back, (N, vox, C) int32, with the extremes of `dtype` (beyond int16 for int32) in every block"""
    rng = np.random.default_rng([36, np.dtype(dtype).itemsize] + list(shape))
    lo, hi, ext = {np.uint8: (0, 200, [255, 0]), np.int16: (-3000, 3000, [32767, -32767, -32768]), np.int32: (-30000, 30000, [70000, -70000])}[dtype]
    x = rng.integers(lo, hi, shape).astype(np.int32)
    flat = x.reshape(shape[0], -1)
    for n in range(shape[0]):
        flat[n, rng.permutation(flat.shape[1])[:len(ext)]] = ext
    return x


def qdev(ctx, q):
    return torch.tensor(list(q), dtype=torch.uint8, device=ctx.device)


# ---- the three kernels against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_quantize_step_pack_is_the_restatement(ctx, shape):
    v = quant_values(shape, QS)
    ntiles = L.lib().pcc_symbols_tiles(shape[0], shape[1], shape[2])
    vd, qd = dev(ctx, v), qdev(ctx, QS)
    seen_wide = False
    for kind in (None, 'dyadic'):
        med = P.medians_of(kind, shape[-1])
        md = dev(ctx, med)
        for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
            rsym, rdeq = R.quantize_step(v, QS, med, mode)
            seen_wide |= bool(np.abs(rsym).max() > 32767)
            for cf in (True, False):
                for dst_bytes in (1, 2, 4):
                    what = f'medians {kind}, mode {mode}, channels_first {cf}, dst_bytes {dst_bytes}'
                    sym, deq = Guarded(shape, torch.int32, ctx.device), Guarded(shape, torch.float32, ctx.device)
                    dst, tm = Guarded(stream_shape(shape, cf), _TORCH[dst_bytes], ctx.device), Guarded((ntiles,), torch.int32, ctx.device)
                    ops.quantize_step_pack(ctx, vd, md, mode, cf, dst.ptr(), dst_bytes, qd, tm.ptr(), sym=sym.t, deq=deq.t)
                    assert_array_equal(sym.np(), rsym, err_msg=what)
                    assert_array_equal(bits(deq.np()), bits(rdeq), err_msg=what)
                    assert_array_equal(dst.np(), stream(rsym, cf, _NP[dst_bytes]), err_msg=what)
                    assert_array_equal(tm.np(), P.tile_max(rsym), err_msg=what)
                    for g, name in ((sym, 'sym'), (deq, 'deq'), (dst, 'dst'), (tm, 'tile_max')):
                        g.check(f'{name} ({what})')
            # deq = None and no tile maxima: accepted, the other outputs unchanged
            sym2, dst2 = Guarded(shape, torch.int32, ctx.device), Guarded(stream_shape(shape, True), torch.int16, ctx.device)
            _, none = ops.quantize_step_pack(ctx, vd, md, mode, True, dst2.ptr(), 2, qd, None, want_deq=False, sym=sym2.t)
            assert none is None
            assert_array_equal(sym2.np(), rsym)
            sym2.check('sym without deq')
            dst2.check('dst without deq')
            # no destination for the packed copy (a coder that reads the int32 tensors): accepted, the other outputs unchanged
            sym3, tm3 = Guarded(shape, torch.int32, ctx.device), Guarded((ntiles,), torch.int32, ctx.device)
            for cf in (True, False):
                ops.quantize_step_pack(ctx, vd, md, mode, cf, None, 4, qd, tm3.ptr(), want_deq=False, sym=sym3.t)
                assert_array_equal(sym3.np(), rsym)
                assert_array_equal(tm3.np(), P.tile_max(rsym))
                sym3.check('sym without dst')
                tm3.check('tile_max without dst')
    assert seen_wide, 'degenerate test: no symbol beyond int16'


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_index_pack_step_is_the_restatement(ctx, shape):
    s = sigma_values(shape, QS)
    ref = R.index_step(s, TABLE, QS)
    assert ref.min() == 0 and ref.max() == len(TABLE) - 1                          # below table[0] and above the last entry
    sd, td, qd = dev(ctx, s), dev(ctx, TABLE), qdev(ctx, QS)
    for cf in (True, False):
        for dst_bytes in (1, 2, 4):
            what = f'channels_first {cf}, dst_bytes {dst_bytes}'
            idx, dst = Guarded(shape, torch.int32, ctx.device), Guarded(stream_shape(shape, cf), _TORCH[dst_bytes], ctx.device)
            ops.index_pack_step(ctx, sd, td, cf, dst.ptr(), dst_bytes, qd, idx=idx.t)
            assert_array_equal(idx.np(), ref, err_msg=what)
            assert_array_equal(dst.np(), stream(ref, cf, _NP[dst_bytes]), err_msg=what)
            idx.check(f'idx ({what})')
            dst.check(f'dst ({what})')
    # a table that does not ascend takes the literal count inside the kernel: the same formula
    shuffled = P.scale_tables()['shuffled']
    dst = Guarded(stream_shape(shape, True), torch.int32, ctx.device)
    idx = ops.index_pack_step(ctx, sd, dev(ctx, shuffled), True, dst.ptr(), 4, qd)
    assert_array_equal(idx.cpu().numpy(), R.index_step(s, shuffled, QS))
    dst.check('dst (shuffled table)')
    for cf in (True, False):                                                         # no destination for the packed copy
        idx = Guarded(shape, torch.int32, ctx.device)
        ops.index_pack_step(ctx, sd, td, cf, None, 1, qd, idx=idx.t)
        assert_array_equal(idx.np(), ref)
        idx.check('idx without dst')


@pytest.mark.parametrize('dst_bytes', [1, 2, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_unpack_dequantize_step_is_the_restatement(ctx, shape, dst_bytes):
    want = stream_values(shape, _NP[dst_bytes])
    med = P.medians_of('random', shape[-1])
    qd = qdev(ctx, QS)
    for cf in (True, False):
        src = dev(ctx, stream(want, cf, _NP[dst_bytes]))
        for m in (None, med):
            what = f'channels_first {cf}, medians {"none" if m is None else "random"}'
            sym, deq = Guarded(shape, torch.int32, ctx.device), Guarded(shape, torch.float32, ctx.device)
            ops.unpack_dequantize_step(ctx, src, shape, cf, qd, dev(ctx, m), sym=sym.t, deq=deq.t)
            assert_array_equal(sym.np(), want, err_msg=what)
            assert_array_equal(bits(deq.np()), bits(R.dequantize_step(want, QS, m)), err_msg=what)
            sym.check(f'sym ({what})')
            deq.check(f'deq ({what})')


# ---- q = 16 everywhere: the un-stepped twins, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_step_one_is_the_unstepped_twin(ctx, shape):
    ones = (16,) * shape[0]
    qd = qdev(ctx, ones)
    v, s = quant_values(shape, ones), sigma_values(shape, ones)
    vd, sd, td = dev(ctx, v), dev(ctx, s), dev(ctx, TABLE)
    ntiles = L.lib().pcc_symbols_tiles(shape[0], shape[1], shape[2])
    for cf in (True, False):
        for kind in (None, 'random'):
            md = dev(ctx, P.medians_of(kind, shape[-1]))
            for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
                out = []
                for stepped in (False, True):
                    dst, tm = Guarded(stream_shape(shape, cf), torch.int16, ctx.device), Guarded((ntiles,), torch.int32, ctx.device)
                    if stepped:
                        sym, deq = ops.quantize_step_pack(ctx, vd, md, mode, cf, dst.ptr(), 2, qd, tm.ptr())
                    else:
                        sym, deq = ops.quantize_pack(ctx, vd, md, mode, cf, dst.ptr(), 2, tm.ptr())
                    out.append((sym, deq.view(torch.int32), dst.t, tm.t))
                assert all(torch.equal(a, b) for a, b in zip(*out)), f'quantize: channels_first {cf}, medians {kind}, mode {mode}'
            # the decoder side, on the symbols the un-stepped encoder packed
            src = out[0][2].reshape(stream_shape(shape, cf)).contiguous()
            a = ops.unpack_dequantize(ctx, src, shape, cf, md)
            b = ops.unpack_dequantize_step(ctx, src, shape, cf, qd, md)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), f'unpack: channels_first {cf}, medians {kind}'
        out = []
        for stepped in (False, True):
            dst = Guarded(stream_shape(shape, cf), torch.uint8, ctx.device)
            idx = ops.index_pack_step(ctx, sd, td, cf, dst.ptr(), 1, qd) if stepped else ops.index_pack(ctx, sd, td, cf, dst.ptr(), 1)
            out.append((idx, dst.t))
        assert all(torch.equal(a, b) for a, b in zip(*out)), f'index: channels_first {cf}'


def test_stepped_kernels_past_one_grid_pass(ctx):
    """More 64 x 64 tiles than num_cu * 8 workgroups (the grid of one pass of the stand-alone element-wise kernels): every tile of a large
    launch is its own workgroup and lands at its own place, the last voxel and channel tiles partial; per-block steps as above."""
    shape = (5, 64 * 300 + 3, 65)
    assert L.lib().pcc_symbols_tiles(*shape) > ctx.num_cu * 8
    q = (16, 0, 37, 63, 9)
    rng = np.random.default_rng(33)
    step = steps_of(q)[:, None, None]
    v = (rng.standard_normal(shape) * 3).astype(F32) * step
    v[:, -64:, -1] = ((np.arange(-32, 32) + 0.5) * step[:, 0, :].astype(np.float64)).astype(F32)              # ties in the last tiles
    s = np.exp(rng.uniform(np.log(0.01), np.log(600), shape)).astype(F32) * step
    qd = qdev(ctx, q)
    for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
        rsym, rdeq = R.quantize_step(v, q, None, mode)
        dst = torch.empty(stream_shape(shape, True), dtype=torch.int16, device=ctx.device)
        tm = torch.empty((L.lib().pcc_symbols_tiles(*shape),), dtype=torch.int32, device=ctx.device)
        sym, deq = ops.quantize_step_pack(ctx, dev(ctx, v), None, mode, True, dst.data_ptr(), 2, qd, tm.data_ptr())
        assert_array_equal(sym.cpu().numpy(), rsym)
        assert_array_equal(bits(deq.cpu().numpy()), bits(rdeq))
        assert_array_equal(dst.cpu().numpy(), stream(rsym, True, np.int16))
        assert_array_equal(tm.cpu().numpy(), P.tile_max(rsym))
        sym2, deq2 = ops.unpack_dequantize_step(ctx, dst, shape, True, qd)
        assert_array_equal(sym2.cpu().numpy(), rsym)
        assert_array_equal(bits(deq2.cpu().numpy()), bits(rdeq))
    dst = torch.empty(stream_shape(shape, True), dtype=torch.uint8, device=ctx.device)
    idx = ops.index_pack_step(ctx, dev(ctx, s), dev(ctx, TABLE), True, dst.data_ptr(), 1, qd)
    ref = R.index_step(s, TABLE, q)
    assert_array_equal(idx.cpu().numpy(), ref)
    assert_array_equal(dst.cpu().numpy(), stream(ref, True, np.uint8))


# ---- the rate ladder -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gaussian():
    from pcc_geo_cnn_v2_amd.entropy_models import GaussianConditional, scale_table
    return GaussianConditional(scale_table(0.11, 256, 64))              # (its rows have different cdf_size)


@functools.lru_cache(maxsize=None)
def ladder_case(vox):
    """y ~ N(0, sigma) with outliers that escape on both sides at the fine steps, sigma log-uniform from below table[0] to above the last
    entry; the reference sums over all 64 steps, computed once"""
    gc = gaussian()
    rng = np.random.default_rng([34, vox])
    shape = (3, vox, 64)
    sigma = np.exp(rng.uniform(np.log(0.005), np.log(2000), shape)).astype(F32)
    y = (rng.standard_normal(shape) * sigma).astype(F32)
    out = rng.permutation(y.size)[:40]
    y.reshape(-1)[out] = (rng.choice([-1.0, 1.0], 40) * rng.uniform(20, 60000, 40)).astype(F32)
    cost = R.cost_table(gc.quantized_cdf, gc.cdf_length, gc.precision)
    ref = {mode: R.rate_ladder(y, sigma, gc.scale_table_f32, mode, range(64), cost, gc.cdf_length, gc.offset, 4) for mode in (P.FLOOR_HALF, P.HALF_EVEN)}
    return y, sigma, ref


@pytest.mark.parametrize('vox', [27, 65])
def test_rate_ladder_is_the_restatement_whatever_the_launch_geometry(ctx, vox):
    gc = gaussian()
    assert len(set(gc.cdf_length.tolist())) > 8
    y, sigma, ref = ladder_case(vox)
    # what the inputs reach: rows 0 and L - 1, escapes below and above the table at the finest step
    rows = R.index_step(sigma, gc.scale_table_f32, [0, 0, 0])
    sym, _ = R.quantize_step(y, [0, 0, 0], None, P.FLOOR_HALF)
    v = sym.astype(np.int64) - gc.offset[rows]
    assert rows.min() == 0 and rows.max() == 63 and (v < 0).any() and (v >= gc.cdf_length[rows] - 2).any()
    yd, sd, td = dev(ctx, y), dev(ctx, sigma), dev(ctx, gc.scale_table_f32)
    for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
        got = ops.rate_ladder(ctx, yd, sd, np.arange(64), td, gc.table, mode)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 64)
        assert_array_equal(got.cpu().numpy(), ref[mode])
        for groups in (1, 2):                                                       # fewer workgroups than tiles: the stride loop
            assert_array_equal(ops.rate_ladder(ctx, yd, sd, np.arange(64), td, gc.table, mode, groups_per_block=groups).cpu().numpy(), ref[mode])
        split = torch.cat([ops.rate_ladder(ctx, yd[n:n + 1].contiguous(), sd[n:n + 1].contiguous(), np.arange(64), td, gc.table, mode) for n in range(3)])
        assert_array_equal(split.cpu().numpy(), ref[mode])                          # another batch split
        for q in (0, 16, 63):                                                       # J = 1
            assert_array_equal(ops.rate_ladder(ctx, yd, sd, [q], td, gc.table, mode).cpu().numpy(), ref[mode][:, q:q + 1])
    assert_array_equal(ops.rate_ladder(ctx, yd, sd, [40, 3, 3], td, gc.table).cpu().numpy(), ref[P.FLOOR_HALF][:, [40, 3, 3]])
    for bad in ([], [64], list(range(64)) + [0], [-1]):
        with pytest.raises(AssertionError, match='rate_ladder'):
            ops.rate_ladder(ctx, yd, sd, bad, td, gc.table)


def test_rate_ladder_many_tiles_and_the_cached_cost_table(ctx):
    """A block of many 2048-element tiles, one workgroup each, against three workgroups striding over them; the cost table is uploaded
    once per (context, table) and again when the table's arrays change"""
    gc = gaussian()
    rng = np.random.default_rng(35)
    shape = (2, 8 * 8 * 8 + 1, 64)                                                  # 17 tiles per block, the last one partial
    sigma = np.exp(rng.uniform(np.log(0.05), np.log(400), shape)).astype(F32)
    y = (rng.standard_normal(shape) * sigma * 1.5).astype(F32)
    cost = R.cost_table(gc.quantized_cdf, gc.cdf_length, gc.precision)
    steps = [0, 8, 16, 24, 40, 63]
    ref = R.rate_ladder(y, sigma, gc.scale_table_f32, P.FLOOR_HALF, steps, cost, gc.cdf_length, gc.offset, 4)
    yd, sd, td = dev(ctx, y), dev(ctx, sigma), dev(ctx, gc.scale_table_f32)
    a = ops.rate_ladder(ctx, yd, sd, steps, td, gc.table)
    b = ops.rate_ladder(ctx, yd, sd, steps, td, gc.table, groups_per_block=3)
    assert_array_equal(a.cpu().numpy(), ref)
    assert_array_equal(b.cpu().numpy(), ref)
    first = ops.device_cost_table(ctx, gc.table)
    assert ops.device_cost_table(ctx, gc.table)[0] is first[0]
    assert_array_equal(first[0].cpu().numpy().view(np.uint32), cost)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
RES, LEVEL, NB = 16, 1, 5                                                          # the smallest V2 block grid of tests/test_codec_gpu.py


@functools.lru_cache(maxsize=None)
def cloud():
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    from test_codec_gpu import make_blocks
    blocks8 = make_blocks(NB, RES, seed=3)
    pts = np.vstack([b + np.array([(i & 1), (i >> 1) & 1, (i >> 2) & 1]) * RES for i, b in enumerate(blocks8)])
    blocks, binstr = partition_octree(pts, [0, 0, 0], [2 * RES] * 3, LEVEL)
    assert len(blocks) == NB
    return pts, blocks, binstr


def models(coder='range'):
    from test_codec_gpu import scaled_weights
    enc = ModelConfigType['c3p'].build(batch_size=2, entropy_coder=coder)
    enc.compress([1, 1, RES, RES, RES])
    enc.set_weights(scaled_weights(enc, 2.2))
    dec = ModelConfigType['c3p'].build(batch_size=3, entropy_coder=coder)           # different chunking on purpose
    dec.decompress()
    dec.set_weights({k: v for k, v in enc.get_weights().items() if not k.startswith(('analysis/', 'hyper_analysis/'))})
    return enc, dec


def test_step_16_writes_the_unstepped_strings_and_decodes_the_same_points(ctx):
    pts, blocks, binstr = cloud()
    enc, dec = models()
    plain, meta_p, _ = enc.compress_blocks(ctx, blocks, binstr, pts, 2 * RES, LEVEL, fixed_threshold=True)
    stepped, meta_s, _ = enc.compress_blocks(ctx, blocks, binstr, pts, 2 * RES, LEVEL, fixed_threshold=True, latent_step=16)
    assert meta_s[0]['latent_step'] == 16 and 'latent_step' not in meta_p[0]
    for (sp, tp), (ss, ts) in zip(plain[0], stepped[0]):
        assert len(sp) == 2 and len(ss) == 3 and tuple(ss[:2]) == tuple(sp) and ss[2] == b'\x10' and tp == ts
    a, _ = dec.decompress_blocks(ctx, plain[0], [RES] * 3)
    b, _ = dec.decompress_blocks(ctx, stepped[0], [RES] * 3, layers='step')
    assert sum(len(p) for p in a) > 0
    for pa, pb, pe in zip(a, b, meta_s[0]['x_hat_list']):
        assert np.array_equal(pa, pb) and np.array_equal(pb, pe)


@pytest.mark.parametrize('coder', ['range', 'rans'])
def test_per_block_steps_round_trip(ctx, coder):
    pts, blocks, binstr = cloud()
    enc, dec = models(coder)
    q = [0, 16, 37, 63, 9]
    data, meta, dbg_e = enc.compress_blocks(ctx, blocks, binstr, pts, 2 * RES, LEVEL, fixed_threshold=True, debug=True, latent_step=q)
    assert meta[0]['latent_step'] == q
    assert [s[2] for s, _ in data[0]] == [bytes([v]) for v in q]
    raw = MS.save_compressed_file(binstr, data[0], 2 * RES, LEVEL, strict=True)           # through the container, as the CLIs do
    _, _, _, back = MS.load_compressed_file(io.BytesIO(raw))
    dec_blocks, dbg_d = dec.decompress_blocks(ctx, back, [RES] * 3, debug=True, layers='step')
    for j in range(NB):
        for key in ('z_hat', 'sigma_hat', 'indexes', 'symbols', 'y_hat', 'x_hat'):
            assert np.array_equal(dbg_e[j][key].view(np.int32), dbg_d[j][key].view(np.int32)), (j, key)
        assert np.array_equal(meta[0]['x_hat_list'][j], dec_blocks[j])
        sym, y_hat = R.quantize_step(dbg_e[j]['y'], [q[j]], None, enc.round_mode)
        assert np.array_equal(dbg_e[j]['symbols'], sym) and np.array_equal(bits(dbg_e[j]['y_hat']), bits(y_hat))
        assert np.array_equal(dbg_e[j]['indexes'], R.index_step(dbg_e[j]['sigma_hat'], enc.conditional_bottleneck.scale_table_f32, [q[j]]))
    assert len({len(s[0]) for s, _ in data[0]}) > 1 and sum(len(p) for p in dec_blocks) > 0
    broken = [((s[0], s[1], bytes([64])), t) if j == 3 else (s, t) for j, (s, t) in enumerate(back)]
    with pytest.raises(RuntimeError, match='block 3'):
        dec.decompress_blocks(ctx, broken, [RES] * 3, layers='step')


def test_rate_target_picks_the_finest_step_that_fits(ctx, caplog):
    from pcc_geo_cnn_v2_amd import model_types as MT
    from test_latent_step_cpu import MEASURED_UNDER_BITS, TERMINATION_BITS
    pts, blocks, binstr = cloud()
    enc, _ = models()
    _, info = enc.choose_latent_step(ctx, blocks, binstr, len(pts), 1e9)
    pred = np.array(info['predictions'])
    assert pred.shape == (64,) and pred[0] > pred[63]
    k = next(k for k in range(8, 63) if pred[:k + 1].min() >= pred[k] > pred[k + 1])                     # two neighbouring steps
    budget = (pred[k] + pred[k + 1]) / 2.0
    want = int(np.flatnonzero(pred <= budget)[0])
    assert want == k + 1
    data, meta, _ = enc.compress_blocks(ctx, blocks, binstr, pts, 2 * RES, LEVEL, fixed_threshold=True, target_bpp=8.0 * budget / len(pts))
    assert meta[0]['latent_step'] == want and meta[0]['rate_target']['predicted_bytes'] == pred[want]
    assert all(s[2] == bytes([want]) for s, _ in data[0])
    actual = len(MS.save_compressed_file(binstr, data[0], 2 * RES, LEVEL, strict=True))
    # The prediction carries the measured margin per block (model_types.rate_margin_bits16), so the container fits it.  From below: a y
    # string is at most MEASURED_UNDER_BITS + 8 bits shorter than the model's sum, and the prediction is the sum plus the margin rounded
    # up to a byte, so per block it exceeds the string by less than (margin + UNDER + 8) / 8 + 1 bytes.
    ybits = 8 * max(len(s[0]) for s, _ in data[0])
    margin = int(MT.rate_margin_bits16(np.int64(ybits << 16))) / 65536.0 + 1                                 # (of a sum no larger than the string)
    slack = int(np.floor((margin + MEASURED_UNDER_BITS + TERMINATION_BITS) / 8 + 1))
    print(f'predicted {pred[want]} bytes, container {actual} bytes, {NB} blocks, at most {slack} bytes of slack per block')
    assert 0 <= pred[want] - actual <= slack * NB
    assert actual <= budget                                                                              # the chosen step really fits
    # out of reach: the coarsest step, with a warning that states the prediction
    with caplog.at_level(logging.WARNING, logger='pcc_geo_cnn_v2_amd.model_types'):
        q, info = enc.choose_latent_step(ctx, blocks, binstr, len(pts), 1e-6)
    assert q == 63 and info['predicted_bytes'] == pred[63]
    assert any('out of reach' in r.getMessage() and str(pred[63]) in r.getMessage() for r in caplog.records)


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_latent_step_round_trip(tmp_path):
    from pcc_geo_cnn_v2_amd.utils import pc_io
    from test_cli_gpu import _cloud
    res, level = 128, 2
    src = str(tmp_path / 'in.ply')
    pc_io.write_df(src, pc_io.pa_to_df(_cloud(res, 0)))
    ck = str(tmp_path / 'ckpt')
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, '-m'] + list(a), cwd=ROOT, env=env, check=True, capture_output=True, text=True)
    # (a final bias beside the fixed threshold: the coarser latents still decode to points, so the comparison below is not of two empty files)
    run('pcc_geo_cnn_v2_amd.init_checkpoint', '--model_config', 'c3p', '--checkpoint_dir', ck, '--final_bias', '0.47', '--gain_analysis', '2.2')
    out, dec_enc, dec = str(tmp_path / 'in.ply.bin'), str(tmp_path / 'enc.ply'), str(tmp_path / 'dec.ply')
    run('pcc_geo_cnn_v2_amd.compress_octree', '--input_files', src, '--output_files', out, '--dec_files', dec_enc, '--checkpoint_dir', ck,
        '--model_config', 'c3p', '--resolution', str(res), '--octree_level', str(level), '--opt_metrics', 'd1_mse', '--latent_step', '24',
        '--fixed_threshold')
    assert MS.read_gzip_tag(out).endswith('/qs1')
    with gzip.open(out, 'rb') as f:
        _, _, _, blocks = MS.load_compressed_file(f)
    assert len(blocks) > 8 and all(len(s) == 3 and s[2] == bytes([24]) for s, _ in blocks)
    met = json.load(open(out + '.enc.metric.json'))
    assert met['latent_step'] == 24 and met['latent_step_size'] == 2.0 and met['codec_numerics'].endswith('/qs1') and 'd1_psnr' in met
    run('pcc_geo_cnn_v2_amd.decompress_octree', '--input_files', out, '--output_files', dec, '--checkpoint_dir', ck, '--model_config', 'c3p')
    a, b = pc_io.load_pc(dec_enc), pc_io.load_pc(dec)
    assert a.shape == b.shape and np.array_equal(a, b) and len(b) > 0
