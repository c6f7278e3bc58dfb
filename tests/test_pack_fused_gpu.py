"""GPU: the fused quantise / index / pack kernels of the codec graphs (pcc_quantize_pack, pcc_index_pack, pcc_unpack_dequantize;
csrc/elementwise.hip) against the plain numpy restatement tests/_pack_ref.py (held against the oracle in test_pack_ref_cpu.py) AND
against the stand-alone kernels, at one shape per branch of the kernels, on inputs with the boundary values planted in every
64 x 64 tile.  Every comparison is exact: a wrong symbol or CDF row is not a small error, it is a stream the decoder cannot read.
Every destination sits between 64 sentinel elements on each side, which must come back untouched."""
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops

import _pack_ref as R

pytestmark = pytest.mark.gpu

SHAPE_IDS = [R.shape_id(s) for s in R.SHAPES]
GUARD = 64
_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_SENTINEL = {torch.uint8: 0xA5, torch.int16: -21931, torch.int32: 0x5A5A5A5A, torch.float32: -777.25}


class Guarded:
    """A destination of `shape` inside a buffer with GUARD sentinel elements before and after it (the payload starts as
    sentinels too: an element the kernel does not write cannot pass for written)."""

    def __init__(self, shape, dtype, device):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), _SENTINEL[dtype], dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(tuple(shape))
        self.edges = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).clone()

    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def check(self, what):
        assert torch.equal(torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]), self.edges), f'{what}: written outside the destination'


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stream_shape(shape, cf):
    return (shape[0], shape[-1]) + tuple(shape[1:-1]) if cf else tuple(shape)


def dev(ctx, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


@functools.lru_cache(maxsize=None)
def quant_case(shape, kind, int16_run):
    """inputs and references of one (shape, medians, width) -- computed once, shared by the channels_first / _last runs, read only"""
    med = R.medians_of(kind, shape[-1])
    v = R.quant_values(shape, med, int16_run)
    ref = {mode: R.quantize(v, med, mode) for mode in (R.FLOOR_HALF, R.HALF_EVEN)}
    return med, v, ref


@pytest.mark.parametrize('cf', [True, False], ids=['channels_first', 'channels_last'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_quantize_pack(ctx, shape, cf):
    ntiles = L.lib().pcc_symbols_tiles(shape[0], int(np.prod(shape[1:-1])), shape[-1])
    for kind in (None, 'dyadic', 'random'):
        for dst_bytes in (2, 4):
            med, v, ref = quant_case(shape, kind, dst_bytes == 2)
            vd, md = dev(ctx, v), dev(ctx, med)
            for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
                what = f'medians {kind}, dst_bytes {dst_bytes}, mode {mode}'
                dt = _TORCH[dst_bytes]
                sym, deq = Guarded(shape, torch.int32, ctx.device), Guarded(shape, torch.float32, ctx.device)
                dst, tm = Guarded(stream_shape(shape, cf), dt, ctx.device), Guarded((ntiles,), torch.int32, ctx.device)
                ops.quantize_pack(ctx, vd, md, mode, cf, dst.ptr(), dst_bytes, tm.ptr(), sym=sym.t, deq=deq.t)
                rsym, rdeq = ref[mode]
                assert_array_equal(sym.np(), rsym, err_msg=what)
                assert_array_equal(bits(deq.np()), bits(rdeq), err_msg=what)
                ssym, sdeq = ops.quantize(ctx, vd, md, mode)                    # the stand-alone kernel on the same input
                assert torch.equal(sym.t, ssym) and torch.equal(deq.t, sdeq), what
                assert_array_equal(dst.np(), R.to_stream(rsym, cf, dst.np().dtype), err_msg=what)
                assert_array_equal(tm.np(), R.tile_max(rsym), err_msg=what)
                for g, name in ((sym, 'sym'), (deq, 'deq'), (dst, 'dst'), (tm, 'tile_max')):
                    g.check(f'{name} ({what})')
                # deq = None (and no tile maxima): accepted, the other outputs unchanged
                sym2, dst2 = Guarded(shape, torch.int32, ctx.device), Guarded(stream_shape(shape, cf), dt, ctx.device)
                _, none = ops.quantize_pack(ctx, vd, md, mode, cf, dst2.ptr(), dst_bytes, None, want_deq=False, sym=sym2.t)
                assert none is None and torch.equal(sym2.t, sym.t) and torch.equal(dst2.t, dst.t), what
                sym2.check(f'sym without deq ({what})')
                dst2.check(f'dst without deq ({what})')


@functools.lru_cache(maxsize=None)
def index_case(shape, name):
    tab = R.scale_tables()[name]
    s = R.sigma_values(shape, tab)
    return tab, s, R.scale_index(s, tab)


@pytest.mark.parametrize('name', list(R.scale_tables()))
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_index_pack(ctx, shape, name):
    """NaN sigma is bounded to table[0] like every value that is not >= table[0] (test_pack_ref_cpu.py says why): the restatement,
    the stand-alone kernel and the fused kernel -- binary search on ascending tables, literal count on 'desc' / 'shuffled' -- agree."""
    tab, s, ref = index_case(shape, name)
    sd, td = dev(ctx, s), dev(ctx, tab)
    alone = ops.scale_to_index(ctx, sd, td)
    assert_array_equal(alone.cpu().numpy(), ref)
    for cf in (True, False):
        for dst_bytes in (1, 4):
            what = f'channels_first {cf}, dst_bytes {dst_bytes}'
            idx, dst = Guarded(shape, torch.int32, ctx.device), Guarded(stream_shape(shape, cf), _TORCH[dst_bytes], ctx.device)
            ops.index_pack(ctx, sd, td, cf, dst.ptr(), dst_bytes, idx=idx.t)
            assert_array_equal(idx.np(), ref, err_msg=what)
            assert torch.equal(idx.t, alone), what
            assert_array_equal(dst.np(), R.to_stream(ref, cf, dst.np().dtype), err_msg=what)
            idx.check(f'idx ({what})')
            dst.check(f'dst ({what})')


@pytest.mark.parametrize('dtype', [torch.int16, torch.int32, torch.uint8], ids=['int16', 'int32', 'uint8'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_unpack_dequantize(ctx, shape, dtype):
    npdt = {torch.int16: np.int16, torch.int32: np.int32, torch.uint8: np.uint8}[dtype]
    want = R.stream_values(shape, npdt)                                          # what the decoder must get back, NDHWC int32
    med = R.medians_of('random', shape[-1])
    for cf in (True, False):
        src = dev(ctx, R.to_stream(want, cf, npdt))
        assert_array_equal(R.from_stream(src.cpu().numpy(), shape, cf), want)    # the planted extremes fit the stream's type
        for m in (None, med):
            what = f'channels_first {cf}, medians {"none" if m is None else "random"}'
            md = dev(ctx, m)
            sym, deq = Guarded(shape, torch.int32, ctx.device), Guarded(shape, torch.float32, ctx.device)
            ops.unpack_dequantize(ctx, src, shape, cf, md, sym=sym.t, deq=deq.t)
            assert_array_equal(sym.np(), want, err_msg=what)
            assert_array_equal(bits(deq.np()), bits(R.dequantize(want, m)), err_msg=what)
            assert torch.equal(deq.t, ops.dequantize(ctx, sym.t.contiguous(), md)), what
            assert torch.equal(sym.t, ops.symbols_unpack(ctx, src, shape, cf)), what
            sym.check(f'sym ({what})')
            deq.check(f'deq ({what})')


def test_stand_alone_kernels_past_one_grid_pass(ctx, oracle):
    """k_quantize / k_dequantize / k_scale_index launch at most num_cu * 8 blocks of 256 threads and stride over the rest:
    2^21 + 77 elements are more than 256 CUs * 8 * 256 threads, so the stride loop makes further passes (the last one partial), and
    with C = 7 the channel i % C does not line up with the stride."""
    n, C = 2 ** 21 + 77, 7
    assert n > ctx.num_cu * 8 * 256, 'one grid pass covers the tensor: the test no longer reaches the stride loop'
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(n) * 3).astype(np.float32)
    v[-64:] = np.arange(-32, 32) + 0.5                                           # ties in the second pass
    med = R.medians_of('dyadic', C)
    pad = np.concatenate([v, np.zeros(-n % C, np.float32)]).reshape(-1, C)       # the oracle takes C from the last axis
    vd, md = dev(ctx, v), dev(ctx, med)
    for mode in (L.PCC_ROUND_FLOOR_HALF, L.PCC_ROUND_HALF_EVEN):
        osym, odeq = (a.ravel()[:n] for a in oracle.quantize(pad, med, mode))
        sym, deq = ops.quantize(ctx, vd, md, mode, channels=C)
        assert_array_equal(sym.cpu().numpy(), osym)
        assert_array_equal(bits(deq.cpu().numpy()), bits(odeq))
        assert_array_equal(bits(ops.dequantize(ctx, sym, md, channels=C).cpu().numpy()), bits(odeq))
    tab = R.scale_tables()['ref64']
    s = np.exp(rng.uniform(np.log(0.01), np.log(600), n)).astype(np.float32)
    near = np.concatenate([tab, np.nextafter(tab, np.float32(np.inf)), np.nextafter(tab, np.float32(-np.inf)), R.SIGMA_SPECIALS])
    s[:near.size], s[-near.size:] = near, near                                   # first and second pass
    idx = ops.scale_to_index(ctx, dev(ctx, s), dev(ctx, tab))
    assert_array_equal(idx.cpu().numpy(), oracle.scale_index(s, tab))
