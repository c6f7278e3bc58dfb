"""CPU-only: the numpy restatement the fused quantise / index / pack GPU tests compare with (tests/_pack_ref.py) equals the
oracle's C loops bit for bit on the very input sets those tests use -- so a GPU mismatch is the kernel's -- and its permutation /
tile-maximum helpers are what their definitions say.

Special sigma values.  The reference computes the row as `len(table) - 1 - #{j : scale <= table[j]}` over table[:-1]
(src/utils/patch_gaussian_conditional.py:104-116) on a scale that :57-58 has already lower-bounded at table[0].  The
specification here is include/pcc_geo.h's C restatement of that, which the oracle (oracle/pcc_oracle.c) and _pack_ref.scale_index
both spell out: the bound is `s >= table[0] ? s : table[0]`, every comparison with NaN is false.  Hence 0 and -1 take table[0]'s
row, +inf takes row L-1, and NaN is bounded to table[0] like any other value that is not >= table[0] (tf.maximum would hand NaN
on and :112 would then count nothing, i.e. row L-1; no finite network output gets there, and what matters to the codec is that
encoder and decoder agree).  The oracle and the literal count agree on all four (asserted below), so the GPU tests keep them in
and compare with the restatement AND with the stand-alone kernel.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _pack_ref as R

SHAPE_IDS = [R.shape_id(s) for s in R.SHAPES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('shape', R.SHAPES, ids=SHAPE_IDS)
def test_quantisers_equal_the_oracle_bit_for_bit(oracle, shape):
    for kind in (None, 'dyadic', 'random'):
        med = R.medians_of(kind, shape[-1])
        for int16_run in (False, True):
            v = R.quant_values(shape, med, int16_run)
            for mode in (R.FLOOR_HALF, R.HALF_EVEN):
                sym, deq = R.quantize(v, med, mode)
                osym, odeq = oracle.quantize(v, med, mode)
                assert sym.dtype == np.int32 and deq.dtype == np.float32
                assert_array_equal(sym, osym, err_msg=f'{kind} {int16_run} {mode}')
                assert_array_equal(bits(deq), bits(odeq), err_msg=f'{kind} {int16_run} {mode}')
                assert_array_equal(bits(R.dequantize(sym, med)), bits(odeq))


def test_planted_ties_are_ties_and_land_in_every_tile():
    """the inputs hold what they claim: with dyadic (or no) medians v - m is exactly k + 0.5 for all 64 k in every tile, so the
    two rounding modes differ there (floor(x + 0.5) rounds half up, rint half to even)"""
    for shape in R.SHAPES:
        for kind in (None, 'dyadic'):
            med = R.medians_of(kind, shape[-1])
            v = R.quant_values(shape, med, True)
            d = (v.astype(np.float64) - (0 if med is None else med.astype(np.float64))).reshape(shape[0], -1, shape[-1])
            v3 = v.reshape(d.shape)
            for _, n, vs, cs in R.tiles(shape):
                have = set(d[n, vs, cs].ravel().tolist())
                assert all(k + 0.5 in have for k in range(-32, 32)), (shape, kind)
                t = v3[n, vs, cs].ravel()
                assert np.float32(0.49999997) in t and np.float32(40000) in t and np.float32(-32767.4) in t
                assert np.any((t == 0) & np.signbit(t))
            a, _ = R.quantize(v, med, R.FLOOR_HALF)
            assert len(set(R.tile_max(a).tolist())) == sum(1 for _ in R.tiles(shape))      # every tile has a maximum of its own
            b, _ = R.quantize(v, med, R.HALF_EVEN)
            assert np.count_nonzero(a != b) >= 32 * sum(1 for _ in R.tiles(shape))      # the odd-k ties of every tile


@pytest.mark.parametrize('name', list(R.scale_tables()))
def test_literal_count_equals_the_oracle_on_every_table(oracle, name):
    tab = R.scale_tables()[name]
    if name == 'ref64':
        assert_array_equal(tab, oracle.scale_table().astype(np.float32))
    for shape in R.SHAPES:
        s = R.sigma_values(shape, tab)
        for special in R.SIGMA_SPECIALS:                        # 0, -1, +inf, NaN: in every tile
            hit = np.isnan(s) if np.isnan(special) else s == special
            h3 = hit.reshape(shape[0], -1, shape[-1])
            assert all(h3[n, vs, cs].any() for _, n, vs, cs in R.tiles(shape))
        got, want = R.scale_index(s, tab), oracle.scale_index(s, tab)
        assert got.dtype == np.int32 and got.min() >= 0 and got.max() <= len(tab) - 1
        assert_array_equal(got, want, err_msg=f'{name} {shape}')
    # what the special values come to (module docstring): the same in the oracle and in the literal count
    sp = R.scale_index(R.SIGMA_SPECIALS, tab)
    assert_array_equal(sp, oracle.scale_index(R.SIGMA_SPECIALS, tab))
    row0 = int(R.scale_index(tab[:1], tab)[0])
    assert sp[0] == sp[1] == sp[3] == row0 and sp[2] == len(tab) - 1
    if name in ('ref64', 'asc256', 'L2'):                       # strictly ascending: table[j] itself takes row j, its successor row j + 1
        assert_array_equal(R.scale_index(tab, tab), np.arange(len(tab)))
        up = np.nextafter(tab, np.float32(np.inf))
        assert_array_equal(R.scale_index(up, tab), np.minimum(np.arange(len(tab)) + 1, len(tab) - 1))


def test_every_table_value_and_its_neighbours_are_planted_somewhere():
    for name, tab in R.scale_tables().items():
        seen = set()
        for shape in R.SHAPES:
            seen |= set(R.sigma_values(shape, tab).ravel().tolist())
        near = np.concatenate([tab, np.nextafter(tab, np.float32(np.inf)), np.nextafter(tab, np.float32(-np.inf))])
        assert all(float(x) in seen for x in near), name


def test_stream_order_narrowing_and_tile_maxima():
    rng = np.random.default_rng(0)
    shape = (2, 5, 3, 7, 66)
    x = rng.integers(-70000, 70000, shape).astype(np.int32)
    x[1, 4, 2, 6, 65] = -80000
    cf = R.to_stream(x, True, np.int16)
    assert cf.shape == (2, 66, 5, 3, 7) and cf.dtype == np.int16
    for n, d, h, w, c in [(0, 0, 0, 0, 0), (1, 4, 2, 6, 65), (1, 2, 1, 3, 17)]:
        want = ((int(x[n, d, h, w, c]) + 32768) % 65536) - 32768                      # two's-complement wrap
        assert int(cf[n, c, d, h, w]) == want
    assert_array_equal(R.to_stream(x, False, np.int32), x)
    assert_array_equal(R.from_stream(R.to_stream(x, True, np.int32), shape, True), x)
    assert_array_equal(R.from_stream(R.to_stream(x, False, np.int32), shape, False), x)
    rows = np.abs(x) % 300
    assert_array_equal(R.to_stream(rows, True, np.uint8), np.moveaxis(rows % 256, -1, 1))
    with pytest.raises(AssertionError):
        R.to_stream(x, True, np.uint8)
    # tile maxima: 105 voxels x 66 channels -> 2 x 2 tiles per block, channel tile fastest
    tm = R.tile_max(x)
    assert tm.shape == (8,) and tm.dtype == np.int32
    x3 = np.abs(x.reshape(2, 105, 66))
    assert tm[0] == x3[0, :64, :64].max() and tm[1] == x3[0, :64, 64:].max() and tm[2] == x3[0, 64:, :64].max()
    assert tm[7] == x3[1, 64:, 64:].max() == 80000
    for dtype, ext in ((np.uint8, [255]), (np.int16, [32767, -32767, -32768]), (np.int32, [70000, -70000])):
        for shp in R.SHAPES:
            s3 = R.stream_values(shp, dtype).reshape(shp[0], -1, shp[-1])
            assert all(e in s3[n, vs, cs] for e in ext for _, n, vs, cs in R.tiles(shp))


def test_flat_channel_rule_of_the_stand_alone_kernels(oracle):
    """channel of element i = i % C on a flat tensor whose length is no multiple of C (the large stand-alone GPU test uses C = 7)"""
    rng = np.random.default_rng(1)
    n, C = 1000 * 7 + 3, 7
    v = (rng.standard_normal(n) * 3).astype(np.float32)
    med = R.medians_of('random', C)
    pad = np.concatenate([v, np.zeros(C - n % C, np.float32)]).reshape(-1, C)
    for mode in (R.FLOOR_HALF, R.HALF_EVEN):
        sym, deq = R.quantize(v, med, mode, channels=C)
        osym, odeq = oracle.quantize(pad, med, mode)
        assert_array_equal(sym, osym.ravel()[:n])
        assert_array_equal(bits(deq), bits(odeq.ravel()[:n]))
        assert_array_equal(bits(R.dequantize(sym, med, channels=C)), bits(odeq.ravel()[:n]))
