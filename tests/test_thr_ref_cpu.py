"""The host reference of the fixed-threshold occupancy decision (tests/_thr_ref.py) checked without a GPU: the word packer against an
unpack that shares no code with it and against the C oracle's argwhere, the boundary thresholds, and the cases against the restated
launcher at 256 CUs."""
import numpy as np
import pytest

import _direct_cases as DC
import _thr_ref as TR


def _block(seed, shape=(4, 8, 16)):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.normal(0.5, 0.6, shape), -0.9).astype(np.float32)        # below 0 and above 1, never down to the threshold -1
    x[rng.random(shape) < 0.2] = 0.0
    x[rng.random(shape) < 0.1] = 1.0
    return x


def test_pack_words_puts_voxel_32j_plus_i_into_bit_i_of_word_j():
    sel = np.zeros((2, 4, 16), bool)
    for n in (0, 1, 31, 32, 33, 95, 127):
        sel.reshape(-1)[n] = True
    w = TR.pack_words(sel)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000003, 0x00000003, 0x80000000, 0x80000000]
    one = np.zeros((1, 2, 16), bool)
    one[0, 1, 3] = True                                       # voxel 16 + 3
    assert TR.pack_words(one).tolist() == [1 << 19]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_pack_unpack_round_trip(seed):
    x = _block(seed)
    sel = x > np.float32(0.5)
    words = TR.pack_words(sel)
    assert words.size == sel.size // 32
    assert np.array_equal(TR.unpack_words(words, sel.shape), sel)
    assert int(sum(bin(int(w)).count('1') for w in words)) == int(sel.sum())
    assert TR.pack_words(np.ones((2, 4, 4), bool)).tolist() == [0xFFFFFFFF]
    assert TR.pack_words(np.zeros((2, 4, 4), bool)).tolist() == [0]


@pytest.mark.parametrize('clip', [False, True])
def test_reference_equals_the_c_oracle_at_the_boundaries(oracle, clip):
    """Rows, counts and words against oracle.threshold_argwhere (C, float32 compare) for every recipe, the drawn one included: a voxel
    that equals its threshold is not selected."""
    x = _block(7)
    v = oracle.clip01(x) if clip else x
    for recipe in TR.RECIPES:
        thr = TR.drawn(x) if recipe == 'drawn' else np.float32(recipe)
        rows, count, words = TR.reference(x, thr, clip)
        want = oracle.threshold_argwhere(v, thr)
        assert rows.dtype == np.float32 and np.array_equal(rows, want) and count == len(want), recipe
        sel = TR.unpack_words(words, x.shape)
        assert np.array_equal(np.argwhere(sel).astype(np.float32), want), recipe
        if recipe == 'drawn':
            eq = TR.value(x, clip) == thr
            assert eq.any() and not sel[eq].any() and 0 < count < x.size
        if recipe == -1.0:
            assert count == x.size and set(words.tolist()) == {0xFFFFFFFF}
        if recipe == float('inf'):
            assert count == 0 and not words.any()
    # clipping decides the masses at 0 and 1: above 1 the decoder still selects at thr = 1, the encoder does not
    assert (x > 1).any() and (x < 0).any()
    assert TR.reference(x, 1.0, True)[1] == 0 and TR.reference(x, 1.0, False)[1] == int((x > 1).sum())
    assert TR.reference(x, 0.0, True)[1] == int((x > 0).sum()) and TR.reference(x, -0.0, False)[1] == int((x > 0).sum())


def test_recipes_are_normal_numbers_on_the_products_grid():
    vals = [r for r in TR.RECIPES if r != 'drawn']
    assert len(TR.RECIPES) == 12 and not any(np.isnan(v) for v in vals)
    tiny = np.finfo(np.float32).tiny
    assert all(v == 0 or abs(np.float32(v)) >= tiny for v in vals)
    assert np.signbit(np.float32(TR.RECIPES[2])) and TR.RECIPES[2] == 0.0
    assert np.float32(TR.RECIPES[4]) < 1 and np.nextafter(np.float32(TR.RECIPES[4]), np.float32(2)) == 1
    for i in (0, 1, 128, 254, 255):
        assert float(np.float32(np.linspace(0, 1.0, 256)[i])) in vals
    sets = TR.threshold_sets(np.stack([_block(s) for s in range(5)]))
    assert len(sets) == 3
    assert set(map(str, sum((r for _, r in sets), []))) == set(map(str, TR.RECIPES))
    assert len(TR.threshold_sets(np.stack([_block(s) for s in range(12)]))) == 1


def test_cases_reach_the_four_fusing_instantiations_at_256_cus():
    cases = TR.cases(256)
    assert [(c['res'], c['batch']) for c in cases] == [(16, 2), (32, 5), (64, 3), (64, 64), (64, 32), (64, 16), (128, 2), (8, 12)]
    named = set()
    for c in cases:
        for precision in ('fp32', 'fp16'):
            sel = TR.last_layer(c, precision, 256)
            assert sel['kernel'] == TR.kernel_name(c, precision), (c['id'], precision, sel)
            assert sel['zsp'] == c['zsp'] and sel['fused'] == (c['res'] % 16 == 0), (c['id'], sel)
            assert sel['kernel'] in DC.ALL_INSTANCES
            named.add(sel['kernel'])
    assert set(DC.GRAPH_ONLY) <= named
    assert {(c['T'], c['zsp']) for c in cases if c['T'] == 32} == {(32, 1), (32, 2), (32, 4), (32, 8)}
