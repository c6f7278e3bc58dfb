"""CPU: the catalogue of tests/_search_adversarial.py is what it claims to be -- shapes, types, the size cap of the brute force, the
grouping of thresholds into distinct level sets, and the property every family is named after -- and the reachability fact the
product rests on: under clip with linspace(0, 1, 256) no float32 has a level above 255."""
import time

import numpy as np
import pytest

import _search_adversarial as A
import _ties_ref as R

CAT = A.catalogue()


def _mask(case, b, t):
    x = case.x_hat[b]
    return (np.clip(x, 0, 1) if case.clip else x) > np.float32(case.thr[t])


def test_the_catalogue_holds_every_family_the_search_can_go_wrong_on():
    fam = {c.family for c in CAT.values()}
    assert fam == {'far', 'empty', 'maskword', 'envelope', 'ties', 'levels', 'chunk', 'noncubic', 'level256'}
    shapes = {c.shape for c in CAT.values()}
    assert {(128, 128, 128), (4, 128, 128), (2, 128, 64), (2, 64, 64), (8, 24, 16), (6, 10, 12), (64, 64, 64)} <= shapes
    assert all(max(c.shape) <= 32 for c in CAT.values() if c.family in ('empty', 'ties', 'levels', 'level256'))
    assert all(len(c.blocks) == 1 for c in CAT.values() if max(c.shape) == 128)


@pytest.mark.parametrize('name', A.names(reference=False))
def test_shapes_types_and_thresholds(name):
    c = CAT[name]
    B = len(c.blocks)
    assert c.x_hat.dtype == np.float32 and c.x_hat.shape == (B,) + c.shape and max(c.shape) <= 128
    assert c.thr.dtype == np.float32 and 1 <= len(c.thr) <= 256 and np.all(np.diff(c.thr) > 0)
    for blk in c.blocks:
        assert blk.dtype == np.float64 and blk.ndim == 2 and blk.shape[1] == 6 and 1 <= len(blk) <= A.MAX_ROWS
        xyz = blk[:, :3]
        assert np.array_equal(xyz, np.round(xyz)) and xyz.min() >= 0 and np.all(xyz.max(0) < np.array(c.shape))
        assert len(np.unique(xyz, axis=0)) == len(xyz)
        assert np.allclose(np.linalg.norm(blk[:, 3:], axis=1), 1.0, rtol=1e-12)


@pytest.mark.parametrize('name', A.names())
def test_thresholds_are_grouped_by_level_set_and_the_reference_stays_within_the_cap(name, oracle):
    """Level sets are nested, so two thresholds with equal masks share every mask between them: the first and the last threshold of a
    group give the same mask, the threshold after it another one, and the set is empty from tcount on.  Both references then run, each
    within the size cap (asserted inside them) and in about the time the cap was chosen for; their exact columns agree."""
    c = CAT[name]
    t0 = time.perf_counter()
    for b in range(len(c.blocks)):
        tcount, groups = A.level_groups(c.x_hat[b], c.thr, c.clip)
        assert [lo for lo, _ in groups] == ([0] + [hi for _, hi in groups])[:len(groups)] and (groups[-1][1] if groups else 0) == tcount
        for lo, hi in groups:
            first = _mask(c, b, lo)
            assert first.any() and first.sum() <= A.MAX_SET and np.array_equal(first, _mask(c, b, hi - 1))
            assert hi == len(c.thr) or _mask(c, b, hi).sum() < first.sum()
        assert tcount == len(c.thr) or not _mask(c, b, tcount).any()
        tp, pick = A.reference_pick(name, b)
        tm, mean = A.reference_mean(name, b)
        assert tp == tm == tcount == len(pick) and len(mean) == len(groups)
        for lo, hi, ref, bounds, pairs in mean:
            assert np.array_equal(pick[lo:hi, :3], np.tile(ref['tally'][:3], (hi - lo, 1)))
            assert pairs >= len(c.blocks[b]) and all(np.isfinite(bounds))
    assert time.perf_counter() - t0 < 60 * len(c.blocks)


# ---- the named property of every family -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', A.names('far'))
def test_far_corner_cases_reach_the_largest_distance_of_the_grid(name):
    c = CAT[name]
    _, mean = A.reference_mean(name, 0)
    got = max(max(ref['tally'][5], ref['tally'][6]) for _, _, ref, _, _ in mean)
    assert got == c.props['max_d2']
    assert c.props['max_d2'] == (127 ** 2 if name == 'far_corners_to_face' else 48387)


def test_three_far_corner_cases_carry_48387_and_it_fits_uint16_unsaturated():
    assert sum(CAT[n].props['max_d2'] == 3 * 127 ** 2 == 48387 for n in A.names('far')) == 3 and 48387 < 65535


@pytest.mark.parametrize('name', A.names('ties'))
def test_tie_cases_hold_a_tie_set_and_a_voxel_chosen_by_two_rows(name):
    c = CAT[name]
    _, mean = A.reference_mean(name, 0)
    assert any(ref['C'] > 1 for _, _, ref, _, _ in mean) and any(ref['V'] > 1 for _, _, ref, _, _ in mean)
    b_t = np.argwhere(_mask(c, 0, 0))
    rows, vox, _ = R.tie_sets(b_t, c.blocks[0][:, :3].astype(np.int64))
    assert np.bincount(rows).max() > 1 and np.bincount(vox, minlength=len(b_t)).max() > 1
    if 'orphan' in c.props:
        chosen = {tuple(v) for v in b_t[vox]}
        assert tuple(c.props['orphan']) not in chosen and tuple(c.props['orphan']) in {tuple(v) for v in b_t}
        assert sum(tuple(v) == tuple(c.props['shared']) for v in b_t[vox]) == 2
        sizes = np.bincount(rows)
        assert (sizes == 2).sum() == 13          # one row midway along each of the 13 axis and diagonal directions


def test_midway_rows_resolve_to_the_lowest_xyz():
    """The reference of the `pick` engine takes the first minimum in argwhere order: for every midway row that is centre - direction."""
    c = CAT['ties32_midway']
    a = c.blocks[0][:, :3].astype(np.int64)
    b_t = np.argwhere(_mask(c, 0, 0))
    d = ((a[:, None, :] - b_t[None, :, :]) ** 2).sum(-1)
    tied = (d == d.min(1, keepdims=True)).sum(1) == 2
    pick = b_t[d.argmin(1)]
    assert tied.sum() == 13 and all(tuple(p) < tuple(r) for p, r in zip(pick[tied], a[tied]))


def test_levels_cases_populate_what_they_say():
    c = CAT['levels_at_and_above_every_threshold']
    lev = A.levels_of(c.x_hat[0], c.thr, c.clip)
    assert np.array_equal(lev[tuple(c.props['voxels'].T)], c.props['expect'])
    assert len(np.unique(lev[lev > 0])) == c.props['populated'] == 255 and lev.max() == 255
    for k in (0, 1, 100, 254, 255):              # equal to threshold k: not selected by it; the next float32: selected
        at, above = c.props['voxels'][k], c.props['voxels'][256 + k]
        assert not _mask(c, 0, k)[tuple(at)] and (_mask(c, 0, k)[tuple(above)] or k == 255)
    c = CAT['levels_specials']
    assert np.array_equal(A.levels_of(c.x_hat[0], c.thr, c.clip)[tuple(c.props['voxels'].T)], c.props['expect'])
    assert A.level_groups(CAT['levels_all_one'].x_hat[0], A.T256, True) == (255, [(0, 255)])
    c = CAT['levels_empty_beside_full']
    assert [A.level_groups(x, c.thr, c.clip)[0] for x in c.x_hat] == c.props['tcounts'] == [0, 255]


@pytest.mark.parametrize('name', [n for n in A.names() if 'changes' in CAT[n].props])
def test_chunk_boundary_cases_change_the_level_set_exactly_at_the_boundaries(name):
    """n_B changes at the stated thresholds and nowhere else below tcount; every change is a multiple of a chunk size given by the
    formulae of the kernels' host code, and no other change lies within two thresholds of it."""
    c = CAT[name]
    B, nvox = len(c.blocks), int(np.prod(c.shape))
    npts = sum(len(b) for b in c.blocks)
    sizes = {'chunk_d2_16': {A.ties_chunk(B, *c.shape), A.d2_chunk(B, nvox, npts)}}.get(name, {A.d1_chunk(B, nvox)})
    assert all(any(t % s == 0 for s in sizes) for t in c.props['changes'])
    if name == 'chunk_d2_16':            # every boundary of both D2 engines
        assert c.props['changes'] == sorted({s * k for s in sizes for k in range(1, 256) if s * k <= 250}) and len(c.props['changes']) >= 3
    for b in range(B):
        tcount, pick = A.reference_pick(name, b)
        n_b = pick[:, 0]
        assert [t for t in range(1, tcount) if n_b[t] != n_b[t - 1]] == c.props['changes']
        assert tcount - c.props['changes'][-1] > 2 and all(q - p > 2 for p, q in zip([0] + c.props['changes'], c.props['changes']))
        for t in c.props['changes']:
            assert not np.array_equal(pick[t - 1], pick[t])
    assert A.d1_chunk(1, 128 ** 3) == 128 and A.d1_chunk(5, 64 ** 3) == 204 and A.d1_chunk(4, 32 ** 3) == 256


def test_equal_parabola_cases_have_distinct_minimisers_of_equal_value():
    """In the plane x = 0 the row (20, 20) is 10 away from (10, 20) and from (20, 30); in the plane x = 1 a third voxel (30, 20) joins
    them: F(10) = 100, F(20) = 500, F(30) = 900 make both of the envelope's intersection abscissae exactly 20."""
    for H in (128, 64):
        c = CAT[f'envelope{H}_equal_parabolas']
        a = c.blocks[0][:, :3].astype(np.int64)
        b_t = np.argwhere(_mask(c, 0, 0))
        for row, want in zip(c.props['equal_rows'], (2, 3)):
            assert (a == row).all(1).any()
            plane = b_t[b_t[:, 0] == row[0]]
            d = ((plane - row) ** 2).sum(1)
            assert (d == d.min()).sum() == want and d.min() == 100
        assert (500 - 100) * (30 - 20) == (900 - 500) * (20 - 10)        # the pop test's two sides
        assert 500 - 2 * 20 * 20 == 100 - 2 * 20 * 10                    # the take-over test's two sides at p = 20


def test_mask_word_cases_keep_rows_and_columns_in_different_words():
    for name in A.names('maskword'):
        c = CAT[name]
        z_set = np.unique(np.argwhere(_mask(c, 0, 0))[:, 2]).tolist()
        z_rows = c.blocks[0][:, 2]
        assert z_set == c.props['columns']
        if len({z >> 6 for z in z_set}) == 1:
            assert set((z_rows.astype(int) >> 6).tolist()) == {1 - (z_set[0] >> 6)}
        else:
            assert {0, 1} == set((z_rows.astype(int) >> 6).tolist())


# ---- what the product can reach -------------------------------------------------------------------------------------------------------
def test_no_float32_reaches_level_256_under_clip_and_the_products_thresholds():
    """The encoder clips x_hat to [0, 1] and searches linspace(0, 1, 256): the largest float32 after the clip is 1.0 = thr[255], which
    is not above it.  Every float32 is covered by monotonicity: the level is non-decreasing in the clipped value, and the clipped
    value is at most 1.0.  NaN survives the clip and compares false: level 0.  Without the clip 1.5 is above all 256 thresholds."""
    thr = np.linspace(0, 1.0, 256).astype(np.float32)
    assert thr[255] == np.float32(1.0) and np.all(np.diff(thr) > 0)
    big = np.finfo(np.float32).max
    x = np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, big, np.inf, np.nan, -np.inf, -1.0, 0.0, -0.0,
                  np.nextafter(np.float32(1), np.float32(0))], np.float32)
    count = lambda v: np.array([(e > thr).sum() for e in v])
    clipped = np.clip(x, 0, 1)
    assert count(clipped).tolist() == [255, 255, 255, 255, 255, 0, 0, 0, 0, 0, 255]
    assert np.array_equal(A.levels_of(x, thr, True), count(clipped))
    assert np.nanmax(clipped) == 1.0 and count(np.array([1.0], np.float32))[0] == 255
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32)      # any float32 bit pattern
    assert A.levels_of(bits, thr, True).max() <= 255
    assert count(x)[2] == 256 and A.levels_of(x, thr, False)[2] == 256
    for name in A.names('level256', reference=False):
        c = CAT[name]
        tcounts = [A.level_groups(xh, c.thr, c.clip)[0] for xh in c.x_hat]
        assert [b for b, t in enumerate(tcounts) if t == 256] == c.props['blocks'] and len(c.thr) == 256
