"""CPU-only: the numpy restatements the threshold-compaction and voxelise GPU tests compare with (tests/_compact_cases.py) equal the
oracle's C loops (oracle/pcc_oracle.c) and model_types.sparse_to_dense on every block of the catalogue; every named block has the
property it is named for; and the catalogue tells small wrong variants of the restatement apart from the right one."""
import numpy as np
import pytest

import _compact_cases as K

f32 = np.float32


def _flat(rows, dhw):
    """float32 (x, y, z) rows -> voxel indexes (C order)"""
    r = rows.astype(np.int64)
    return (r[:, 0] * dhw[1] + r[:, 1]) * dhw[2] + r[:, 2]


def _rows(idx, dhw):
    idx = np.asarray(idx, np.int64)
    hw = dhw[1] * dhw[2]
    return np.stack([idx // hw, idx % hw // dhw[2], idx % hw % dhw[2]], -1).astype(np.float32).reshape(-1, 3)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('name', K.LAUNCHES)
def test_restatement_equals_the_oracle_on_every_block(oracle, name):
    dhw, blocks = K.launch(name)
    assert len(blocks) == 256 if name == K.ALL_256 else 30 <= len(blocks)
    for clip in (0, 1):
        for b, got in zip(blocks, K.refs(name, clip)):
            assert b.x.dtype == np.float32 and b.x.shape == dhw
            want = oracle.threshold_argwhere(oracle.clip01(b.x) if clip else b.x, b.thr)
            assert got.dtype == np.float32 and _same(got, want), (name, b.name, clip, len(got), len(want))


def test_shapes_cover_the_paths_they_are_listed_for():
    n = {s: int(np.prod(s)) for s in K.SHAPES}
    assert [n[s] for s in K.SHAPES] == [1, 3, 105, 1023, 1728, 4092, 4096, 4100, 4107, 4352, 8000, 33792]
    scalar = [s for s in K.SHAPES if n[s] % 4]
    assert [n[s] for s in scalar] == [1, 3, 105, 1023, 4107]
    assert max(-(-v // K.CHUNK) for v in n.values()) == 9 and n[(4, 25, 41)] - K.CHUNK == 4 and K.CHUNK - n[(4, 31, 33)] == 4
    assert sum(len(set(s)) == 3 for s in K.SHAPES) == 4                 # D, H, W pairwise distinct: a wrong split shows


@pytest.mark.parametrize('dhw', K.SHAPES, ids=K.shape_id)
def test_named_blocks_have_the_property_they_are_named_for(dhw):
    name = K.shape_id(dhw)
    _, blocks = K.launch(name)
    by = {b.name: (b, K.refs(name, 0)[i], K.refs(name, 1)[i]) for i, b in enumerate(blocks)}
    n = int(np.prod(dhw))
    chunks = -(-n // K.CHUNK)
    masks = K.patterns(dhw)
    for pat, mask in masks.items():                                        # the values realise the mask, clipped or not
        b, r0, r1 = by[pat]
        want = np.flatnonzero(mask.ravel())
        assert np.array_equal(_flat(r0, dhw), want) and np.array_equal(_flat(r1, dhw), want), pat
    hits = {pat: set(np.flatnonzero(m.ravel()).tolist()) for pat, m in masks.items()}
    assert hits['none'] == set() and hits['all'] == set(range(n)) and hits['first'] == {0} and hits['last'] == {n - 1}
    assert by['last'][1].tolist() == [[dhw[0] - 1, dhw[1] - 1, dhw[2] - 1]]
    assert ('chunk-seams' in hits) == (n >= K.CHUNK) and ('middle-chunk' in hits) == (chunks >= 3) and ('thread-seams' in hits) == (n > 255)
    if 'chunk-seams' in hits:
        assert hits['chunk-seams'] == {v for v in (4095, 4096, 8191, 8192) if v < n} and 4095 in hits['chunk-seams']
    if n > 4096:
        assert {4095, 4096} <= hits['chunk-seams']
    if n > 8192:
        assert {8191, 8192} <= hits['chunk-seams']
    if 'thread-seams' in hits:
        assert hits['thread-seams'] == {v for v in [255, 256] + list(range(1019, 1029)) if v < n}
    if 'middle-chunk' in hits:
        assert hits['middle-chunk'] == set(range(4096, 8192))
    for e in range(4):
        assert hits[f'lane{e}'] == set(range(e, n, 4))
    if n > 1:
        d, h, w = np.unravel_index(np.arange(n), dhw)
        assert hits['checkerboard'] == set(np.flatnonzero((d + h + w) % 2).tolist()) and 0 < len(hits['checkerboard']) < n
    if n >= 1000:
        assert 0 < len(hits['random1']) < 0.03 * n and 0.4 * n < len(hits['random50']) < 0.6 * n and 0.97 * n < len(hits['random99']) < n
    assert len({b.thr for b in blocks[:len(masks)]}) == len(masks)          # a threshold of its own per pattern block
    for thr in K.VALUE_THRS:
        tag = f'thr{int(np.flatnonzero(K.LINSPACE == thr)[0])}'
        t = f32(thr)
        b, r0, r1 = by[f'equal-{tag}']
        assert b.thr == thr and (b.x == t).all() and len(r0) == len(r1) == 0
        b, r0, r1 = by[f'ulp-{tag}']
        up, down = b.x == np.nextafter(t, f32(np.inf)), b.x == np.nextafter(t, f32(-np.inf))
        assert (up | down).all() and (n == 1 or (up.any() and down.any()))
        assert np.array_equal(_flat(r0, dhw), np.flatnonzero(up.ravel()))
        assert np.array_equal(_flat(r1, dhw), np.flatnonzero(up.ravel()) if thr < 1 else [])   # one ulp above 1 is clipped to 1
        held = np.concatenate([by[k][0].x.ravel() for k in by if k.startswith('special') and k.endswith('-' + tag)]).view(np.uint32)
        assert set(K.SPECIALS.view(np.uint32).tolist()) <= set(held.tolist())
    assert np.isnan(K.SPECIALS[0]) and K.SPECIALS[4] == f32(2.0 ** -149) and K.SPECIALS[5] == f32(2.0 ** -126) - f32(2.0 ** -149)
    assert np.signbit(K.SPECIALS[3]) and K.SPECIALS[3] == 0 and K.SPECIALS[8] == 1 + f32(2.0 ** -23)
    for thr in K.BAD_THRS:
        for kind in ('special0', 'uniform'):
            b, r0, r1 = by[f'{kind}-bad{thr}']
            assert np.array_equal(b.thr, thr, equal_nan=True)
            nan = np.isnan(b.x)
            assert nan.any() == (kind == 'special0')
            if np.isnan(thr) or thr == np.inf:
                assert len(r0) == len(r1) == 0
            else:                                                           # clipped, every voxel but the NaN ones is above a negative threshold
                assert np.array_equal(_flat(r1, dhw), np.flatnonzero(~nan.ravel()))
                assert len(r0) <= len(r1)


def test_all_256_thresholds_block_t_sits_on_threshold_t():
    dhw, blocks = K.launch(K.ALL_256)
    assert dhw == (5, 7, 3) and len(blocks) == 256
    for t, b in enumerate(blocks):
        v = f32(np.linspace(0, 1.0, 256)[t])
        assert b.thr == K.LINSPACE[t]
        at, up, down = b.x == v, b.x == np.nextafter(v, f32(np.inf)), b.x == np.nextafter(v, f32(-np.inf))
        assert at.any() and up.any() and down.any() and (at | up | down).all()
        assert np.array_equal(_flat(K.refs(K.ALL_256, 0)[t], dhw), np.flatnonzero(up.ravel()))


def test_cap_case_has_mixed_counts_and_caps_on_both_sides_of_them():
    dhw, blocks, caps = K.cap_case()
    counts = [len(r) for r in K.launch_ref(blocks, 1)]
    n = int(np.prod(dhw))
    assert dhw == (17, 16, 16) and 0 in counts and max(counts) == n - 1 and len(set(counts)) >= 6
    assert caps == [0, 1, 2, n - 2, n - 1, n, n + 5] and min(c for c in counts if c) == 2
    assert sum(b.thr < 0 for b in blocks) == 2                              # thr < 0 under clip: what a hittable tail shows on, cap > D*H*W


# ---- mutants: small wrong variants of the restatement; each has to differ from it on at least one block -------------------------
def _clipped(x, clip):
    with np.errstate(invalid='ignore'):
        return np.clip(x, 0, 1) if clip else x


def _m_greater_equal(x, thr, clip):
    with np.errstate(invalid='ignore'):
        return np.argwhere(_clipped(x, clip) >= f32(thr)).astype(np.float32)


def _m_hw_swapped(x, thr, clip):
    D, H, W = x.shape
    idx = _flat(K.argwhere_ref(x, thr, clip), x.shape)
    r = idx % (H * W)
    return np.stack([idx // (H * W), r // H, r % H], -1).astype(np.float32).reshape(-1, 3)


def _m_hittable_tail(x, thr, clip):
    """the voxels past D*H*W of the last chunk are padded with -inf BEFORE the clip, which turns them into 0"""
    flat = np.full(-(-x.size // K.CHUNK) * K.CHUNK, -np.inf, np.float32)
    flat[:x.size] = x.ravel()
    with np.errstate(invalid='ignore'):
        return _rows(np.flatnonzero(_clipped(flat, clip) > f32(thr)), x.shape)


def _m_nan_clipped_to_zero(x, thr, clip):
    v = np.fmin(np.fmax(x, f32(0)), f32(1)) if clip else x                # fmaxf(NaN, 0) = 0
    with np.errstate(invalid='ignore'):
        return np.argwhere(v > f32(thr)).astype(np.float32)


def _m_float64_compare(x, thr, clip):
    with np.errstate(invalid='ignore'):
        return np.argwhere(_clipped(x, clip).astype(np.float64) > np.float64(thr)).astype(np.float32)


def _caught_by(mutant, whole_launch=False):
    """[(launch, block, clip)] on which the mutant's result differs from the restatement's"""
    out = []
    for name in K.LAUNCHES:
        _, blocks = K.launch(name)
        for clip in (0, 1):
            got = mutant(blocks, clip) if whole_launch else K.launch_ref(blocks, clip, mutant)
            out += [(name, b.name, clip) for b, g, r in zip(blocks, got, K.refs(name, clip)) if not _same(g, r)]
    return out


def test_catalogue_catches_greater_equal():
    caught = _caught_by(_m_greater_equal)
    assert caught and all(any(c[0] == K.shape_id(s) and c[1].startswith('equal-') for c in caught) for s in K.SHAPES)


def test_catalogue_catches_h_and_w_swapped():
    caught = _caught_by(_m_hw_swapped)
    distinct = [s for s in K.SHAPES if s[1] != s[2] and int(np.prod(s)) > 3]
    assert len(distinct) >= 4 and all(any(c[0] == K.shape_id(s) for c in caught) for s in distinct)


def test_catalogue_catches_a_hittable_tail():
    caught = _caught_by(_m_hittable_tail)
    partial = [s for s in K.SHAPES if int(np.prod(s)) % K.CHUNK]
    assert len(partial) == len(K.SHAPES) - 1
    for s in partial:                                                       # on every shape with a partial last chunk, and only under clip
        assert any(c[0] == K.shape_id(s) and 'bad-' in c[1] for c in caught), s
    assert all(c[2] == 1 for c in caught) and not any(c[0] == '16x16x16' for c in caught)


def test_catalogue_catches_nan_clipped_to_zero():
    caught = _caught_by(_m_nan_clipped_to_zero)
    assert all(c[2] == 1 and c[1].startswith('special') for c in caught)
    assert all(any(c[0] == K.shape_id(s) for c in caught) for s in K.SHAPES)


def test_catalogue_catches_a_float64_compare():
    caught = _caught_by(_m_float64_compare)
    assert any(c[0] == K.ALL_256 for c in caught) and any(c[0] != K.ALL_256 for c in caught)


def test_catalogue_catches_every_block_reading_the_first_threshold():
    caught = _caught_by(lambda blocks, clip: [K.argwhere_ref(b.x, blocks[0].thr, clip) for b in blocks], whole_launch=True)
    assert all(any(c[0] == name for c in caught) for name in K.LAUNCHES)


# ---- voxelise ---------------------------------------------------------------------------------------------------------------------
def _all_voxel_cases():
    return [c for g in K.GRIDS for c in K.voxel_cases(g)] + [K.voxel_grid_pass_case(256)]


def test_voxelize_restatement_equals_sparse_to_dense_on_every_in_range_case():
    from pcc_geo_cnn_v2_amd.model_types import sparse_to_dense
    seen = 0
    for c in _all_voxel_cases():
        D, H, W = c.dhw
        ext = np.array(c.dhw)
        bof = np.zeros(len(c.pts), np.int64) if c.block_of is None else c.block_of.astype(np.int64)
        inside = ((c.pts >= 0) & (c.pts < ext)).all(1) & (bof >= 0) & (bof < c.B)
        assert inside.all() == c.in_range, c.name
        got = K.voxelize_ref(c.pts, c.block_of, c.B, D, H, W)
        assert got.dtype == np.float32 and got.shape == (c.B, D, H, W) and set(np.unique(got).tolist()) <= {0.0, 1.0}
        assert int(got.sum()) == len(np.unique(np.column_stack([bof[inside], c.pts[inside]]), axis=0)), c.name
        if not c.in_range:
            continue
        seen += 1
        if c.name.startswith('grid-pass'):                                  # the first 5 and the last 5 points own their voxels
            assert len(c.pts) == 256 * 8 * 256 + 5 and c.B == 4 and c.dhw == (16, 16, 16) and got[..., 15].sum() == 10
        for b in range(c.B):
            want = sparse_to_dense(c.pts[bof == b].astype(np.float64), (1, 1, D, H, W), 'channels_first')[0, 0]
            assert np.array_equal(got[b], want), (c.name, c.dhw, b)
    assert seen == 3 * 9 + 1


@pytest.mark.parametrize('dhw', K.GRIDS, ids=K.shape_id)
def test_voxel_cases_have_the_property_they_are_named_for(dhw):
    D, H, W = dhw
    by = {c.name: c for c in K.voxel_cases(dhw)}
    assert [by[f'axis{a}'].pts.tolist() for a in range(3)] == [[[D - 1, 0, 0]], [[0, H - 1, 0]], [[0, 0, W - 1]]]
    assert len(set(map(tuple, by['corners'].pts.tolist()))) == 8
    faces = K.voxelize_ref(by['faces'].pts, None, 1, D, H, W)[0]
    inner = np.zeros(dhw, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert np.array_equal(faces == 0, inner)
    assert len(by['repeat'].pts) == 1000 and len(set(map(tuple, by['repeat'].pts.tolist()))) == 1
    out = by['coordinates-outside'].pts
    for a, ext in enumerate(dhw):
        assert {-1, ext, K.I32_MIN, K.I32_MAX} <= set(out[:, a].tolist())
    assert {-1, 3, K.I32_MAX} <= set(by['block-outside'].block_of.tolist()) and by['block-outside'].B == 3
    assert by['no-block-of-B1'].block_of is None and by['no-block-of-B3'].block_of is None
    assert (by['no-block-of-B1'].B, by['no-block-of-B3'].B) == (1, 3)
    assert K.voxelize_ref(by['no-block-of-B3'].pts, None, 3, D, H, W)[1:].sum() == 0
    assert len(by['no-points'].pts) == 0
