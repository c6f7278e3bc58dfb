"""CPU: the hash input generator of the recorded-bits tests, and the bookkeeping around tests/golden/family_bits.json and the committed
streams -- what must fail on ANY machine when PCC_KERNEL_FAMILY is bumped without a regeneration or a case is dropped silently."""
import json
import os

import numpy as np

import _bits_ref as BR
import _codec_pins as CP
import _family_cases as FC


def _golden():
    with open(FC.GOLDEN) as fh:
        return json.load(fh)


def test_hash_generator_values_are_pinned():
    """splitmix64 against its published first outputs for seed 0 (Steele, Lea, Flood 2014; the constants of java.util.SplittableRandom), FNV-1a
    against its published vectors, and a few elements of every kind."""
    assert [int(v) for v in BR.splitmix64(0, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert BR.tag_seed('') == 0xCBF29CE484222325 and BR.tag_seed('a') == 0xAF63DC4C8601EC8C
    assert BR.tag_seed('pin') == 0x77AF761956600B54
    act = BR.tensor('pin', (2, 3), 'act')
    assert act.dtype == np.float32 and act.shape == (2, 3)
    assert (act * 4096).tolist() == [[-6853.0, -5237.0, -6150.0], [0.0, 0.0, -1983.0]]
    assert (BR.tensor('pin', (3,), 'residual') * 4096).tolist() == [-6853.0, -5237.0, -6150.0]
    assert (BR.tensor('pin', (4,), 'bias') * 4096).tolist() == [-709.0, 907.0, -6.0, -361.0]
    w = BR.tensor('pin', (1, 1, 1, 2, 2), 'weight')             # fan_in 2: (k / 2^12) / sqrt(2) rounded to fp32 once
    k = np.array([-2757.0, -1141.0, -2054.0, 1687.0])
    assert np.array_equal(w.reshape(-1), (k / 4096 / np.sqrt(2.0)).astype(np.float32))
    assert np.array_equal(BR.tensor('pin', (1, 1, 1, 2, 2), 'weight', fan_in=1).reshape(-1), (k / 4096).astype(np.float32))
    # element i depends on (tag, i) only: a longer tensor starts with the shorter one; another tag gives other values
    assert np.array_equal(BR.tensor('pin', (7,), 'act')[:6], act.reshape(-1))
    assert not np.array_equal(BR.tensor('pim', (2, 3), 'act'), act)
    big = BR.tensor('stat', (200000,), 'act')
    assert 0.29 < np.mean(big == 0) < 0.31 and -2 <= big.min() and big.max() < 2 and abs(float(big.mean())) < 0.02
    assert np.array_equal(big * 4096, np.round(big * 4096))
    assert BR.digest(np.arange(4, dtype=np.float32)) == BR.digest(np.arange(8, dtype=np.float32)[:4])
    assert len(BR.digest(act)) == 32


def test_golden_family_number_is_the_header_s():
    """Bumping PCC_KERNEL_FAMILY without regenerating the recorded bits (or the reverse) fails here."""
    g = _golden()
    assert g['family'] == g['header']['kernel_family'] == FC.family_number()
    assert g['header']['num_cu'] > 0 and g['header']['rocm'] and g['header']['kernels_of_commit']


def test_golden_cases_are_the_case_table():
    g = _golden()
    assert sorted(g['cases']) == sorted(FC.BY_ID), 'a case was dropped, added or renamed without regenerating tests/golden/family_bits.json'
    for cid, e in g['cases'].items():
        c = FC.BY_ID[cid]
        assert e['family'] == c['family'] and tuple(e['shape']) == c['geo'] and len(e['digest']) == 32, cid
    assert sorted(g['training']) == sorted(FC.TRAINING)
    assert sorted(g['codec']) == sorted(CP.combo_id(*c) for c in CP.COMBOS)
    for cid, e in g['codec'].items():
        want = {'y_symbols', 'x_hat', 'points', 'strings_range_y', 'strings_rans_y', 'strings_occ', 'y_symbols_nonzero'}
        if cid.startswith('c3p'):
            want |= {'z_symbols', 'scale_indexes', 'strings_range_z', 'strings_rans_z'}
        assert set(e) == want and e['y_symbols_nonzero'] >= 0.01, cid


def test_every_family_of_the_route_is_pinned_at_least_twice():
    """The 18 names of pcc_conv_kernel_family, as FAMILY_CASES of tests/test_round6_gpu.py enumerates them (read from its source: the
    module itself imports torch), each with two cases or more, none larger than 32^3 x 2 voxels, one of them plain."""
    import ast
    src = open(os.path.join(FC.ROOT, 'tests', 'test_round6_gpu.py')).read()
    table = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', '') == 'FAMILY_CASES')
    prefixes = {elt.elts[0].value for elt in table.value.elts}
    g = _golden()
    names = {e['family'] for e in g['cases'].values()}
    assert len(names) == 18 and names == set(FC.FAMILIES.values())
    for n in names:
        assert any(n.startswith(p) for p in prefixes), f'{n} is not a family FAMILY_CASES knows'
    for p in prefixes:
        assert any(n.startswith(p) for n in names), p
    for n in names:
        mine = [c for c in FC.CASES if c['family'] == n]
        assert len(mine) >= 2 and any(not (c['bias'] or c['relu'] or c['res']) for c in mine), n
        # (odd D wherever the family takes one: the stride-2 forward layers of conv_cin1 need even dimensions)
        assert any(c['bias'] and c['relu'] and c['geo'][0] == 2 and (c['geo'][1] % 2 == 1 or n == FC.FAMILIES['cin1']) for c in mine), n
    for c in FC.CASES:
        N, D, H, W = c['geo'][:4]
        assert N <= 2 and D * H * W <= 32 ** 3, c['id']
    # the sensitivity pairs really share a layer and its inputs
    assert len(FC.SENSITIVITY) >= 5
    for left, right in FC.SENSITIVITY:
        a, b = FC.BY_ID[left], FC.BY_ID[right[0] if isinstance(right, tuple) else right]
        assert a['geo'] == b['geo'] and (a['bias'], a['relu'], a['res']) == (b['bias'], b['relu'], b['res'])
        if isinstance(right, str):
            assert g['cases'][left]['digest'] != g['cases'][right]['digest'], (left, right)


def test_committed_streams_match_their_listing():
    from pcc_geo_cnn_v2_amd import model_syntax
    g = _golden()
    folder = CP.streams_dir(g['family'])
    listing = CP.load_listing(g['family'])
    assert listing['family'] == g['family'] and sorted(listing['streams']) == sorted(CP.STREAMS)
    assert sorted(os.listdir(folder)) == sorted([e['file'] for e in listing['streams'].values()] + ['streams.json'])
    assert len(listing['streams']) <= 16
    for name, e in listing['streams'].items():
        path = os.path.join(folder, e['file'])
        tag = model_syntax.read_gzip_tag(path)
        assert tag == e['tag'] and tag.startswith(f"pcc_geo_cnn_v2_amd/k{g['family']}/"), name
        assert tag.split('/')[3] == e['precision'] and ('rans1' in tag.split('/')) == (e['coder'] == 'rans') and tag.endswith('/occ1') == e['lossless']
        assert os.path.getsize(path) == e['bytes'] < 16384 and e['points'] > 0 and len(e['point_digest']) == 32
        flags = CP.STREAM_FLAGS.get(name, [])       # (the layer a flag asks for is the one the tag names)
        assert e.get('flags', []) == flags and tag.endswith('/cnt1') == any(f.startswith('--count_') for f in flags)
        assert tag.endswith('/qs1') == bool({'--latent_step', '--target_bpp'} & set(flags))
        resolution, level, _, blocks = model_syntax.load_compressed_file(__import__('io').BytesIO(CP.payload_of(path)))
        assert (resolution, level, len(blocks)) == (e['resolution'], e['octree_level'], CP.B), name
