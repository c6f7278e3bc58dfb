"""The table of the direct conv kernels (tests/_direct_cases.py) checked without a GPU: its inputs keep every row exact, its rows
reach every instantiation the launchers can select, every tiled row has a partial tile, and the plan covers every row."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _direct_cases as DC
from pcc_geo_cnn_v2_amd import _lib as L

WINDOWED = DC.windowed_rows(DC.CPU_NUM_CU)
ALL = DC.ROWS + WINDOWED
DOC = os.path.join(DC.FC.ROOT, 'profiles', 'direct_instantiations.md')


def _ids(rows):
    return [r['id'] for r in rows]


@pytest.mark.parametrize('row', DC.ROWS, ids=_ids(DC.ROWS))
def test_inputs_keep_the_row_exact(oracle, row):
    """Conditions on the inputs, not tolerances.  fp32 output: the sum of |terms| of every output (the reference on |x|, |w|, |bias|,
    |residual|), counted in units of the smallest power of two a term of that output channel carries (2^min(e, 0)), is below 2^24.  fp16 output: the
    reference values lie within +-2048."""
    mag = DC.reference(row, absolute=True) * np.exp2(-np.minimum(DC.exponents(row), 0))        # per output channel, in its unit
    assert mag.max() < 2 ** 24, (row['id'], mag.max())
    assert mag.max() <= DC.magnitude_bound(row)                   # the closed form the windowed rows are held to
    if row['mode'] == 'out16':
        ref = DC.reference(row)
        assert np.abs(ref).max() <= 2048 and np.array_equal(ref, np.round(ref)), row['id']
    x, w, b, r = DC.inputs(row)
    e = DC.exponents(row)
    for a in (x, r):
        assert a is None or np.array_equal(a, np.round(a))
    ws = w * np.exp2(-e)[:, None] if row['geo'][8] else w * np.exp2(-e)
    assert np.array_equal(ws, np.round(ws)) and np.abs(ws).max() <= 2
    if row['set'] == 'B' or row['geo'][4] == 1:
        assert set(np.unique(x)) <= {0.0, 1.0}
    else:
        assert 0.35 < np.mean(x == 0) < 0.65


@pytest.mark.parametrize('row', WINDOWED, ids=_ids(WINDOWED))
def test_inputs_keep_the_windowed_row_exact(row):
    """The same condition by its closed form (taps x channels x max |x| x max |w| + |bias| + |residual|): these tensors are large."""
    assert DC.magnitude_bound(row) < 2 ** 24
    N, D, H, W, cin, cout, k, s, tr = row['geo']
    od, oh, ow = DC.out_dims(row['geo'])
    assert max(N * D * H * W * cin, N * od * oh * ow * (row['ocs'] or cout)) * 4 <= 300e6, 'no tensor above 300 MB'


def test_every_instantiation_has_a_row():
    chosen = {}
    for row in ALL:
        sel = DC.select(row, DC.flags_of(row), row['switches'], DC.CPU_NUM_CU)
        assert sel['kernel'] == row['kernel'], (row['id'], sel['kernel'], row['kernel'])
        assert row['kernel'] in DC.ALL_INSTANCES, row['id']
        chosen.setdefault(row['kernel'], []).append(row['id'])
    missing = [n for n in DC.ALL_INSTANCES if n not in chosen]
    assert not missing, missing
    assert not set(DC.UNREACHABLE) & set(chosen)
    for name in ('tr2_old', 'p16', 'cout1_t16'):
        assert any(r['switches'].get(name) for r in ALL), name
    # switch-only kernels carry ids of their own, so that one can be taken out without touching the rest
    for r in ALL:
        assert bool(r['switches'].get('tr2_old')) == ('tr2old' in r['id']) and bool(r['switches'].get('p16')) == ('p16' in r['id'])


def test_windowed_rows_at_256_cus():
    by = {r['id']: r for r in WINDOWED}
    assert by['big-64-64']['geo'][0] == 13
    one = dict(by['big-64-64'], geo=(1,) + by['big-64-64']['geo'][1:])
    assert DC.select(one, DC.flags_of(one), {}, 256)['kernel'] == 'conv_fwd_kernel<64,64,3,1,16,2,4,16,2,4>'     # one block: the small tile
    for r in WINDOWED:
        sel = DC.select(r, DC.flags_of(r), r['switches'], 256)
        if r['group'] in ('pers', 'tr2g'):
            assert sel['ntiles'] > sel['slots'] and sel['ntiles'] % sel['slots'], (r['id'], sel)
            assert sel['ntiles'] < 2 * sel['slots']                # and some workgroups see one tile, some two
    assert DC.select(by['cout1m-t32-zsp1'], DC.flags_of(by['cout1m-t32-zsp1']), {}, 256)['zsp'] == 1
    assert DC.select(by['cout1m-t32-zsp2'], DC.flags_of(by['cout1m-t32-zsp2']), {}, 256)['zsp'] == 2
    assert by['cout1m-t32-zsp2']['geo'][1] == 33                  # slabs of 17 and 16 planes


def test_every_tiled_row_has_a_partial_tile():
    for row in ALL:
        tile = DC.select(row, DC.flags_of(row), row['switches'], DC.CPU_NUM_CU)['tile']
        if tile is None or row['group'] == 'cout1' or row['kernel'].startswith('conv_tr2m_kernel'):
            continue              # whole 16 x 16 / 32 x 32 columns marched along z: the shape rules admit no partial column
        ext = DC.base_dims(row['geo'])
        partial = [e % t != 0 for e, t in zip(ext, tile)]
        assert any(partial), (row['id'], ext, tile)
        if row['group'] in ('pers', 'tr2g', 'big'):
            assert partial[0] and partial[1], (row['id'], ext, tile)
        if row['kernel'].startswith(('conv_fwd_kernel', 'conv_tr2_kernel', 'conv_tr2g_kernel', 'conv16_pers')):
            assert partial[1] and (partial[0] or tile[0] == 1), (row['id'], ext, tile)


def test_base_rows_alternate_direction_epilogue_and_offset():
    s1 = [r for r in DC.ROWS if r['kernel'].startswith(('conv_fwd_kernel', 'conv16_pers')) and r['geo'][7] == 1]
    assert {r['geo'][8] for r in s1} == {0, 1}
    assert sum(1 for r in DC.ROWS if r['ocs']) >= len(DC.ROWS) // 2 - 4
    assert any(r.get('clip') for r in DC.ROWS) and any(not r['bias'] for r in DC.ROWS) and any(r['res'] for r in DC.ROWS)
    for r in DC.ROWS:
        if r['ocs']:
            assert r['ocs'] == r['geo'][5] + 8 and r['oco'] == (3 if r['family'].startswith(('generic', 'conv_cout1')) else 8)


@pytest.mark.parametrize('row', ALL, ids=_ids(ALL))
def test_the_plan_covers_the_row(row):
    N, D, H, W, cin, cout, k, s, tr = row['geo']
    d = L.ConvDesc(N, D, H, W, cin, cout, k, s, tr, DC.FC._flags(row, L), getattr(L, 'PCC_IMPL_' + row['impl']), row['ocs'], row['oco'])
    want = 0 if row['id'] == 'generic-tr' or row['id'] == 'generic-fwd' else 1
    assert L.lib().pcc_conv_mfma_supported(C.byref(d)) == want


def _doc_switches():
    """{switch: cell of the 'set by' column} of the numerics-switch table of profiles/direct_instantiations.md."""
    rows = {}
    for line in open(DOC):
        m = re.match(r'\|\s*`(\w+)`\s*\|[^|]*\|\s*([^|]*?)\s*\|\s*$', line)
        if m and m.group(1) in L.PCC_NUM:
            rows[m.group(1)] = m.group(2)
    return rows


def test_document_lists_every_instantiation_and_switch():
    text = open(DOC).read()
    for name in DC.ALL_INSTANCES + DC.UNREACHABLE:
        assert '`' + name + '`' in text, name
    for row in ALL:
        assert '`' + row['id'] + '`' in text, row['id']
    sw = _doc_switches()
    assert set(sw) == set(L.PCC_NUM)
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(DC.FC.ROOT, 'tests', '*.py'))}
    for name, cell in sw.items():
        files = re.findall(r'`(tests/[\w.]+)`', cell)
        for f in files:
            assert re.search(r'\b%s\b' % name, sources[os.path.basename(f)]), (name, f)
        if not files:
            # recorded as set by no test (split_tile8 belongs to conv_split.hip, outside this table): still true?
            assert cell.startswith('none'), (name, cell)
            users = [f for f, src in sources.items() if re.search(r"""['"]%s['"]|\b%s=""" % (name, name), src)]
            assert not users, (name, users)
