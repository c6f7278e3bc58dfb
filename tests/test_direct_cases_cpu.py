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
    if row['mode'] in ('out16', 'in16-out16'):
        ref = DC.reference(row)
        assert np.abs(ref).max() <= 2048 and np.array_equal(ref, np.round(ref)), row['id']
    if row['kernel'].startswith(('conv_f16_kernel', 'conv_tr2m_f16_kernel', 'conv_cout1_mfma_kernel<true')):
        assert row['set'] == 'B' and DC.magnitude_bound(row) <= 27 * 64 + 1 + 2 < 2048
    if DC.is_sub(row):
        # the raw fp16 partial sums of input half 0, which the second launch reads back: integers that fp16 holds
        part, mag = DC.partial_reference(row), DC.partial_reference(row, absolute=True)
        assert mag.max() <= DC.partial_bound(row) == 864 < 2048 and np.abs(part).max() <= mag.max(), row['id']
        assert np.array_equal(part, np.round(part)) and np.array_equal(part.astype(np.float16).astype(np.float64), part), row['id']
        assert part.any(), row['id']
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
    missing = [n for n in DC.ALL_INSTANCES if n not in chosen and n not in DC.GRAPH_ONLY]
    assert not missing, missing
    # the threshold-fusing instantiations have no row: the codec graph launches them (tests/_thr_ref.py names the cases)
    assert len(DC.ALL_INSTANCES) == 151 and len(DC.GRAPH_ONLY) == 4 and not set(DC.GRAPH_ONLY) & set(chosen)
    import _thr_ref as TR
    graph = {TR.last_layer(c, p, DC.CPU_NUM_CU)['kernel'] for c in TR.cases(DC.CPU_NUM_CU) for p in ('fp32', 'fp16')}
    assert set(DC.GRAPH_ONLY) <= graph, sorted(set(DC.GRAPH_ONLY) - graph)
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
    cout1 = [r for r in WINDOWED if r['group'] == 'cout1']
    assert sorted((r['zsp'], r['mode']) for r in cout1 if not r['switches']) == [(z, m) for z in (1, 2, 4, 8) for m in ('fp32', 'in16-out32')]
    for r in cout1:
        assert DC.select(r, DC.flags_of(r), r['switches'], 256)['zsp'] == r['zsp'], r['id']
        assert not (r['mode'] == 'in16-out32' and r['res']), 'the 16 -> 1 layer reads its residual as fp32'
    assert by['cout1m-t32-zsp4']['geo'][:2] == (64, 64) and by['cout1m-t32-zsp8']['geo'][:2] == (32, 128)     # slabs of 16 planes


def test_every_tiled_row_has_a_partial_tile():
    for row in ALL:
        tile = DC.select(row, DC.flags_of(row), row['switches'], DC.CPU_NUM_CU)['tile']
        if tile is None or row['group'] == 'cout1' or row['kernel'].startswith(('conv_tr2m_kernel', 'conv_tr2m_f16_kernel', 'conv_f16_kernel')):
            continue              # whole 16 x 16 / 8 x 16 / 32 x 32 columns marched along z: the shape rules admit no partial column
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
    takes_offset = [r for r in DC.ROWS if not r['kernel'].startswith('conv_f16_kernel')]      # pcc_f16_eligible refuses an offset
    assert sum(1 for r in takes_offset if r['ocs']) >= len(takes_offset) // 2 - 4
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


def test_fp16_storage_rows_sit_on_their_edges_in_z():
    """conv_f16_kernel: every instantiation with one slab (odd D) and with the smallest slab of the launcher's first loop (4 planes),
    more than one tile in x or y, a residual on both output types, both orientations per channel count; conv_tr2m_f16_kernel: D = 1,
    odd, and z-split, ReLU on and off, two channel-offset outputs."""
    f16 = [r for r in DC.ROWS if r['kernel'].startswith('conv_f16_kernel')]
    assert len(f16) == 12
    for name in DC.INSTANCES['pcc_conv_f16']:
        got = {}
        for r in f16:
            if r['kernel'] == name:
                sel = DC.select(r, DC.flags_of(r), r['switches'], DC.CPU_NUM_CU)
                assert sel['zsplit'] == r['zsplit'] and r['geo'][0] == 2, r['id']
                assert (r['geo'][2] // sel['tile'][1]) * (r['geo'][3] // 16) > 1, r['id']
                got[sel['zsplit']] = sel['zlen']
        assert got == {1: 5, 4: 4}, (name, got)
    for out in ('in16-out16', 'in16-out32'):
        assert any(r['res'] for r in f16 if r['mode'] == out)
        assert {e for r in f16 if r['mode'] == out for e in [(r['bias'], r['res'])]} == {(False, False), (True, False), (True, True)}
    for C in (16, 32, 64):
        assert {r['geo'][8] for r in f16 if r['geo'][4] == C} == {0, 1}
    assert all(any(r['res'] for r in f16 if r['kernel'] == n) for n in DC.INSTANCES['pcc_conv_f16'][4:])      # both SUB instantiations
    tm = [r for r in DC.ROWS if r['kernel'].startswith('conv_tr2m_f16_kernel')]
    assert sorted(r['geo'][1] for r in tm) == [1, 5, 9, 32] and sum(1 for r in tm if r['ocs']) == 2
    assert {r['kernel'] for r in tm} == set(DC.INSTANCES['pcc_conv_tr2m_f16'])
    assert DC.select(tm[3], DC.flags_of(tm[3]), {}, DC.CPU_NUM_CU)['zsplit'] == 8
    # the tiled rows of the same layers keep their kernels: no_tr2m holds the fp16 hand-over off the march (conv_route.hip:261)
    for r in DC.ROWS:
        if r['mode'] == 'out16' and r['geo'][7] == 2 and r['geo'][8] and r['switches'].get('no_tr2m'):
            assert r['kernel'].startswith(('conv_tr2_kernel', 'conv_tr2g_kernel')), r['id']


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
