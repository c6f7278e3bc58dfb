"""CPU: what an encode may combine (stream_layers.plan_encode) over the full grid of its options, against the refusals of the commit
before the rule table existed (tests/golden/encode_options.json: recorded there by calling the checks it replaced in the order
compress_blocks called them), and the plan of what passes.

The comparison is exact, per combination: refused or not, and which option the message names first.
"""
import itertools
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encode_options.json')
N_BLOCKS = 3

# axis -> its values, in the order of the recording; the combinations are itertools.product over the axes in this order
AXES = [
    ('count_scale', (None, 1.0)), ('count_search', (None, (0.5, 2.0, 5))), ('fixed_threshold', (False, True)), ('lossless', (False, True)),
    ('latent_step', (None, 16)), ('target_bpp', (None, 1.0)), ('world', (1, 2)), ('version', (1, 2)), ('precision', ('fp32', 'fp16')),
    ('entropy_coder', ('range', 'rans')), ('search_ties', ('pick', 'mean')), ('opt_metrics', (('d1_mse',), ('d1_mse', 'd2_mse'))),
    ('d2_gpu', (False, True)), ('dhw', ((64,) * 3, (256,) * 3)),
]
# the words a refusal can name: the keywords of plan_encode (d2_search is how the messages call d2_gpu)
OPTION_NAMES = ('count_scale', 'count_search', 'fixed_threshold', 'lossless', 'latent_step', 'target_bpp', 'version', 'precision',
                'entropy_coder', 'world', 'search_ties', 'opt_metrics', 'd2_gpu', 'd2_search', 'dhw', 'n_blocks', 'metrics_device', 'd2_ties')


def combinations():
    names = [n for n, _ in AXES]
    for values in itertools.product(*(v for _, v in AXES)):
        yield dict(zip(names, values))


def first_named(message):
    """the option name that stands first in a refusal's message"""
    found = [(message.find(n), -len(n), n) for n in OPTION_NAMES if n in message]
    assert found, f'the refusal names no option: {message}'
    return min(found)[2]


def outcome(check, combo):
    """None when `check(**combo)` passes, else the option its AssertionError names first"""
    try:
        check(**combo)
    except AssertionError as e:
        return first_named(str(e))
    return None


def test_the_grid_is_the_recorded_one():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert g['axes'] == [[n, [list(v) if isinstance(v, tuple) else v for v in vals]] for n, vals in AXES]
    assert len(g['codes']) == int(np.prod([len(v) for _, v in AXES])) == 2 ** 14
    assert set(g['codes']) <= set('.' + ''.join(chr(ord('a') + i) for i in range(len(g['options']))))
    assert 0 < g['codes'].count('.') < len(g['codes'])


def test_every_combination_is_refused_as_before_and_names_the_same_option_first():
    from pcc_geo_cnn_v2_amd.stream_layers import plan_encode
    with open(GOLDEN) as fh:
        g = json.load(fh)
    wrong = []
    for code, combo in zip(g['codes'], combinations()):
        want = None if code == '.' else g['options'][ord(code) - ord('a')]
        got = outcome(lambda **kw: plan_encode(n_blocks=N_BLOCKS, metrics_device='host', d2_ties='pick', **kw), combo)
        if got != want:
            wrong.append((combo, want, got))
    assert not wrong, f'{len(wrong)} combinations differ from the recorded refusals, the first: {wrong[0]}'


def test_the_plan_of_what_passes():
    from pcc_geo_cnn_v2_amd.model_opt import count_ladder
    from pcc_geo_cnn_v2_amd.stream_layers import plan_encode
    base = dict(count_scale=None, count_search=None, fixed_threshold=False, lossless=False, latent_step=None, target_bpp=None, version=2,
                precision='fp32', entropy_coder='range', world=1, search_ties='pick', opt_metrics=('d1_mse',), d2_gpu=False, dhw=(64,) * 3,
                n_blocks=N_BLOCKS, metrics_device='host', d2_ties='pick')
    p = plan_encode(**base)
    assert (p.policy, p.ladder, p.steps, p.layers) == ('search', None, None, ())
    with pytest.raises(AttributeError):
        p.policy = 'fixed'
    assert plan_encode(**{**base, 'fixed_threshold': True, 'lossless': True}).layers == ('occ1',)
    assert plan_encode(**{**base, 'fixed_threshold': True}).policy == 'fixed'
    p = plan_encode(**{**base, 'count_scale': 0.5})
    assert (p.policy, p.layers) == ('count', ('cnt1',))
    p = plan_encode(**{**base, 'count_search': (0.5, 2.0, 5)})
    assert (p.policy, p.layers) == ('count_search', ('cnt1',)) and np.array_equal(p.ladder, count_ladder(0.5, 2.0, 5))
    p = plan_encode(**{**base, 'latent_step': 16})
    assert p.layers == ('qs1',) and p.steps.dtype == np.uint8 and p.steps.tolist() == [16] * N_BLOCKS
    assert plan_encode(**{**base, 'latent_step': [0, 16, 37]}).steps.tolist() == [0, 16, 37]
    p = plan_encode(**{**base, 'target_bpp': 1.5})                      # the step is chosen later: the layer is known, the steps are not
    assert p.layers == ('qs1',) and p.steps is None
    # a callable d2_gpu is asked only when a d2_* metric is requested beside the count search
    plan_encode(**{**base, 'count_search': (0.5, 2.0, 5), 'd2_gpu': lambda: pytest.fail('asked without a d2 metric')})
    assert plan_encode(**{**base, 'count_search': (0.5, 2.0, 5), 'opt_metrics': ('d1_mse', 'd2_mse'), 'd2_gpu': lambda: True}).policy == 'count_search'


def test_a_blocks_strings_are_composed_and_split_in_the_order_of_the_layer_table():
    from pcc_geo_cnn_v2_amd import _lib as L
    from pcc_geo_cnn_v2_amd import stream_layers as SL
    assert [layer.name for layer in SL.LAYERS] == ['qs1', 'occ1', 'cnt1']
    base = (b'yy', b'z')
    assert SL.compose_strings(base) == base
    assert SL.compose_strings(base, cnt1=SL.count_to_bytes(7), qs1=SL.step_to_bytes(21)) == base + (b'\x15', b'\x07\0\0\0')
    assert SL.compose_strings(base, occ1=b'occ', qs1=b'\x10') == base + (b'\x10', b'occ')
    held = SL.compose_strings(base, cnt1=[SL.count_to_bytes(k) for k in (3, 4, 5)])           # the count search: one count per metric name
    assert held == base + (b'\x03\0\0\0', b'\x04\0\0\0', b'\x05\0\0\0')
    assert SL.split_strings(held, 2, ('cnt1',), candidates=3) == (base, {'cnt1': list(held[2:])})
    assert SL.split_strings(held[:3], 2, ('cnt1',), candidates=1) == (base, {'cnt1': [held[2]]})           # (one metric name: still a list)
    assert SL.split_strings(base + (b'\x10', b'occ'), 2, ('qs1', 'occ1')) == (base, {'qs1': b'\x10', 'occ1': b'occ'})
    assert SL.split_strings((b'y', b'occ'), 1, ('occ1',)) == ((b'y',), {'occ1': b'occ'})
    with pytest.raises(AssertionError):
        SL.compose_strings(base, cnt2=b'')
    blocks = [(base + (SL.count_to_bytes(k),), 128) for k in (0, 9, 2 ** 32 - 1)]
    assert SL.layer_values('cnt1', blocks, 2) == [0, 9, 2 ** 32 - 1]
    for broken in ([(base, 128)], [(base + (b'\x01\0\0',), 128)], [(base + (b'\x01\0\0\0', b''), 128)]):
        with pytest.raises(L.PccError, match=f'block 0.*status {L.PCC_ERR_CORRUPT}'):
            SL.layer_values('cnt1', broken, 2)
    with pytest.raises(RuntimeError, match='block 0: 2 strings'):
        SL.layer_values('qs1', [(base, 128)], 2)
    # which layer a decode reads, and the mode a stream's layers ask for
    assert [SL.carried_layer(m, blocks, 2) for m in ('all', 'base', 'count', 'step')] == ['occ1', None, 'cnt1', 'qs1']
    assert SL.carried_layer('all', [(base, 128)], 2) is None and SL.carried_layer('all', [], 2) is None
    assert [SL.decode_mode(layers) for layers in ((), ('occ1',), ('cnt1',), ('qs1',))] == ['all', 'all', 'count', 'step']
    assert [SL.decode_mode(layers, True) for layers in ((), ('occ1',), ('cnt1',), ('qs1',))] == ['base', 'base', 'base', 'step']


def test_base_only_is_logged_as_without_effect_where_it_has_none(caplog):
    import logging
    from pcc_geo_cnn_v2_amd import stream_layers as SL
    with caplog.at_level(logging.WARNING, logger=SL.logger.name):
        for layers, noted in (((), True), (('qs1',), True), (('occ1',), False), (('cnt1',), False)):
            caplog.clear()
            SL.decode_mode(layers, True, 'a.bin')
            assert any('--base_only has no effect on a.bin' in r.getMessage() for r in caplog.records) == noted, layers
        caplog.clear()
        SL.decode_mode((), False, 'a.bin')
        assert not caplog.records
