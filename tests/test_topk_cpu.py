"""CPU-only: the top-k selection rule's two restatements against each other, the '/cnt1' stream tag, the container with the count string,
the count arithmetic and the CLI refusals of --count_threshold."""
import io

import numpy as np
import pytest

import _topk_ref as T
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax as MS
from pcc_geo_cnn_v2_amd import stream_layers as SL

BASE = 'pcc_geo_cnn_v2_amd/abi4/fp32/default'


@pytest.mark.parametrize('dhw', T.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_the_two_restatements_agree_on_every_case(dhw):
    group = T.cases(dhw)
    assert len({name for name, _, _ in group}) == len(group) >= 9 * 8
    for name, x, k in group:
        a, b = T.taken_lexsort(x, k), T.taken_kth(x, k)
        assert np.array_equal(a, b), name
        key = T.keys(x)
        assert len(a) == min(max(k, 0), np.count_nonzero(key)) and (key[a] > 0).all(), name
        assert len(a) == 0 or len(a) == key.size or key[a].min() >= np.delete(key, a).max(), name
    assert len(T.cases()) == sum(len(T.cases(s)) for s in T.SHAPES)


def test_keys_of_the_special_values_and_the_row_layout():
    x = np.array([np.nan, -0.0, 0.0, -1.0, np.inf, 1e-45, 2.5, 1.0], np.float32)
    assert T.keys(x).tolist() == [0, 0, 0, 0, 0x7f800000, 1, 0x40200000, 0x3f800000]
    rows, n = T.select(x, 3, (2, 2, 2))
    assert n == 3 and rows.tolist() == [[1, 0, 0], [1, 1, 0], [1, 1, 1]]            # +inf, 2.5, 1.0 in voxel order
    assert T.select(x, 99, (2, 2, 2))[1] == 4 and T.select(x, -3, (2, 2, 2))[1] == 0
    ties = np.array([0.5, 0.25, 0.5, 0.5], np.float32)
    assert T.taken_kth(ties, 2).tolist() == T.taken_lexsort(ties, 2).tolist() == [0, 2]


def test_stream_tag_names_the_count_layer_and_refuses_both_layers():
    for coder, mid in (('range', ''), ('rans', '/rans1')):
        tag = MS.stream_tag(BASE, coder, count=True)
        assert tag == BASE + mid + '/cnt1'
        assert MS.split_stream_tag(tag) == (BASE, coder, ('cnt1',))
        assert MS.stream_layers(tag, BASE) == (coder, ('cnt1',))
        # what was accepted before answers as before
        assert MS.stream_tag(BASE, coder) == MS.stream_tag(BASE, coder, False) == BASE + mid
        assert MS.stream_tag(BASE, coder, True) == MS.stream_tag(BASE, coder, lossless=True) == BASE + mid + '/occ1'
        assert MS.split_stream_tag(BASE + mid) == (BASE, coder, ())
        assert MS.split_stream_tag(BASE + mid + '/occ1') == (BASE, coder, ('occ1',))
        assert MS.stream_layers(BASE + mid + '/occ1', BASE) == (coder, ('occ1',))
        for both in ('/occ1/cnt1', '/cnt1/occ1'):
            with pytest.raises(RuntimeError):
                MS.split_stream_tag(BASE + mid + both)
    assert MS.split_stream_tag(None) == (None, None, ()) and MS.split_stream_tag('other/cnt1') == ('other/cnt1', None, ())
    with pytest.raises(AssertionError):
        MS.stream_tag(BASE, 'range', lossless=True, count=True)
    with pytest.raises(RuntimeError):
        MS.split_stream_tag(BASE + '/cnt2')
    assert SL.BY_NAME['cnt1'].name == 'cnt1' and SL.BY_NAME['occ1'].name == 'occ1' and [layer.name for layer in SL.LAYERS] == ['qs1', 'occ1', 'cnt1']


def test_container_roundtrips_blocks_with_the_count_string():
    blocks = [((b'yy' * (i + 1), b'z' * i, MS.count_to_bytes(k)), 128) for i, k in enumerate((0, 1, 262144, 2 ** 32 - 1))]
    raw = MS.save_compressed_file([1, 0, 255], blocks, 128, 1, strict=True)
    res, level, binstr, got = MS.load_compressed_file(io.BytesIO(raw))
    assert (res, level, binstr.tolist()) == (128, 1, [1, 0, 255])
    assert [(tuple(s), t) for s, t in got] == blocks
    assert [MS.count_from_bytes(s[-1]) for s, _ in got] == [0, 1, 262144, 2 ** 32 - 1]
    assert got[2][0][-1] == b'\x00\x00\x04\x00'                                         # little-endian uint32
    assert MS.count_from_bytes(b'\x01\x00\x00') is None and MS.count_from_bytes(b'') is None and MS.count_from_bytes(b'\0' * 5) is None


def test_count_arithmetic_matches_hand_worked_values():
    from pcc_geo_cnn_v2_amd.model_types import block_count

    def check_count_scale(count_scale, fixed_threshold, lossless, world=1, entry='compress_blocks'):
        SL.plan_encode(count_scale=count_scale, fixed_threshold=fixed_threshold, lossless=lossless, world=world, entry=entry)
    n = 64 ** 3
    table = [  # (rho, N, n, k)
        (1.0, 0, n, 0), (1.0, 1, n, 1), (1.0, 4321, n, 4321), (1.0, n, n, n),
        (0.5, 0, n, 0), (0.5, 1, n, 1), (0.5, 3, n, 2), (0.5, 5, n, 3), (0.5, 4, n, 2), (0.5, 4321, n, 2161),     # x.5 rounds up
        (1.5, 3, n, 5), (0.3, 10, n, 3), (0.25, 2, n, 1), (0.25, 1, n, 0), (0.1, 4, n, 0), (0.1, 5, n, 1),
        (2.0, n, n, n), (1.0, 100, 64, 64), (3.0, 30, 64, 64), (1e9, 7, n, n),                                    # the clamp at n
    ]
    for rho, N, nv, k in table:
        assert block_count(N, rho, nv) == k, (rho, N, nv)
        assert isinstance(block_count(N, rho, nv), int)
    check_count_scale(None, True, True, 8, entry='encode_block_range')      # off: its rules refuse nothing
    check_count_scale(0.5, False, False)
    for bad in (0.0, -1.0, float('nan'), float('inf'), '1.0'):
        with pytest.raises(AssertionError, match='count_scale'):
            check_count_scale(bad, False, False)
    for kw in (dict(fixed_threshold=True, lossless=False), dict(fixed_threshold=False, lossless=True),
               dict(fixed_threshold=False, lossless=False, world=2)):
        with pytest.raises(AssertionError, match='count_scale'):
            check_count_scale(1.0, **kw)


def _parse(*extra):
    from pcc_geo_cnn_v2_amd import compress_octree
    return compress_octree.build_parser().parse_args(
        ['--input_files', '/nonexistent/in.ply', '--output_files', '/nonexistent/out.bin', '--checkpoint_dir', '/nonexistent/ckpt',
         '--model_config', 'c3p', '--resolution', '128', '--octree_level', '1', '--opt_metrics', 'd1_mse', *extra])


def test_count_threshold_parses_with_and_without_a_scale():
    assert _parse().count_threshold is None
    assert _parse('--count_threshold').count_threshold == 1.0
    assert _parse('--count_threshold', '0.5').count_threshold == 0.5
    from pcc_geo_cnn_v2_amd import ev_experiment
    ev = ['--output_dir', 'o', '--model_dir', 'm', '--model_config', 'c3p', '--pc_name', 'p', '--input_pc', 'i', '--opt_metrics', 'd1_mse',
          '--max_deltas', 'inf']
    assert ev_experiment.build_parser().parse_args(ev).count_threshold is None
    assert ev_experiment.build_parser().parse_args(ev + ['--count_threshold', '0.75']).count_threshold == 0.75


@pytest.mark.parametrize('extra,world,match', [
    (('--fixed_threshold',), '1', '--fixed_threshold'), (('--lossless',), '1', '--lossless'), ((), '2', 'single-process'),
    (('--search_ties', 'mean', '--opt_metrics', 'd2_mse', '--estimate_normals'), '1', '--search_ties mean'),
    (('--d2_search', 'gpu'), '1', '--d2_search gpu')])
def test_cli_refuses_count_threshold_with_what_it_replaces_before_the_gpu_is_touched(monkeypatch, extra, world, match):
    """compress() itself on parsed arguments: the refusal comes before the input is read, the process group joined or a context made"""
    from pcc_geo_cnn_v2_amd import compress_octree
    monkeypatch.setenv('WORLD_SIZE', world)
    with pytest.raises(AssertionError, match=f'--count_threshold.*{match}'):
        compress_octree.compress(_parse('--count_threshold', *extra))
    with pytest.raises(AssertionError, match='--count_threshold'):
        compress_octree.compress(_parse('--count_threshold', '0'))


def test_library_exports_the_two_new_symbols_with_argtypes():
    lib = L.lib()
    assert {'pcc_topk_workspace_bytes', 'pcc_topk_compact'} <= set(L.EXPORTS)
    assert len(lib.pcc_topk_compact.argtypes) == 14 and len(lib.pcc_topk_workspace_bytes.argtypes) == 2
    n = 64 ** 3
    one, many = lib.pcc_topk_workspace_bytes(1, n), lib.pcc_topk_workspace_bytes(32, n)
    assert 0 < one and many == 32 * one and lib.pcc_topk_workspace_bytes(1, 1) > 0
    assert lib.pcc_topk_workspace_bytes(0, n) == 0 and lib.pcc_topk_workspace_bytes(1, (1 << 28) + 1) == 0 and lib.pcc_topk_workspace_bytes(1, -1) == 0
