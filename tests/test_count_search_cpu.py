"""Count search without a GPU: the rank-level rule restated twice, the ladder, the decision mapping, the refusals and the ABI."""
import os
import re

import numpy as np
import pytest

import _count_search_ref as R
import _topk_ref as T
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_opt as MO
from pcc_geo_cnn_v2_amd import model_types as MT
from pcc_geo_cnn_v2_amd.stream_layers import plan_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in T.SHAPES if np.prod(s) <= 4096]
NEW = ('pcc_rank_levels_workspace_bytes', 'pcc_rank_levels', 'pcc_d1_count_stats', 'pcc_d12_count_stats')


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dhw', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_the_two_restatements_agree_and_every_level_set_is_the_top_k_set(dhw):
    for name, x in R.inputs(dhw).items():
        key = T.keys(x)
        P = int(np.count_nonzero(key))
        for lname, c in R.ladders(x).items():
            lev, tcount = R.levels_lexsort(x, c)
            lev2, tcount2 = R.levels_kth(x, c)
            assert np.array_equal(lev, lev2) and tcount == tcount2, f'{name} {lname}'
            assert tcount == (int(np.count_nonzero(c >= 1)) if P else 0), f'{name} {lname}: tcount'
            assert not lev[key == 0].any()
            for j, k in enumerate(c):
                rows, ke = T.select(x, int(k), dhw)
                assert ke == min(max(int(k), 0), P)
                assert np.array_equal(T.rows_of(np.flatnonzero(lev > j), dhw), rows), f'{name} {lname}: candidate {j} (k = {k})'


def test_restatement_on_a_64_cube_and_a_row_out_of_order():
    dhw = (64, 64, 64)
    x = R.inputs(dhw)['64x64x64-levels8']
    c = R.ladders(x)['tie-cut']
    lev, tcount = R.levels_lexsort(x, c)
    assert np.array_equal(lev, R.levels_kth(x, c)[0]) and tcount == 4
    # not non-increasing: the formula still is the output (lev = how many entries exceed the rank), the sets just are not nested by j
    mixed = np.array([2, 5, 0, 3], np.int32)
    lev, tcount = R.levels_lexsort(x, mixed)
    assert np.array_equal(lev, R.levels_kth(x, mixed)[0]) and tcount == 3
    assert np.count_nonzero(lev == 3) == 2 and np.count_nonzero(lev == 2) == 1 and np.count_nonzero(lev == 1) == 2


# ---- the ladder -------------------------------------------------------------------------------------------------------------------------
def test_count_ladder_endpoints_monotone_rows_and_one_step():
    for lo, hi, steps in [(0.5, 2.0, 33), (0.1, 7.3, 255), (1.0, 1.0, 4), (0.3, 0.9, 2), (1e-3, 1e3, 17)]:
        rho = MO.count_ladder(lo, hi, steps)
        assert rho.dtype == np.float64 and rho.shape == (steps,)
        assert rho[0] == np.float64(hi) and rho[-1] == np.float64(lo)               # exact, not up to rounding
        assert np.all(np.diff(rho) <= 0) and np.all((rho >= lo) & (rho <= hi))
        mid = hi * (lo / hi) ** (np.arange(steps) / (steps - 1))
        assert np.allclose(rho, mid, rtol=1e-12, atol=0)
        blocks = [np.zeros((n, 3)) for n in (1, 7, 500, 4097, 300000)]
        rows = MO.count_rows(blocks, rho, 64 ** 3)
        assert rows.dtype == np.int32 and rows.shape == (len(blocks), steps)
        assert np.all(np.diff(rows.astype(np.int64), axis=1) <= 0)
        assert all(rows[b, j] == MT.block_count(len(blk), rho[j], 64 ** 3) for b, blk in enumerate(blocks) for j in (0, steps // 2, steps - 1))
    one = MO.count_ladder(0.5, 2.0, 1)
    assert one.tolist() == [2.0] and one.dtype == np.float64
    assert MO.count_ladder(0.5, 2.0, np.int64(3)).tolist() == [2.0, 1.0, 0.5]


@pytest.mark.parametrize('args', [(0.0, 2.0, 3), (-1.0, 2.0, 3), (2.0, 0.5, 3), (0.5, np.inf, 3), (np.nan, 2.0, 3), (0.5, 2.0, 0), (0.5, 2.0, 256),
                                  (0.5, 2.0, 3.0), (0.5, 2.0, True), ('a', 2.0, 3)])
def test_count_ladder_refuses_bad_arguments(args):
    with pytest.raises(AssertionError, match='count_search'):
        MO.count_ladder(*args)


# ---- the decision mapping ---------------------------------------------------------------------------------------------------------------
def _tally(n_b, ab, ba):
    t = np.zeros(5)
    t[:3] = n_b, ab, ba
    return t


def test_decision_maps_indices_to_counts_guard_empty_block_and_ineligible_pool():
    blk = np.array([[x, y, 0] for x in range(4) for y in range(4)], np.float64)              # 16 rows on a plane
    far = blk + np.array([40, 40, 40])
    rows = np.array([[32, 16, 8, 0]] * 4, np.int32)
    good = np.array([_tally(32, 16, 40), _tally(16, 0, 0), _tally(8, 30, 0)])                  # candidate 1 is the block itself
    bad = np.array([_tally(32, 1e9, 1e9), _tally(16, 1e9, 1e9), _tally(8, 1e9, 1e9)])          # worse than the single mean point
    empty = np.zeros((0, 5))
    names, ks, idx = MO.decide_counts_from_tallies([blk, blk, far, blk], [good, bad, empty, good], rows, 64, ['d1_mse'], [np.inf, 1.2])
    assert names == ['d1_mse_inf', 'd1_mse_1.2']
    assert ks[0] == [16, 16] and idx[0] == [1, 1]
    assert ks[1] == [0, 0] and idx[1] == [4, 4]                     # the guard: 'emit nothing' is index J = 4
    assert ks[2] == [0, 0] and idx[2] == [4, 4]                     # no positive score: no candidate, k = 0 for every name
    # a max_delta that leaves no eligible candidate falls back to all of them (the threshold search's rule)
    narrow = np.array([_tally(32, 16, 40), _tally(8, 30, 0)])
    _, ks1, idx1 = MO.decide_counts_from_tallies([blk], [narrow], np.array([[32, 8, 0, 0]], np.int32), 64, ['d1_mse'], [1.2])
    assert idx1 == [[int(np.argmin([max(16 / 16, 40 / 32), max(30 / 16, 0)]))]] and ks1 == [[32]]
    # the same tables through the threshold search's function give the same indices: it is called unchanged
    assert MO.select_thresholds_from_stats(16, good, MO.mean_point_tally(blk, False), 5, 64, ['d1_mse'], [np.inf, 1.2])[1] == idx[0] == [1, 1]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _parse(*extra):
    from pcc_geo_cnn_v2_amd import compress_octree
    return compress_octree.build_parser().parse_args(
        ['--input_files', '/nonexistent/in.ply', '--output_files', '/nonexistent/out.bin', '--checkpoint_dir', '/nonexistent/ckpt',
         '--model_config', 'c3p', '--resolution', '128', '--octree_level', '1', '--opt_metrics', 'd1_mse', *extra])


def test_count_search_flag_parses_bare_and_with_values():
    from pcc_geo_cnn_v2_amd import compress_octree as CO, ev_experiment
    assert CO.count_search_of(_parse()) is None
    assert CO.count_search_of(_parse('--count_search')) == (0.5, 2.0, 33) == CO.COUNT_SEARCH_DEFAULT
    assert CO.count_search_of(_parse('--count_search', '0.7', '1.5', '9')) == (0.7, 1.5, 9)
    assert 'not a tuned value' in re.sub(r'\s+', ' ', CO.build_parser().format_help())
    ev = ['--output_dir', 'o', '--model_dir', 'm', '--model_config', 'c3p', '--pc_name', 'p', '--input_pc', 'i', '--opt_metrics', 'd1_mse',
          '--max_deltas', 'inf']
    assert ev_experiment.build_parser().parse_args(ev).count_search is None
    assert CO.count_search_of(ev_experiment.build_parser().parse_args(ev + ['--count_search', '0.5', '1.5', '5'])) == (0.5, 1.5, 5)


@pytest.mark.parametrize('values,extra,world,match', [
    ((), ('--count_threshold',), '1', '--count_threshold'), ((), ('--fixed_threshold',), '1', '--fixed_threshold'), ((), ('--lossless',), '1', '--lossless'),
    ((), (), '2', 'single-process'),
    ((), ('--search_ties', 'mean', '--opt_metrics', 'd2_mse', '--estimate_normals', '--d2_search', 'gpu'), '1', '--search_ties mean'),
    ((), ('--opt_metrics', 'd1_mse', 'd2_mse', '--estimate_normals'), '1', '--d2_search gpu'),
    ((), ('--opt_metrics', 'd2_mse', '--estimate_normals', '--d2_search', 'kdtree'), '1', '--d2_search gpu'),
    ((), ('--resolution', '1024', '--octree_level', '2'), '1', '128'),
    (('1.0', '2.0'), (), '1', 'LO HI STEPS'), (('2.0', '0.5', '3'), (), '1', 'lo'), (('0.5', '2.0', '300'), (), '1', 'steps'),
    (('0.5', '2.0', '3.5'), (), '1', 'LO HI STEPS'), (('0.5', 'x', '3'), (), '1', 'LO HI STEPS')])
def test_cli_refuses_count_search_before_the_gpu_is_touched(monkeypatch, values, extra, world, match):
    """compress() itself on parsed arguments: the refusal comes before the input is read, the process group joined or a context made"""
    from pcc_geo_cnn_v2_amd import compress_octree
    monkeypatch.setenv('WORLD_SIZE', world)
    with pytest.raises(AssertionError, match=f'--count_search.*{match}'):
        compress_octree.compress(_parse(*extra, '--count_search', *values))


def test_count_threshold_refusals_are_unchanged(monkeypatch):
    from pcc_geo_cnn_v2_amd import compress_octree
    monkeypatch.setenv('WORLD_SIZE', '1')
    for extra, match in [(('--fixed_threshold',), '--fixed_threshold'), (('--lossless',), '--lossless'), (('--d2_search', 'gpu'), '--d2_search gpu')]:
        with pytest.raises(AssertionError, match=f'--count_threshold.*{match}'):
            compress_octree.compress(_parse('--count_threshold', *extra))
    for bad in [dict(count_scale=0.0), dict(count_scale=1.0, fixed_threshold=True), dict(count_scale=1.0, lossless=True), dict(count_scale=1.0, world=2)]:
        with pytest.raises(AssertionError, match='count_scale'):
            plan_encode(**bad)
    assert plan_encode(entry='encode_block_range', count_scale=None, fixed_threshold=True, lossless=True, world=4).policy == 'fixed'      # off


def test_model_refuses_count_search_with_what_it_excludes(monkeypatch):
    ok = dict(count_search=(0.5, 2.0, 5))
    def ladder(count_search, **kw):
        return plan_encode(count_search=count_search, **kw).ladder
    # off: its rules refuse nothing (what count_scale excludes on its own is test_count_threshold_refusals_are_unchanged's)
    assert ladder(None, world=4, search_ties='mean', opt_metrics=('d2_mse',), d2_gpu=False, dhw=(256,) * 3) is None
    assert ladder(None, entry='encode_block_range', count_scale=1.0, search_ties='mean', opt_metrics=('d2_mse',), d2_gpu=False, dhw=(256,) * 3) is None
    assert np.array_equal(ladder((0.5, 2.0, 5), opt_metrics=('d1_mse',), dhw=(64,) * 3), MO.count_ladder(0.5, 2.0, 5))
    assert ladder((0.5, 2.0, 5), opt_metrics=('d1_mse', 'd2_mse'), d2_gpu=lambda: True, dhw=(128,) * 3) is not None
    for kw, match in [(dict(count_scale=1.0), 'count_scale'), (dict(fixed_threshold=True), 'fixed_threshold'), (dict(lossless=True), 'lossless'),
                      (dict(world=2), 'single-process'), (dict(search_ties='mean'), "search_ties 'mean'"),
                      (dict(opt_metrics=('d1_mse', 'd2_mse'), d2_gpu=False), "d2_search 'gpu'"),
                      (dict(opt_metrics=('d2_mse',), d2_gpu=lambda: False), "d2_search 'gpu'"), (dict(dhw=(256, 64, 64)), '128')]:
        with pytest.raises(AssertionError, match=f'count_search.*{match}'):
            ladder((0.5, 2.0, 5), **kw)
    for bad in [(0.5, 2.0), 1.0, (2.0, 0.5, 5), (0.5, 2.0, 0)]:
        with pytest.raises(AssertionError, match='count_search'):
            ladder(bad)
    # the model's own entry points refuse before a context is made: no GPU here, and sess = None would create the default one
    from pcc_geo_cnn_v2_amd import ops, sharding
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    monkeypatch.setattr(ops, 'get_context', lambda *a, **k: pytest.fail('a context was asked for'))
    blocks = [np.zeros((4, 3), np.float32)]
    m = ModelConfigType['c1'].build(batch_size=2)
    m.x_shape = [1, 1, 64, 64, 64]
    for kw, match in [(dict(count_scale=1.0), 'count_scale'), (dict(fixed_threshold=True), 'fixed_threshold')]:
        with pytest.raises(AssertionError, match=f'count_search.*{match}'):
            m.encode_block_range(None, blocks, 128, **ok, **kw)
        with pytest.raises(AssertionError, match=f'count_search.*{match}'):
            m.compress_blocks(None, blocks, [], blocks[0], 128, 1, **ok, **kw)
    m.search_ties = 'mean'
    with pytest.raises(AssertionError, match='count_search.*search_ties'):
        m.encode_block_range(None, blocks, 128, **ok)
    m.search_ties, m.d2_search = 'pick', 'kdtree'
    with pytest.raises(AssertionError, match="count_search.*d2_search 'gpu'"):
        m.encode_block_range(None, blocks, 128, with_normals=True, opt_metrics=('d1_mse', 'd2_mse'), **ok)
    m.x_shape = [1, 1, 256, 256, 256]
    with pytest.raises(AssertionError, match='count_search.*128'):
        m.compress_blocks(None, blocks, [], blocks[0], 256, 0, **ok)
    m.x_shape = [1, 1, 64, 64, 64]
    monkeypatch.setattr(sharding, 'world_info', lambda: (0, 2))
    with pytest.raises(AssertionError, match='count_search.*single-process'):
        m.compress_blocks(None, blocks, [], blocks[0], 128, 1, **ok)
    lossless = ModelConfigType['c1'].build(batch_size=2, lossless=True)
    lossless.x_shape = [1, 1, 64, 64, 64]
    with pytest.raises(AssertionError, match='count_search.*lossless'):
        lossless.encode_block_range(None, blocks, 128, **ok)


def test_python_wrapper_refuses_rows_that_are_no_ladder():
    import torch
    from pcc_geo_cnn_v2_amd.ops import check_count_rows
    assert check_count_rows(torch.tensor([[5, 5, 3, 0], [9, 1, 1, -2]], dtype=torch.int32), 2) == 4
    for rows, B in [(torch.tensor([[3, 5]], dtype=torch.int32), 1), (torch.tensor([[5, 3]], dtype=torch.int64), 1),
                    (torch.zeros((1, 256), dtype=torch.int32), 1), (torch.zeros((1, 0), dtype=torch.int32), 1), (torch.zeros((2, 3), dtype=torch.int32), 1)]:
        with pytest.raises(L.PccError, match='count rows'):
            check_count_rows(rows, B)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    header = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(rf'\b(int|size_t)\s+{name}\s*\(', header), f'{name} is not declared in include/pcc_geo.h'
        assert name in L.EXPORTS and hasattr(lib, name)
    assert len(lib.pcc_rank_levels.argtypes) == 12 and len(lib.pcc_d1_count_stats.argtypes) == 19 and len(lib.pcc_d12_count_stats.argtypes) == 24
    assert L.ABI_VERSION == 4 and lib.pcc_abi_version() == 4
    assert lib.pcc_rank_levels_workspace_bytes(0, 64) == 0 and lib.pcc_rank_levels_workspace_bytes(1, (1 << 28) + 1) == 0
    assert lib.pcc_rank_levels_workspace_bytes(65536, 1) == 0 and lib.pcc_rank_levels_workspace_bytes(16, 1 << 28) == 0       # B n >= 2^31
    assert lib.pcc_rank_levels_workspace_bytes(1, -1) == 0
