"""CPU: the colour transfer surface that needs no GPU -- utils/pc_metric.transfer_colors_host against an independent all-pairs
restatement (tests/_transfer_cases.py), the two C ABI symbols and their argument refusals, the input checks of ops.transfer_colors
that run before any GPU call, the benefit of the transfer over rank 1 as a condition, and the map_color / ev_experiment parsers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _color_ref as R
import _transfer_cases as T
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ev_experiment, ev_run_experiment, map_color, ops
from pcc_geo_cnn_v2_amd.utils import pc_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pcc_cloud_transfer_workspace_bytes', 'pcc_cloud_transfer_colors')
CASES = T.cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_restatement_equals_brute_force(name):
    a, ca, b = CASES[name]
    assert max(len(a), len(b)) <= 50000
    got, votes = pc_metric.transfer_colors_host(a, ca, b)
    ref, ref_votes = T.transfer_brute(a, ca, b)
    assert got.dtype == np.uint8 and got.shape == (len(b), 3) and votes.dtype == np.int64 and votes.shape == (len(b),)
    assert np.array_equal(votes, ref_votes)
    assert np.array_equal(got, ref)


def test_the_cases_are_what_they_are_meant_to_be():
    """Each edge the cases are there for, checked on the brute-force result."""
    out = {k: T.transfer_brute(*v) for k, v in CASES.items() if k != 'random256'}
    a, ca, b = CASES['identity']
    assert np.array_equal(out['identity'][0], ca) and (out['identity'][1] == 1).all()
    assert np.array_equal(out['na1_nb1'][0], CASES['na1_nb1'][1]) and out['na1_nb1'][1].tolist() == [1]
    col, votes = out['large_tie_set']
    assert (votes[:30] >= 1).all() and votes[30] == 0                      # the centre votes for all 30 shell points
    assert out['rounding'][0].tolist() == [[1, 0, 2]] and out['rounding'][1].tolist() == [2]     # 0.5 -> 1, 0 -> 0, 1.5 -> 2
    assert (out['fallback_far'][1] == 0).sum() >= 51 and (out['fallback_far'][1] > 0).any()
    share = (out['fallback_jitter'][1] == 0).mean()
    assert 0.1 < share < 0.3, share                                        # about a fifth of the jittered rows fall back
    a, ca, b = CASES['duplicates']
    col, votes = out['duplicates']
    _, first, inv = np.unique(b, axis=0, return_index=True, return_inverse=True)
    assert len(first) < len(b)
    assert np.array_equal(col, col[first][inv.reshape(-1)]) and np.array_equal(votes, votes[first][inv.reshape(-1)])
    a, ca, b = CASES['domain_edges']
    assert a.min() == 0 and a.max() == T.TOP and b.min() == 0 and b.max() == T.TOP
    col, votes = out['many_voters']
    a, ca, b = CASES['many_voters']
    s = ca.astype(np.int64).sum(0)
    assert votes.tolist() == [len(a)] and col.tolist() == [((2 * s + len(a)) // (2 * len(a))).tolist()]
    assert len(T._shell9()) >= 30


def test_host_result_ignores_the_row_order_of_either_cloud():
    a, ca, b = CASES['fallback_jitter']
    ref, votes = pc_metric.transfer_colors_host(a, ca, b)
    rng = np.random.default_rng(2)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    got, v = pc_metric.transfer_colors_host(a[pa], ca[pa], b)
    assert np.array_equal(got, ref) and np.array_equal(v, votes)
    got, v = pc_metric.transfer_colors_host(a, ca, b[pb])
    assert np.array_equal(got, ref[pb]) and np.array_equal(v, votes[pb])


def test_transfer_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', hdr), name
        assert name in L.EXPORTS
        assert hasattr(C.CDLL(L.LIB_PATH), name)
    assert 'not TMC13-conformant' in hdr.replace('NOT', 'not')


def test_sizes_outside_the_range_and_null_arguments_are_refused():
    lib = L.lib()
    ws = lib.pcc_cloud_transfer_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1 << 31, 5) == 0 and ws(5, 1 << 31) == 0 and ws(5, -1) == 0
    assert ws(1, 1) > 0 and ws(7, 100000) >= 100000 * 28 > ws(7, 10)       # three 64-bit sums and a 32-bit count per row of B
    # refused before the context is touched: a dummy non-NULL handle never gets dereferenced
    h, p = C.c_void_p(16), C.c_void_p(256)
    call = lambda na, nb: lib.pcc_cloud_transfer_colors(h, p, na, p, p, nb, p, None, p, None)
    for na, nb in ((0, 5), (5, 0), (-1, 5), (1 << 31, 5), (5, 1 << 31)):
        assert call(na, nb) == L.PCC_ERR_ARG, (na, nb)
        assert 'outside [1, 2^31)' in lib.pcc_last_error().decode()
    nulls = [(None, p, p, p, p, p), (h, None, p, p, p, p), (h, p, None, p, p, p), (h, p, p, None, p, p), (h, p, p, p, None, p),
             (h, p, p, p, p, None)]
    for ctx, ia, ca, ib, out, work in nulls:
        assert lib.pcc_cloud_transfer_colors(ctx, ia, 5, ca, ib, 5, out, None, work, None) == L.PCC_ERR_ARG
        assert 'NULL' in lib.pcc_last_error().decode()


class _NoGpu:
    """A context that fails on use: the input checks must raise before anything touches it."""
    def __getattr__(self, name):
        raise AssertionError(f'GPU context used ({name}) before the inputs were checked')


GOOD = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.int32)
GOOD_C = np.array([[1, 2, 3], [4, 5, 6], [250, 0, 9]], np.uint8)


@pytest.mark.parametrize('kw,what', [
    (dict(a_colors=GOOD_C[:2]), r'\(3, 3\)'),
    (dict(a_colors=GOOD_C.astype(np.float32)), 'integers in 0..255'),
    (dict(a_colors=GOOD_C.astype(np.int16) + 200), 'integers in 0..255'),
    (dict(a_colors=GOOD_C.astype(np.int32) - 10), 'integers in 0..255'),
    (dict(index_a=np.array([[0.5, 1, 2], [1, 1, 1], [2, 2, 2]])), 'integers'),
    (dict(index_a=np.zeros((0, 3), np.int32), a_colors=np.zeros((0, 3), np.uint8)), r'\(N, 3\)'),
    (dict(queries=np.array([[-1, 0, 0]])), r'\[0, 2097152\)'),
    (dict(queries=np.array([[0, 0, 1 << 21]])), r'\[0, 2097152\)'),
    (dict(queries=np.zeros((2, 2), np.int32)), r'\(N, 3\)'),
    (dict(queries=GOOD + 0.25), 'integers'),
])
def test_transfer_colors_checks_its_inputs_before_any_gpu_call(kw, what):
    args = dict(index_a=GOOD, a_colors=GOOD_C, queries=GOOD)
    args.update(kw)
    with pytest.raises(L.PccError, match=what):
        ops.transfer_colors(_NoGpu(), args['index_a'], args['a_colors'], args['queries'])


def test_transfer_colors_of_no_queries_is_empty_and_needs_no_gpu():
    out = ops.transfer_colors(_NoGpu(), GOOD, GOOD_C, np.zeros((0, 3), np.int32))
    assert out.shape == (0, 3) and out.dtype == np.uint8
    out, votes = ops.transfer_colors(_NoGpu(), GOOD, GOOD_C, np.zeros((0, 3)), return_votes=True)
    assert out.shape == (0, 3) and votes.shape == (0,) and votes.dtype == np.int32


def test_transfer_never_loses_to_rank_one_on_the_original_to_decoded_sums():
    """The condition the transfer exists for: the mean of the voters minimises each original point's squared error against its
    nearest decoded points, so on the A->B half of the colour tally (Y, U and V: BT.709 is linear in RGB) it is at or below the
    rank-1 copy; rounding the mean to uint8 is all that could break it, and the margins are two orders of magnitude beyond that.
    Fixtures: voxelised sphere shells (2 826 and 10 974 points) with a white-noise texture against a 60 % subset, a +-1 jitter and
    coordinates floored to even."""
    fixtures = T.benefit_fixtures()
    assert len(fixtures) == 6
    for name, (a, ca, b) in fixtures.items():
        transfer = pc_metric.transfer_colors_host(a, ca, b)[0]
        rank1 = R.map_ref(a, ca, b, 1)[0]
        t = pc_metric.color_tally_host(a, ca, b, transfer)[:3]
        r = pc_metric.color_tally_host(a, ca, b, rank1)[:3]
        print(name, 'A->B Y/U/V mse, transfer', t / len(a), 'rank 1', r / len(a))
        assert (t <= r).all(), (name, t, r)


def test_map_color_parser_defaults_and_refusals(capsys):
    a = map_color.parse_args(['a.ply', 'b.ply', 'o.ply'])
    assert (a.mode, a.rank) == ('rank', 2)
    assert map_color.parse_args(['a.ply', 'b.ply', 'o.ply', '--rank', '1']).rank == 1
    a = map_color.parse_args(['a.ply', 'b.ply', 'o.ply', '--mode', 'transfer'])
    assert a.mode == 'transfer'
    for bad in (['--mode', 'transfer', '--rank', '2'], ['--rank', '1', '--mode', 'transfer'], ['--mode', 'mean'], ['--rank', '3']):
        with pytest.raises(SystemExit) as e:
            map_color.parse_args(['a.ply', 'b.ply', 'o.ply'] + bad)
        assert e.value.code == 2
    assert '--rank' in capsys.readouterr().err
    with pytest.raises(ValueError, match='mode'):
        map_color.map_color('a.ply', 'b.ply', 'o.ply', mode='mean')


def test_report_names_the_recolouring_only_when_it_is_transfer(tmp_path):
    import pandas as pd
    from pcc_geo_cnn_v2_amd import ev_report
    from pcc_geo_cnn_v2_amd.utils import pc_io
    a, ca, b = CASES['fallback_jitter']
    cb = pc_metric.transfer_colors_host(a, ca, b)[0]
    for f, p, c in (('a.ply', a, ca), ('b.ply', b, cb)):
        pc_io.write_ply(str(tmp_path / f), pd.DataFrame({'x': p[:, 0].astype(np.float32), 'y': p[:, 1].astype(np.float32),
                                                         'z': p[:, 2].astype(np.float32), 'red': c[:, 0], 'green': c[:, 1], 'blue': c[:, 2]}))
    open(tmp_path / 'a.bin', 'wb').write(b'\x00' * 100)
    paths = [str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a.bin')]
    plain = ev_report.build_report(*paths, 32, color=True)
    assert 'recolor' not in plain and ev_report.build_report(*paths, 32, color=True, recolor='rank2') == plain
    assert ev_report.build_report(*paths, 32, color=True, recolor='transfer') == {**plain, 'recolor': 'transfer'}
    with pytest.raises(AssertionError, match='--color'):
        ev_report.build_report(*paths, 32, recolor='transfer')
    with pytest.raises(AssertionError, match='recolor'):
        ev_report.build_report(*paths, 32, color=True, recolor='mean')


def test_experiment_recolor_option_defaults_to_rank2():
    need = ['--output_dir', 'o', '--model_dir', 'm', '--model_config', 'c3p', '--pc_name', 'x', '--input_pc', 'x.ply', '--opt_metrics',
            'd1_mse', '--max_deltas', 'inf']
    p = ev_experiment.build_parser()
    assert p.parse_args(need).recolor == 'rank2'
    assert p.parse_args(need + ['--recolor', 'transfer']).recolor == 'transfer'
    with pytest.raises(SystemExit):
        p.parse_args(need + ['--recolor', 'rank1'])
    assert 'recolor' in ev_run_experiment.RUN_KEYS
    with pytest.raises(AssertionError, match='recolor'):
        ev_experiment.run_experiment('o', 'm', 'c3p', 'x', 'x.ply', resolution=64, recolor='rank1')
