"""CPU: the tie-averaged D2 rule (--d2_ties mean, DESIGN.md "Tie-averaged D2") on the host path -- pc_metric.tie_mean_tally against
the brute-force restatement tests/_ties_ref.py within the derived rounding bound, bit equality with the default rule where no ties
exist, row-order independence (which the default rule does not have on a tie-heavy input), the ABI surface that needs no GPU and
the command-line contract of ev_report / compress_octree."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import _ties_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import compress_octree, ev_report, model_types, ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
EXACT = [0, 1, 2, 5, 6]           # N_B, D1 sums, H1 maxima
PLANE = [3, 4, 7, 8]              # D2 sums, H2 maxima


def _host(a, b, n, ties='mean'):
    return pc_metric.cloud_tally_host(a.astype(np.float64), b.astype(np.float64), n, ties=ties)


def _within(got, want, bound, what):
    print(what, 'got', got[PLANE], 'want', want[PLANE], 'diff', np.abs(got - want)[PLANE], 'bound', bound[PLANE])
    assert np.array_equal(got[EXACT], want[EXACT]), (what, got, want)
    assert np.all(np.abs(got - want)[PLANE] <= bound[PLANE]), (what, np.abs(got - want)[PLANE], bound[PLANE])


def _permuted(a, b, n, seed):
    rng = np.random.default_rng(seed)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    return a[pa], b[pb], n[pa]


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_mean_matches_the_brute_force(name):
    a, b, n = CASES[name]
    ref = R.tally_ref(a, b, n)
    _within(_host(a, b, n), ref['tally'], R.bounds(ref), name)
    # without normals the D2 / H2 slots are 0 and the rest is unchanged
    bare = _host(a, b, None)
    assert np.array_equal(bare[EXACT], ref['tally'][EXACT]) and not bare[PLANE].any()


def test_the_inputs_have_the_ties_they_are_named_for():
    a, b, _ = CASES['shell']
    shell = R.tally_ref(*CASES['shell'])
    assert shell['C'] >= 3 and shell['V'] >= 3
    assert len(R.tie_sets(b, a)[0]) > 1.5 * len(a) and len(R.tie_sets(a, b)[0]) > 1.5 * len(b)      # tie-heavy: 1.8 / 1.9 per point
    assert R.tally_ref(*CASES['faces'])['C'] == 6 and R.tally_ref(*CASES['faces_swapped'])['V'] == 6
    assert R.tally_ref(*CASES['single_b'])['V'] == len(CASES['single_b'][0])
    q, j, best = R.tie_sets(np.array([[0, 0, 0], [2, 0, 0], [5, 5, 5]]), np.array([[1, 0, 0]]))
    assert q.tolist() == [0, 0] and j.tolist() == [0, 1] and best.tolist() == [1]


def test_hand_computed_tie_average():
    """One original point between two decoded points: both are its nearest, each takes its normal, the term is the mean of the two."""
    a = np.array([[10, 10, 10]], np.int32)
    b = np.array([[9, 10, 10], [10, 10, 12]], np.int32)
    n = np.array([[0.0, 0.0, 1.0]])
    t = _host(a, np.array([[9, 10, 10], [10, 11, 10]], np.int32), np.array([[1.0, 0.0, 0.0]]))
    assert t.tolist() == [2, 1, 2, 0.5, 1, 1, 1, 0.5, 1]                  # A->B: mean(1, 0); B->A: 1 + 0
    t = _host(a, b, n)                                                    # no tie: b0 is the nearest, b1 an orphan
    assert t.tolist() == [2, 1, 5, 0, 4, 1, 4, 0, 4]
    assert np.array_equal(t, R.tally_ref(a, b, n)['tally'])


def test_mean_equals_pick_bit_for_bit_without_ties():
    a, b, n = R.singleton_case()
    ref = R.tally_ref(a, b, n)
    assert R.all_singletons(ref) and ref['V'] >= 1                        # the precondition, by brute force
    q, _, _ = R.tie_sets(b, a)
    assert np.array_equal(q, np.arange(len(a)))
    mean, pick = _host(a, b, n, 'mean'), _host(a, b, n, 'pick')
    assert mean.tobytes() == pick.tobytes(), (mean, pick)
    m = pc_metric.cloud_metrics_batch(a.astype(np.float64), [b.astype(np.float64)], 1023, n, ties='mean')[0]
    p = pc_metric.cloud_metrics_batch(a.astype(np.float64), [b.astype(np.float64)], 1023, n)[0]
    assert m == p


@pytest.mark.parametrize('name', ['shell', 'duplicates', 'sparse'])
def test_mean_does_not_depend_on_the_row_order(name):
    a, b, n = CASES[name]
    ref = R.tally_ref(a, b, n)
    base = _host(a, b, n)
    for seed in (1, 2):
        _within(_host(*_permuted(a, b, n, seed)), base, R.bounds(ref), (name, seed))
    # the brute force itself is row-order independent within the same bound
    _within(R.tally_ref(*_permuted(a, b, n, 3))['tally'], ref['tally'], R.bounds(ref), (name, 'ref'))


def test_pick_depends_on_the_row_order_on_the_shell():
    """The input can tell the two rules apart: the same permutation that leaves `mean` within the bound moves `pick` past it."""
    a, b, n = CASES['shell']
    bound = R.bounds(R.tally_ref(a, b, n))
    base = _host(a, b, n, 'pick')
    moved = [np.abs(_host(*_permuted(a, b, n, seed), 'pick') - base) for seed in (1, 2)]
    print('pick moves by', [m[[3, 4]] for m in moved], 'bound', bound[[3, 4]])
    assert all(np.array_equal(_host(*_permuted(a, b, n, seed), 'pick')[EXACT], base[EXACT]) for seed in (1, 2))
    assert any((m[[3, 4]] > bound[[3, 4]]).any() for m in moved), (moved, bound)


def test_metric_tables_take_the_rule():
    a, b, n = CASES['shell']
    A, B = a.astype(np.float64), b.astype(np.float64)
    tally = _host(a, b, n)
    want = pc_metric.metrics_table(len(a), tally[:5], 1023)
    got = pc_metric.cloud_metrics_batch(A, [B, np.zeros((0, 3))], 1023, n, ties='mean')
    assert got[1] is None and got[0] == want
    assert pc_metric.cloud_metrics_batch(A, [B], 1023, ties='mean')[0] == pc_metric.cloud_metrics_batch(A, [B], 1023)[0]      # D1 only
    with pytest.raises(AssertionError, match='ties'):
        pc_metric.cloud_metrics_batch(A, [B], 1023, n, ties='median')
    with pytest.raises(AssertionError, match='ties'):
        pc_metric.cloud_tally_host(A, B, n, ties='min')


def _ties_args(rule):
    return compress_octree.build_parser().parse_args(['--input_files', 'a.ply', '--output_files', 'a.bin', '--checkpoint_dir', 'ck',
                                                      '--model_config', 'c3p', '--opt_metrics', 'd1_mse', '--d2_ties', rule])


def test_mean_is_refused_across_ranks():
    class TwoRanks(pc_metric.SingleProcess):
        world = 2
    a, b, n = CASES['sparse']
    with pytest.raises(AssertionError, match='single-process'):
        pc_metric.cloud_metrics_batch(a.astype(np.float64), [b.astype(np.float64)], 1023, n, comm=TwoRanks(), ties='mean')
    with pytest.raises(AssertionError, match='--d2_ties.*single-process'):
        compress_octree.check_encode_options(_ties_args('mean'), 2)
    compress_octree.check_encode_options(_ties_args('mean'), 1)
    compress_octree.check_encode_options(_ties_args('pick'), 4)
    with pytest.raises(AssertionError, match='ties'):
        model_types.select_best_per_opt_metric([], [], 1, [], np.zeros((0, 3)), 64, False, d2_ties='max')


def test_compress_octree_flag_and_metric_json(tmp_path):
    base = ['--input_files', 'a.ply', '--output_files', 'a.bin', '--checkpoint_dir', 'ck', '--model_config', 'c3p', '--opt_metrics', 'd1_mse']
    parser = compress_octree.build_parser()
    assert parser.parse_args(base).d2_ties == 'pick'
    assert parser.parse_args(base + ['--d2_ties', 'mean']).d2_ties == 'mean'
    with pytest.raises(SystemExit):
        parser.parse_args(base + ['--d2_ties', 'max'])
    assert 'threshold search keeps' in ' '.join(parser.format_help().split())
    records = {}
    for rule in ('pick', 'mean'):
        args = parser.parse_args(base + ['--d2_ties', rule])
        args.resolution, args.octree_level, args.debug = 64, 1, False
        target = str(tmp_path / f'{rule}.bin')
        info = {'numerics_tag': 'tag', 'metrics': {'d1_mse': 0.5, 'd2_mse': 0.25}}
        compress_octree._write_rate_point(target, None, [1, 0, 0, 0, 0, 0, 0, 0], [([b'ab', b'c'], 7)], info, args, [], [])
        records[rule] = open(target + '.enc.metric.json').read()
    assert json.loads(records['mean']) == dict(json.loads(records['pick']), d2_ties='mean')
    assert 'd2_ties' not in json.loads(records['pick'])
    args = parser.parse_args(base)
    args.resolution, args.octree_level, args.debug = 64, 1, False
    del args.d2_ties                                                     # a caller that predates the flag
    compress_octree._write_rate_point(str(tmp_path / 'old.bin'), None, [1, 0, 0, 0, 0, 0, 0, 0], [([b'ab', b'c'], 7)], info, args, [], [])
    assert open(str(tmp_path / 'old.bin') + '.enc.metric.json').read() == records['pick']


def test_ev_report_end_to_end_on_the_host(tmp_path):
    a, b, n = CASES['shell']
    pa, pb, pn, enc = (str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a_n.ply', 'a.bin'))
    pc_io.write_pc(pa, a.astype(np.float32))
    pc_io.write_pc(pb, b.astype(np.float32))
    pc_io.write_df(pn, pd.DataFrame(np.hstack([a, n]).astype(np.float32), columns=['x', 'y', 'z', 'nx', 'ny', 'nz']))
    open(enc, 'wb').write(b'\x00' * 100)
    nrm = pc_io.load_normals(pn)
    assert nrm.shape == (len(a), 3)

    def run(out, *extra):
        cmd = [sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_report', '--input_pc', pa, '--decoded_pc', pb, '--enc_pc', enc, '--input_norm', pn,
               '--resolution', '64', '--hausdorff', '--output', str(tmp_path / out), *extra]
        return subprocess.run(cmd, cwd=ROOT, capture_output=True)

    assert run('plain.json').returncode == 0
    assert run('pick.json', '--d2_ties', 'pick').returncode == 0
    assert run('mean.json', '--d2_ties', 'mean', '--metrics_device', 'host').returncode == 0
    assert run('bad.json', '--d2_ties', 'max').returncode != 0
    plain, pick, mean = (open(tmp_path / f).read() for f in ('plain.json', 'pick.json', 'mean.json'))
    assert plain == pick and 'd2_ties' not in json.loads(plain)         # the default report: byte-identical
    mean = json.loads(mean)
    assert mean.pop('d2_ties') == 'mean' and set(mean) == set(json.loads(plain))
    # the report's numbers are the brute force's (normals as the file stores them: float32)
    ref = R.tally_ref(a, b, np.asarray(nrm, np.float64))
    bound = R.bounds(ref)
    t = ref['tally']
    assert mean['d1_mse'] == json.loads(plain)['d1_mse'] == max(t[1] / len(a), t[2] / len(b))
    assert abs(mean['d2_mse'] - max(t[3] / len(a), t[4] / len(b))) <= max(bound[3] / len(a), bound[4] / len(b))
    assert abs(mean['d2_hausdorff'] - max(t[7], t[8])) <= max(bound[7], bound[8])
    assert mean['d2_mse'] != json.loads(plain)['d2_mse']
    assert ev_report.build_report(pa, pb, enc, 64, input_norm=pn, hausdorff=True, d2_ties='mean') == dict(mean, d2_ties='mean')


def test_abi_surface_and_argument_checks():
    lib = L.lib()
    assert L.ABI_VERSION == 4 and lib.pcc_abi_version() == 4
    ws = lib.pcc_cloud_distortion_ties_workspace_bytes
    assert ws(100, 50, 0, 0) == lib.pcc_cloud_distortion_workspace_bytes(100, 50)      # pick: the existing call's workspace
    assert ws(0, 5, 1, 10) == 0 and ws(5, 0, 1, 10) == 0 and ws(5, 5, 2, 10) == 0 and ws(5, 5, 1, 0) == 0 and ws(5, 5, 1, 1 << 31) == 0
    small, large = ws(1000, 800, 1, 1000), ws(1000, 800, 1, 5000)
    assert small >= lib.pcc_cloud_distortion_workspace_bytes(1000, 800)
    assert large - small >= 4000 * 16                                     # the sizing rule: four 32-bit arrays per pair (+ sort space)
    assert ops.tie_pair_capacity(1000) == 5024 and ops.tie_pair_capacity(1 << 30) == (1 << 31) - 1
    assert ops.TIE_MODES == {'pick': 0, 'mean': 1}

    class NoGpu:
        device = None
    good = np.zeros((2, 3), np.int32)
    with pytest.raises(L.PccError, match='ties'):
        ops.cloud_distortion(NoGpu(), good, good, ties='median')
    e = ops.TiePairOverflow(12, 5)
    assert isinstance(e, L.PccError) and e.pairs == 12 and 'max_pairs >= 12' in str(e)
