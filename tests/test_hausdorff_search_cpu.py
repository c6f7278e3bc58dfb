"""Hausdorff objectives of the per-block search, the parts that need no GPU: the host restatement
(model_opt.host_threshold_stats(hausdorff=True)) against an O(|A| |B_t|) brute force, the names and their validation, the decision rule
on nine-slot tallies, and every refusal."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hausdorff_search_ref as R  # noqa: E402
from pcc_geo_cnn_v2_amd import _lib as L  # noqa: E402
from pcc_geo_cnn_v2_amd import model_opt as MO  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import pc_metric as PM  # noqa: E402

THR17 = np.linspace(0.0, 1.0, 17)
REFERENCE_NAMES = ['d1_sum_AB', 'd1_sum_BA', 'd1_sum_max', 'd1_sum_mean', 'd1_mse_AB', 'd1_mse_BA', 'd1_mse',
                   'd2_sum_AB', 'd2_sum_BA', 'd2_sum_max', 'd2_sum_mean', 'd2_mse_AB', 'd2_mse_BA', 'd2_mse']
NEW_NAMES = ['d1_hausdorff_AB', 'd1_hausdorff_BA', 'd1_hausdorff', 'd2_hausdorff_AB', 'd2_hausdorff_BA', 'd2_hausdorff']


# ---- host restatement against brute force -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(8, 8, 8), (6, 7, 5)])
def test_host_d1_slots_equal_brute_force(shape):
    """Dense random blocks (ties everywhere: D1 does not depend on the pick): every D1 slot, sums and maxima, of every level set."""
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        block, x_hat = R.random_block(rng, shape, n_points=23, fill=0.35)
        tallies, mean_tally = MO.host_threshold_stats(block, x_hat, THR17, hausdorff=True)
        want = R.brute_tallies(block, x_hat, THR17)
        assert tallies.shape == want.shape and tallies.shape[1] == 9 and len(tallies) >= 3
        d1 = [PM.N_B, PM.D1_AB, PM.D1_BA, PM.H1_AB, PM.H1_BA]
        assert np.array_equal(tallies[:, d1], want[:, d1])
        assert not tallies[:, [PM.D2_AB, PM.D2_BA, PM.H2_AB, PM.H2_BA]].any()          # no normals: the d2 slots stay zero
        plain, plain_mean = MO.host_threshold_stats(block, x_hat, THR17)
        assert np.array_equal(plain, tallies[:, :5]) and np.array_equal(plain_mean, mean_tally[:5])      # the five sum slots are the plain call's
        # the guard: the single rounded mean point
        sq = ((block[:, :3] - np.round(block[:, :3].mean(0))) ** 2).sum(1)
        assert mean_tally[PM.H1_AB] == sq.max() and mean_tally[PM.H1_BA] == sq.min()
        assert np.array_equal(MO.mean_point_d1_tally(block, hausdorff=True), mean_tally)
        assert np.array_equal(MO.mean_point_d1_tally(block), mean_tally[:5])


@pytest.mark.parametrize('shape', [(8, 8, 8), (6, 7, 5)])
def test_host_d2_slots_equal_brute_force_tie_free(shape):
    """Sparse blocks drawn until no point of any level set has two equidistant nearest neighbours (the construction of
    tests/golden/model_opt_d2_tiefree.npz: a handful of points in a mostly empty block), so that the KD-tree's pick and the brute
    force's are the same links and all nine slots are equal bits."""
    found = 0
    for seed in range(400):
        rng = np.random.default_rng(7000 + seed)
        block, x_hat = R.random_block(rng, shape, n_points=4, fill=0.02, normals=True)
        want = R.brute_tallies(block, x_hat, THR17, tie_free_only=True)
        if want is None or len(want) < 2:
            continue
        found += 1
        tallies, mean_tally = MO.host_threshold_stats(block, x_hat, THR17, normals=block[:, 3:], hausdorff=True)
        assert np.array_equal(tallies, want), (seed, tallies - want)
        assert (tallies[:, PM.H2_AB] <= tallies[:, PM.D2_AB]).all() and (tallies[:, PM.H2_BA] <= tallies[:, PM.D2_BA]).all()
        assert np.array_equal(MO.mean_point_tally(block, True, hausdorff=True)[:5], MO.mean_point_tally(block, True))
        if found == 4:
            break
    assert found == 4, f'only {found} tie-free blocks in 400 draws'


def test_host_decision_is_the_brute_force_argmin():
    """compute_optimal_thresholds with the new names: the first minimum of the brute-force column, or 'emit nothing' where the mean
    point is strictly better."""
    rng = np.random.default_rng(5)
    block, x_hat = R.random_block(rng, (8, 8, 8), n_points=30, fill=0.4)
    names, best = MO.compute_optimal_thresholds(block, x_hat, THR17, 8, opt_metrics=['d1_mse', 'd1_hausdorff', 'd1_hausdorff_AB', 'd1_hausdorff_BA'])
    assert names == ['d1_mse_inf', 'd1_hausdorff_inf', 'd1_hausdorff_AB_inf', 'd1_hausdorff_BA_inf']
    want = R.brute_tallies(block, x_hat, THR17)
    guard = MO.mean_point_d1_tally(block, hausdorff=True)
    cols = {'d1_hausdorff': np.maximum(want[:, PM.H1_AB], want[:, PM.H1_BA]), 'd1_hausdorff_AB': want[:, PM.H1_AB], 'd1_hausdorff_BA': want[:, PM.H1_BA]}
    gv = {'d1_hausdorff': max(guard[PM.H1_AB], guard[PM.H1_BA]), 'd1_hausdorff_AB': guard[PM.H1_AB], 'd1_hausdorff_BA': guard[PM.H1_BA]}
    for name, got in zip(names[1:], best[1:]):
        col = cols[name[:-4]]
        k = int(np.argmin(col))
        assert got == (len(THR17) - 1 if col[k] > gv[name[:-4]] else k)
    assert best[0] == MO.compute_optimal_thresholds(block, x_hat, THR17, 8, opt_metrics=['d1_mse'])[1][0]


# ---- names and validation -----------------------------------------------------------------------------------------------------------
def test_names_and_validation():
    assert PM.avail_opt_metrics == REFERENCE_NAMES                     # the reference's list, untouched
    assert PM.hausdorff_opt_metrics == NEW_NAMES
    PM.validate_opt_metrics(NEW_NAMES[:3])
    PM.validate_opt_metrics(NEW_NAMES + REFERENCE_NAMES, with_normals=True)
    with pytest.raises(AssertionError, match=re.escape('d2_hausdorff_AB not available without normals')):
        PM.validate_opt_metrics(['d1_hausdorff', 'd2_hausdorff_AB'])
    with pytest.raises(AssertionError, match=re.escape(f'd1_hausdorf not found in {REFERENCE_NAMES}')):
        PM.validate_opt_metrics(['d1_hausdorf'])
    assert PM.wants_hausdorff(['d1_mse', 'd2_hausdorff']) and not PM.wants_hausdorff(['d1_mse', 'd2_mse']) and not PM.wants_hausdorff(())


def test_metrics_table_columns():
    rng = np.random.default_rng(1)
    t9 = rng.integers(1, 50, (6, 9)).astype(np.float64)
    plain, full = PM.metrics_table(11, t9[:, :5], 63), PM.metrics_table(11, t9, 63)
    assert set(full) - set(plain) == set(NEW_NAMES)
    for k in plain:
        assert np.array_equal(plain[k], full[k])
    h = PM.hausdorff_table(t9, 63, with_normals=True)
    for k in NEW_NAMES:
        assert np.array_equal(full[k], h[k])
    assert set(PM.metrics_table(11, t9[0], 63, ['d1'])) - set(PM.metrics_table(11, t9[0, :5], 63, ['d1'])) == set(NEW_NAMES[:3])


def test_abi_declares_the_hausdorff_entries():
    with open(os.path.join(ROOT, 'include', 'pcc_geo.h')) as f:
        hdr = f.read()
    for sym in ('pcc_d1_threshold_stats', 'pcc_d12_threshold_stats', 'pcc_d1_count_stats', 'pcc_d12_count_stats'):
        assert re.search(rf'\bint {sym}_hausdorff\(', hdr) and f'{sym}_hausdorff' in L.EXPORTS
    assert not re.search(r'_stats_ties_hausdorff|_stats_hausdorff_ties', hdr)
    assert L.ABI_VERSION == 4 and re.search(r'#define\s+PCC_ABI_VERSION\s+4\b', hdr)


# ---- selection ------------------------------------------------------------------------------------------------------------------------
def _tallies(n_b, h_ab, h_ba):
    t = np.zeros((len(n_b), 9), np.float64)
    t[:, PM.N_B], t[:, PM.H1_AB], t[:, PM.H1_BA] = n_b, h_ab, h_ba
    t[:, PM.D1_AB], t[:, PM.D1_BA] = t[:, PM.H1_AB] * 3, t[:, PM.H1_BA] * 2
    return t


def _guard(h_ab, h_ba):
    g = np.zeros(9, np.float64)
    g[PM.N_B], g[PM.H1_AB], g[PM.H1_BA], g[PM.D1_AB], g[PM.D1_BA] = 1, h_ab, h_ba, 1e9, 1e9
    return g


def test_selection_plateau_takes_the_first_minimum():
    t = _tallies([50, 40, 30, 20, 10], [9, 4, 4, 4, 6], [1, 2, 4, 3, 9])
    names, best = MO.select_thresholds_from_stats(25, t, _guard(100, 100), 17, 64, ['d1_hausdorff_AB', 'd1_hausdorff', 'd1_hausdorff_BA'], [np.inf])
    assert names == ['d1_hausdorff_AB_inf', 'd1_hausdorff_inf', 'd1_hausdorff_BA_inf']
    assert best == [1, 1, 0]        # AB: plateau 4,4,4 -> index 1;  symmetric: max = 9,4,4,4,9 -> index 1;  BA: index 0


def test_selection_guard_wins_only_when_strictly_better():
    t = _tallies([50, 40, 30], [9, 5, 7], [1, 2, 4])
    assert MO.select_thresholds_from_stats(25, t, _guard(4, 0), 17, 64, ['d1_hausdorff_AB'], [np.inf])[1] == [16]       # 4 < 5: emit nothing
    assert MO.select_thresholds_from_stats(25, t, _guard(5, 0), 17, 64, ['d1_hausdorff_AB'], [np.inf])[1] == [1]        # a tie keeps the candidate
    # mixed with a sum metric: each name decides on its own column
    assert MO.select_thresholds_from_stats(25, t, _guard(4, 0), 17, 64, ['d1_sum_AB', 'd1_hausdorff_AB'], [np.inf])[1] == [1, 16]


def test_selection_max_delta_without_an_eligible_candidate():
    t = _tallies([500, 400, 300], [9, 5, 7], [1, 2, 4])        # |B| / |A| >= 12: nothing inside (1/2, 2), so every candidate stays in the pool
    assert MO.select_thresholds_from_stats(25, t, _guard(100, 100), 17, 64, ['d1_hausdorff_AB'], [2.0])[1] == [1]
    t[2, PM.N_B] = 30                                          # now only candidate 2 is eligible
    assert MO.select_thresholds_from_stats(25, t, _guard(100, 100), 17, 64, ['d1_hausdorff_AB'], [2.0, np.inf])[1] == [2, 1]


def test_selection_slot_width_follows_the_metrics():
    t = _tallies([50, 40, 30], [9, 5, 7], [1, 2, 4])
    with pytest.raises(AssertionError, match='9-slot tallies expected'):
        MO.select_thresholds_from_stats(25, t[:, :5], _guard(1, 1)[:5], 17, 64, ['d1_hausdorff'], [np.inf])
    assert MO.select_thresholds_from_stats(25, t[:, :5], _guard(1, 1)[:5], 17, 64, ['d1_sum_AB'], [np.inf])[1] == [1]
    assert MO.select_thresholds_from_stats(25, np.zeros((0, 9)), _guard(1, 1), 17, 64, ['d1_hausdorff'], [np.inf])[1] == [16]
    blocks = [np.array([[1, 1, 1], [3, 2, 1], [2, 2, 6]], np.float64)]
    names, best = MO.decide_from_tallies(blocks, [t], 17, 64, ['d1_hausdorff_AB'], [np.inf])
    assert best == [[1]]       # the guard of this block: H1_AB = 13 > 5
    names, ks, idx = MO.decide_counts_from_tallies(blocks, [t], np.array([[9, 6, 3]], np.int32), 64, ['d1_hausdorff_AB'], [np.inf])
    assert idx == [[1]] and ks == [[6]]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_flag():
    MO.check_hausdorff_search(['d1_mse', 'd2_mse'], 'mean', False, 4)            # no Hausdorff metric: nothing to refuse
    MO.check_hausdorff_search(['d1_hausdorff'], 'pick', False, 1)                # d1 never needs the D2 engine
    MO.check_hausdorff_search(['d2_hausdorff'], 'pick', True, 1)
    with pytest.raises(AssertionError, match='--d2_search gpu'):
        MO.check_hausdorff_search(['d1_mse', 'd2_hausdorff_BA'], 'pick', False, 1)
    with pytest.raises(AssertionError, match='--d2_search gpu'):
        MO.check_hausdorff_search(['d2_hausdorff'], 'pick', lambda: False, 1)
    with pytest.raises(AssertionError, match='--search_ties'):
        MO.check_hausdorff_search(['d1_hausdorff', 'd2_mse'], 'mean', True, 1)
    with pytest.raises(AssertionError, match='--gpus 1'):
        MO.check_hausdorff_search(['d1_hausdorff'], 'pick', True, 2)
    with pytest.raises(AssertionError, match="ties='pick'"):
        MO.host_threshold_stats(np.zeros((1, 6)), np.zeros((2, 2, 2), np.float32), THR17, np.zeros((1, 3)), ties='mean', hausdorff=True)
    with pytest.raises(AssertionError, match='--search_ties'):
        MO.compute_optimal_thresholds(np.zeros((1, 6)), np.zeros((2, 2, 2), np.float32), THR17, 8, normals=np.zeros((1, 3)),
                                      opt_metrics=['d2_hausdorff'], ties='mean')


def test_cli_refuses_at_argument_time():
    from pcc_geo_cnn_v2_amd import compress_octree as CO
    base = ['--input_files', 'a.ply', '--checkpoint_dir', 'x', '--model_config', 'c3p', '--input_normals', 'a.n.ply']
    parse = lambda *extra: CO.build_parser().parse_args(base + list(extra))
    two = ['--output_files', 'o1', 'o2', '--opt_metrics', 'd1_hausdorff', 'd2_hausdorff']
    CO.check_encode_options(parse(*two, '--d2_search', 'gpu'), 1)
    CO.check_encode_options(parse('--output_files', 'o1', '--opt_metrics', 'd1_hausdorff'), 1)
    CO.check_encode_options(parse(*two, '--fixed_threshold'), 1)              # no search runs
    with pytest.raises(AssertionError, match=r'--opt_metrics: opt metric d2_hausdorff.*--d2_search gpu'):
        CO.check_encode_options(parse(*two), 1)
    with pytest.raises(AssertionError, match=r'--d2_search gpu'):
        CO.check_encode_options(parse(*two, '--d2_search', 'kdtree'), 1)
    with pytest.raises(AssertionError, match=r'--opt_metrics: opt metric d1_hausdorff.*--search_ties mean'):
        CO.check_encode_options(parse(*two, '--d2_search', 'gpu', '--search_ties', 'mean'), 1)
    with pytest.raises(AssertionError, match=r'world size 2.*--gpus 1'):
        CO.check_encode_options(parse('--output_files', 'o1', '--opt_metrics', 'd1_hausdorff'), 2)
    help_text = CO.build_parser().format_help().replace('\n', ' ')
    help_text = re.sub(r'\s+', ' ', help_text)
    assert help_text.index("'d2_mse']") < help_text.index("'d1_hausdorff_AB'")      # the new names follow the existing ones
    from pcc_geo_cnn_v2_amd import ev_experiment as EV
    ev_help = re.sub(r'\s+', ' ', EV.build_parser().format_help())
    assert ev_help.index("'d2_mse']") < ev_help.index("'d1_hausdorff_AB'")
