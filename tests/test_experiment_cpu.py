"""CPU: the experiment YAML (utils/experiment.py), the job list of ev_run_experiment and the training plan of tr_train_all, the
trainer replaced by a recorder."""
import math
import os

import pytest
import yaml

from pcc_geo_cnn_v2_amd import ev_experiment, ev_run_experiment, tr_train_all
from pcc_geo_cnn_v2_amd.utils import experiment as E

YAML = """
MPEG_TMC13_DIR: "/nowhere/tmc13"
PCERROR: "/nowhere/pc_error_d"
MPEG_DATASET_DIR: "{root}/dataset"
TRAIN_DATASET_PATH: "{root}/blocks/**/*.ply"
TRAIN_RESOLUTION: 64
EXPERIMENT_DIR: "{root}/exp"
model_configs:
  - id: 'c4-ws'
    config: 'c3p'
    lambdas: [3.0e-4, 1.0e-4, 5.0e-5]
    alpha: 0.75
    train_mode: 'warm_seq'
    fixed_threshold: False
    label: 'c6'
  - id: 'c4'
    checkpoint_id: 'c3p-a0.75'
    config: 'c3p'
    lambdas: [3.0e-4, 1.0e-4]
    alpha: 0.75
    fixed_threshold: False
    opt_metrics: ['d1_mse']
    max_deltas: [1, .inf]
  - id: 'c3p-a0.75'
    config: 'c3p'
    lambdas: [3.0e-4, 1.0e-4]
    alpha: 0.75
    label: 'c4'
  - id: 'c1'
    config: 'c1'
    lambdas: [2.0e-4, 0.000005]
    batch_size: 16
    gamma: 1.5
opt_metrics: ['d1_mse', 'd2_mse']
max_deltas: [.inf]
alpha: 0.9
gamma: 2.0
batch_size: 32
train_mode: 'independent'
fixed_threshold: True
mpeg_modes:
  - id: 'trisoup-predlift/lossy-geom-lossy-attrs'
    label: 'G-PCC trisoup'
eval_modes:
  - id: 'main'
    lims: [[None, 1.0, 57.5, 75.5], [None, 1.0, 62, 80.5]]
    modes:
      - id: 'c4-ws'
      - id: 'c4'
        label: 'c5'
      - id: 'trisoup-predlift/lossy-geom-lossy-attrs'
bd_ignore: ['c4-ws/1.00e-05']
pcerror_mpeg_mode: 'trisoup-predlift/lossy-geom-lossy-attrs'
data:
  - pc_name: loot_vox10_1200
    cfg_name: loot_vox10_1200
    input_pc: People/loot_vox10_1200.ply
    input_norm: People/loot_vox10_1200_n.ply
    resolution: 1024
  - pc_name: soldier_vox10_0690
    input_pc: People/soldier_vox10_0690.ply
    input_norm: People/soldier_vox10_0690_n.ply
    pcerror_cfg: "{root}/soldier_pcerror.cfg"
    octree_level: 3
"""


@pytest.fixture
def exp(tmp_path):
    path = tmp_path / 'experiment.yml'
    path.write_text(YAML.format(root=tmp_path))
    (tmp_path / 'soldier_pcerror.cfg').write_text('uniqueSplitBySensor: 1\nresolution: 1023\ncolor: 0\n')
    return E.load_experiment(str(path))


def _models(exp):
    return E.index_by_id(exp['model_configs'])


def test_settings_fall_through_from_the_top_level_to_a_model(exp):
    m = _models(exp)
    assert E.coding_settings(exp, m['c4-ws']) == dict(opt_metrics=['d1_mse', 'd2_mse'], max_deltas=[math.inf], fixed_threshold=False)
    assert E.coding_settings(exp, m['c4']) == dict(opt_metrics=['d1_mse'], max_deltas=[1., math.inf], fixed_threshold=False)
    assert E.coding_settings(exp, m['c1']) == dict(opt_metrics=['d1_mse', 'd2_mse'], max_deltas=[math.inf], fixed_threshold=True)
    assert E.training_settings(exp, m['c4-ws']) == dict(alpha=0.75, gamma=2.0, batch_size=32, train_mode='warm_seq')
    assert E.training_settings(exp, m['c1']) == dict(alpha=0.9, gamma=1.5, batch_size=16, train_mode='independent')
    assert E.opt_groups(['d1_mse']) == ['d1'] and E.opt_groups(['d2_mse', 'd1_mse']) == ['d1', 'd2']


def test_directories_checkpoint_id_and_lambda_names(exp):
    m, root = _models(exp), exp['EXPERIMENT_DIR']
    assert E.lmbda_to_str(3.0e-4) == '3.00e-04' and E.lmbda_to_str(0.000005) == '5.00e-06' and E.lmbda_to_str('1e-4') == '1.00e-04'
    assert E.model_dir(exp, m['c4-ws'], 5.0e-5) == os.path.join(root, 'models', 'c4-ws', '5.00e-05')
    assert E.model_dir(exp, m['c4'], 1.0e-4) == os.path.join(root, 'models', 'c3p-a0.75', '1.00e-04')      # checkpoint_id redirects
    assert E.model_log_path(exp, m['c4'], 1.0e-4) == os.path.join(root, 'models', 'c3p-a0.75', '1.00e-04.log')
    assert E.output_dir(exp, 'loot_vox10_1200', m['c4'], 1.0e-4) == os.path.join(root, 'loot_vox10_1200', 'c4', '1.00e-04')   # not redirected


def test_resolution_from_a_literal_key_or_a_pcerror_cfg(exp):
    loot, soldier = exp['data']
    assert E.cloud_resolution(exp, loot) == 1024
    assert E.cloud_resolution(exp, soldier) == 1024            # the cfg holds the peak value 1023
    with pytest.raises(AssertionError, match='resolution'):
        E.cloud_resolution(exp, {'pc_name': 'x', 'cfg_name': 'x'})          # the reference's cfg tree is not there


def test_unknown_mode_ids_raise_and_labels_resolve(exp):
    modes = exp['eval_modes'][0]['modes']
    assert [E.mode_label(exp, m['id'], m) for m in modes] == ['c6', 'c5', 'G-PCC trisoup']
    assert E.mode_label(exp, 'c1', {'id': 'c1'}) == 'c1'
    with pytest.raises(RuntimeError, match='Unknown mode c7'):
        E.mode_label(exp, 'c7', {'id': 'c7'})


def test_jobs_only_for_trained_checkpoints_grouped_by_checkpoint(exp, tmp_path, caplog):
    m = _models(exp)
    trained = [(m['c4-ws'], 3.0e-4), (m['c3p-a0.75'], 1.0e-4), (m['c3p-a0.75'], 3.0e-4)]
    for mc, l in trained:
        os.makedirs(E.model_dir(exp, mc, l))
        open(os.path.join(E.model_dir(exp, mc, l), 'done'), 'w').close()
    os.makedirs(E.model_dir(exp, m['c1'], 2.0e-4))               # a directory without `done`: skipped
    with caplog.at_level('WARNING'):
        jobs = ev_run_experiment.build_jobs(exp)
    assert 'not finished' in caplog.text
    root = exp['EXPERIMENT_DIR']
    rel = lambda p: os.path.relpath(p, root)
    # c4 reads c3p-a0.75's checkpoints; all jobs of one checkpoint are adjacent, checkpoints in order of first use
    assert [(rel(j['model_dir']), rel(j['output_dir'])) for j in jobs] == [
        ('models/c4-ws/3.00e-04', 'loot_vox10_1200/c4-ws/3.00e-04'), ('models/c4-ws/3.00e-04', 'soldier_vox10_0690/c4-ws/3.00e-04'),
        ('models/c3p-a0.75/3.00e-04', 'loot_vox10_1200/c4/3.00e-04'), ('models/c3p-a0.75/3.00e-04', 'loot_vox10_1200/c3p-a0.75/3.00e-04'),
        ('models/c3p-a0.75/3.00e-04', 'soldier_vox10_0690/c4/3.00e-04'), ('models/c3p-a0.75/3.00e-04', 'soldier_vox10_0690/c3p-a0.75/3.00e-04'),
        ('models/c3p-a0.75/1.00e-04', 'loot_vox10_1200/c4/1.00e-04'), ('models/c3p-a0.75/1.00e-04', 'loot_vox10_1200/c3p-a0.75/1.00e-04'),
        ('models/c3p-a0.75/1.00e-04', 'soldier_vox10_0690/c4/1.00e-04'), ('models/c3p-a0.75/1.00e-04', 'soldier_vox10_0690/c3p-a0.75/1.00e-04')]
    j = jobs[2]
    assert j['opt_metrics'] == ['d1_mse'] and j['fixed_threshold'] is False and j['max_deltas'] == [1., math.inf]
    assert j['model_config'] == 'c3p' and j['pc_name'] == 'loot_vox10_1200' and j['resolution'] == 1024 and j['octree_level'] == 4
    assert j['input_pc'] == str(tmp_path / 'dataset' / 'People' / 'loot_vox10_1200.ply')
    assert j['input_norm'] == str(tmp_path / 'dataset' / 'People' / 'loot_vox10_1200_n.ply')
    assert jobs[1]['octree_level'] == 3 and jobs[1]['resolution'] == 1024
    assert jobs[3]['fixed_threshold'] is True and jobs[3]['opt_metrics'] == ['d1_mse', 'd2_mse']
    import inspect
    assert set(j) <= set(inspect.signature(ev_experiment.run_experiment).parameters)


def test_more_than_one_rank_is_refused(monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(AssertionError, match='one process'):
        ev_experiment.Resident()


def test_run_experiment_checks_its_arguments_before_touching_the_gpu(tmp_path):
    common = dict(output_dir=str(tmp_path / 'o'), model_dir=str(tmp_path), model_config='c3p', pc_name='x', input_pc=str(tmp_path / 'x.ply'))
    with pytest.raises(AssertionError, match='consistency'):
        ev_experiment.run_experiment(**common, resolution=64, consistency='ignore')
    with pytest.raises(AssertionError, match='resolution'):
        ev_experiment.run_experiment(**common)
    with pytest.raises(AssertionError):                          # a d2 metric without normals
        ev_experiment.run_experiment(**common, resolution=64, opt_metrics=['d1_mse', 'd2_mse'])


# ---- tr_train_all
class Recorder:
    """Stands in for the child process: records the call and leaves `done` behind, as a finished tr_train does."""

    def __init__(self):
        self.calls = []

    def __call__(self, argv, log_path, timeout):
        self.calls.append((list(argv), log_path, timeout))
        assert os.path.isdir(argv[1])                            # the checkpoint directory exists before the child starts
        open(os.path.join(argv[1], 'done'), 'w').close()


def _expected_argv(exp, model_id, lmbda_str, alpha, gamma, batch, config, ckpt_id=None, warm=None, extra=()):
    d = os.path.join(exp['EXPERIMENT_DIR'], 'models', ckpt_id or model_id)
    argv = [exp['TRAIN_DATASET_PATH'], os.path.join(d, lmbda_str), '--resolution', '64', '--lmbda', lmbda_str, '--alpha', str(alpha),
            '--gamma', str(gamma), '--batch_size', str(batch), '--model_config', config]
    if warm:
        argv += ['--warm_start', os.path.join(d, warm)]
    return argv + list(extra)


def test_train_all_builds_the_reference_arguments_and_the_warm_start_chain(exp):
    rec = Recorder()
    started = tr_train_all.train_all(exp, runner=rec)
    want = [_expected_argv(exp, 'c4-ws', '3.00e-04', 0.75, 2.0, 32, 'c3p'),
            _expected_argv(exp, 'c4-ws', '1.00e-04', 0.75, 2.0, 32, 'c3p', warm='3.00e-04'),
            _expected_argv(exp, 'c4-ws', '5.00e-05', 0.75, 2.0, 32, 'c3p', warm='1.00e-04'),
            _expected_argv(exp, 'c4', '3.00e-04', 0.75, 2.0, 32, 'c3p', ckpt_id='c3p-a0.75'),       # independent: no warm start
            _expected_argv(exp, 'c4', '1.00e-04', 0.75, 2.0, 32, 'c3p', ckpt_id='c3p-a0.75'),
            # c3p-a0.75's own two lambdas are the directories c4 has just trained: done, not started again
            _expected_argv(exp, 'c1', '2.00e-04', 0.9, 1.5, 16, 'c1'),
            _expected_argv(exp, 'c1', '5.00e-06', 0.9, 1.5, 16, 'c1')]
    assert [c[0] for c in rec.calls] == want
    assert [c[1] for c in rec.calls] == [a[1] + '.log' for a in want] and all(c[2] is None for c in rec.calls)
    assert [j['model_id'] for j in started] == ['c4-ws'] * 3 + ['c4'] * 2 + ['c1'] * 2
    assert os.path.exists(os.path.join(exp['EXPERIMENT_DIR'], 'tr_train_all.log'))
    # every argument is one tr_train knows
    from pcc_geo_cnn_v2_amd import tr_train
    for argv in want:
        tr_train.build_parser().parse_args(argv)


def test_train_all_skips_what_is_done_and_passes_overrides(exp):
    m = _models(exp)
    for l in (3.0e-4, 5.0e-5):
        os.makedirs(E.model_dir(exp, m['c4-ws'], l))
        open(os.path.join(E.model_dir(exp, m['c4-ws'], l), 'done'), 'w').close()
    rec = Recorder()
    tr_train_all.train_all(exp, overrides={'max_steps': 3, 'validation_interval': 2, 'validation_steps': None}, timeout=60, runner=rec)
    extra = ['--max_steps', '3', '--validation_interval', '2']
    assert rec.calls[0][0] == _expected_argv(exp, 'c4-ws', '1.00e-04', 0.75, 2.0, 32, 'c3p', warm='3.00e-04', extra=extra)
    assert rec.calls[0][2] == 60 and len(rec.calls) == 1 + 2 + 2
    again = Recorder()
    assert tr_train_all.train_all(exp, runner=again) == [] and again.calls == []


def test_train_all_fails_when_a_child_leaves_no_done_file(exp):
    with pytest.raises(AssertionError, match='done'):
        tr_train_all.train_all(exp, runner=lambda argv, log, timeout: None)
    exp['train_mode'] = 'sequential'
    with pytest.raises(AssertionError, match='train_mode'):
        tr_train_all.training_plan(exp)
