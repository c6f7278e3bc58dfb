"""GPU: the experiment loop end to end -- ev_run_experiment and ev_run_compare from one YAML, the resident runner against the
separate CLI calls, the d2 group with estimated normals, resuming, and tr_train_all.  The cloud is tools/rd_sweep.py's 256^3
synthetic shell at octree level 2 and the checkpoints are designed c3p weights (init_checkpoint.make_cell_codec_weights), as
in tests/test_rd_sweep_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import yaml

from pcc_geo_cnn_v2_amd import ev_report, ev_run_compare, ev_run_experiment
from pcc_geo_cnn_v2_amd.ev_experiment import DIFF_KEY, Resident, run_experiment
from pcc_geo_cnn_v2_amd.init_checkpoint import cell_codec_expected_points, make_cell_codec_weights
from pcc_geo_cnn_v2_amd.utils import bd, pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = [3.0e-4, 1.0e-4, 5.0e-5]            # decreasing lambda = increasing rate, as in the paper's lists
LEVELS = [3, 4, 5]                            # the designed cell codec standing in for each lambda
LSTR = ['3.00e-04', '1.00e-04', '5.00e-05']
PC = 'shell256'
CLI_TIMEOUT = 300


def _cloud():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import rd_sweep
    return rd_sweep.synthetic_cloud(256)


def _checkpoints(root, ckpt_id='fixed'):
    for lv, ls in zip(LEVELS, LSTR):
        d = os.path.join(root, 'models', ckpt_id, ls)
        os.makedirs(d)
        np.savez(os.path.join(d, 'model.npz'), **make_cell_codec_weights(lv))
        open(os.path.join(d, 'done'), 'w').close()


def _experiment(tmp_path, **top):
    root = str(tmp_path / 'exp')
    src = str(tmp_path / 'data' / f'{PC}.ply')
    pts = _cloud()
    pc_io.write_df(src, pc_io.pa_to_df(pts))
    exp = {'EXPERIMENT_DIR': root, 'MPEG_DATASET_DIR': str(tmp_path / 'data'),
           'model_configs': [{'id': 'fixed', 'config': 'c3p', 'lambdas': LAMBDAS, 'label': 'fixed threshold'},
                             {'id': 'adaptive', 'checkpoint_id': 'fixed', 'config': 'c3p', 'lambdas': LAMBDAS, 'fixed_threshold': False,
                              'opt_metrics': ['d1_mse']}],
           'opt_metrics': ['d1_mse'], 'max_deltas': [float('inf')], 'fixed_threshold': True, 'octree_level': 2, 'codec_batch_size': 16,
           'mpeg_modes': [{'id': 'octree-predlift/lossy-geom-lossy-attrs', 'label': 'G-PCC octree'}], 'bd_ignore': [],
           'eval_modes': [{'id': 'main', 'modes': [{'id': 'fixed'}, {'id': 'adaptive', 'label': 'adaptive threshold'},
                                                   {'id': 'octree-predlift/lossy-geom-lossy-attrs'}]}],
           'data': [{'pc_name': PC, 'input_pc': f'{PC}.ply', 'resolution': 256}]}
    exp.update(top)
    _checkpoints(root)
    path = str(tmp_path / 'experiment.yml')
    with open(path, 'w') as f:
        yaml.safe_dump(exp, f)
    return path, exp, src, pts


def _cli(*args):
    r = subprocess.run([sys.executable, '-m'] + [str(a) for a in args], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=CLI_TIMEOUT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _report(path):
    with open(path) as f:
        return json.load(f)


def test_run_experiment_then_run_compare(tmp_path):
    yml, exp, src, pts = _experiment(tmp_path)
    root = exp['EXPERIMENT_DIR']
    resident = ev_run_experiment.run(exp)
    # one context, the cloud loaded once, one encoder model per checkpoint for the two ids that share it
    assert resident.stats == {'clouds_loaded': 1, 'models_built': 3, 'jobs': 6}
    curves = {}
    for mid in ('fixed', 'adaptive'):
        rows = []
        for lv, ls in zip(LEVELS, LSTR):
            d = os.path.join(root, PC, mid, ls)
            assert sorted(os.listdir(d)) == ['report_d1.json', f'{PC}_d1.ply.bin', f'{PC}_d1.ply.bin.enc.metric.json', f'{PC}_d1.ply.bin.ply']
            rep = _report(os.path.join(d, 'report_d1.json'))
            enc, dec = os.path.join(d, f'{PC}_d1.ply.bin'), os.path.join(d, f'{PC}_d1.ply.bin.ply')
            want = ev_report.build_report(src, dec, enc, 256)
            assert {k: v for k, v in rep.items() if k != DIFF_KEY} == want          # the same keys, the same numbers
            assert rep[DIFF_KEY] < 0.01                                             # the reference's encoder / decoder check passed
            assert rep[DIFF_KEY] == abs(_report(enc + '.enc.metric.json')['d1_psnr'] - rep['d1_psnr'])
            if mid == 'fixed':                                                      # designed weights: the decoded set has a closed form
                got = pc_io.load_pc(dec).astype(np.int64)
                assert np.array_equal(got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))], cell_codec_expected_points(pts, lv))
            rows.append((rep['pos_bits_per_input_point'], rep['d1_psnr']))
        bpp, psnr = zip(*rows)
        assert all(x < y for x, y in zip(bpp, bpp[1:])) and all(x < y for x, y in zip(psnr, psnr[1:])), rows
        curves[mid] = np.array(rows)

    merged = ev_run_compare.run(exp)                 # the G-PCC mode has no report tree: omitted with a warning
    per = os.path.join(root, PC, 'results', 'main')
    assert sorted(os.listdir(per)) == ['d1_opt_rd_curve_d1' + s for s in ('.log', '.pdf', '.png', '_bdrate.csv', '_bdsnr.csv', '_data.csv')]
    for name, fn in (('bdrate', bd.bdrate), ('bdsnr', bd.bdsnr)):
        tab = pd.read_csv(os.path.join(per, f'd1_opt_rd_curve_d1_{name}.csv'), index_col=0, float_precision='round_trip')
        assert list(tab.mode_id) == ['fixed', 'adaptive'] and list(tab.label) == ['fixed threshold', 'adaptive threshold']
        m = tab[['fixed', 'adaptive']].values
        assert np.isfinite(m).all() and m[0, 0] == 0. and m[1, 1] == 0.
        assert m[0, 1] == fn(curves['adaptive'], curves['fixed']) and m[1, 0] == fn(curves['fixed'], curves['adaptive'])
        assert np.array_equal(merged[name][['fixed', 'adaptive']].values, m)
    data = pd.read_csv(os.path.join(root, 'results', 'data.csv'), index_col=0, float_precision='round_trip')
    assert len(data) == 6 and set(data.pc_name) == {PC} and set(data.opt_group) == {'d1'} and set(data.eval_id) == {'main'}
    assert np.array_equal(data[data.mode_id == 'adaptive'][['x', 'y']].values, curves['adaptive'])


def test_resident_runner_equals_separate_cli_calls(tmp_path):
    """The adaptive-threshold job of the SECOND checkpoint, run after the jobs of the first one on the same resident state,
    against compress_octree / decompress_octree / ev_report as processes of their own."""
    yml, exp, src, pts = _experiment(tmp_path)
    root = exp['EXPERIMENT_DIR']
    jobs = [j for j in ev_run_experiment.build_jobs(exp) if not j['model_dir'].endswith(LSTR[2])]
    assert [os.path.basename(j['model_dir']) for j in jobs] == [LSTR[0]] * 2 + [LSTR[1]] * 2          # another checkpoint comes first
    resident = Resident()
    for job in jobs:
        run_experiment(resident=resident, **job)
    ours = os.path.join(root, PC, 'adaptive', LSTR[1])
    ckpt = os.path.join(root, 'models', 'fixed', LSTR[1])
    hand = tmp_path / 'hand'
    enc, dec, rep = str(hand / f'{PC}_d1.ply.bin'), str(hand / f'{PC}_d1.ply.bin.ply'), str(hand / 'report_d1.json')
    _cli('pcc_geo_cnn_v2_amd.compress_octree', '--input_files', src, '--output_files', enc, '--checkpoint_dir', ckpt, '--model_config', 'c3p',
         '--opt_metrics', 'd1_mse', '--max_deltas', 'inf', '--resolution', 256, '--octree_level', 2, '--batch_size', 16)
    _cli('pcc_geo_cnn_v2_amd.decompress_octree', '--input_files', enc, '--output_files', dec, '--checkpoint_dir', ckpt, '--model_config', 'c3p',
         '--batch_size', 16)
    _cli('pcc_geo_cnn_v2_amd.ev_report', '--input_pc', src, '--decoded_pc', dec, '--enc_pc', enc, '--resolution', 256, '--output', rep)
    name = f'{PC}_d1.ply.bin'
    assert open(os.path.join(ours, name), 'rb').read() == open(enc, 'rb').read()
    assert _report(os.path.join(ours, name + '.enc.metric.json')) == _report(enc + '.enc.metric.json')
    assert np.array_equal(pc_io.load_pc(os.path.join(ours, name + '.ply')), pc_io.load_pc(dec))
    mine = _report(os.path.join(ours, 'report_d1.json'))
    assert {k: v for k, v in mine.items() if k != DIFF_KEY} == _report(rep)
    # the same job through the ev_experiment CLI, decoder instead of merged coding: the same files again
    alone = tmp_path / 'alone'
    _cli('pcc_geo_cnn_v2_amd.ev_experiment', '--output_dir', alone, '--model_dir', ckpt, '--model_config', 'c3p', '--pc_name', PC, '--input_pc', src,
         '--resolution', 256, '--octree_level', 2, '--opt_metrics', 'd1_mse', '--max_deltas', 'inf', '--no_merge_coding', '--batch_size', 16)
    assert open(alone / name, 'rb').read() == open(enc, 'rb').read()
    assert np.array_equal(pc_io.load_pc(str(alone / (name + '.ply'))), pc_io.load_pc(dec))
    assert _report(alone / 'report_d1.json') == mine


def test_d2_group_with_estimated_normals_colours_and_resume(tmp_path):
    yml, exp, src, pts = _experiment(tmp_path)
    rng = np.random.default_rng(3)
    colored = str(tmp_path / 'data' / 'colored.ply')
    pc_io.write_df(colored, pc_io.pa_to_df(np.hstack([pts, rng.integers(0, 256, (len(pts), 3)).astype(np.float32)])))
    ckpt = os.path.join(exp['EXPERIMENT_DIR'], 'models', 'fixed', LSTR[1])
    out = str(tmp_path / 'out')
    job = dict(output_dir=out, model_dir=ckpt, model_config='c3p', pc_name=PC, input_pc=colored, estimate_normals=True,
               opt_metrics=['d1_mse', 'd2_mse'], max_deltas=[np.inf], fixed_threshold=False, metrics_device='gpu', d2_ties='mean',
               consistency='warn', resolution=256, octree_level=2, batch_size=16)
    resident = Resident()
    reports = run_experiment(resident=resident, **job)
    files = sorted(os.listdir(out))
    stems = [f'{PC}_{g}.ply.bin' for g in ('d1', 'd2')]
    assert files == sorted([s + e for s in stems for e in ('', '.enc.metric.json', '.ply', '.ply.color.ply')] + ['report_d1.json', 'report_d2.json'])
    for g in ('d1', 'd2'):
        rep = _report(os.path.join(out, f'report_{g}.json'))
        assert rep == reports[g] and np.isfinite(rep['d2_psnr']) and np.isfinite(rep['d1_psnr']) and rep['d2_ties'] == 'mean'
        dec = os.path.join(out, f'{PC}_{g}.ply.bin.ply')
        want = ev_report.build_report(colored, dec, os.path.join(out, f'{PC}_{g}.ply.bin'), 256, estimate_normals=True, metrics_device='gpu',
                                      d2_ties='mean')
        assert {k: v for k, v in rep.items() if k != DIFF_KEY} == want
        col = pc_io.read_ply(dec + '.color.ply')
        assert list(col.columns) == ['x', 'y', 'z', 'red', 'green', 'blue'] and np.array_equal(col[['x', 'y', 'z']].values, pc_io.load_pc(dec))
        # recorded, not asserted (the d2 rate point of an adaptive d1_mse d2_mse run)
        print(f"{g}: enc.metric d1_psnr {_report(os.path.join(out, stems[0 if g == 'd1' else 1] + '.enc.metric.json'))['d1_psnr']:.4f} "
              f"report d1_psnr {rep['d1_psnr']:.4f} {DIFF_KEY} {rep[DIFF_KEY]:.6f}")

    # resume: one report and one decoded cloud removed -> only those come back
    removed = [os.path.join(out, 'report_d2.json'), os.path.join(out, stems[0] + '.ply')]
    before = {f: (os.stat(os.path.join(out, f)).st_mtime_ns, open(os.path.join(out, f), 'rb').read()) for f in files}
    for f in removed:
        os.remove(f)
    run_experiment(resident=resident, **job)
    assert sorted(os.listdir(out)) == files
    for f in files:
        mtime, content = before[f]
        assert open(os.path.join(out, f), 'rb').read() == content, f
        if os.path.join(out, f) in removed:
            assert os.stat(os.path.join(out, f)).st_mtime_ns > mtime, f
        else:
            assert os.stat(os.path.join(out, f)).st_mtime_ns == mtime, f


def test_consistency_assert_fails_after_writing_the_report(tmp_path):
    yml, exp, src, pts = _experiment(tmp_path)
    ckpt = os.path.join(exp['EXPERIMENT_DIR'], 'models', 'fixed', LSTR[0])
    out = str(tmp_path / 'out')
    job = dict(output_dir=out, model_dir=ckpt, model_config='c3p', pc_name=PC, input_pc=src, fixed_threshold=True, resolution=256,
               octree_level=2, batch_size=16)
    resident = Resident()
    run_experiment(resident=resident, **job)
    metric = os.path.join(out, f'{PC}_d1.ply.bin.enc.metric.json')
    rec = _report(metric)
    rec['d1_psnr'] += 0.5                          # an encoder that claims half a dB more than the decoded cloud has
    with open(metric, 'w') as f:
        json.dump(rec, f)
    os.remove(os.path.join(out, 'report_d1.json'))
    with pytest.raises(AssertionError, match='but decoded'):
        run_experiment(resident=resident, **job)
    assert abs(_report(os.path.join(out, 'report_d1.json'))[DIFF_KEY] - 0.5) < 1e-9
    os.remove(os.path.join(out, 'report_d1.json'))
    assert abs(run_experiment(resident=resident, consistency='warn', **job)['d1'][DIFF_KEY] - 0.5) < 1e-9


def _write_blocks(root, res, n_train, n_test, seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).astype(np.float64)
    for sub, n in (('train', n_train), ('test', n_test)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for i in range(n):
            shell = np.abs(np.linalg.norm(g - res / 2 - rng.uniform(-2, 2, 3), axis=-1) - rng.uniform(res / 5, res / 2.5)) < .6
            pc_io.write_df(os.path.join(root, sub, f'b{i:03d}.ply'), pc_io.pa_to_df(np.argwhere(shell).astype(np.float32)))


def test_tr_train_all_warm_sequence(tmp_path):
    from pcc_geo_cnn_v2_amd import train
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    data = str(tmp_path / 'blocks')
    _write_blocks(data, 16, 8, 2, 21)
    exp = {'EXPERIMENT_DIR': str(tmp_path / 'exp'), 'TRAIN_DATASET_PATH': os.path.join(data, '**', '*.ply'), 'TRAIN_RESOLUTION': 16,
           'model_configs': [{'id': 'ws', 'config': 'c3p', 'lambdas': [1.0e-2, 5.0e-3], 'train_mode': 'warm_seq'}],
           'alpha': 0.9, 'gamma': 2.0, 'batch_size': 2, 'train_mode': 'independent'}
    yml = str(tmp_path / 'experiment.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(exp, f)
    cmd = ['pcc_geo_cnn_v2_amd.tr_train_all', yml, '--max_steps', 3, '--validation_interval', 3, '--validation_steps', 1, '--timeout', CLI_TIMEOUT]
    _cli(*cmd)
    first, second = [os.path.join(exp['EXPERIMENT_DIR'], 'models', 'ws', s) for s in ('1.00e-02', '5.00e-03')]
    for d in (first, second):
        assert os.path.exists(os.path.join(d, 'done')) and os.path.exists(os.path.join(d, 'model.npz')) and os.path.exists(d + '.log')
    assert '--warm_start' not in open(first + '.log').readline()
    assert f'--warm_start {first}' in open(second + '.log').readline()
    # what the second child saw at step 0: a trainer started the same way holds the first model's saved weights, and its step-0
    # validation loss is the one the child logged
    with np.load(os.path.join(first, 'model.npz')) as f:
        saved = {k: f[k] for k in f.files}
    load = lambda sub: [np.asarray(pc_io.load_pc(os.path.join(data, sub, n)))[:, :3] for n in sorted(os.listdir(os.path.join(data, sub)))]
    t = train.Trainer(ModelConfigType['c3p'].build(seed=42), str(tmp_path / 'probe'), load('train'), load('test'), resolution=16, batch_size=2,
                      lmbda=5.0e-3, alpha=0.9, gamma=2.0, max_steps=3, seed=42, validation_interval=3, validation_steps=1,
                      warm_start=first, log=None)
    step0 = t.graph.export_weights()
    assert set(step0) == set(saved)
    for k in saved:
        assert np.array_equal(step0[k], saved[k]), k
    logged = [json.loads(l) for l in open(os.path.join(second, 'log.jsonl'))]
    assert logged[0]['step'] == 0 and logged[0]['val_loss'] == t.validate()
    assert [r['step'] for r in logged if 'loss' in r] == [1, 2, 3]
    # rerunning does nothing
    stamp = {d: os.stat(os.path.join(d, 'train_state.pt')).st_mtime_ns for d in (first, second)}
    logs = {d: open(d + '.log').read() for d in (first, second)}
    _cli(*cmd)
    assert stamp == {d: os.stat(os.path.join(d, 'train_state.pt')).st_mtime_ns for d in (first, second)}
    assert logs == {d: open(d + '.log').read() for d in (first, second)}
