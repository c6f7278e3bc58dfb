#!/usr/bin/env python
"""Wall clock of one experiment sweep: ev_run_experiment (one process, resident context / cloud / index) against the same jobs as
the separate CLI calls the reference's ev_experiment.py makes -- per rate point one compress_octree (--dec_files: merged
coding) and one ev_report in place of pc_error; the cloud has no colours, so no map_color.

The cloud is bench.py's 614 k-point stand-in (1024^3, octree level 4), the model ids one c3p family over six designed rate points
(init_checkpoint.make_cell_codec_weights levels 1..6) with fixed_threshold and d1_mse.  Both ways are run once to warm the box
(page cache, code objects, clocks), then once more into an empty experiment directory for the number; every process runs under its
own time limit.  Both write the same files (the reports are compared).

    python tools/bench_experiment.py [--out profiles/experiment_bench.json] [--work DIR] [--timeout 600]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = [1, 2, 3, 4, 5, 6]
LAMBDAS = [3.0e-4, 2.0e-4, 1.0e-4, 5.0e-5, 2.0e-5, 1.0e-5]
PC = 'standin_vox10'


def _run(argv, timeout):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, '-m'] + argv, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return time.perf_counter() - t0


def _experiment(work, name, cloud):
    import yaml
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_cell_codec_weights
    from pcc_geo_cnn_v2_amd.utils.experiment import lmbda_to_str
    root = os.path.join(work, name)
    for lv, l in zip(LEVELS, LAMBDAS):
        d = os.path.join(root, 'models', 'c3p', lmbda_to_str(l))
        os.makedirs(d)
        np.savez(os.path.join(d, 'model.npz'), **make_cell_codec_weights(lv))
        open(os.path.join(d, 'done'), 'w').close()
    exp = {'EXPERIMENT_DIR': root, 'model_configs': [{'id': 'c3p', 'config': 'c3p', 'lambdas': LAMBDAS}], 'opt_metrics': ['d1_mse'],
           'max_deltas': [float('inf')], 'fixed_threshold': True, 'data': [{'pc_name': PC, 'input_pc': cloud, 'resolution': 1024}]}
    path = os.path.join(work, name + '.yml')
    with open(path, 'w') as f:
        yaml.safe_dump(exp, f)
    return path, exp


def one_process(yml, timeout):
    return _run(['pcc_geo_cnn_v2_amd.ev_run_experiment', yml], timeout)


def process_per_step(exp, cloud, timeout):
    from pcc_geo_cnn_v2_amd.utils import experiment as E
    mc, total = exp['model_configs'][0], 0.
    for l in LAMBDAS:
        out = E.output_dir(exp, PC, mc, l)
        enc = os.path.join(out, f'{PC}_d1.ply.bin')
        total += _run(['pcc_geo_cnn_v2_amd.compress_octree', '--input_files', cloud, '--output_files', enc, '--dec_files', enc + '.ply',
                       '--checkpoint_dir', E.model_dir(exp, mc, l), '--model_config', 'c3p', '--opt_metrics', 'd1_mse', '--max_deltas', 'inf',
                       '--resolution', '1024', '--fixed_threshold'], timeout)
        total += _run(['pcc_geo_cnn_v2_amd.ev_report', '--input_pc', cloud, '--decoded_pc', enc + '.ply', '--enc_pc', enc, '--resolution', '1024',
                       '--output', os.path.join(out, 'report_d1.json')], timeout)
    return total


def _reports(exp):
    from pcc_geo_cnn_v2_amd.utils import experiment as E
    out = []
    for l in LAMBDAS:
        with open(os.path.join(E.output_dir(exp, PC, exp['model_configs'][0], l), 'report_d1.json')) as f:
            r = json.load(f)
        r.pop('enc_dec_d1_psnr_diff', None)
        out.append(r)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'experiment_bench.json'))
    ap.add_argument('--work', default=None, help='scratch directory (default: a temporary one, removed afterwards)')
    ap.add_argument('--timeout', type=float, default=600, help='time limit of each process in seconds')
    a = ap.parse_args(argv)
    import bench
    from pcc_geo_cnn_v2_amd.utils import pc_io
    work = a.work or tempfile.mkdtemp(prefix='pcc_exp_bench_')
    os.makedirs(work, exist_ok=True)
    try:
        cloud = os.path.join(work, PC + '.ply')
        pts = bench.standin_cloud()
        pc_io.write_df(cloud, pc_io.pa_to_df(pts))
        times = {}
        for phase in ('warmup', 'measured'):
            yml, exp_one = _experiment(work, f'one_{phase}', cloud)
            times[f'one_process_{phase}_s'] = one_process(yml, a.timeout)
            _, exp_sep = _experiment(work, f'sep_{phase}', cloud)
            times[f'process_per_step_{phase}_s'] = process_per_step(exp_sep, cloud, a.timeout)
        same = _reports(exp_one) == _reports(exp_sep)
        assert same, 'the two ways wrote different reports'
        result = dict(cloud=PC, points=int(len(pts)), resolution=1024, octree_level=4, rate_points=len(LAMBDAS), fixed_threshold=True,
                      processes_per_step_way=2 * len(LAMBDAS), reports_equal=same, **{k: round(v, 3) for k, v in times.items()},
                      ratio=round(times['process_per_step_measured_s'] / times['one_process_measured_s'], 3),
                      reports=[{k: r[k] for k in ('pos_bits_per_input_point', 'd1_psnr')} for r in _reports(exp_one)])
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=2)
        print(json.dumps(result))
    finally:
        if a.work is None:
            shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
