"""Trains every (model, lambda) of an experiment YAML -- the role of the reference's src/tr_train_all.py.

  python -m pcc_geo_cnn_v2_amd.tr_train_all experiment.yml [--max_steps N] [--validation_interval N] [--validation_steps N]
      [--summary_interval N] [--timeout SECONDS]

The YAML: utils/experiment.py (TRAIN_DATASET_PATH, TRAIN_RESOLUTION, EXPERIMENT_DIR, model_configs, and alpha, gamma, batch_size,
train_mode at the top level or per model).  For every model and every lambda, in the YAML's order, whose checkpoint directory
EXPERIMENT_DIR/models/<checkpoint_id>/<lambda as %.2e>/ has no `done` file, one tr_train run with the reference's arguments:

    tr_train TRAIN_DATASET_PATH <dir> --resolution R --lmbda <lambda> --alpha A --gamma G --batch_size B --model_config CONFIG
             [--warm_start <dir of the previous lambda of this model>]       train_mode warm_seq, from the second lambda on

Its output goes to <dir>.log (the command line first).  Each run is a fresh child process (subprocess; its device memory and
training context end with it) under its own time limit (--timeout; none by default), and must leave `done` behind: a child that
fails or times out ends the sweep with an error.  An interrupted tr_train resumes from its train_state.pt, so rerunning the command
continues a killed sweep, and a finished sweep starts no process at all.  The overrides --max_steps etc. are passed through
to every child (tr_train's defaults otherwise).  tr_train_all.log in EXPERIMENT_DIR records the sweep.
"""
import argparse
import logging
import os
import subprocess
import sys

from .utils import experiment as E

logger = logging.getLogger(__name__)

OVERRIDES = ('max_steps', 'validation_interval', 'validation_steps', 'summary_interval')


def training_plan(exp, overrides=None):
    """-> one dict per (model, lambda) in training order: model_id, lmbda_str, model_dir, log_path, warm_start (a directory or
    None) and argv, the argument list of tr_train."""
    plan = []
    for mc in exp['model_configs']:
        s = E.training_settings(exp, mc)
        lambdas = mc['lambdas']
        for i, lmbda in enumerate(lambdas):
            ckpt = E.model_dir(exp, mc, lmbda)
            warm = E.model_dir(exp, mc, lambdas[i - 1]) if s['train_mode'] == 'warm_seq' and i > 0 else None
            argv = [str(exp['TRAIN_DATASET_PATH']), ckpt, '--resolution', str(exp['TRAIN_RESOLUTION']), '--lmbda', E.lmbda_to_str(lmbda),
                    '--alpha', str(s['alpha']), '--gamma', str(s['gamma']), '--batch_size', str(s['batch_size']),
                    '--model_config', mc['config']]
            if warm is not None:
                argv += ['--warm_start', warm]
            for key in OVERRIDES:
                if overrides and overrides.get(key) is not None:
                    argv += [f'--{key}', str(overrides[key])]
            plan.append(dict(model_id=mc['id'], lmbda_str=E.lmbda_to_str(lmbda), model_dir=ckpt, log_path=E.model_log_path(exp, mc, lmbda),
                             warm_start=warm, train_mode=s['train_mode'], argv=argv))
    return plan


def run_child(argv, log_path, timeout=None):
    """tr_train in a fresh interpreter, stdout and stderr to log_path."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env['PYTHONPATH'] = root + (os.pathsep + env['PYTHONPATH'] if env.get('PYTHONPATH') else '')
    cmd = [sys.executable, '-m', 'pcc_geo_cnn_v2_amd.tr_train'] + list(argv)
    with open(log_path, 'w') as f:
        f.write(' '.join(cmd) + '\n')
        f.flush()
        subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, check=True, env=env, timeout=timeout)


def train_all(exp, overrides=None, timeout=None, runner=run_child):
    """Runs the plan; `runner(argv, log_path, timeout)` trains one model.  Returns the plan entries that were started."""
    os.makedirs(exp['EXPERIMENT_DIR'], exist_ok=True)
    handler = logging.FileHandler(os.path.join(exp['EXPERIMENT_DIR'], 'tr_train_all.log'))
    handler.setFormatter(logging.Formatter('%(asctime)s %(levelname)s %(message)s'))
    logger.addHandler(handler)
    started = []
    try:
        plan = training_plan(exp, overrides)
        logger.info('Starting training')
        for n, job in enumerate(plan):
            done = os.path.join(job['model_dir'], 'done')
            if os.path.exists(done):
                logger.info(f"{n + 1}/{len(plan)} {job['model_id']} lambda {job['lmbda_str']}: done, skipped")
                continue
            logger.info(f"{n + 1}/{len(plan)} training {job['model_id']} lambda {job['lmbda_str']} with train_mode {job['train_mode']}"
                        + (f", warm start from {job['warm_start']}" if job['warm_start'] else ''))
            os.makedirs(job['model_dir'], exist_ok=True)
            started.append(job)
            runner(job['argv'], job['log_path'], timeout)
            assert os.path.exists(done), f"{job['model_dir']}: training ended without `done` (see {job['log_path']})"
        logger.info('Done')
    finally:
        logger.removeHandler(handler)
        handler.close()
    return started


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='tr_train_all.py', description='Train all models for an experimental setup.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('experiment_path', help='Experiments file path.')
    for key in OVERRIDES:
        p.add_argument(f'--{key}', type=int, default=None, help=f"tr_train's --{key} for every model (default: tr_train's own).")
    p.add_argument('--timeout', type=float, default=None, help='Time limit of each training process in seconds.')
    a = p.parse_args(argv)
    exp = E.load_experiment(a.experiment_path)
    for key in ('TRAIN_DATASET_PATH', 'TRAIN_RESOLUTION'):
        assert key in exp, f'{a.experiment_path}: {key} is missing'
    train_all(exp, {k: getattr(a, k) for k in OVERRIDES}, a.timeout)
    return 0


if __name__ == '__main__':
    sys.exit(main())
