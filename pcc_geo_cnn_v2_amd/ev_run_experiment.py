"""Every (cloud, model, lambda) experiment of an experiment YAML, in one process on one GPU -- the role of the reference's
src/ev_run_experiment.py.

  python -m pcc_geo_cnn_v2_amd.ev_run_experiment experiment.yml

The YAML and the directory layout: utils/experiment.py.  Each job is ev_experiment.run_experiment, writing to
EXPERIMENT_DIR/<pc_name>/<id>/<lambda>/ from the checkpoint EXPERIMENT_DIR/models/<checkpoint_id>/<lambda>/.  A checkpoint
without its `done` file is skipped with a warning, as in the reference.  The reference starts one process per job and, inside,
one per step; here all jobs share one ev_experiment.Resident: one GPU context, each original cloud (points, normals, octree
partition, KD-tree, GPU index) loaded once, and the jobs ordered by checkpoint so that each checkpoint's weights are uploaded
once, for all the clouds and model ids that use it.  Finished steps are skipped (ev_experiment), so the command resumes.
The optional top-level key `recolor` (rank2 | transfer, ev_experiment --recolor) picks the colour step of every job.
--num_parallel and --no_stream_redirection are accepted and ignored.  More than one rank (torch.distributed.run) is refused.
"""
import argparse
import logging
import os
import sys
import time

from .utils import experiment as E

logger = logging.getLogger(__name__)

RUN_KEYS = ('estimate_normals', 'metrics_device', 'd2_ties', 'consistency', 'no_merge_coding', 'recolor')


def build_jobs(exp):
    """-> the run_experiment keyword dictionaries of all jobs whose checkpoint is trained, ordered by checkpoint directory (first
    use first), then as the YAML lists clouds and models."""
    jobs = []
    for entry in exp['data']:
        pc_name = entry['pc_name']
        resolution = None
        for mc in exp['model_configs']:
            settings = E.coding_settings(exp, mc)
            for lmbda in mc['lambdas']:
                ckpt = E.model_dir(exp, mc, lmbda)
                if not os.path.exists(os.path.join(ckpt, 'done')):
                    logger.warning(f'Model training is not finished: skipping {ckpt} for {pc_name}')
                    continue
                if resolution is None:
                    resolution = E.cloud_resolution(exp, entry)
                job = dict(output_dir=E.output_dir(exp, pc_name, mc, lmbda), model_dir=ckpt, model_config=mc['config'], pc_name=pc_name,
                           input_pc=E.data_path(exp, entry['input_pc']), input_norm=E.data_path(exp, entry.get('input_norm')),
                           resolution=resolution, octree_level=int(entry.get('octree_level', exp.get('octree_level', 4))),
                           batch_size=int(exp.get('codec_batch_size', 32)), **settings)
                job.update({k: exp[k] for k in RUN_KEYS if k in exp})
                if job.get('estimate_normals'):
                    job['input_norm'] = None
                jobs.append(job)
    order = {}
    for job in jobs:
        order.setdefault(job['model_dir'], len(order))
    return sorted(jobs, key=lambda j: order[j['model_dir']])       # stable: the YAML's order within a checkpoint


def run(exp, resident=None):
    from .ev_experiment import Resident, run_experiment
    assert os.path.isdir(exp['EXPERIMENT_DIR']), f"{exp['EXPERIMENT_DIR']} not found"
    resident = resident if resident is not None else Resident()
    jobs = build_jobs(exp)
    logger.info(f'Starting {len(jobs)} experiments')
    t0 = time.perf_counter()
    for n, job in enumerate(jobs):
        logger.info(f"{n + 1}/{len(jobs)} {job['pc_name']} {job['model_dir']} -> {job['output_dir']}")
        run_experiment(resident=resident, **job)
    logger.info(f'Done: {len(jobs)} experiments in {time.perf_counter() - t0:.2f} s, {resident.stats}')
    return resident


def main(argv=None):
    from . import want_hw_queues
    want_hw_queues()        # before torch (the HIP runtime) loads
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ev_run_experiment.py', description='Run experiments.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('experiment_path', help='Experiments file path.')
    p.add_argument('--num_parallel', type=int, default=1, help='Accepted and ignored: the jobs run in this process.')
    p.add_argument('--no_stream_redirection', default=False, action='store_true', help='Accepted and ignored.')
    a = p.parse_args(argv)
    run(E.load_experiment(a.experiment_path))
    return 0


if __name__ == '__main__':
    sys.exit(main())
