"""RD curves and BD tables of every (cloud, eval mode, optimisation group) of an experiment YAML, and the merged tables -- the
role of the reference's src/ev_run_compare.py.

  python -m pcc_geo_cnn_v2_amd.ev_run_compare experiment.yml [--path_filter REGEXP]

The YAML and the directory layout: utils/experiment.py.  For every cloud of data[], eval mode and group g in (d1, d2),
ev_compare.run draws the eval mode's modes into EXPERIMENT_DIR/<pc_name>/results/<eval_id>/ with the prefix <g>_opt_:
a model id contributes EXPERIMENT_DIR/<pc_name>/<id>/**/report_<g>.json, a G-PCC mode id (mpeg_modes)
EXPERIMENT_DIR/gpcc/<mode id>/<pc_name>/**/report.json.  The reference computes the G-PCC reports itself (mp_run / mp_report
drive the TMC13 binary; not part of this project): here the tree is used when present -- ev_anchors writes one from a table
of published points -- and a G-PCC mode without one is omitted with a warning, as a model without a folder or reports is.  A mode
id that is neither a model nor an mpeg mode raises RuntimeError.

Merged over all conditions into EXPERIMENT_DIR/results/: data.csv, bdrate.csv, bdsnr.csv = the rows of the per-condition
<g>_opt_rd_curve_<g>_{data,bdrate,bdsnr}.csv plus the columns pc_name, eval_id, opt_group and csv_file, columns in alphabetical
order (the reference's concat(sort=True)); the reference's leftover row-number column `Unnamed: 0` is not carried.  One legend
figure per eval mode goes to results/<eval_id>/legend.png / .pdf.  --num_parallel and --no_stream_redirection are accepted and
ignored: the comparisons run in this process.
"""
import argparse
import glob
import logging
import os
import sys

import pandas as pd

from . import ev_compare
from .utils import experiment as E

logger = logging.getLogger(__name__)

DATA_TYPES = ('data', 'bdrate', 'bdsnr')


def mode_sources(exp, pc_name, eval_mode, group):
    """-> (path, pattern, mode id, label) of every mode of the eval set that has reports for this cloud and group."""
    mpeg_modes, model_configs = E.index_by_id(exp.get('mpeg_modes')), E.index_by_id(exp['model_configs'])
    root, out = exp['EXPERIMENT_DIR'], []
    for mode in eval_mode['modes']:
        mode_id = mode['id']
        label = E.mode_label(exp, mode_id, mode)         # raises for an unknown id
        if mode_id in mpeg_modes:
            folder, pattern = os.path.join(root, 'gpcc', mode_id, pc_name), '**/report.json'
        else:
            folder, pattern = os.path.join(root, pc_name, mode_id), f'**/report_{group}.json'
        if not os.path.exists(folder):
            logger.warning(f'Folder {folder} was not found: omitting {mode_id}')
        elif not glob.glob(os.path.join(folder, pattern), recursive=True):
            logger.warning(f'No reports found in {os.path.join(folder, pattern)}')
        else:
            out.append((folder, pattern, mode_id, label))
    return out


def run(exp, path_filter=None):
    root = exp['EXPERIMENT_DIR']
    eval_modes = exp.get('eval_modes') or []
    for eval_mode in eval_modes:                          # unknown ids raise before anything is drawn
        for mode in eval_mode['modes']:
            E.mode_label(exp, mode['id'], mode)
    opt_metrics = exp.get('opt_metrics', ['d1_mse', 'd2_mse'])
    logger.info('Rendering legends')
    import matplotlib
    matplotlib.use('Agg')
    for eval_mode in eval_modes:
        labels = [E.mode_label(exp, m['id'], m) for m in eval_mode['modes']]
        folder = os.path.join(root, 'results', eval_mode['id'])
        os.makedirs(folder, exist_ok=True)
        with matplotlib.rc_context({**ev_compare.RC_DEFAULTS, **(eval_mode.get('rcParams') or {})}):
            ev_compare.render_legend(labels, os.path.join(folder, 'legend'))

    logger.info('Starting comparisons')
    conditions = []
    for entry in exp['data']:
        pc_name = entry['pc_name']
        for eval_mode in eval_modes:
            lims = eval_mode.get('lims') or [None] * len(E.OPT_GROUPS)
            for group, group_lims in zip(E.OPT_GROUPS, lims):
                if not any(m.startswith(group) for m in opt_metrics):
                    continue
                sources = mode_sources(exp, pc_name, eval_mode, group)
                if not sources:
                    logger.warning(f"Omitting eval condition {eval_mode['id']} {group} for {pc_name}")
                    continue
                out_dir = os.path.join(root, pc_name, 'results', eval_mode['id'])
                paths, patterns, ids, labels = zip(*sources)
                ev_compare.run(paths, patterns, labels, ids, out_dir, f'{group}_opt_', path_filter, [group], exp.get('bd_ignore') or (),
                               eval_mode.get('no_legend', False), group_lims, eval_mode.get('rcParams'))
                conditions.append({'pc_name': pc_name, 'eval_id': eval_mode['id'], 'opt_group': group})

    logger.info('Merging data')
    merged_dir = os.path.join(root, 'results')
    os.makedirs(merged_dir, exist_ok=True)
    merged = {}
    for data_type in DATA_TYPES:
        frames = []
        for cond in conditions:
            csv_file = os.path.join(root, cond['pc_name'], 'results', cond['eval_id'],
                                    f"{cond['opt_group']}_opt_rd_curve_{cond['opt_group']}_{data_type}.csv")
            df = pd.read_csv(csv_file, index_col=0, float_precision='round_trip')      # the numbers as written, to the last bit
            for k, v in cond.items():
                df.insert(0, k, v)
            df['csv_file'] = csv_file
            frames.append(df)
        if frames:
            merged[data_type] = pd.concat(frames, ignore_index=True, sort=True)
            merged[data_type].to_csv(os.path.join(merged_dir, data_type + '.csv'))
    logger.info('Finished')
    return merged


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ev_run_compare.py', description='Run eval compare between experiments.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('experiment_path', help='Experiments file path.')
    p.add_argument('--num_parallel', type=int, default=1, help='Accepted and ignored.')
    p.add_argument('--no_stream_redirection', default=False, action='store_true', help='Accepted and ignored.')
    p.add_argument('--path_filter', help='Path based result filtering (see ev_compare).')
    a = p.parse_args(argv)
    run(E.load_experiment(a.experiment_path), a.path_filter)
    return 0


if __name__ == '__main__':
    sys.exit(main())
