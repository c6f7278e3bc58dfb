"""Report trees from a table of published RD points, so that they can sit on ev_run_compare's plots and in its BD tables.

  python -m pcc_geo_cnn_v2_amd.ev_anchors experiment.yml points.csv

points.csv has the columns of the merged data.csv that ev_run_compare writes (and the paper's authors published): mode_id,
pc_name, opt_group, metric, x, y (others are ignored).  x is bits per input point, y the PSNR named by `metric` (d1_psnr or
d2_psnr).  Rows of a mode id listed under the YAML's mpeg_modes become EXPERIMENT_DIR/gpcc/<mode id>/<pc_name>/rNN/report.json,
NN counting up with the rate: the k-th rows of the d1 and the d2 group are one stream and share a report (with d1_psnr and
d2_psnr) when the groups list the same rates, otherwise every row is a report of its own.  Rows of a model id become EXPERIMENT_DIR/<pc_name>/<id>/pNN/report_<opt_group>.json.  Rows of any other mode id raise.
Existing files are overwritten.
"""
import argparse
import json
import os
import sys

import pandas as pd

from .utils import experiment as E

ANCHOR_NOTE = ('The G-PCC anchor points that circulate with the paper are its numbers for the four 8i clouds (loot_vox10_1200, '
               'redandblack_vox10_1550, longdress_vox10_1300, soldier_vox10_0690): they mean nothing for any other cloud.')


def write_report_trees(exp, table):
    """table: DataFrame with mode_id, pc_name, opt_group, metric, x, y.  Returns the report paths written."""
    mpeg_modes, model_configs = E.index_by_id(exp.get('mpeg_modes')), E.index_by_id(exp['model_configs'])
    root, written = exp['EXPERIMENT_DIR'], []
    for (mode_id, pc_name), rows in table.groupby(['mode_id', 'pc_name'], sort=False):
        if mode_id in mpeg_modes:
            # one G-PCC stream gives one row per group: the k-th rows (in rate order) of all groups are one report when their
            # rates agree; otherwise every row is a report of its own
            by_group = [g.sort_values('x', kind='stable') for _, g in rows.groupby('opt_group', sort=False)]
            if len({tuple(g['x']) for g in by_group}) == 1:
                reports = [{'pos_bits_per_input_point': float(by_group[0]['x'].iloc[k]),
                            **{g['metric'].iloc[k]: float(g['y'].iloc[k]) for g in by_group}} for k in range(len(by_group[0]))]
            else:
                reports = [{'pos_bits_per_input_point': float(r['x']), r['metric']: float(r['y'])} for g in by_group for _, r in g.iterrows()]
            for n, report in enumerate(reports):
                written.append(os.path.join(root, 'gpcc', mode_id, pc_name, f'r{n + 1:02d}', 'report.json'))
                _dump(written[-1], report)
        elif mode_id in model_configs:
            for group, of_group in rows.groupby('opt_group', sort=False):
                for n, (_, r) in enumerate(of_group.sort_values('x', kind='stable').iterrows()):
                    written.append(os.path.join(root, pc_name, mode_id, f'p{n + 1:02d}', f'report_{group}.json'))
                    _dump(written[-1], {'pos_bits_per_input_point': float(r['x']), r['metric']: float(r['y'])})
        else:
            raise RuntimeError(f'Unknown mode {mode_id}: neither under mpeg_modes nor under model_configs')
    return written


def _dump(path, report):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(report, f, sort_keys=True, indent=4)


def main(argv=None):
    p = argparse.ArgumentParser(prog='ev_anchors', description='Write report.json trees from a CSV of RD points in the column layout '
                                'of data.csv (mode_id, pc_name, opt_group, metric, x, y).  ' + ANCHOR_NOTE)
    p.add_argument('experiment_path', help='Experiments file path (EXPERIMENT_DIR, mpeg_modes, model_configs).')
    p.add_argument('points_csv', help='CSV of RD points.')
    a = p.parse_args(argv)
    written = write_report_trees(E.load_experiment(a.experiment_path), pd.read_csv(a.points_csv, float_precision='round_trip'))
    print(f'{len(written)} reports written')
    return 0


if __name__ == '__main__':
    sys.exit(main())
