"""D1 / D2 experiment report without the external MPEG `pc_error` binary -- SURVEY.md §8f row 4.

Replaces the report step of /root/reference/src/ev_experiment.py:139-162 (which shells out to `pc_error`, parses its log
with utils/mpeg_parsing.py:38-75 and writes `report_{d1,d2}.json`): the same keys -- pos_total_size_in_bytes,
pos_bits_per_input_point, input_point_count, d1_mse, d1_psnr (+ d2_mse, d2_psnr with normals) -- are computed by
utils/pc_metric.compute_metrics, the module the encoder itself uses for its `.enc.metric.json`
(compress_octree.py:117-118), so the reference's encoder/decoder consistency check (`|d1_psnr diff| < 0.01`,
ev_experiment.py:158-162) carries over.

    python -m pcc_geo_cnn_v2_amd.ev_report --input_pc a.ply --decoded_pc a.ply.bin.ply --enc_pc a.ply.bin \\
        --resolution 1024 [--input_norm a_n.ply | --estimate_normals] [--metrics_device host|gpu] [--d2_ties pick|mean] [--hausdorff] [--color] --output report_d1.json

`--metrics_device gpu` computes the metrics with the GPU engine (include/pcc_geo.h "cloud metrics": neighbour ties to the lowest
row); `--hausdorff` adds pc_error's Hausdorff terms (utils/pc_metric.hausdorff_table); `--color` adds pc_error's colour keys
y/u/v_mse and y/u/v_psnr (utils/pc_metric.color_table; both clouds must carry colours: recolour a decoded cloud with map_color).
`--d2_ties mean` evaluates D2 (and its Hausdorff terms) over ALL equidistant nearest points instead of one of them (DESIGN.md
"Tie-averaged D2"): the same numbers on either device up to float64 rounding, whatever the row order of the files; the report then
carries "d2_ties".  `--color --recolor transfer` records that map_color --mode transfer coloured the decoded cloud: the report then
carries "recolor": "transfer" (a label, not checked).  Without them the report is unchanged.
"""
import argparse
import json
import logging
import os

import numpy as np

from .utils import pc_io
from .utils.pc_metric import (check_ties, cloud_tally_host, cloud_tallies_gpu, color_table, color_tally_host, compute_metrics,
                              hausdorff_table, metrics_table)

logger = logging.getLogger(__name__)


def build_report(input_pc, decoded_pc, enc_pc, resolution, input_norm=None, estimate_normals=False, normals_k=16,
                 metrics_device='host', hausdorff=False, color=False, d2_ties='pick', recolor='rank2'):
    check_ties(d2_ties)
    if recolor not in ('rank2', 'transfer'):
        raise AssertionError(f"recolor must be rank2 or transfer, got {recolor!r}")
    if recolor != 'rank2' and not color:
        raise AssertionError('--recolor names the rule that coloured the decoded cloud: it goes with --color')
    if input_norm and estimate_normals:
        raise AssertionError('--estimate_normals and --input_norm are mutually exclusive')
    p1 = pc_io.load_pc(input_pc)
    p2 = pc_io.load_pc(decoded_pc)
    if color:
        c1, c2 = load_report_colors(input_pc, decoded_pc)
    n1 = pc_io.load_normals(input_norm) if input_norm else None
    if estimate_normals:
        from . import ops
        n1 = ops.estimate_normals(ops.get_context(), p1, k=normals_k)
    if n1 is not None:
        assert len(n1) == len(p1), 'normals file must have one normal per input point'
    a, b = np.asarray(p1, np.float64)[:, :3], np.asarray(p2, np.float64)[:, :3]
    if metrics_device == 'gpu':
        from . import ops
        assert len(b), 'compute_metrics: empty decoded cloud'
        ctx = ops.get_context()
        index_a = ops.CloudIndex(ctx, a)
        tally = cloud_tallies_gpu(ctx, a, [b], n1, index_a=index_a, ties=d2_ties)[0]
        m = metrics_table(len(a), tally[:5], resolution - 1, ('d1', 'd2') if n1 is not None else ('d1',))
        color_tally = ops.cloud_color_distortion(ctx, index_a, c1, b, c2) if color else None
    elif metrics_device == 'host':
        if d2_ties == 'pick':
            m = compute_metrics(a, b, resolution - 1, p1_n=n1)
            tally = cloud_tally_host(a, b, n1) if hausdorff else None
        else:
            assert len(b), 'compute_metrics: empty decoded cloud'
            tally = cloud_tally_host(a, b, n1, ties=d2_ties)
            m = metrics_table(len(a), tally[:5], resolution - 1, ('d1', 'd2') if n1 is not None else ('d1',))
        color_tally = color_tally_host(a, c1, b, c2) if color else None
    else:
        raise AssertionError(f'metrics_device must be host or gpu, got {metrics_device!r}')
    size = os.stat(enc_pc).st_size
    data = {'pos_total_size_in_bytes': size, 'pos_bits_per_input_point': size * 8 / len(p1), 'input_point_count': len(p1)}
    data.update({k: float(v) for k, v in m.items() if k in ('d1_mse', 'd1_psnr', 'd2_mse', 'd2_psnr')})
    if hausdorff:
        data.update({k: float(v) for k, v in hausdorff_table(tally, resolution - 1, n1 is not None).items()})
    if color:
        data.update({k: float(v) for k, v in color_table(color_tally, len(a), len(b)).items()})
    if d2_ties != 'pick':      # the default writes exactly the keys it always wrote
        data['d2_ties'] = d2_ties
    if recolor != 'rank2':
        data['recolor'] = recolor
    return data


def load_report_colors(input_pc, decoded_pc):
    """The colours of --color: both clouds must carry them.  A decoded cloud straight from the codec has none; map_color gives it
    the original's."""
    c1 = pc_io.load_colors(input_pc)
    try:
        c2 = pc_io.load_colors(decoded_pc)
    except ValueError as e:
        raise ValueError(f'--color: {e}; recolour the decoded cloud first: python -m pcc_geo_cnn_v2_amd.map_color {input_pc} '
                         f'{decoded_pc} <output.ply>') from None
    return c1, c2


def main():
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ev_report.py', description='D1/D2 report for one decoded point cloud.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--input_pc', required=True, help='Path to input point cloud')
    p.add_argument('--decoded_pc', required=True, help='Path to the decoded point cloud')
    p.add_argument('--enc_pc', required=True, help='Path to the compressed file (its size gives the rate)')
    p.add_argument('--input_norm', default=None, help='Path to input point cloud normals (enables D2)')
    p.add_argument('--estimate_normals', default=False, action='store_true',
                   help='Estimate the input normals on the GPU (enables D2 without --input_norm; new)')
    p.add_argument('--normals_k', type=int, default=16, help='Neighbours per point of --estimate_normals (3..64)')
    p.add_argument('--metrics_device', choices=('host', 'gpu'), default='host',
                   help='Where the metrics run: host = scipy KD-trees, gpu = the HIP engine (ties to the lowest row; new)')
    p.add_argument('--d2_ties', choices=('pick', 'mean'), default='pick',
                   help='Which of several equidistant nearest points the D2 terms read: pick = one of them (the KD-tree\'s choice on the '
                        'host, the lowest row on the gpu), mean = the average over all of them (row-order independent; new)')
    p.add_argument('--hausdorff', default=False, action='store_true',
                   help="Add pc_error's Hausdorff terms: d1_hausdorff[_AB|_BA|_psnr] (+ d2_* with normals; new)")
    p.add_argument('--color', default=False, action='store_true',
                   help="Add pc_error's colour keys y/u/v_mse and y/u/v_psnr (both clouds need red green blue; see map_color; new)")
    p.add_argument('--recolor', choices=('rank2', 'transfer'), default='rank2',
                   help='With --color: the rule that coloured the decoded cloud (map_color --mode); recorded in the report as '
                        '"recolor" when it is transfer, not checked (new)')
    p.add_argument('--resolution', type=int, required=True, help='Voxel grid resolution of the input (peak = resolution - 1)')
    p.add_argument('--output', required=True, help='Report JSON path')
    args = p.parse_args()
    if args.input_norm and args.estimate_normals:
        p.error('--estimate_normals and --input_norm are mutually exclusive')
    if args.recolor != 'rank2' and not args.color:
        p.error('--recolor goes with --color')
    data = build_report(args.input_pc, args.decoded_pc, args.enc_pc, args.resolution, args.input_norm, args.estimate_normals, args.normals_k,
                        args.metrics_device, args.hausdorff, args.color, args.d2_ties, args.recolor)
    with open(args.output, 'w') as f:
        json.dump(data, f, sort_keys=True, indent=4)
    enc_metric = args.enc_pc + '.enc.metric.json'
    if os.path.exists(enc_metric):                       # ev_experiment.py:158-162
        with open(enc_metric) as f:
            enc = json.load(f)
        if 'd1_psnr' in enc:
            diff = abs(enc['d1_psnr'] - data['d1_psnr'])
            logger.info(f'D1 PSNR diff between encoder and decoder: {diff}')
            assert diff < 0.01, f'encoded {args.enc_pc} with D1 {enc["d1_psnr"]} but decoded {args.decoded_pc} with D1 {data["d1_psnr"]}dB'
    logger.info('Done')


if __name__ == '__main__':
    main()
