"""The octree anchor (anchor_octree.py) over every cloud and rate of an experiment YAML: the baseline of ev_run_compare's RD curves and
BD tables for clouds that have no published anchor.

  python -m pcc_geo_cnn_v2_amd.ev_run_anchor experiment.yml

It is NOT G-PCC.  It writes the tree ev_run_compare reads for an id listed under the YAML's mpeg_modes:

  EXPERIMENT_DIR/gpcc/<anchor id>/<pc_name>/<rate>/<pc_name>.ply.bin                        the stream
                                                   <pc_name>.ply.bin.decoded.ply            the decoded cloud
                                                   <pc_name>.ply.bin.decoded.ply.color.ply  with the original's colours (map_color), if it has any
                                                   report.json                              ev_report.build_report's dictionary

so the user lists the id under mpeg_modes with a label of their own and under an eval mode; ev_run_compare does not change.  A label
that contains "G-PCC" is refused.  Every decoded cloud is checked against the encoder's own reconstruction (anchor_octree.reconstruct).

YAML keys, all optional: anchor_id (default 'octree-anchor'); anchor_rates, a mapping rate name -> [num, den]; anchor_device (or
device): gpu (default) or host, where the tree and its contexts are computed; metrics_device, d2_ties, estimate_normals as in
ev_run_experiment, which also resolves resolutions and normals the same way.

The default rates r01 .. r06 = 1/8, 1/4, 1/2, 3/4, 7/8, 15/16 are the scales of the MPEG common test conditions for lossy octree
geometry on 10-bit clouds AS RECALLED by the author of this step: nothing available to this project confirms them.  Give
anchor_rates when the exact conditions matter.

--codec surface (or both) runs the surface anchor (anchor_surface.py; not G-PCC, not trisoup-conformant) the same way
under its own id: YAML keys surface_anchor_id (default 'surface-anchor') and surface_rates, a mapping rate name -> node_log2 (default
r01 .. r04 = 5, 4, 3, 2: four points, because the BD fits need four).  The default, --codec octree, writes what it always wrote.

--color (off by default: without it every file written is what it always was) also codes the colours that map_color put on each
decoded cloud with the colour anchor (anchor_color.py; not G-PCC, not RAHT-conformant).  YAML key color_rates, a
mapping rate name -> qstep in 1 .. 255 (default r01 .. r06 = 48, 32, 24, 16, 8, 4: this project's choice, nobody's test conditions).
A rate directory that has a .color.ply and an entry in color_rates gains

                                                   <pc_name>.ply.bin.color.bin                         the colour stream
                                                   <pc_name>.ply.bin.decoded.ply.coded.color.ply       the decoded cloud with the coded colours
                                                   report_color.json                                   colour bytes and bits per input point, geometry +
                                                                                                       colour bits per input point, ev_report --color's
                                                                                                       y/u/v mse and psnr of the coded-colour cloud

and the decoded colours are checked against anchor_color.reconstruct.  report.json is untouched.  The optional top-level YAML key
recolor (rank2 | transfer, as ev_experiment --recolor) picks the rule that colours the decoded clouds; with transfer, and only then,
report_color.json gains "recolor": "transfer".

A step whose outputs exist is skipped, so the command resumes.  The GPU context, each cloud (points, normals, KD-tree / GPU index)
and its quantisation input stay resident across the rates (ev_experiment.Resident); the reports of all rates of a cloud are measured
in one pass.
"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

from .utils import experiment as E

logger = logging.getLogger(__name__)

DEFAULT_ID = 'octree-anchor'
DEFAULT_RATES = {'r01': (1, 8), 'r02': (1, 4), 'r03': (1, 2), 'r04': (3, 4), 'r05': (7, 8), 'r06': (15, 16)}
SURFACE_DEFAULT_ID = 'surface-anchor'
SURFACE_DEFAULT_RATES = {'r01': 5, 'r02': 4, 'r03': 3, 'r04': 2}
COLOR_DEFAULT_RATES = {'r01': 48, 'r02': 32, 'r03': 24, 'r04': 16, 'r05': 8, 'r06': 4}
CODECS = ('octree', 'surface', 'both')
FORBIDDEN_LABEL = 'G-PCC'


def anchor_settings(exp):
    """-> (anchor id, {rate: (num, den)}, device).  Raises for a bad scale or a label that claims to be G-PCC."""
    from . import anchor_octree as A
    anchor_id = exp.get('anchor_id', DEFAULT_ID)
    rates = exp.get('anchor_rates') or DEFAULT_RATES
    assert isinstance(rates, dict) and rates, 'anchor_rates: a mapping rate name -> [num, den]'
    rates = {str(k): A.check_scale(tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in rates.items()}
    device = exp.get('anchor_device', exp.get('device', 'gpu'))
    A.check_device(device)
    _check_labels(exp, anchor_id, 'octree')
    return anchor_id, rates, device


def _check_labels(exp, anchor_id, what):
    labels = [m.get('label', '') for m in exp.get('mpeg_modes') or () if m.get('id') == anchor_id]
    labels += [m.get('label', '') for ev in exp.get('eval_modes') or () for m in ev.get('modes') or () if m.get('id') == anchor_id]
    for label in labels:
        if FORBIDDEN_LABEL.lower() in str(label).lower():
            raise ValueError(f'label {label!r} of {anchor_id}: the {what} anchor is not G-PCC and must not be labelled so')


def surface_settings(exp):
    """-> (anchor id, {rate: node_log2}, device).  Raises for a bad node_log2 or a label that claims to be G-PCC."""
    from . import anchor_surface as S
    anchor_id = exp.get('surface_anchor_id', SURFACE_DEFAULT_ID)
    rates = exp.get('surface_rates') or SURFACE_DEFAULT_RATES
    assert isinstance(rates, dict) and rates, 'surface_rates: a mapping rate name -> node_log2'
    rates = {str(k): S.check_node_log2(v) for k, v in rates.items()}
    device = exp.get('anchor_device', exp.get('device', 'gpu'))
    S.check_device(device)
    _check_labels(exp, anchor_id, 'surface')
    return anchor_id, rates, device


def color_settings(exp):
    """-> {rate: qstep} of --color.  Raises for a qstep outside 1 .. 255."""
    from . import anchor_color as AC
    rates = exp.get('color_rates') or COLOR_DEFAULT_RATES
    assert isinstance(rates, dict) and rates, 'color_rates: a mapping rate name -> qstep'
    return {str(k): AC.check_qstep(v) for k, v in rates.items()}


class _Octree:
    """One codec of run(): its id, its rates and the three functions of a rate's parameter."""

    def __init__(self, exp):
        from . import anchor_octree as A
        self.codec, (self.anchor_id, self.rates, self.device) = A, anchor_settings(exp)

    def describe(self, scale):
        return f'scale {scale[0]}/{scale[1]}'


class _Surface(_Octree):
    def __init__(self, exp):
        from . import anchor_surface as S
        self.codec, (self.anchor_id, self.rates, self.device) = S, surface_settings(exp)

    def describe(self, node_log2):
        return f'node_log2 {node_log2}'


def rate_dir(exp, anchor_id, pc_name, rate):
    return os.path.join(exp['EXPERIMENT_DIR'], 'gpcc', anchor_id, pc_name, rate)


def run(exp, resident=None, codec='octree', color=False):
    """Returns {'coded': n, 'reports': n}: the steps that ran (0, 0 when everything existed), with color=True also 'colors': n.
    codec: one of CODECS."""
    from .ev_experiment import Resident
    assert codec in CODECS, f'codec must be one of {CODECS}, got {codec!r}'
    assert os.path.isdir(exp['EXPERIMENT_DIR']), f"{exp['EXPERIMENT_DIR']} not found"
    anchors = [cls(exp) for name, cls in (('octree', _Octree), ('surface', _Surface)) if codec in (name, 'both')]     # every label checked first
    assert len({a.anchor_id for a in anchors}) == len(anchors), 'anchor_id and surface_anchor_id must differ'
    res = resident if resident is not None else Resident()
    color_rates = color_settings(exp) if color else None
    done = {'coded': 0, 'reports': 0, **({'colors': 0} if color else {})}
    for anchor in anchors:
        for key, n in _run_one(exp, res, anchor, color_rates).items():
            done[key] += n
    return done


def _code_colors(res, original, device, enc, dec, col, report, qstep, recolor='rank2'):
    """The --color step of one rate directory: the colour stream, the coded-colour cloud and report_color.json (which names the
    recolouring rule when it is not the default)."""
    from . import anchor_color as AC
    from . import ops
    from .utils import pc_io
    from .utils.pc_metric import color_table
    pts, colors = pc_io.load_pc(col), pc_io.load_colors(col)
    # a decoder's clip to the grid can put two points on one voxel: they carry one mapped colour, which is coded once
    upts, first, inverse = np.unique(np.asarray(pts, np.int64), axis=0, return_index=True, return_inverse=True)
    ctx = res.ctx if device == 'gpu' else None
    data = AC.encode(upts, colors[first], qstep, device, ctx)
    coded = AC.decode(data, upts, device, ctx)
    assert np.array_equal(coded, AC.reconstruct(upts, colors[first], qstep)), f'{col}: the decoded colours are not the encoder\'s reconstruction'
    coded = coded[inverse.reshape(-1)]
    tally = ops.cloud_color_distortion(res.ctx, original.index, original.colors, np.asarray(pts, np.float64)[:, :3], coded)
    n, geometry = len(original.points), os.stat(enc).st_size
    out = {'color_qstep': qstep, 'color_total_size_in_bytes': len(data), 'color_bits_per_input_point': len(data) * 8 / n,
           'total_bits_per_input_point': (geometry + len(data)) * 8 / n, 'input_point_count': n}
    out.update({k: float(v) for k, v in color_table(tally, n, len(pts)).items()})
    if recolor != 'rank2':
        out['recolor'] = recolor
    pc_io.write_df(dec + '.coded.color.ply', pc_io.pa_to_df(np.concatenate([np.asarray(pts, np.float64), coded], axis=1)))
    with open(enc + '.color.bin.tmp', 'wb') as f:
        f.write(data)
    os.replace(enc + '.color.bin.tmp', enc + '.color.bin')
    with open(report + '.tmp', 'w') as f:
        json.dump(out, f, sort_keys=True, indent=4)
    os.replace(report + '.tmp', report)


def _run_one(exp, res, anchor, color_rates=None):
    from .ev_experiment import _recolor, measure
    from .utils import pc_io
    A, anchor_id, rates, device = anchor.codec, anchor.anchor_id, anchor.rates, anchor.device
    metrics_device, d2_ties = exp.get('metrics_device', 'host'), exp.get('d2_ties', 'pick')
    recolor = exp.get('recolor', 'rank2')
    done = {'coded': 0, 'reports': 0, **({'colors': 0} if color_rates is not None else {})}
    t0 = time.perf_counter()
    for entry in exp['data']:
        pc_name = entry['pc_name']
        input_norm = None if exp.get('estimate_normals') else E.data_path(exp, entry.get('input_norm'))
        original = res.original(E.data_path(exp, entry['input_pc']), input_norm, bool(exp.get('estimate_normals')))
        resolution = E.cloud_resolution(exp, entry)
        todo = []
        for rate, scale in rates.items():
            out = rate_dir(exp, anchor_id, pc_name, rate)
            enc = os.path.join(out, pc_name + '.ply.bin')
            dec, report = enc + '.decoded.ply', os.path.join(out, 'report.json')
            col = dec + '.color.ply'
            os.makedirs(out, exist_ok=True)
            if os.path.exists(enc) and os.path.exists(dec):
                logger.info(f'[{original.input_pc}] -> [{enc}, {dec}] (exists)')
            else:
                logger.info(f'[{original.input_pc}] -> [{enc}, {dec}] {anchor.describe(scale)}')
                ctx = res.ctx if device == 'gpu' else None
                data = A.encode(original.points, resolution, scale, device, ctx)
                pts = A.decode(data, device, ctx)
                want = A.reconstruct(original.points, resolution, scale)
                assert np.array_equal(pts, want), f'{pc_name} {rate}: the decoded cloud is not the encoder\'s reconstruction'
                with open(enc + '.tmp', 'wb') as f:
                    f.write(data)
                pc_io.write_df(dec, pc_io.pa_to_df(pts))
                os.replace(enc + '.tmp', enc)
                done['coded'] += 1
            if os.path.exists(col):
                logger.info(f'[{dec}] -> [{col}] (exists)')
            elif original.colors is not None:
                logger.info(f'[{dec}] -> [{col}]')
                _recolor(res, original, dec, col, recolor)
            if color_rates is not None and rate in color_rates and os.path.exists(col):
                creport = os.path.join(out, 'report_color.json')
                if os.path.exists(creport):
                    logger.info(f'[{col}] -> [{creport}] (exists)')
                else:
                    logger.info(f'[{col}] -> [{enc}.color.bin, {dec}.coded.color.ply, {creport}] qstep {color_rates[rate]}')
                    _code_colors(res, original, device, enc, dec, col, creport, color_rates[rate], recolor)
                    done['colors'] += 1
            if not os.path.exists(report):
                todo.append((dec, enc, report))
        if todo:
            logger.info(f"[{pc_name}] -> [{', '.join(t[2] for t in todo)}]")
            reports = measure(res, original, [t[0] for t in todo], [t[1] for t in todo], resolution, metrics_device, d2_ties)
            for (_, _, path), data in zip(todo, reports):
                with open(path + '.tmp', 'w') as f:
                    json.dump(data, f, sort_keys=True, indent=4)
                os.replace(path + '.tmp', path)
                done['reports'] += 1
    logger.info(f'Done: {done} in {time.perf_counter() - t0:.2f} s')
    return done


def main(argv=None):
    from . import want_hw_queues
    want_hw_queues()        # before torch (the HIP runtime) loads
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ev_run_anchor.py', description='Code every cloud of an experiment with the octree anchor (a conventional '
                                'baseline; not G-PCC) at every rate and write the report tree ev_run_compare reads.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('experiment_path', help='Experiments file path.')
    p.add_argument('--codec', choices=CODECS, default='octree', help='Which anchor to run: the octree anchor, the surface anchor (a triangle-soup '
                   'class codec; not G-PCC, not trisoup-conformant) or both')
    p.add_argument('--color', default=False, action='store_true', help='Also code the colours map_color put on each decoded cloud with the colour '
                   'anchor (not G-PCC, not RAHT-conformant) and write report_color.json beside report.json')
    a = p.parse_args(argv)
    run(E.load_experiment(a.experiment_path), codec=a.codec, color=a.color)
    return 0


if __name__ == '__main__':
    sys.exit(main())
