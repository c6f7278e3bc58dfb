"""RD curves and Bjøntegaard tables from report JSONs -- the interface of the reference's src/ev_compare.py.

  python -m pcc_geo_cnn_v2_amd.ev_compare --paths DIR [DIR ...] --patterns '**/report_d1.json' [...] --labels L [...] --mode_ids ID [...]
      --output_path OUT [--output_prefix P] [--path_filter REGEXP] [--modes d1 d2] [--bd_ignore SUBSTR ...] [--no_legend]
      [--lims xmin xmax ymin ymax] [--rcParams JSON]

Mode k is the reports matching paths[k]/patterns[k] (recursive glob), drawn as one curve with labels[k] (`_` becomes a space) and
named mode_ids[k] in the tables.  The reports of a mode are ordered by pos_bits_per_input_point.  A report whose PSNR is not
finite (a lossless point: mse 0) is left out of the curve, of the data CSV and of the BD numbers.  A report whose path
contains one of the --bd_ignore strings is drawn but left out of the BD numbers (to compare curves over the same rate points).  A mode without any report
is left out.  For each g of --modes, files in OUT:

  <P>rd_curve_<g>.png / .pdf     <g>_psnr over bits per input point
  <P>rd_curve_<g>_data.csv       one row per drawn point: mode_id, label, metric, ylabel, x, y
  <P>rd_curve_<g>_bdrate.csv     all pairs: one row per mode (metric, mode_id, label), one column per mode id; row i, column j =
  <P>rd_curve_<g>_bdsnr.csv      utils.bd.bdrate / bdsnr (points of mode j, points of mode i), i.e. mode i measured against anchor j
  <P>rd_curve_<g>.log            both tables as text

--path_filter keeps the reports whose PATH the regular expression matches (re.search).  The reference's branch applies the
expression to the report's dictionary and raises TypeError; searching the path is its evident intent.  A BD pair that utils.bd
cannot evaluate (ValueError: a mode with a single point, two points at one rate) is written as NaN with a warning instead of
ending the run.  The reference's LaTeX text rendering is not used: labels go through matplotlib's own mathtext.
"""
import argparse
import glob
import itertools
import json
import logging
import os
import re
import sys

import numpy as np
import pandas as pd

from .utils import bd

logger = logging.getLogger(__name__)

X_COL = 'pos_bits_per_input_point'
CURVES = {'d1': ('d1_psnr', 'D1 PSNR (dB)'), 'd2': ('d2_psnr', 'D2 PSNR (dB)')}
DATA_COLUMNS = ['mode_id', 'label', 'metric', 'ylabel', 'x', 'y']
RC_DEFAULTS = {'axes.labelsize': 20, 'xtick.labelsize': 20, 'ytick.labelsize': 20, 'legend.fontsize': 12, 'font.family': 'serif',
               'figure.figsize': (7.3, 4.2), 'legend.framealpha': 0.65}
LINESTYLES = ('-', '--', '-.')
MARKERS = ('s', '+', 'o', '*', 'x', 'D', 'v', 'h')


def _pyplot():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    return matplotlib, plt


def parse_lims(lims):
    """xmin xmax ymin ymax; None or 'None' leaves a limit to matplotlib."""
    if lims is None:
        return None
    return [None if x is None or x == 'None' else float(x) for x in lims]


def gather(paths, patterns, labels, mode_ids, path_filter=None, bd_ignore=()):
    """-> one dict per non-empty mode: mode_id, label, reports (DataFrame ordered by rate: path, bd_mask + the report's keys)."""
    for path in paths:
        assert os.path.exists(path), f'{path} does not exist'
    assert len(paths) == len(patterns) == len(labels) == len(mode_ids), 'one pattern, label and mode id per path'
    regexp = re.compile(path_filter) if path_filter is not None else None
    modes = []
    for path, pattern, label, mode_id in zip(paths, patterns, labels, mode_ids):
        rows = []
        for report_path in sorted(glob.glob(os.path.join(path, pattern), recursive=True)):
            if regexp is not None and not regexp.search(report_path):
                logger.info(f'Ignoring {report_path}')
                continue
            with open(report_path) as f:
                report = json.load(f)
            clash = {'path', 'bd_mask'} & set(report)
            assert not clash, f'{report_path}: key conflict {clash}'
            bd_mask = not any(s in report_path for s in bd_ignore or ())
            if not bd_mask:
                logger.info(f'Ignoring {report_path} for BD computations')
            rows.append({'path': report_path, 'bd_mask': bd_mask, **report})
        if not rows:
            logger.info(f'Ignoring {path} {pattern}')
            continue
        reports = pd.DataFrame(rows).sort_values(by=X_COL, kind='stable').reset_index(drop=True)
        modes.append({'mode_id': mode_id, 'label': label.replace('_', ' '), 'path': path, 'pattern': pattern, 'reports': reports})
    return modes


def curve_points(mode, column, for_bd=False):
    """(n, 2) array of (rate, PSNR) of a mode's finite points in rate order; for_bd drops the --bd_ignore reports too."""
    df = mode['reports']
    if column not in df.columns:
        return np.zeros((0, 2))
    y = pd.to_numeric(df[column], errors='coerce').values.astype(np.float64)
    keep = np.isfinite(y)
    if for_bd:
        keep &= df['bd_mask'].values.astype(bool)
    return np.stack([df[X_COL].values.astype(np.float64)[keep], y[keep]], 1)


def bd_tables(modes, column):
    """{'bdrate': DataFrame, 'bdsnr': DataFrame}: row = mode, one column per mode id (see the module docstring)."""
    points = [curve_points(m, column, for_bd=True) for m in modes]
    out = {}
    for name, fn in (('bdrate', bd.bdrate), ('bdsnr', bd.bdsnr)):
        rows = []
        for i, mi in enumerate(modes):
            row = {'metric': column, 'mode_id': mi['mode_id'], 'label': mi['label']}
            for j, mj in enumerate(modes):
                try:
                    row[mj['mode_id']] = float(fn(points[j], points[i]))
                except ValueError as e:
                    logger.warning(f"{name} {mj['mode_id']} / {mi['mode_id']} ({column}): {e}; written as NaN")
                    row[mj['mode_id']] = float('nan')
            rows.append(row)
        out[name] = pd.DataFrame(rows)
    return out


def build_curves(modes, group, filename, output_path, no_legend=False, lims=None, legend_loc='lower right'):
    column, ylabel = CURVES[group]
    logger.info(f'Building curves with {ylabel}')
    _, plt = _pyplot()
    fig, ax = plt.subplots()
    summary = []
    for mode, marker, linestyle in zip(modes, itertools.cycle(MARKERS), itertools.cycle(LINESTYLES)):
        pts = curve_points(mode, column)
        ax.plot(pts[:, 0], pts[:, 1], label=mode['label'], linestyle=linestyle, marker=marker)
        summary += [{'mode_id': mode['mode_id'], 'label': mode['label'], 'metric': column, 'ylabel': ylabel, 'x': x, 'y': y}
                    for x, y in pts]
    pd.DataFrame(summary, columns=DATA_COLUMNS).to_csv(os.path.join(output_path, filename + '_data.csv'))
    ax.set(xlabel='bits per input point', ylabel=ylabel)
    ax.set_xlim(left=0)
    if lims is not None:
        for lim, setter, key in zip(lims, (ax.set_xlim, ax.set_xlim, ax.set_ylim, ax.set_ylim), ('left', 'right', 'bottom', 'top')):
            if lim is not None:
                setter(**{key: lim})
    if not no_legend:
        ax.legend(loc=legend_loc)
    ax.locator_params(axis='x', nbins=6)
    ax.locator_params(axis='y', nbins=6)
    ax.grid(True)
    fig.tight_layout()
    for ext in ('.pdf', '.png'):
        fig.savefig(os.path.join(output_path, filename + ext))
    plt.close(fig)

    message = ''
    for name, table in bd_tables(modes, column).items():
        text = table.to_string()
        message += text + '\n'
        logger.info(f'{name}\n{text}')
        table.to_csv(os.path.join(output_path, f'{filename}_{name}.csv'))
    with open(os.path.join(output_path, filename + '.log'), 'w') as f:
        f.write(message)


def render_legend(labels, path_stem):
    """A figure that holds only the legend of `labels` (the eval sets drawn with no_legend share it): <path_stem>.pdf / .png."""
    _, plt = _pyplot()
    fig, ax = plt.subplots()
    lines = [ax.plot([0], [0], linestyle=ls, marker=mk)[0] for _, ls, mk in zip(labels, itertools.cycle(LINESTYLES), itertools.cycle(MARKERS))]
    legend_fig = plt.figure(figsize=(sum(0.4 + 0.166 * len(l) for l in labels) + 0.4, 0.4))
    legend_fig.legend(lines, labels, loc='center', frameon=False, ncol=max(len(labels), 1))
    for ext in ('.pdf', '.png'):
        legend_fig.savefig(path_stem + ext)
    plt.close(fig)
    plt.close(legend_fig)


def run(paths, patterns, labels, mode_ids, output_path, output_prefix='', path_filter=None, modes=('d1', 'd2'), bd_ignore=(),
        no_legend=False, lims=None, rc_params=None):
    for m in modes:
        assert m in CURVES, f'--modes: {m!r} is not one of {list(CURVES)}'
    data = gather(paths, patterns, labels, mode_ids, path_filter, bd_ignore)
    os.makedirs(output_path, exist_ok=True)
    matplotlib, _ = _pyplot()
    with matplotlib.rc_context({**RC_DEFAULTS, **(rc_params or {})}):
        for m in modes:
            build_curves(data, m, f'{output_prefix}rd_curve_{m}', output_path, no_legend=no_legend, lims=parse_lims(lims))
    return data


def build_parser():
    p = argparse.ArgumentParser(prog='ev_compare.py', description='Gathers reports and produces summary.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--paths', help='Input paths.', nargs='+', required=True)
    p.add_argument('--patterns', help='Search patterns (ex: **/report.json).', nargs='+', required=True)
    p.add_argument('--labels', help='Labels.', nargs='+', required=True)
    p.add_argument('--mode_ids', help='Identifiers.', nargs='+', required=True)
    p.add_argument('--output_path', help='Output directory path.', required=True)
    p.add_argument('--output_prefix', help='Prefix for output files.', default='')
    p.add_argument('--path_filter', help='Keep the reports whose path this regular expression matches.')
    p.add_argument('--modes', help='Modes to use for output: d1, d2 or both.', default=['d1', 'd2'], nargs='+')
    p.add_argument('--rcParams', help='Dictionary of parameters to pass to rcParams (JSON format).', type=json.loads)
    p.add_argument('--bd_ignore', help='Ignore certain reports (usually to make BD metrics comparables).', nargs='+')
    p.add_argument('--no_legend', help='Remove legend.', default=False, action='store_true')
    p.add_argument('--lims', help='xmin xmax ymin ymax. None for auto.', nargs='+')
    return p


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    a = build_parser().parse_args(argv)
    run(a.paths, a.patterns, a.labels, a.mode_ids, a.output_path, a.output_prefix, a.path_filter, a.modes, a.bd_ignore or (),
        a.no_legend, a.lims, a.rcParams)
    return 0


if __name__ == '__main__':
    sys.exit(main())
