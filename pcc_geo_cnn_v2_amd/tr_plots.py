"""Training curves from the event files tr_train --summary_interval writes -- the role of src/ut_tensorboard_plots.py, without its
experiment YAML.

  python -m pcc_geo_cnn_v2_amd.tr_plots CKPT_DIR [CKPT_DIR ...] --out OUT [--tags loss mbpov/total ...] [--split train|val]
      [--yscale log]

For every scalar tag: OUT/<tag>.png and .pdf with one curve per checkpoint directory (labelled by the directory's name), and
OUT/<tag>.csv with the numbers drawn (step, then one column per directory; empty where a directory has no value at a step).
A `/` in a tag becomes `_` in the file name.
"""
import argparse
import csv
import os
import sys

from .utils import tf_summary


def build_parser():
    ap = argparse.ArgumentParser(prog='tr_plots', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('checkpoint_dirs', nargs='+', help='Checkpoint directories of tr_train runs with --summary_interval.')
    ap.add_argument('--out', required=True, help='Output directory.')
    ap.add_argument('--tags', nargs='*', default=None, help='Scalar tags to draw (default: every scalar tag found).')
    ap.add_argument('--split', default='train', choices=('train', 'val'), help='Which event directory to read.')
    ap.add_argument('--yscale', default='linear', choices=('linear', 'log'), help='y axis scale.')
    return ap


def file_stem(tag):
    return tag.replace('/', '_')


def collect(dirs, split, tags=None):
    """{tag: {label: [(step, value)]}}; labels are the directories' names (made unique by their order when two coincide)."""
    labels = []
    for d in dirs:
        name = os.path.basename(os.path.normpath(d))
        labels.append(name if name not in labels else f'{name}#{len(labels)}')
    logdirs = [os.path.join(d, split) for d in dirs]
    for ld in logdirs:
        assert tf_summary.event_files(ld), f'no event files under {ld}'
    if tags is None:
        found = {}
        for ld in logdirs:
            found.update({t: 1 for t, kind in tf_summary.tags(ld).items() if kind == 'scalar'})
        tags = list(found)
    return {t: {lab: tf_summary.scalars(ld, t) for lab, ld in zip(labels, logdirs)} for t in tags}


def write_csv(path, curves):
    steps = sorted({s for c in curves.values() for s, _ in c})
    by = {lab: dict(c) for lab, c in curves.items()}
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['step'] + list(curves))
        for s in steps:
            w.writerow([s] + [repr(by[lab][s]) if s in by[lab] else '' for lab in curves])


def main(argv=None):
    a = build_parser().parse_args(argv)
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    os.makedirs(a.out, exist_ok=True)
    data = collect(a.checkpoint_dirs, a.split, a.tags)
    for tag, curves in data.items():
        assert any(curves.values()), f'no scalar {tag!r} in the {a.split} event files'
        stem = os.path.join(a.out, file_stem(tag))
        write_csv(stem + '.csv', curves)
        fig, ax = plt.subplots(figsize=(6, 4))
        for lab, c in curves.items():
            if c:
                ax.plot([s for s, _ in c], [v for _, v in c], label=lab)
        ax.set_xlabel('step')
        ax.set_ylabel(tag)
        ax.set_yscale(a.yscale)
        ax.grid(True, alpha=.3)
        ax.legend()
        fig.tight_layout()
        fig.savefig(stem + '.png', dpi=120)
        fig.savefig(stem + '.pdf')
        plt.close(fig)
    return 0


if __name__ == '__main__':
    sys.exit(main())
