"""Select the n largest files of a folder -- the reference's src/ds_select_largest.py (host only).

    python -m pcc_geo_cnn_v2_amd.ds_select_largest source dest n

The n largest files under source (recursive; equal sizes in path order) are linked into dest at the same relative paths.  The
links point at absolute paths, so they resolve wherever dest is.
"""
import argparse
import logging
import os
from glob import glob

logger = logging.getLogger(__name__)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ds_select_largest.py', description='Selects the N largest files from a folder',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('source', help='Source directory')
    p.add_argument('dest', help='Destination directory')
    p.add_argument('n', help='Number of largest files to keep.', type=int)
    args = p.parse_args(argv)

    assert os.path.exists(args.source), f'{args.source} does not exist'
    assert args.n > 0
    paths = [x for x in sorted(glob(os.path.join(args.source, '**', '*'), recursive=True)) if os.path.isfile(x)]
    assert len(paths) > 0
    logger.info(f'Found {len(paths)} models in {args.source}')
    largest = sorted(paths, key=lambda x: -os.stat(x).st_size)[:args.n]
    for path in largest:
        target = os.path.join(args.dest, os.path.relpath(path, args.source))
        os.makedirs(os.path.dirname(target) or '.', exist_ok=True)
        os.symlink(os.path.abspath(path), target)
    logger.info(f'{len(largest)} models linked into {args.dest}')


if __name__ == '__main__':
    main()
