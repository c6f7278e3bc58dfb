"""Divide a folder of point clouds into octree blocks -- the reference's src/ds_pc_octree_blocks.py (host only).

    python -m pcc_geo_cnn_v2_amd.ds_pc_octree_blocks source dest [--vg_size 64] [--level 3] [--source_extension .ply]
                                                      [--target_extension .ply]

Every `source/**/*{source_extension}` cloud is cut by utils/octree_coding.partition_octree over [0, vg_size)^3 at `level`; block i
(Morton order, coordinates relative to the block) is written to `dest/<relative path without extension>_{i:03d}{target_extension}`
as binary PLY with the source's columns and dtypes.
"""
import argparse
import logging
import os
from glob import glob

import pandas as pd

from .utils import pc_io
from .utils.octree_coding import partition_octree

logger = logging.getLogger(__name__)


def split_file(ori_path, target_stem, vg_size, level, target_extension):
    """Writes the blocks of one cloud; returns their number."""
    df = pc_io.read_ply(ori_path)
    blocks, _ = partition_octree(df.values, [0, 0, 0], [vg_size] * 3, level)
    for i, block in enumerate(blocks):
        out = pd.DataFrame({c: block[:, j].astype(df[c].dtype) for j, c in enumerate(df.columns)})
        pc_io.write_ply(target_stem + f'_{i:03d}{target_extension}', out)
    return len(blocks)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ds_pc_octree_blocks.py', description='Divides a folder of point clouds into octree blocks',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('source', help='Source directory')
    p.add_argument('dest', help='Destination directory')
    p.add_argument('--vg_size', type=int, help='Voxel Grid resolution for x, y, z dimensions', default=64)
    p.add_argument('--level', type=int, help='Octree decomposition level.', default=3)
    p.add_argument('--source_extension', help='Point cloud files extension', default='.ply')
    p.add_argument('--target_extension', help='Point cloud extension', default='.ply')
    args = p.parse_args(argv)

    assert os.path.exists(args.source), f'{args.source} does not exist'
    assert args.vg_size > 0, 'vg_size must be positive'
    paths = sorted(glob(os.path.join(args.source, '**', f'*{args.source_extension}'), recursive=True))
    files = [os.path.relpath(x, args.source) for x in paths]
    assert len(files) > 0
    logger.info(f'Found {len(files)} models in {args.source}')
    for rel in files:
        stem, _ = os.path.splitext(os.path.join(args.dest, rel))
        split_file(os.path.join(args.source, rel), stem, args.vg_size, args.level, args.target_extension)
    logger.info(f'{len(files)} models written to {args.dest}')


if __name__ == '__main__':
    main()
