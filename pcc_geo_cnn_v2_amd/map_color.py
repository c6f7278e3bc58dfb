"""Colour a decoded cloud from its original -- the colour step of the reference's evaluation (its src/map_color.py, run by
ev_experiment.py between decompression and pc_error).

    python -m pcc_geo_cnn_v2_amd.map_color ori_file target_file output_file [--rank {1,2}]

Every point of target_file takes the colour of its rank-th nearest point of ori_file, points ordered by (squared distance, row)
(ops.map_colors, include/pcc_geo.h "cloud colours"; GPU).  The default rank 2 is the reference's output: it takes the second of a
k = 2 KD-tree query.  The output is binary PLY with the target's x, y, z columns (their types kept) and uchar red, green, blue;
an empty target gives a header-only file.  Both clouds are voxelised: integer coordinates in [0, 2^21).
"""
import argparse
import logging

import pandas as pd

from .utils import pc_io

logger = logging.getLogger(__name__)


def map_color(ori_file, target_file, output_file, rank=2, ctx=None):
    """Writes output_file (see the module docstring) and returns its (n,3) uint8 colours."""
    from . import ops
    ori = pc_io.read_ply(ori_file)
    colors = pc_io.load_colors(ori_file)
    target = pc_io.read_ply(target_file)[['x', 'y', 'z']]
    if ctx is None and len(target):
        ctx = ops.get_context()
    mapped = ops.map_colors(ctx, pc_io.df_to_pc(ori), colors, target.values, rank=rank)
    out = pd.concat([target.reset_index(drop=True),
                     pd.DataFrame({c: mapped[:, k] for k, c in enumerate(pc_io.COLOR_COLUMNS)})], axis=1)
    pc_io.write_ply(output_file, out)
    logger.info(f'{output_file}: {len(out)} points coloured from {ori_file} (rank {rank})')
    return mapped


def main():
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='map_color.py', description='Map colors from one PC to another.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ori_file', help='Original point cloud (with red green blue).')
    p.add_argument('target_file', help='Point cloud to colour (e.g. a decoded cloud).')
    p.add_argument('output_file', help='Output PLY: the target points with the mapped colours.')
    p.add_argument('--rank', type=int, choices=(1, 2), default=2,
                   help='Take the colour of the rank-th nearest original point (2: the reference map_color.py; new)')
    args = p.parse_args()
    map_color(args.ori_file, args.target_file, args.output_file, args.rank)


if __name__ == '__main__':
    main()
