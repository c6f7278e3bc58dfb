"""Colour a decoded cloud from its original -- the colour step of the reference's evaluation (its src/map_color.py, run by
ev_experiment.py between decompression and pc_error).

    python -m pcc_geo_cnn_v2_amd.map_color ori_file target_file output_file [--rank {1,2} | --mode transfer]

--mode rank (the default): every point of target_file takes the colour of its rank-th nearest point of ori_file, points ordered by
(squared distance, row) (ops.map_colors, include/pcc_geo.h "cloud colours"; GPU).  The default rank 2 is the reference's output:
it takes the second of a k = 2 KD-tree query.  --mode transfer (new): every original point votes for its nearest target points
and a target point takes the mean colour of its voters (ops.transfer_colors, DESIGN.md §4.9 "Colour transfer"; a simplified
MPEG-style recolouring, not TMC13-conformant); it has no rank.  The output is binary PLY with the target's x, y, z columns (their
types kept) and uchar red, green, blue; an empty target gives a header-only file.  Both clouds are voxelised: integer coordinates
in [0, 2^21).
"""
import argparse
import logging

import pandas as pd

from .utils import pc_io

logger = logging.getLogger(__name__)

MODES = ('rank', 'transfer')


def map_color(ori_file, target_file, output_file, rank=2, ctx=None, mode='rank'):
    """Writes output_file (see the module docstring) and returns its (n,3) uint8 colours."""
    from . import ops
    if mode not in MODES:
        raise ValueError(f'map_color: mode must be one of {MODES}, got {mode!r}')
    ori = pc_io.read_ply(ori_file)
    colors = pc_io.load_colors(ori_file)
    target = pc_io.read_ply(target_file)[['x', 'y', 'z']]
    if ctx is None and len(target):
        ctx = ops.get_context()
    if mode == 'transfer':
        mapped = ops.transfer_colors(ctx, pc_io.df_to_pc(ori), colors, target.values)
    else:
        mapped = ops.map_colors(ctx, pc_io.df_to_pc(ori), colors, target.values, rank=rank)
    out = pd.concat([target.reset_index(drop=True),
                     pd.DataFrame({c: mapped[:, k] for k, c in enumerate(pc_io.COLOR_COLUMNS)})], axis=1)
    pc_io.write_ply(output_file, out)
    logger.info(f'{output_file}: {len(out)} points coloured from {ori_file} ({"transfer" if mode == "transfer" else f"rank {rank}"})')
    return mapped


def build_parser():
    p = argparse.ArgumentParser(prog='map_color.py', description='Map colors from one PC to another.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ori_file', help='Original point cloud (with red green blue).')
    p.add_argument('target_file', help='Point cloud to colour (e.g. a decoded cloud).')
    p.add_argument('output_file', help='Output PLY: the target points with the mapped colours.')
    p.add_argument('--rank', type=int, choices=(1, 2), default=None,
                   help='--mode rank: take the colour of the rank-th nearest original point (default 2: the reference map_color.py; new)')
    p.add_argument('--mode', choices=MODES, default='rank',
                   help='rank: copy one neighbour\'s colour; transfer: the mean colour of the original points nearest to each target '
                        'point (least squares for the colour metric, not TMC13-conformant; new)')
    return p


def parse_args(argv=None):
    """The parsed arguments with rank filled in; --rank together with --mode transfer is an argument error."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.mode == 'transfer' and args.rank is not None:
        p.error('--rank has no meaning with --mode transfer')
    if args.rank is None:
        args.rank = 2
    return args


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    args = parse_args(argv)
    map_color(args.ori_file, args.target_file, args.output_file, args.rank, mode=args.mode)


if __name__ == '__main__':
    main()
