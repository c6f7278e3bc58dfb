"""Normals file for a voxelised cloud, estimated on the GPU (new: the reference has no such tool; it relies on the `_n.ply` files
that ship with the MPEG test clouds).

    python -m pcc_geo_cnn_v2_amd.estimate_normals --input_files a.ply --output_files a_n.ply [--k 16] [--viewpoint x y z]

Writes `x y z nx ny nz` (float32) like the MPEG `_n.ply` files, so the result feeds `compress_octree --input_normals` and
`ev_report --input_norm` unchanged.  Definition of the normals: include/pcc_geo.h "point normals" (DESIGN.md).
"""
import argparse
import logging

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)


def normals_frame(points, normals):
    """The `_n.ply` vertex table: the points as loaded (float32) and their normals (float32)."""
    points = np.asarray(points)
    normals = np.asarray(normals, np.float32)
    cols = {c: points[:, i].astype(np.float32) for i, c in enumerate('xyz')}
    cols.update({c: normals[:, i] for i, c in enumerate(('nx', 'ny', 'nz'))})
    return pd.DataFrame(cols)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='estimate_normals.py', description='Estimate point normals of voxelised clouds on the GPU.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--input_files', nargs='+', required=True, help='Input PLY files (integer coordinates in [0, 2^21)).')
    p.add_argument('--output_files', nargs='+', required=True, help='Output normals PLY files, one per input file.')
    p.add_argument('--k', type=int, default=16, help='Neighbours per point, counting the point itself (3..64).')
    p.add_argument('--viewpoint', nargs=3, type=float, default=None,
                   help='Normals point away from this point (default: the centroid of each cloud).')
    args = p.parse_args(argv)
    if len(args.input_files) != len(args.output_files):
        raise AssertionError(f'{len(args.input_files)} input files need as many output files, got {len(args.output_files)}')
    import torch
    from . import ops
    from .utils import pc_io
    ctx = ops.get_context(torch.device('cuda', 0))
    for src, dst in zip(args.input_files, args.output_files):
        points = pc_io.load_pc(src)
        normals = ops.estimate_normals(ctx, points, k=args.k, viewpoint=args.viewpoint)
        pc_io.write_df(dst, normals_frame(points, normals))
        logger.info(f'{src}: {len(points)} normals (k = {args.k}) -> {dst}')


if __name__ == '__main__':
    main()
