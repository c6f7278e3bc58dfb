"""Convert a folder of meshes to voxelised point clouds -- the reference's src/ds_mesh_to_pc.py, the first step of its dataset
recipe (ds_mesh_to_pc -> ds_pc_octree_blocks -> ds_select_largest).

    python -m pcc_geo_cnn_v2_amd.ds_mesh_to_pc source dest [--vg_size 64] [--n_samples 500000] [--source_extension .off]
                                                [--target_extension .ply] [--seed 0] [--device gpu|host]

Every `source/**/*{source_extension}` mesh (utils/mesh_io.read_mesh: .off or .ply) becomes `dest/<same relative path with
target_extension>`: binary PLY with float x, y, z, the voxels of ops.mesh_to_points (include/pcc_geo.h "mesh sampling").  dest must
not exist.  Unlike the reference (unseeded), the output is reproducible: the file's seed is the first 8 bytes (little endian) of
blake2b(f'{seed}:{relpath}', digest_size=8) with relpath = os.path.relpath(file, source), so it does not depend on the order or
the number of files.  --device host runs the numpy path (utils/mesh_sampling), which writes the same bytes.
"""
import argparse
import hashlib
import logging
import os
from glob import glob

import pandas as pd

from .utils import mesh_io, mesh_sampling, pc_io

logger = logging.getLogger(__name__)


def file_seed(seed, relpath):
    return int.from_bytes(hashlib.blake2b(f'{seed}:{relpath}'.encode('utf-8'), digest_size=8).digest(), 'little')


def convert(ori_path, target_path, vg_size, n_samples, seed, ctx=None):
    """One mesh -> one PLY; returns the number of points written.  ctx None: the host path."""
    v, f = mesh_io.read_mesh(ori_path)
    if ctx is None:
        pts = mesh_sampling.mesh_to_points(v, f, n_samples, vg_size, seed)
    else:
        from . import ops
        pts = ops.mesh_to_points(ctx, v, f, n_samples, vg_size, seed)
    pc_io.write_ply(target_path, pd.DataFrame({c: pts[:, i] for i, c in enumerate('xyz')}))
    return len(pts)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='ds_mesh_to_pc.py', description='Converts a folder containing meshes to point clouds',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('source', help='Source directory')
    p.add_argument('dest', help='Destination directory')
    p.add_argument('--vg_size', type=int, help='Voxel Grid resolution for x, y, z dimensions', default=64)
    p.add_argument('--n_samples', type=int, help='Number of samples', default=500000)
    p.add_argument('--source_extension', help='Mesh files extension', default='.off')
    p.add_argument('--target_extension', help='Point cloud extension', default='.ply')
    p.add_argument('--seed', type=int, default=0, help='Base seed; each file derives its own from it and its relative path (new)')
    p.add_argument('--device', choices=('gpu', 'host'), default='gpu', help='Where to sample (new); both write the same bytes')
    args = p.parse_args(argv)

    assert os.path.exists(args.source), f'{args.source} does not exist'
    assert not os.path.exists(args.dest), f'{args.dest} already exists'
    assert args.vg_size > 0, 'vg_size must be positive'
    assert args.n_samples > 0, 'n_samples must be positive'

    paths = sorted(glob(os.path.join(args.source, '**', f'*{args.source_extension}'), recursive=True))
    files = [os.path.relpath(x, args.source) for x in paths]
    assert len(files) > 0
    logger.info(f'Found {len(files)} models in {args.source}')
    ctx = None
    if args.device == 'gpu':
        from . import ops
        ctx = ops.get_context()
    for rel in files:
        target, _ = os.path.splitext(os.path.join(args.dest, rel))
        target += args.target_extension
        os.makedirs(os.path.dirname(target) or '.', exist_ok=True)
        m = convert(os.path.join(args.source, rel), target, args.vg_size, args.n_samples, file_seed(args.seed, rel), ctx)
        logger.debug(f'{rel}: {m} points')
    logger.info(f'{len(files)} models written to {args.dest}')


if __name__ == '__main__':
    main()
