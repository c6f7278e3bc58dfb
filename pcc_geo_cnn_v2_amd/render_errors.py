"""Error maps of decoded clouds -- the "visual comparisons" of the reference's ut_run_render.py without its experiment layout:
every decoded point coloured by its squared D1 residual to the original (compute_d1_res_ba) on an inferno scale capped at a
percentile of all residuals, rendered from the original's camera and cropped to the original's trim box.

    python -m pcc_geo_cnn_v2_amd.render_errors original.ply dec1.ply [dec2.ply ...] --camera camera.json --out_dir D
        [--percentile 99] [--point_size 1.0] [--device gpu|host]

Writes, for every decoded cloud, D/<stem>.res.ply (its points with the error colours as red green blue) and D/<stem>.res.png, and
D/errors.json: min (0.0, as the reference sets it), p<percentile> (np.percentile of all residuals, linear), max, the 33 edges of
np.histogram([0, max], bins=32) and the 32 counts of every cloud.  gpu (ops.error_map, ops.render_points) and host (cKDTree, numpy)
write the same bytes.
"""
import argparse
import json
import logging
import os

import numpy as np
import pandas as pd

from . import pc_to_img as P
from .utils import pc_io, render

logger = logging.getLogger(__name__)


def residuals_host(a, b):
    """Squared distance of every row of b to its nearest point of a (exact integers, int64)."""
    from scipy.spatial import cKDTree
    if len(b) == 0:
        return np.zeros(0, np.int64)
    _, idx = cKDTree(a.astype(np.float64)).query(b.astype(np.float64))
    d = a[idx].astype(np.int64) - b.astype(np.int64)
    return (d * d).sum(1)


def _stem(path):
    name = os.path.basename(path)
    return name[:-4] if name.lower().endswith('.ply') else name


def render_errors(original, decoded, camera_path, out_dir, percentile=99.0, point_size=1.0, device='gpu', ctx=None):
    """Writes the files of the module docstring; returns the errors.json dictionary."""
    from . import ops
    if device == 'gpu' and ctx is None:
        ctx = ops.get_context()
    camera = render.read_camera(camera_path)
    s = P.point_size_px(point_size)
    df_a = pc_io.read_ply(original)
    a = ops._voxel_points(pc_io.df_to_pc(df_a), 'render_errors')
    img_a = P.render_cloud(a, camera, P.cloud_colors(df_a, camera), s, device=device, ctx=ctx)
    box = render.trim_bbox(img_a)
    index_a = ops.CloudIndex(ctx, a) if device == 'gpu' else None
    clouds, res = [], []
    for path in decoded:
        b = pc_io.read_ply(path)[['x', 'y', 'z']]
        bp = ops._voxel_points(b.values, 'render_errors') if len(b) else np.zeros((0, 3), np.int32)
        r = ops.error_map(ctx, index_a, bp) if device == 'gpu' else residuals_host(a, bp)
        clouds.append((path, b, bp))
        res.append(r.astype(np.float64))
    allr = np.concatenate(res)
    if len(allr) == 0:
        raise ValueError('render_errors: the decoded clouds have no points')
    pmax, gmax = float(np.percentile(allr, percentile)), float(allr.max())
    edges = np.histogram([0.0, gmax], bins=32)[1]
    os.makedirs(out_dir, exist_ok=True)
    report = {'min': 0.0, f'p{percentile:g}': pmax, 'max': gmax, 'percentile': percentile, 'edges': edges.tolist(), 'clouds': {}}
    for (path, b, bp), r in zip(clouds, res):
        stem = _stem(path)
        col = render.error_colors(r, pmax)
        out = pd.concat([b.reset_index(drop=True), pd.DataFrame({c: col[:, k] for k, c in enumerate(pc_io.COLOR_COLUMNS)})], axis=1)
        pc_io.write_ply(os.path.join(out_dir, stem + '.res.ply'), out)
        img = P.render_cloud(bp, camera, col, s, device=device, ctx=ctx)
        render.write_png(os.path.join(out_dir, stem + '.res.png'), render.crop(img, box))
        report['clouds'][stem] = {'file': path, 'n': int(len(r)), 'counts': np.histogram(r, bins=edges)[0].tolist()}
        logger.info(f'{stem}: {len(r)} points, max residual {r.max() if len(r) else 0:g}')
    with open(os.path.join(out_dir, 'errors.json'), 'w') as f:
        json.dump(report, f, indent=1)
    return report


def main():
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='render_errors.py', description='Renders per-point D1 error maps of decoded point clouds.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('original', help='Original point cloud (ply).')
    p.add_argument('decoded', nargs='+', help='Decoded point clouds (ply).')
    p.add_argument('--camera', required=True, help='Camera params path (pc_to_camera_params).')
    p.add_argument('--out_dir', required=True, help='Output directory.')
    p.add_argument('--percentile', type=float, default=99.0, help='Top of the colour scale, as a percentile of all residuals.')
    p.add_argument('--point_size', type=float, default=1.0, help='Point size.')
    p.add_argument('--device', choices=('gpu', 'host'), default='gpu', help='Residuals and renders on the GPU or on the host.')
    a = p.parse_args()
    render_errors(a.original, a.decoded, a.camera, a.out_dir, a.percentile, a.point_size, a.device)


if __name__ == '__main__':
    main()
