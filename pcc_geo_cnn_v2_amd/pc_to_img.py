"""Render a point cloud to a PNG image -- the reference's utils/pc_to_img.py without Open3D or a window (include/pcc_geo.h "point
rendering": every point a square of point_size pixels, z-buffered; GPU by default, numpy with --device host, the same bytes).

    python -m pcc_geo_cnn_v2_amd.pc_to_img input.ply out.png camera.json [--point_size 1.0] [--device gpu|host]
        [--background R G B] [--no_trim] [--bbox_out F.json] [--bbox_in F.json] [--shade {auto,none}] [--estimate_normals]

Colour comes from the file's red green blue if present; otherwise it is shaded from the file's nx ny nz (or, with
--estimate_normals, from normals estimated on the GPU) unless --shade none, and otherwise it is flat grey.  The image is trimmed to
the box of non-background pixels, as the reference does (an empty image is an error); --bbox_out writes that box as JSON, --bbox_in
crops to a box written before (how decoded renders are cropped like their original's).
"""
import argparse
import json
import logging
import sys

import numpy as np

from .utils import pc_io, render

logger = logging.getLogger(__name__)


def point_size_px(point_size):
    """The reference's float --point_size as the integer side of a point's square."""
    return max(1, int(np.floor(float(point_size) + 0.5)))


def cloud_colors(df, camera, shade='auto', normals=None):
    """(n,3) uint8 colours of a cloud (None: flat grey): its red green blue, else shading of `normals` or of its nx ny nz."""
    if all(c in df.columns for c in pc_io.COLOR_COLUMNS):
        c = df[list(pc_io.COLOR_COLUMNS)].values
        if c.dtype.kind not in 'iu':
            if not np.isfinite(c).all() or not np.array_equal(c, np.round(c)):
                raise ValueError('colours must be integers in 0..255')
            c = c.astype(np.int64)
        return c
    if shade == 'none':
        return None
    if normals is None and all(c in df.columns for c in ('nx', 'ny', 'nz')):
        normals = df[['nx', 'ny', 'nz']].values
    return None if normals is None else render.shade_colors(normals, camera)


def render_cloud(points, camera, colors=None, point_size=1, background=(255, 255, 255), device='gpu', ctx=None):
    if device == 'host':
        return render.render_host(points, camera, colors, point_size, background)
    from . import ops
    if ctx is None:
        ctx = ops.get_context()
    return ops.render_points(ctx, points, camera, colors, point_size, background)


def pc_to_img(input_path, output_path, camera_path, point_size=1.0, device='gpu', background=(255, 255, 255), trim=True,
              bbox_out=None, bbox_in=None, shade='auto', estimate_normals=False, ctx=None):
    """Writes output_path and returns (image as written, trim box or None)."""
    df = pc_io.read_ply(input_path)
    camera = render.read_camera(camera_path)
    pts = pc_io.df_to_pc(df)
    normals = None
    if estimate_normals and shade != 'none' and not all(c in df.columns for c in pc_io.COLOR_COLUMNS) and len(pts):
        from . import ops
        ctx = ctx or ops.get_context()
        normals = ops.estimate_normals(ctx, pts)
    colors = cloud_colors(df, camera, shade, normals)
    img = render_cloud(pts, camera, colors, point_size_px(point_size), background, device, ctx)
    box = None
    if bbox_in is not None:
        with open(bbox_in) as f:
            box = tuple(int(v) for v in json.load(f))
    elif trim:
        box = render.trim_bbox(img, background)
    if bbox_out is not None:
        with open(bbox_out, 'w') as f:
            json.dump(list(box if box is not None else render.trim_bbox(img, background)), f)
    if box is not None:
        img = render.crop(img, box)
    render.write_png(output_path, img)
    logger.info(f'{output_path}: {len(pts)} points, {img.shape[1]}x{img.shape[0]} pixels ({device})')
    return img, box


def main():
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='pc_to_img.py', description='Converts a point cloud to an image.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('input_path', help='Input point cloud path (ply).')
    p.add_argument('output_path', help='Output image path.')
    p.add_argument('camera_params_path', help='Camera params path.')
    p.add_argument('--point_size', help='Point size.', default=1.0, type=float)
    p.add_argument('--device', choices=('gpu', 'host'), default='gpu', help='Render on the GPU or in numpy (same bytes; new)')
    p.add_argument('--background', type=int, nargs=3, default=(255, 255, 255), help='Background RGB (new)')
    p.add_argument('--no_trim', action='store_true', help='Keep the whole image instead of trimming it to its content (new)')
    p.add_argument('--bbox_out', help='Write the trim box (left, upper, right, lower) as JSON (new)')
    p.add_argument('--bbox_in', help='Crop to a box written by --bbox_out instead of trimming (new)')
    p.add_argument('--shade', choices=('auto', 'none'), default='auto', help='Shade an uncoloured cloud from its normals (new)')
    p.add_argument('--estimate_normals', action='store_true', help='Shade from normals estimated on the GPU (new)')
    a = p.parse_args()
    try:
        pc_to_img(a.input_path, a.output_path, a.camera_params_path, a.point_size, a.device, tuple(a.background), not a.no_trim,
                  a.bbox_out, a.bbox_in, a.shade, a.estimate_normals)
    except (RuntimeError, ValueError) as e:
        logger.error(str(e))
        sys.exit(1)


if __name__ == '__main__':
    main()
