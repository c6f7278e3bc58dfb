"""GPU: point rendering (include/pcc_geo.h "point rendering") -- ops.render_points against utils/render.render_host byte for byte
(image and rows) over clouds, cameras, point sizes and image sizes; repeat calls; ops.error_map against cKDTree; the
render_errors and pc_to_camera_params -> pc_to_img CLIs on gpu against host."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

from _normals_ref import shell
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.utils import pc_io, render

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(ctx, pts, cam, colors=None, s=1, bg=(255, 255, 255)):
    img, rows = ops.render_points(ctx, pts, cam, colors, s, bg, return_rows=True)
    ref_img, ref_rows = render.render_host(pts, cam, colors, s, bg, return_rows=True)
    assert img.dtype == np.uint8 and img.shape == (cam.height, cam.width, 3) and rows.dtype == np.int32
    bad = np.argwhere(rows != ref_rows)
    assert len(bad) == 0, (len(bad), bad[:3].tolist(), rows[tuple(bad[0])], ref_rows[tuple(bad[0])])
    assert np.array_equal(img, ref_img)
    return rows


@pytest.mark.parametrize('s', [1, 2, 3, 7])
def test_uniform_cloud_matches_host(ctx, s):
    rng = np.random.default_rng(s)
    pts = rng.random((100000, 3)) * 1000
    colors = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    for front in ((0, 0, 1), (1, 1, 1)):
        rows = _same(ctx, pts, render.default_camera(pts, 512, 512, front=front), colors, s, (3, 4, 5))
        assert (rows >= 0).mean() > 0.05


@pytest.mark.parametrize('s', [1, 3])
def test_shell_at_1024_matches_host(ctx, s):
    pts, _ = shell(1024, radius=0.2, half_width=0.5)                                    # 527k points
    assert len(pts) > 500000
    colors = np.random.default_rng(0).integers(0, 256, (len(pts), 3), dtype=np.uint8)
    for front in ((0, 0, 1), (1, 1, 1)):
        _same(ctx, pts, render.default_camera(pts, 1024, 1024, front=front), colors, s)
    _same(ctx, pts, render.default_camera(pts, 1024, 1024, front=(1, 0.2, 0.1), zoom=0.05), None, s)   # inside the cloud


@pytest.mark.parametrize('s', [1, 2, 3, 7])
def test_tie_heavy_lattice_matches_host(ctx, s):
    g = np.arange(0, 60, dtype=np.float64)
    x, y = np.meshgrid(g, g, indexing='ij')
    layer = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)
    pts = np.concatenate([layer, layer, layer + [0.5, 0, 0], layer + [0, 0, 0.0]])          # whole layers repeated at one depth
    cam = render.Camera(np.array([[1, 0, 0, -30], [0, 1, 0, -30], [0, 0, 1, 40], [0, 0, 0, 1.0]]),
                        np.array([[100, 0, 319.5], [0, 100, 239.5], [0, 0, 1.0]]), 640, 480)
    _same(ctx, pts, cam, None, s)


def test_far_camera_puts_the_cloud_on_a_few_pixels(ctx):
    rng = np.random.default_rng(7)
    pts = rng.random((1000000, 3)) * 100
    cam = render.default_camera(pts, 256, 256, zoom=2000.0)
    rows = _same(ctx, pts, cam, rng.integers(0, 256, (len(pts), 3), dtype=np.uint8))
    assert 1 <= (rows >= 0).sum() < 16


def test_odd_sizes_and_input_types(ctx):
    rng = np.random.default_rng(8)
    pts = (rng.random((20000, 3)) * 100).astype(np.float32)
    cam = render.default_camera(pts, 640, 480, front=(-1, 0.3, 0.5))
    _same(ctx, pts, cam)
    _same(ctx, pts.astype(np.float64), cam)
    _same(ctx, np.round(pts).astype(np.int32), cam, None, 2)
    tiny = render.default_camera(pts, 1, 1)
    _same(ctx, pts, tiny)
    img = ops.render_points(ctx, np.zeros((0, 3)), cam, background=(9, 9, 9))
    assert (img == 9).all()


def test_two_calls_give_the_same_bits(ctx):
    rng = np.random.default_rng(9)
    pts = np.floor(rng.random((300000, 3)) * 64)                                           # many depth ties
    cam = render.default_camera(pts, 300, 200, front=(1, 1, 1))
    a = ops.render_points(ctx, pts, cam, None, 3, return_rows=True)
    b = ops.render_points(ctx, pts, cam, None, 3, return_rows=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_error_map_equals_ckdtree(ctx):
    rng = np.random.default_rng(10)
    a = rng.integers(0, 1024, (200000, 3))
    b = np.concatenate([a[:50000] + rng.integers(-3, 4, (50000, 3)), rng.integers(0, 1024, (10000, 3))])
    b = np.clip(b, 0, None)
    d, idx = cKDTree(a.astype(np.float64)).query(b.astype(np.float64))
    ref = ((a[idx] - b) ** 2).sum(1)
    got = ops.error_map(ctx, a, b)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert np.array_equal(ops.error_map(ctx, ops.CloudIndex(ctx, a), b), ref)


def _cli(*args):
    r = subprocess.run([sys.executable, '-m'] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _write(path, pts, colors=None):
    df = pd.DataFrame({c: pts[:, k].astype(np.float32) for k, c in enumerate('xyz')})
    if colors is not None:
        for k, c in enumerate(pc_io.COLOR_COLUMNS):
            df[c] = colors[:, k]
    pc_io.write_ply(path, df)


def test_render_errors_gpu_equals_host(tmp_path):
    rng = np.random.default_rng(11)
    a, _ = shell(256)
    ori = str(tmp_path / 'ori.ply')
    _write(ori, a, rng.integers(0, 256, (len(a), 3)).astype(np.uint8))
    decs = []
    for k in range(2):
        b = np.unique(np.clip(a[rng.random(len(a)) < 0.6] + rng.integers(-2 - k, 3 + k, (1, 3)), 0, 255), axis=0)
        decs.append(str(tmp_path / f'dec{k}.ply'))
        _write(decs[-1], b)
    cam = str(tmp_path / 'cam.json')
    _cli('pcc_geo_cnn_v2_amd.pc_to_camera_params', ori, cam, '--width', '400', '--height', '300', '--front', '1', '1', '1')
    out = {}
    for dev in ('gpu', 'host'):
        d = str(tmp_path / dev)
        _cli('pcc_geo_cnn_v2_amd.render_errors', ori, *decs, '--camera', cam, '--out_dir', d, '--device', dev)
        out[dev] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    assert sorted(out['gpu']) == ['dec0.res.ply', 'dec0.res.png', 'dec1.res.ply', 'dec1.res.png', 'errors.json']
    assert out['gpu'] == out['host']
    import json
    rep = json.loads(out['gpu']['errors.json'])
    allr = np.concatenate([ops.error_map(ops.get_context(), a, pc_io.load_pc(p).astype(np.int64)) for p in decs]).astype(np.float64)
    assert rep['min'] == 0.0 and rep['p99'] == np.percentile(allr, 99) and rep['max'] == allr.max()
    assert rep['edges'] == np.histogram([0, allr.max()], bins=32)[1].tolist() and len(rep['edges']) == 33
    assert sum(sum(c['counts']) for c in rep['clouds'].values()) == len(allr)


def test_camera_then_image_of_a_map_color_output(tmp_path):
    rng = np.random.default_rng(12)
    a, _ = shell(128)
    ori, dec, col = str(tmp_path / 'a.ply'), str(tmp_path / 'a.dec.ply'), str(tmp_path / 'a.dec.color.ply')
    _write(ori, a, rng.integers(0, 256, (len(a), 3)).astype(np.uint8))
    _write(dec, a[rng.random(len(a)) < 0.5])
    _cli('pcc_geo_cnn_v2_amd.map_color', ori, dec, col)
    cam = str(tmp_path / 'cam.json')
    _cli('pcc_geo_cnn_v2_amd.pc_to_camera_params', col, cam, '--front', '0.3', '1', '0.6', '--width', '512', '--height', '384')
    pngs = {}
    for dev in ('gpu', 'host'):
        p = str(tmp_path / f'{dev}.png')
        _cli('pcc_geo_cnn_v2_amd.pc_to_img', col, p, cam, '--device', dev, '--point_size', '2')
        pngs[dev] = open(p, 'rb').read()
    assert pngs['gpu'] == pngs['host']
    p = str(tmp_path / 'shaded.png')
    _cli('pcc_geo_cnn_v2_amd.pc_to_img', dec, p, cam, '--estimate_normals')                 # uncoloured: shaded from GPU normals
    assert open(p, 'rb').read()[:8] == b'\x89PNG\r\n\x1a\n'
