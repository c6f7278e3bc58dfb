"""CPU: point rendering (include/pcc_geo.h "point rendering") -- utils/render.render_host against the brute-force restatement in
tests/_render_ref.py, the default camera and Open3D's camera JSON, the colour tables against matplotlib, the trim box against PIL,
the PNG writer, the argument checks of ops.render_points (before any GPU call) and the pc_to_img / pc_to_camera_params CLIs."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import _render_ref as R
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.utils import pc_io, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(seed, n=300, W=40, H=30):
    """A random cloud seen by a random default camera, with points behind the eye, far off-screen and at one depth on one pixel."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3)) * 20
    front = rng.standard_normal(3)
    cam = render.default_camera(pts, W, H, front=front, up=(0, 1, 0), zoom=rng.uniform(0.3, 1.2), fov=rng.uniform(30, 90))
    eye = -cam.extrinsic[:3, :3].T @ cam.extrinsic[:3, 3]
    k = n // 10
    pts[:k] = eye + (eye - pts[:k]) * rng.uniform(0.1, 2, (k, 1))                       # behind the camera
    pts[k:2 * k] += rng.standard_normal((k, 3)) * 1e4                                  # mostly far off-screen
    pts[2 * k:3 * k] = pts[2 * k]                                                      # one depth, one pixel: the lowest row wins
    pts[3 * k] = eye                                                                   # zc = 0
    colors = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return pts, colors, cam


@pytest.mark.parametrize('s', [1, 2, 3, 5])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_render_host_matches_the_brute_force(seed, s):
    pts, colors, cam = _scene(seed, W=32 + 8 * seed, H=24 + 8 * seed)
    img, rows = render.render_host(pts, cam, colors, s, (10, 20, 30), return_rows=True)
    ref_img, ref_rows = R.render_ref(pts, cam.extrinsic, cam.intrinsic, cam.width, cam.height, s, colors, (10, 20, 30))
    assert np.array_equal(rows, ref_rows)
    assert np.array_equal(img, ref_img)
    assert (rows >= 0).sum() > 10                                                      # the scene is not empty
    tie = rows[rows >= 0]
    assert not np.isin(np.arange(61, 90), tie).any()                                   # the tie block: only its lowest row can win


@pytest.mark.parametrize('s', [1, 2, 3, 5])
def test_points_on_pixel_boundaries(s):
    """u = x exactly (E = I, K = I, z = 1): integers and half-integers are the boundaries of s even and odd."""
    W, H = 12, 9
    g = np.arange(-6, 26) / 2.0
    x, y = np.meshgrid(g, g[:24], indexing='ij')
    pts = np.stack([x.ravel(), y.ravel(), np.ones(x.size)], 1)
    cam = render.Camera(np.eye(4), np.eye(3), W, H)
    rng = np.random.default_rng(s)
    pts[:, 2] = rng.choice([1.0, 2.0], len(pts))
    pts[:, :2] *= pts[:, 2:]                                                           # u, v stay on the grid
    colors = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    img, rows = render.render_host(pts, cam, colors, s, return_rows=True)
    ref_img, ref_rows = R.render_ref(pts, np.eye(4), np.eye(3), W, H, s, colors)
    assert np.array_equal(rows, ref_rows) and np.array_equal(img, ref_img)
    one = render.render_host(np.array([[2.5, 3.0, 1.0]]), cam, return_rows=True)[1]  # s = 1: floor(u + 0.5)
    assert np.argwhere(one >= 0).tolist() == [[3, 3]]


def test_no_colours_is_grey_and_empty_cloud_is_background():
    cam = render.Camera(np.eye(4), np.eye(3), 5, 4)
    img = render.render_host(np.array([[1.0, 1.0, 1.0]]), cam)
    assert img[1, 1].tolist() == [128] * 3 and (img.reshape(-1, 3)[[0, 2, 3]] == 255).all()
    img, rows = render.render_host(np.zeros((0, 3)), cam, background=(1, 2, 3), return_rows=True)
    assert (img == [1, 2, 3]).all() and (rows == -1).all()
    ints = render.render_host(np.array([[1, 1, 1]], np.int16), cam)                   # integer input converts
    assert np.array_equal(ints, render.render_host(np.array([[1.0, 1.0, 1.0]], np.float32), cam))


def test_default_camera_centre_and_framing():
    rng = np.random.default_rng(3)
    pts = rng.random((1000, 3)) * [100, 60, 30] + 7
    W, H = 64, 48
    cam = render.default_camera(pts, W, H)
    lookat = (pts.min(0) + pts.max(0)) / 2
    rows = render.render_host(lookat[None], cam, return_rows=True)[1]
    assert np.argwhere(rows == 0).tolist() == [[H // 2, W // 2]]
    # the plane of the box through lookat, seen along the default axis, lies inside the image at zoom 0.7
    mn, mx = pts.min(0), pts.max(0)
    corners = np.array([[x, y, lookat[2]] for x in (mn[0], mx[0]) for y in (mn[1], mx[1])])
    u, v, zc, kept = render.project(corners, cam)
    assert kept.all() and (u > -0.5).all() and (u < W - 0.5).all() and (v > -0.5).all() and (v < H - 0.5).all()
    # the whole box is in front of the camera and inside the image once the zoom leaves room for its near face
    box = np.array([[x, y, z] for x in (mn[0], mx[0]) for y in (mn[1], mx[1]) for z in (mn[2], mx[2])])
    for front in ((0, 0, 1), (1, 1, 1), (-1, 0.5, 0.2)):
        cam = render.default_camera(pts, W, H, front=front, zoom=1.2)
        u, v, zc, kept = render.project(box, cam)
        assert kept.all() and (u > -0.5).all() and (u < W - 0.5).all() and (v > -0.5).all() and (v < H - 0.5).all(), front
    with pytest.raises(ValueError, match='parallel'):
        render.default_camera(pts, front=(0, 2, 0), up=(0, 1, 0))


def test_camera_json_round_trip_and_column_major(tmp_path):
    cam = render.default_camera(np.random.default_rng(0).random((50, 3)), 640, 480, front=(1, 1, 1))
    p = str(tmp_path / 'cam.json')
    render.write_camera(p, cam)
    back = render.read_camera(p)
    assert np.array_equal(back.extrinsic, cam.extrinsic) and np.array_equal(back.intrinsic, cam.intrinsic)
    assert (back.width, back.height) == (640, 480)
    d = json.load(open(p))
    assert d['class_name'] == 'PinholeCameraParameters' and d['version_major'] == 1 and d['version_minor'] == 0
    hand = {'class_name': 'PinholeCameraParameters', 'version_major': 1, 'version_minor': 0,
            'extrinsic': [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 5, -6, 7, 1],
            'intrinsic': {'width': 8, 'height': 6, 'intrinsic_matrix': [100, 0, 0, 0, 90, 0, 3.5, 2.5, 1]}}
    json.dump(hand, open(p, 'w'))
    c = render.read_camera(p)
    assert c.extrinsic[:3, 3].tolist() == [5, -6, 7] and c.extrinsic[3].tolist() == [0, 0, 0, 1]
    assert c.intrinsic.tolist() == [[100, 0, 3.5], [0, 90, 2.5], [0, 0, 1]]


def test_inferno_and_error_colours_equal_matplotlib():
    mpl = pytest.importorskip('matplotlib')
    from matplotlib.colors import Normalize
    cmap = mpl.colormaps['inferno']
    assert np.array_equal(render.INFERNO_U8, cmap(np.arange(256), bytes=True)[:, :3])
    rng = np.random.default_rng(0)
    sq = np.concatenate([rng.integers(0, 400, 5000), [0, 1, 99, 100, 101, 10 ** 6]]).astype(np.int64)
    for pmax in (100.0, 37.25, 1.0, 399.0, 1e-3):
        assert np.array_equal(render.error_colors(sq, pmax), cmap(Normalize(0, pmax)(sq.astype(np.float64)), bytes=True)[:, :3]), pmax
    assert np.array_equal(render.error_colors(sq, 0.0), cmap(np.zeros(len(sq)), bytes=True)[:, :3])


def test_shade_colours():
    cam = render.Camera(np.eye(4), np.eye(3), 4, 4)                                    # viewing axis w = (0, 0, 1)
    n = np.array([[0, 0, 1], [0, 0, -3], [1, 0, 0], [0, 0, 0], [0, 1, 1]], np.float32)
    got = render.shade_colors(n, cam, base=200)
    c = np.array([1, 1, 0, 0, 1 / np.sqrt(2)])
    assert np.array_equal(got[:, 0], np.minimum(np.floor(200 * (0.3 + 0.7 * c) + 0.5), 255).astype(np.uint8))
    assert (got == got[:, :1]).all()


def test_trim_bbox_equals_pil():
    Image = pytest.importorskip('PIL.Image')
    ImageChops = pytest.importorskip('PIL.ImageChops')
    rng = np.random.default_rng(1)
    for t in range(30):
        H, W = rng.integers(1, 40, 2)
        img = np.full((H, W, 3), 255, np.uint8)
        k = rng.integers(1, 6)
        img[rng.integers(0, H, k), rng.integers(0, W, k), rng.integers(0, 3, k)] = rng.integers(0, 255, k)
        im = Image.fromarray(img)
        ref = ImageChops.difference(im, Image.new(im.mode, im.size, (255, 255, 255))).getbbox()
        assert render.trim_bbox(img) == ref
        assert np.array_equal(render.crop(img, ref), np.asarray(im.crop(ref)))
    with pytest.raises(RuntimeError, match='Empty image'):
        render.trim_bbox(np.full((4, 4, 3), 255, np.uint8))


def test_png_round_trips_through_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(2)
    for H, W in ((1, 1), (7, 13), (64, 3)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        p = str(tmp_path / f'{H}x{W}.png')
        render.write_png(p, img)
        back = Image.open(p)
        assert back.mode == 'RGB' and np.array_equal(np.asarray(back), img)
        assert render.png_bytes(img) == open(p, 'rb').read()


def _bad_calls():
    cam = render.Camera(np.eye(4), np.eye(3), 8, 8)
    pts = np.ones((4, 3))

    def with_cam(E=None, K=None, W=8, H=8):
        return render.Camera(np.eye(4) if E is None else E, np.eye(3) if K is None else K, W, H)
    E_bad = np.eye(4)
    E_bad[3, 0] = 1
    E_nan = np.eye(4)
    E_nan[0, 3] = np.nan
    K_bad = np.eye(3)
    K_bad[1, 0] = 0.5
    K_bad2 = np.eye(3)
    K_bad2[2, 2] = 2
    return [
        (dict(points=pts, camera=with_cam(W=0)), 'image size'),
        (dict(points=pts, camera=with_cam(H=16385)), 'image size'),
        (dict(points=pts, camera=with_cam(E=E_bad)), 'bottom row'),
        (dict(points=pts, camera=with_cam(E=E_nan)), 'finite'),
        (dict(points=pts, camera=with_cam(K=K_bad)), 'intrinsic rows'),
        (dict(points=pts, camera=with_cam(K=K_bad2)), 'intrinsic rows'),
        (dict(points=pts, camera=cam, point_size=0), 'point_size'),
        (dict(points=pts, camera=cam, point_size=65), 'point_size'),
        (dict(points=pts, camera=cam, point_size=1.5), 'point_size'),
        (dict(points=np.ones((4, 2)), camera=cam), 'points must be'),
        (dict(points=pts.astype(complex), camera=cam), 'dtype'),
        (dict(points=pts, camera=cam, colors=np.ones((3, 3), np.uint8)), 'colours must be'),
        (dict(points=pts, camera=cam, colors=np.full((4, 3), 256)), 'colours must be'),
        (dict(points=pts, camera=cam, colors=np.ones((4, 3))), 'colours must be'),
        (dict(points=pts, camera=cam, background=(0, 0, 256)), 'background'),
        (dict(points=pts, camera=cam, background=(0, 0)), 'background'),
    ]


@pytest.mark.parametrize('case', range(len(_bad_calls())))
def test_input_checks_come_before_any_gpu_call(case):
    kw, msg = _bad_calls()[case]
    with pytest.raises(ValueError, match=msg):
        ops.render_points(None, **kw)                     # no context: the check must fire before anything touches the GPU
    with pytest.raises(ValueError, match=msg):
        render.render_host(**kw)


def test_symbols_are_exported():
    from pcc_geo_cnn_v2_amd import _lib as L
    lib = L.lib()
    assert lib.pcc_render_workspace_bytes(1024, 1024) == 8 << 20
    assert lib.pcc_render_workspace_bytes(0, 4) == 0 and lib.pcc_render_workspace_bytes(4, 16385) == 0


def _cli(*args):
    return subprocess.run([sys.executable, '-m'] + list(args), cwd=ROOT, capture_output=True, text=True)


def test_cli_host_end_to_end(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(4)
    pts = np.unique(rng.integers(0, 64, (3000, 3)), axis=0)
    df = pd.DataFrame({'x': pts[:, 0].astype(np.float32), 'y': pts[:, 1].astype(np.float32), 'z': pts[:, 2].astype(np.float32),
                       'red': rng.integers(0, 256, len(pts)).astype(np.uint8), 'green': np.uint8(7) + np.zeros(len(pts), np.uint8),
                       'blue': np.zeros(len(pts), np.uint8)})
    ply, cam, png = str(tmp_path / 'a.ply'), str(tmp_path / 'cam.json'), str(tmp_path / 'a.png')
    pc_io.write_ply(ply, df)
    r = _cli('pcc_geo_cnn_v2_amd.pc_to_camera_params', ply, cam, '--width', '200', '--height', '150', '--front', '1', '1', '1')
    assert r.returncode == 0, r.stderr
    c = render.read_camera(cam)
    assert (c.width, c.height) == (200, 150)
    bbox = str(tmp_path / 'box.json')
    r = _cli('pcc_geo_cnn_v2_amd.pc_to_img', ply, png, cam, '--device', 'host', '--point_size', '2.4', '--bbox_out', bbox)
    assert r.returncode == 0, r.stderr
    full = render.render_host(pc_io.df_to_pc(df), c, df[['red', 'green', 'blue']].values, 2)
    box = render.trim_bbox(full)
    assert json.load(open(bbox)) == list(box)
    got = np.asarray(Image.open(png))
    assert np.array_equal(got, render.crop(full, box)) and got.shape[:2] != (150, 200)
    # shading from normals when the file has no colours; --no_trim keeps the whole image
    dfn = df[['x', 'y', 'z']].assign(nx=np.float32(0), ny=np.float32(0), nz=np.float32(1))
    pc_io.write_ply(ply, dfn)
    r = _cli('pcc_geo_cnn_v2_amd.pc_to_img', ply, png, cam, '--device', 'host', '--no_trim')
    assert r.returncode == 0, r.stderr
    shade = render.shade_colors(dfn[['nx', 'ny', 'nz']].values, c)
    assert np.array_equal(np.asarray(Image.open(png)), render.render_host(pc_io.df_to_pc(dfn), c, shade))
    # an empty image is an error exit
    far = dict(json.load(open(cam)))
    far['extrinsic'] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -1e6, 1]
    json.dump(far, open(cam, 'w'))
    r = _cli('pcc_geo_cnn_v2_amd.pc_to_img', ply, png, cam, '--device', 'host')
    assert r.returncode != 0 and 'Empty image' in r.stderr
