"""Point rendering on the host -- the numpy statement of include/pcc_geo.h "point rendering" (the `--device host` path of pc_to_img
and render_errors) and the pieces around it that the reference takes from Open3D, matplotlib and PIL (its utils/o3d.py,
pc_to_img.py, pc_to_camera_params.py and ut_run_render.py): pinhole cameras in Open3D's JSON layout, a non-interactive default
view, the trim box, a PNG writer, the inferno error colours and a flat shading of normals.

The renderer is defined here, not cloned from Open3D: every point is a square of point_size pixels, z-buffered by a 64-bit key
(float32 depth, then row), so the image does not depend on evaluation order and ops.render_points returns the same bytes.
"""
import json
import struct
import zlib

import numpy as np

MAX_IMAGE_SIDE = 16384
MAX_POINT_SIZE = 64
COORD_LIMIT = float(1 << 30)          # |u|, |v| bound of a kept point
GREY = 128                            # colour of a point cloud without colours


class Camera:
    """Pinhole camera: extrinsic (4,4) world -> camera, row-major; intrinsic (3,3) [[fx, k01, cx], [0, fy, cy], [0, 0, 1]]; image
    width x height pixels.  Pixel centres sit at integer (u, v)."""

    def __init__(self, extrinsic, intrinsic, width, height):
        self.extrinsic = np.array(extrinsic, dtype=np.float64).reshape(4, 4)
        self.intrinsic = np.array(intrinsic, dtype=np.float64).reshape(3, 3)
        self.width, self.height = int(width), int(height)

    def __repr__(self):
        return f'Camera({self.width}x{self.height}, extrinsic={self.extrinsic.tolist()}, intrinsic={self.intrinsic.tolist()})'


def check_camera(camera, what='render'):
    """The camera limits of include/pcc_geo.h "point rendering" (ValueError naming the first one broken)."""
    E, K, W, H = camera.extrinsic, camera.intrinsic, camera.width, camera.height
    if not (1 <= W <= MAX_IMAGE_SIDE and 1 <= H <= MAX_IMAGE_SIDE):
        raise ValueError(f'{what}: image size {W}x{H} outside [1, {MAX_IMAGE_SIDE}] per side')
    if E.shape != (4, 4) or K.shape != (3, 3):
        raise ValueError(f'{what}: extrinsic must be 4x4 and intrinsic 3x3, got {E.shape} and {K.shape}')
    if not (np.isfinite(E).all() and np.isfinite(K).all()):
        raise ValueError(f'{what}: camera values must be finite')
    if not np.array_equal(E[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f'{what}: extrinsic bottom row must be [0, 0, 0, 1], got {E[3].tolist()}')
    if K[1, 0] != 0.0 or not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise ValueError(f'{what}: intrinsic rows 1 and 2 must be [0, fy, cy] and [0, 0, 1], got {K[1:].tolist()}')


def check_render_args(points, colors, camera, point_size, background):
    """Every limit of a render call, checked on the host: returns (float64 (n,3) points, uint8 (n,3) colours or None,
    point size, uint8 (3,) background).  ValueError on the first limit broken."""
    check_camera(camera)
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'render: points must be (n, 3), got {p.shape}')
    if p.dtype.kind not in 'fiu':
        raise ValueError(f'render: unsupported point dtype {p.dtype}')
    if p.shape[0] >= 1 << 31:
        raise ValueError('render: at most 2^31 - 1 points per call')
    p = np.ascontiguousarray(p, np.float64)
    c = None
    if colors is not None:
        c = np.asarray(colors)
        if c.shape != (p.shape[0], 3):
            raise ValueError(f'render: colours must be ({p.shape[0]}, 3), got {c.shape}')
        if c.dtype.kind not in 'iu' or (c.dtype != np.uint8 and c.size and (c.min() < 0 or c.max() > 255)):
            raise ValueError(f'render: colours must be integers in 0..255, got {c.dtype}')
        c = np.ascontiguousarray(c, np.uint8)
    if isinstance(point_size, (bool, np.bool_)) or int(point_size) != point_size or not 1 <= point_size <= MAX_POINT_SIZE:
        raise ValueError(f'render: point_size = {point_size!r} must be an integer in [1, {MAX_POINT_SIZE}]')
    bg = np.asarray(background)
    if bg.shape != (3,) or bg.dtype.kind not in 'iu' or (bg < 0).any() or (bg > 255).any():
        raise ValueError(f'render: background must be 3 integers in 0..255, got {background!r}')
    return p, c, int(point_size), bg.astype(np.uint8)


def project(points, camera):
    """Steps 1-2 of the definition: (u, v, zc, kept) in float64, every operation rounded (numpy does not contract)."""
    E, K = camera.extrinsic, camera.intrinsic
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(all='ignore'):
        xc = ((E[0, 0] * x + E[0, 1] * y) + E[0, 2] * z) + E[0, 3]
        yc = ((E[1, 0] * x + E[1, 1] * y) + E[1, 2] * z) + E[1, 3]
        zc = ((E[2, 0] * x + E[2, 1] * y) + E[2, 2] * z) + E[2, 3]
        u = ((K[0, 0] * xc + K[0, 1] * yc) + K[0, 2] * zc) / zc
        v = (K[1, 1] * yc + K[1, 2] * zc) / zc
        kept = (zc > 0) & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < COORD_LIMIT) & (np.abs(v) < COORD_LIMIT)
    return u, v, zc, kept


def render_keys(points, camera, point_size):
    """The per-pixel minimum key (uint64 (H, W), all ones where no point landed) of the definition's steps 1-4."""
    W, H, s = camera.width, camera.height, point_size
    u, v, zc, kept = project(points, camera)
    rows = np.nonzero(kept)[0]
    h = s / 2 - 1
    i0 = np.floor(u[rows] - h).astype(np.int64)
    j0 = np.floor(v[rows] - h).astype(np.int64)
    keys = (zc[rows].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    order = np.argsort(keys, kind='stable')
    i0, j0, keys = i0[order], j0[order], keys[order]
    zbuf = np.full(W * H, np.iinfo(np.uint64).max, np.uint64)
    for dj in range(s):
        j = j0 + dj
        okj = (j >= 0) & (j < H)
        for di in range(s):
            i = i0 + di
            ok = okj & (i >= 0) & (i < W)
            pix = j[ok] * W + i[ok]
            upix, first = np.unique(pix, return_index=True)      # keys ascend: the first of each pixel is its smallest
            zbuf[upix] = np.minimum(zbuf[upix], keys[ok][first])
    return zbuf.reshape(H, W)


def render_host(points, camera, colors=None, point_size=1, background=(255, 255, 255), return_rows=False):
    """include/pcc_geo.h "point rendering" in numpy: the (H, W, 3) uint8 image (and the (H, W) int32 rows, -1 where no point
    landed, with return_rows=True).  The same arguments and checks as ops.render_points, and the same bytes."""
    p, c, s, bg = check_render_args(points, colors, camera, point_size, background)
    H, W = camera.height, camera.width
    if len(p) == 0:
        img = np.broadcast_to(bg, (H, W, 3)).copy()
        return (img, np.full((H, W), -1, np.int32)) if return_rows else img
    zbuf = render_keys(p, camera, s)
    hit = zbuf != np.iinfo(np.uint64).max
    rows = np.where(hit, (zbuf & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    img = np.broadcast_to(bg, (H, W, 3)).copy()
    img[hit] = GREY if c is None else c[rows[hit]]
    return (img, rows) if return_rows else img


# ---- cameras ---------------------------------------------------------------------------------------------------------------------

def read_camera(path):
    """Open3D's PinholeCameraParameters JSON (matrices stored column-major, as Eigen writes them)."""
    with open(path) as f:
        d = json.load(f)
    E = np.array(d['extrinsic'], np.float64).reshape(4, 4, order='F')
    intr = d['intrinsic']
    K = np.array(intr['intrinsic_matrix'], np.float64).reshape(3, 3, order='F')
    return Camera(E, K, intr['width'], intr['height'])


def write_camera(path, camera):
    d = {'class_name': 'PinholeCameraParameters',
         'extrinsic': camera.extrinsic.ravel(order='F').tolist(),
         'intrinsic': {'height': camera.height, 'intrinsic_matrix': camera.intrinsic.ravel(order='F').tolist(), 'width': camera.width},
         'version_major': 1, 'version_minor': 0}
    with open(path, 'w') as f:
        json.dump(d, f, indent='\t')


def default_camera(points, width=1024, height=1024, front=(0, 0, 1), up=(0, 1, 0), zoom=0.7, fov=60.0):
    """A fixed view of the cloud modelled on Open3D's default view control (the non-interactive stand-in for the reference's
    pc_to_camera_params): looks at the centre of the bounding box from `front`, `up` towards -v, at distance
    zoom * extent / tan(fov / 2).  Refuses front parallel to up."""
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or len(p) == 0:
        raise ValueError(f'default_camera: points must be (n, 3) with n >= 1, got {p.shape}')
    if not (0 < fov < 180) or not zoom > 0:
        raise ValueError(f'default_camera: need 0 < fov < 180 and zoom > 0, got fov={fov}, zoom={zoom}')
    mn, mx = p.min(0), p.max(0)
    lookat = (mn + mx) / 2
    extent = float((mx - mn).max()) or 1.0
    f = np.asarray(front, np.float64)
    upv = np.asarray(up, np.float64)
    if f.shape != (3,) or upv.shape != (3,) or not np.linalg.norm(f) > 0:
        raise ValueError(f'default_camera: front and up must be non-zero 3-vectors, got {front!r}, {up!r}')
    f = f / np.linalg.norm(f)
    r = np.cross(upv, f)
    if not np.linalg.norm(r) > 1e-12 * max(np.linalg.norm(upv), 1e-300):
        raise ValueError(f'default_camera: front {front!r} is parallel to up {up!r}')
    r = r / np.linalg.norm(r)
    u = np.cross(f, r)
    R = np.stack([r, -u, -f])
    t_half = np.tan(np.deg2rad(fov) / 2)
    eye = lookat + f * (zoom * extent / t_half)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    fl = height / (2 * t_half)
    K = np.array([[fl, 0.0, width / 2 - 0.5], [0.0, fl, height / 2 - 0.5], [0.0, 0.0, 1.0]])
    return Camera(E, K, width, height)


# ---- images ----------------------------------------------------------------------------------------------------------------------

def trim_bbox(img, background=(255, 255, 255)):
    """(left, upper, right, lower) of the pixels that differ from `background` (right and lower exclusive): PIL's
    ImageChops.difference(img, bg).getbbox(), as the reference's trim_img_bbox uses it.  Raises on an image of background only."""
    diff = (np.asarray(img) != np.asarray(background, np.uint8)).any(-1)
    cols, rows = np.nonzero(diff.any(0))[0], np.nonzero(diff.any(1))[0]
    if len(cols) == 0:
        raise RuntimeError('Empty image')
    return int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1


def crop(img, bbox):
    """PIL's Image.crop for a box inside the image."""
    left, upper, right, lower = bbox
    return img[upper:lower, left:right]


def png_bytes(img):
    """An (H, W, 3) uint8 image as an 8-bit RGB PNG (no filter, zlib level 6): the same array gives the same bytes."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError(f'png: need a non-empty (H, W, 3) uint8 image, got {img.shape}')
    H, W = img.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), img.reshape(H, W * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_png(path, img):
    with open(path, 'wb') as f:
        f.write(png_bytes(img))


# ---- colours ---------------------------------------------------------------------------------------------------------------------

# matplotlib's colormaps['inferno'](np.arange(256), bytes=True)[:, :3], row after row
INFERNO_U8 = np.frombuffer(bytes.fromhex(''.join((
    '00000300000400000601000701010901010b02010e02021003021204031404031605041806041b07051d08061f090621'
    '0a07230b07260d08280e082a0f092d10092f120a32130a34140b36160b39170b3b190b3e1a0b401c0c431d0c451f0c47'
    '200c4a220b4c240b4e260b50270b52290b542b0a562d0a582e0a5a300a5c32095d34095f3509603709613909623b0964'
    '3c09653e0966400966410967430a68450a69460a69480b6a4a0b6a4b0c6b4d0c6b4f0d6c500d6c520e6c530e6d550f6d'
    '570f6d58106d5a116d5b116e5d126e5f126e60136e62146e63146e65156e66156e68166e6a176e6b176e6d186e6e186e'
    '70196e72196d731a6d751b6d761b6d781c6d7a1c6d7b1d6c7d1d6c7e1e6c801f6b811f6b83206b85206a86216a88216a'
    '8922698b22698d23698e24689024689125679325679526669626669827659928649b28649c29639e2963a02a62a12b61'
    'a32b61a42c60a62c5fa72d5fa92e5eab2e5dac2f5cae305baf315bb1315ab23259b43358b53357b73456b83556ba3655'
    'bb3754bd3753be3852bf3951c13a50c23b4fc43c4ec53d4dc73e4cc83e4bc93f4acb4049cc4148cd4247cf4446d04544'
    'd14643d24742d44841d54940d64a3fd74b3ed94d3dda4e3bdb4f3adc5039dd5238de5337df5436e05634e25733e35832'
    'e45a31e55b30e65c2ee65e2de75f2ce8612be9622aea6428eb6527ec6726ed6825ed6a23ee6c22ef6d21f06f1ff0701e'
    'f1721df2741cf2751af37719f37918f47a16f57c15f57e14f68012f68111f78310f7850ef8870df8880cf88a0bf98c09'
    'f98e08f99008fa9107fa9306fa9506fa9706fb9906fb9b06fb9d06fb9e07fba007fba208fba40afba60bfba80dfbaa0e'
    'fbac10fbae12fbb014fbb116fbb318fbb51afbb71cfbb91efabb21fabd23fabf25fac128f9c32af9c52cf9c72ff8c931'
    'f8cb34f8cd37f7cf3af7d13cf6d33ff6d542f5d745f5d948f4db4bf4dc4ff3de52f3e056f3e259f2e45df2e660f1e864'
    'f1e968f1eb6cf1ed70f1ee74f1f079f1f27df2f381f2f485f3f689f4f78df5f891f6fa95f7fb99f9fc9dfafda0fcfea4'
))), np.uint8).reshape(256, 3)
INFERNO_U8.flags.writeable = False


def error_colors(sq, pmax):
    """Inferno colours of squared residuals on the scale [0, pmax]: index min(floor((sq / pmax) * 256), 255), 0 when pmax is 0 --
    matplotlib's cmap(Normalize(0, pmax)(sq), bytes=True), with its "over" colour above pmax.  Returns (n, 3) uint8."""
    x = np.asarray(sq, np.float64)
    pmax = float(pmax)
    if pmax == 0:
        idx = np.zeros(x.shape, np.int64)
    else:
        idx = np.minimum(np.floor((x / pmax) * 256.0), 255).astype(np.int64)
    return INFERNO_U8[idx]


def shade_colors(normals, camera, base=224):
    """Grey levels for a cloud without colours: c = |n . w| / |n| with w the camera's viewing axis (row 2 of the rotation), 0 for a
    zero normal; level = min(floor(base * (0.3 + 0.7 c) + 0.5), 255).  Returns (n, 3) uint8."""
    n = np.asarray(normals, np.float64)
    w = camera.extrinsic[2, :3]
    with np.errstate(all='ignore'):
        dot = np.abs((w[0] * n[:, 0] + w[1] * n[:, 1]) + w[2] * n[:, 2])
        norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        c = np.where(norm > 0, dot / np.where(norm > 0, norm, 1.0), 0.0)
        level = np.minimum(np.floor(np.asarray(base, np.float64) * (0.3 + 0.7 * c[:, None]) + 0.5), 255)
    return np.ascontiguousarray(np.broadcast_to(level, (len(n), 3)), np.uint8)
