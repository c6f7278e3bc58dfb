"""Independent restatement of include/pcc_geo.h "point rendering" for small cases: Python floats (IEEE float64, every operation
rounded) and loops -- every pixel looks at every point -- instead of numpy's vectorised z-buffer in utils/render.py."""
import math

import numpy as np


def render_ref(points, E, K, W, H, s, colors=None, background=(255, 255, 255)):
    """(image (H,W,3) uint8, rows (H,W) int32) by brute force.  E: 4x4, K: 3x3 nested lists or arrays."""
    E = [[float(v) for v in row] for row in np.asarray(E, np.float64)]
    K = [[float(v) for v in row] for row in np.asarray(K, np.float64)]
    cover = []                                    # (i0, j0, key) of every kept point
    for r, (x, y, z) in enumerate(np.asarray(points, np.float64).tolist()):
        xc = ((E[0][0] * x + E[0][1] * y) + E[0][2] * z) + E[0][3]
        yc = ((E[1][0] * x + E[1][1] * y) + E[1][2] * z) + E[1][3]
        zc = ((E[2][0] * x + E[2][1] * y) + E[2][2] * z) + E[2][3]
        if not zc > 0:
            continue
        try:
            u = ((K[0][0] * xc + K[0][1] * yc) + K[0][2] * zc) / zc
            v = (K[1][1] * yc + K[1][2] * zc) / zc
        except (OverflowError, ZeroDivisionError):
            continue
        if not (math.isfinite(u) and math.isfinite(v) and abs(u) < 2.0 ** 30 and abs(v) < 2.0 ** 30):
            continue
        h = s / 2 - 1
        z32 = int(np.array([zc], np.float64).astype(np.float32).view(np.uint32)[0])
        cover.append((math.floor(u - h), math.floor(v - h), (z32 << 32) | r))
    img = np.empty((H, W, 3), np.uint8)
    rows = np.full((H, W), -1, np.int32)
    for j in range(H):
        for i in range(W):
            best = None
            for i0, j0, key in cover:
                if i0 <= i < i0 + s and j0 <= j < j0 + s and (best is None or key < best):
                    best = key
            if best is None:
                img[j, i] = background
            else:
                row = best & 0xffffffff
                rows[j, i] = row
                img[j, i] = 128 if colors is None else colors[row]
    return img, rows
