"""Meshes for the mesh sampling tests and tools/bench_mesh.py, the reference's voxel lines (src/ds_mesh_to_pc.py) restated literally,
and a plain-Python Philox4x64-10 (Salmon et al., SC'11) to check the host path's random bits against."""
import numpy as np
import pandas as pd

M64 = (1 << 64) - 1


def philox4x64_10(counter, key):
    """Plain-Python Philox4x64-10 of a 4-word counter and a 2-word key: the 4 output words."""
    c, k = list(counter), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B97F4A7C15) & M64, (k[1] + 0xBB67AE8584CAA73B) & M64]
        p0, p1 = 0xD2E7470EE14C6C93 * c[0], 0xCA5A826395121157 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k[0], p1 & M64, (p0 >> 64) ^ c[3] ^ k[1], p0 & M64]
    return c


def reference_voxels(points, vg_size):
    """src/ds_mesh_to_pc.py's lines after sampling, on (n,3) float32 samples (xyz only: drop_duplicates)."""
    pc = pd.DataFrame(np.asarray(points, np.float32), columns=['x', 'y', 'z'])
    points = pc.values
    points = points - np.min(points)
    points = points / np.max(points)
    points = points * (vg_size - 1)
    points = np.round(points)
    pc[['x', 'y', 'z']] = points
    return pc.drop_duplicates().values


def soup(n_tris, seed, zero=0):
    """Random triangle soup in [0, 1]^3 with areas spread from about 1e-12 to 1 (edge scales 10^-6 .. 1); the first `zero`
    triangles have an area of exactly 0 (a repeated vertex, or three points on a line parallel to the x axis)."""
    rng = np.random.default_rng(seed)
    centre = rng.random((n_tris, 1, 3))
    scale = 10.0 ** rng.uniform(-6, 0, (n_tris, 1, 1))
    v = centre + scale * (rng.random((n_tris, 3, 3)) - 0.5)
    for i in range(zero):
        if i % 2:
            v[i, 2] = v[i, 0]
        else:
            v[i, 1:, 1:] = v[i, 0, 1:]
    return v.reshape(-1, 3), np.arange(3 * n_tris, dtype=np.int32).reshape(n_tris, 3)


def icosphere(level):
    """Unit icosphere: 20 * 4^level triangles, shared vertices (each subdivision splits every edge once)."""
    t = (1.0 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        e.sort(axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = m[0], m[1], m[2]
        v = np.concatenate([v, mid])
        f = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)])
    return v, f.astype(np.int32)


def stacked_triangles(areas):
    """One right triangle per area in the plane z = i (disjoint, identifiable by z); area 0 gives a degenerate triangle."""
    v = []
    for i, a in enumerate(areas):
        s = (2.0 * a) ** 0.5
        v += [[0, 0, i], [s, 0, i], [0, s, i]]
    v = np.array(v, np.float64)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)
