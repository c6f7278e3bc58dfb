"""Mesh -> voxelised point cloud: the numpy definition of ops.mesh_to_points (include/pcc_geo.h "mesh sampling")
and its host path.  The GPU path returns the same bits.

The reference's dataset step (its src/ds_mesh_to_pc.py) samples a mesh with pyntcloud's `mesh_random` sampler, scales the samples
by one scalar min and max over all three axes, rounds them onto a vg^3 grid and drops duplicate voxels.  This module pins that
pipeline down bit for bit and makes it reproducible from a seed:

  1. area_i = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v2 - v1) x (v3 - v1), float64, every operation rounded;
  2. w_i = floor(ldexp(area_i / A_max, 32)) (uint64) and C = their inclusive prefix sums, W = C[F-1] < 2^63.  A triangle below
     2^-32 of the largest one has w = 0 and is never picked;
  3. sample s takes the four outputs r0..r3 of Philox4x64-10 with counter (s, 0, 0, 0) and key (seed, 0): row s of
     np.random.Philox(key=seed, counter=2**256-1).random_raw(4 * n).reshape(n, 4);
  4. its triangle is the smallest i with C[i] > umul64hi(r0, W); u = (r1 >> 11) 2^-53, v = (1 - u) ((r2 >> 11) 2^-53), and
     p = ((v1 u) + (v2 v)) + ((1 - (u + v)) v3) in float64, then rounded to float32 (pyntcloud's barycentrics: means 1/2, 1/4, 1/4);
  5. in float32: mn = min over all 3n coordinates, mx = max - mn, q = rint(((p - mn) / mx) * (vg - 1)); mx == 0 gives q = 0;
  6. the first sample of every distinct voxel, in sample order: (M,3) float32 integers in [0, vg) (a zero is +0).
"""
import numpy as np

COORD_LIMIT = 2.0 ** 100          # |vertex coordinate| bound: areas and float32 samples stay finite
VG_LIMIT = 1 << 21
COUNT_LIMIT = 1 << 31             # F and n are below this
_CHUNK = 1 << 20                  # samples per host chunk (bounds the host path's memory)
_M32 = np.uint64(0xffffffff)


def check_mesh(vertices, faces, n_samples, vg_size, seed):
    """The input contract, checked on the host before any GPU call.  Returns (float64 (V,3), int32 (F,3)) contiguous arrays;
    raises ValueError on: shapes, F or n outside [1, 2^31), vg outside [1, 2^21], a seed outside [0, 2^64), non-finite vertices or a
    coordinate beyond 2^100 in magnitude, indices outside [0, V), a total area of 0."""
    v = np.asarray(vertices)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
        raise ValueError(f'mesh_to_points: vertices must be (V, 3) with V >= 1, got {v.shape}')
    if f.ndim != 2 or f.shape[1] != 3 or not 1 <= f.shape[0] < COUNT_LIMIT:
        raise ValueError(f'mesh_to_points: faces must be (F, 3) with 1 <= F < 2^31, got {f.shape}')
    if v.dtype.kind not in 'fiu' or f.dtype.kind not in 'iu':
        raise ValueError(f'mesh_to_points: unsupported dtypes {v.dtype} (vertices) / {f.dtype} (faces)')
    if not 1 <= int(n_samples) < COUNT_LIMIT or int(n_samples) != n_samples:
        raise ValueError(f'mesh_to_points: n_samples = {n_samples!r} outside [1, 2^31)')
    if not 1 <= int(vg_size) <= VG_LIMIT or int(vg_size) != vg_size:
        raise ValueError(f'mesh_to_points: vg_size = {vg_size!r} outside [1, 2^21]')
    if not 0 <= int(seed) < 1 << 64 or int(seed) != seed:
        raise ValueError(f'mesh_to_points: seed = {seed!r} outside [0, 2^64)')
    v = np.ascontiguousarray(v, np.float64)
    if not np.isfinite(v).all():
        raise ValueError('mesh_to_points: vertices must be finite')
    if np.abs(v).max() > COORD_LIMIT:
        raise ValueError('mesh_to_points: vertex coordinates must lie within +-2^100')
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f'mesh_to_points: face indices must lie in [0, {v.shape[0]})')
    f = np.ascontiguousarray(f, np.int32)
    # total area > 0: stop at the first chunk that holds a triangle of nonzero area (a whole pass only for degenerate meshes)
    for s in range(0, f.shape[0], 1 << 14):
        if triangle_areas(v, f[s:s + (1 << 14)]).max() > 0:
            return v, f
    raise ValueError('mesh_to_points: the mesh has a total area of 0')


def triangle_areas(v, f):
    """Step 1: float64 areas, every operation rounded (numpy does not contract)."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def cumulative_weights(v, f):
    """Step 2: C, the inclusive uint64 prefix sums of w_i = floor(ldexp(area_i / A_max, 32))."""
    area = triangle_areas(v, f)
    w = np.floor(np.ldexp(area / area.max(), 32)).astype(np.uint64)
    return np.cumsum(w, dtype=np.uint64)


def philox_rows(seed, start, count):
    """Step 3: (count, 4) uint64, row s - start = the Philox4x64-10 block of counter (s, 0, 0, 0), key (seed, 0)."""
    g = np.random.Philox(key=int(seed), counter=(start - 1) % (1 << 256))
    return g.random_raw(4 * count).reshape(count, 4)


def umul64hi(a, b):
    """High 64 bits of the 128-bit product of uint64 arrays / scalars."""
    a, b = np.asarray(a, np.uint64), np.uint64(b)
    s32 = np.uint64(32)
    al, ah, bl, bh = a & _M32, a >> s32, b & _M32, b >> s32
    ll, hl, lh = al * bl, ah * bl, al * bh
    mid = (ll >> s32) + (hl & _M32) + lh                # < 2^64: (2^32 - 1)^2 + 2 (2^32 - 1)
    return ah * bh + (hl >> s32) + (mid >> s32)


def sample_points(v, f, n, seed, cum=None):
    """Steps 2-4: (n,3) float32 raw samples (checked inputs, see check_mesh)."""
    cum = cumulative_weights(v, f) if cum is None else cum
    W = cum[-1]
    out = np.empty((n, 3), np.float32)
    scale = 2.0 ** -53
    s11 = np.uint64(11)
    for s in range(0, n, _CHUNK):
        m = min(_CHUNK, n - s)
        r = philox_rows(seed, s, m)
        tri = f[np.searchsorted(cum, umul64hi(r[:, 0], W), side='right')]
        u = ((r[:, 1] >> s11).astype(np.float64) * scale)[:, None]
        w = ((1.0 - u[:, 0]) * ((r[:, 2] >> s11).astype(np.float64) * scale))[:, None]
        p = ((v[tri[:, 0]] * u) + (v[tri[:, 1]] * w)) + ((1.0 - (u + w)) * v[tri[:, 2]])
        out[s:s + m] = p.astype(np.float32)
    return out


def key_bits(vg_size):
    """b = max(1, ceil(log2 vg)): bits per axis of a voxel key x | y << b | z << 2b."""
    return max(1, (int(vg_size) - 1).bit_length())


def voxelize_samples(samples, vg_size):
    """Steps 5-6 on (n,3) float32 samples: the first sample of every distinct voxel, in sample order, as (M,3) float32."""
    p = np.asarray(samples, np.float32)
    mn = p.min()
    mx = p.max() - mn
    if mx == 0:
        q = np.zeros_like(p)
    else:
        q = np.rint(((p - mn) / mx) * np.float32(int(vg_size) - 1))
    b = np.uint64(key_bits(vg_size))
    qi = q.astype(np.uint64)
    keys = qi[:, 0] | (qi[:, 1] << b) | (qi[:, 2] << (b + b))
    _, first = np.unique(keys, return_index=True)          # first occurrence of every key
    return q[np.sort(first)] + np.float32(0)                 # sample order; -0 -> +0


def mesh_to_points(vertices, faces, n_samples=500000, vg_size=64, seed=0, return_samples=False):
    """Host path of ops.mesh_to_points, same arguments and the same bits: (M,3) float32 voxels (and the (n,3) float32 samples with
    return_samples=True)."""
    v, f = check_mesh(vertices, faces, n_samples, vg_size, seed)
    samples = sample_points(v, f, int(n_samples), int(seed))
    pts = voxelize_samples(samples, vg_size)
    return (pts, samples) if return_samples else pts
