"""Restatement of the surface anchor codec in plain Python loops, written from the specification; it shares no code
with the package: its own Morton keys (a bit loop), near sets by set membership, the angular order through `sorted` with a comparator,
one leaf, one triangle, one sample at a time, and the bit-at-a-time coder of _anchor_ref.py.  The block stream inside is
_anchor_ref.encode's.

The only shortcut: a triangle's samples are tried inside the bounding box of its projection (widened to whole samples) instead of
over all of [0, W]^2 -- a sample outside the box fails a closed inside-test, so the result is the same.

Results are cached per (cloud, k): the CPU and the GPU tests of one session share them, and nothing modifies them.
"""
import functools
import struct

import numpy as np
from scipy.spatial import cKDTree

import _anchor_ref as AR
from _normals_ref import shell


def morton(c):
    k = 0
    for b in range(int(max(c[0], c[1], c[2])).bit_length()):                  # at most 21; the bits above are 0
        k |= ((c[0] >> b) & 1) << (3 * b + 2) | ((c[1] >> b) & 1) << (3 * b + 1) | ((c[2] >> b) & 1) << (3 * b)
    return k


def others(a):
    return [x for x in (0, 1, 2) if x != a]


def cross(ax, ay, bx, by):
    return ax * by - ay * bx


def leaf_edges(b):
    """The 12 edges (key, corner, axis) of leaf b, edge e = 4 a + 2 du + dv at place e."""
    out = []
    for a in range(3):
        u, v = others(a)
        for du in (0, 1):
            for dv in (0, 1):
                c = list(b)
                c[u] += du
                c[v] += dv
                out.append((morton(c) << 2 | a, tuple(c), a))
    return out


def edge_list(leaves):
    """-> [(key, corner, axis)] of the distinct edges of all leaves, ascending by key: the coded order."""
    edge_set = {}
    for b in leaves:
        for key, c, a in leaf_edges(b):
            edge_set[key] = (c, a)
    return [(key,) + edge_set[key] for key in sorted(edge_set)]


def model(points, k):
    """-> (distinct points, leaves [b], edges [(key, corner, axis)], flags, ts), leaves and edges in their coded order."""
    W = 1 << k
    cloud = set(tuple(int(v) for v in p) for p in points)
    leaves = sorted(set((x >> k, y >> k, z >> k) for x, y, z in cloud), key=morton)
    edges = edge_list(leaves)
    flags, ts = [], []
    for key, c, a in edges:
        u, v = others(a)
        total = n = 0
        for off in range(W):
            for eu in (-1, 0, 1):
                for ev in (-1, 0, 1):
                    p = [0, 0, 0]
                    p[a], p[u], p[v] = W * c[a] + off, W * c[u] + eu, W * c[v] + ev
                    if tuple(p) in cloud:
                        total += off
                        n += 1
        flags.append(1 if n else 0)
        ts.append((2 * total + n) // (2 * n) if n else 0)
    return len(cloud), leaves, edges, flags, ts


def half(x, y):
    if y > 0 or (y == 0 and x > 0):
        return 0
    if y < 0 or (y == 0 and x < 0):
        return 1
    return 2


def leaf_voxels(rs, W):
    """Vertices relative to the origin, in edge-key order -> the set of voxels of the leaf, relative to its origin.  A pure function
    of its arguments: the last few hundred results are kept, for the leaves that several cases of one block share."""
    return _kept_leaf_voxels(tuple(tuple(r) for r in rs), W)


@functools.lru_cache(maxsize=256)
def _kept_leaf_voxels(rs, W):
    return frozenset(_leaf_voxels(rs, W))


def _leaf_voxels(rs, W):
    m = len(rs)
    if m == 0:
        return {(W // 2, W // 2, W // 2)}
    out = set(tuple(r) for r in rs)
    if m < 3:
        return out
    G = [sum(r[a] for r in rs) for a in range(3)]
    d = [[m * r[a] - G[a] for a in range(3)] for r in rs]
    spread = [sum(di[a] ** 2 for di in d) for a in range(3)]
    dom = spread.index(min(spread))
    pu, pv = others(dom)
    xy = [(di[pu], di[pv]) for di in d]

    def compare(i, j):
        hi, hj = half(*xy[i]), half(*xy[j])
        if hi != hj:
            return -1 if hi < hj else 1
        cr = cross(xy[i][0], xy[i][1], xy[j][0], xy[j][1])
        if cr != 0:
            return -1 if cr > 0 else 1
        ni, nj = xy[i][0] ** 2 + xy[i][1] ** 2, xy[j][0] ** 2 + xy[j][1] ** 2
        if ni != nj:
            return -1 if ni < nj else 1
        return -1 if i < j else 1 if i > j else 0

    s = sorted(range(m), key=functools.cmp_to_key(compare))
    for j in range(m):
        A, B, C = G, [m * v for v in rs[s[j]]], [m * v for v in rs[s[(j + 1) % m]]]
        for q in range(3):
            u, v = others(q)
            Bq, Cq = B, C
            area2 = cross(Bq[u] - A[u], Bq[v] - A[v], Cq[u] - A[u], Cq[v] - A[v])
            if area2 == 0:
                continue
            if area2 < 0:
                Bq, Cq = C, B
            ilo, ihi = min(A[u], Bq[u], Cq[u]) // m, -(-max(A[u], Bq[u], Cq[u]) // m)
            jlo, jhi = min(A[v], Bq[v], Cq[v]) // m, -(-max(A[v], Bq[v], Cq[v]) // m)
            for i in range(max(ilo, 0), min(ihi, W) + 1):
                for jj in range(max(jlo, 0), min(jhi, W) + 1):
                    Pu, Pv = m * i, m * jj
                    la = cross(Cq[u] - Bq[u], Cq[v] - Bq[v], Pu - Bq[u], Pv - Bq[v])
                    lb = cross(A[u] - Cq[u], A[v] - Cq[v], Pu - Cq[u], Pv - Cq[v])
                    lc = cross(Bq[u] - A[u], Bq[v] - A[v], Pu - A[u], Pv - A[v])
                    if la < 0 or lb < 0 or lc < 0:
                        continue
                    lam = la + lb + lc
                    h = (2 * (la * A[q] + lb * Bq[q] + lc * Cq[q]) + m * lam) // (2 * m * lam)
                    vox = [0, 0, 0]
                    vox[q], vox[u], vox[v] = h, i, jj
                    out.add(tuple(vox))
    return out


def reconstruction(leaves, edges, flags, ts, k, resolution, per_leaf=False):
    W = 1 << k
    where = {key: n for n, (key, _, _) in enumerate(edges)}
    cloud, leafwise = set(), []
    for b in leaves:
        mine = []
        for key, c, a in leaf_edges(b):
            n = where[key]
            if flags[n]:
                r = [W * (c[x] - b[x]) for x in range(3)]
                r[a] += ts[n]
                mine.append((n, r))
        rel = leaf_voxels([r for _, r in sorted(mine)], W)
        leafwise.append(rel)
        for vox in rel:
            cloud.add(tuple(min(W * b[x] + vox[x], resolution - 1) for x in range(3)))
    out = np.array(sorted(cloud, key=morton), np.int32).reshape(-1, 3)
    return (out, leafwise) if per_leaf else out


def payload(edges, flags, ts, k):
    e = AR.RefEncoder()
    prev = 0
    for (key, c, a), f, t in zip(edges, flags, ts):
        e.encode(2 * a + prev, f)
        if f:
            m = 1
            for b in range(k - 1, -1, -1):
                bit = t >> b & 1
                e.encode(8 + m, bit)
                m = 2 * m + bit
        prev = f
    return e.finish()


def coded_points(points, resolution, k):
    """-> dict(stream, decoded, leaf_keys, edge_keys, flags, t, leaves, edges, leafwise) of a cloud, by the restatement alone."""
    W = 1 << k
    ndistinct, leaves, edges, flags, ts = model(points, k)
    blocks = np.array(leaves, np.int64)
    octree = AR.encode(blocks, -(-resolution // W), 1, 1)
    head = struct.pack('<4sBIBIIIII', b'PCSA', 1, resolution, k, len(leaves), len(edges), sum(flags), ndistinct, len(octree))
    decoded, leafwise = reconstruction(leaves, edges, flags, ts, k, resolution, per_leaf=True)
    decoded.setflags(write=False)
    return dict(stream=head + octree + payload(edges, flags, ts, k), decoded=decoded, leaves=leaves, edges=edges, leafwise=leafwise,
                leaf_keys=np.array([morton(b) for b in leaves], np.uint64), edge_keys=np.array([e[0] for e in edges], np.uint64),
                flags=np.array(flags, np.uint8), t=np.array(ts, np.uint8))


@functools.lru_cache(maxsize=None)
def coded(name, k):
    """coded_points of a small cloud: computed once, shared, read only."""
    points, resolution = small_clouds()[name]
    return coded_points(points, resolution, k)


@functools.lru_cache(maxsize=None)
def small_clouds():
    """{name: (points, resolution)} -- the small cases of the CPU and GPU tests."""
    rng = np.random.default_rng(11)
    out = {'shell64': (shell(64)[0].astype(np.int64), 64), 'shell128': (shell(128)[0].astype(np.int64), 128)}
    g = np.arange(5, 41)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    out['plane_axis'] = (np.stack([x, y, np.full_like(x, 20)], 1), 64)
    g = np.arange(48)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    z = (900 - 10 * x - 7 * y + 6) // 13                                   # x + 0.7 y + 1.3 z = 90: every raster axis sees area
    keep = (z >= 0) & (z < 64)
    out['plane_tilted'] = (np.stack([x, y, z], 1)[keep], 64)
    out['sparse300'] = (rng.integers(0, 256, (300, 3)), 256)               # most leaves have fewer than 3 vertices, many have none
    out['one_point'] = (np.array([[5, 0, 9]]), 16)
    g = np.arange(50, 64)
    y, z = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    top = np.concatenate([np.stack([np.full_like(y, 63), y, z], 1), np.stack([y, np.full_like(y, 63), z], 1),
                          np.stack([g, np.full_like(g, 63), np.full_like(g, 63)], 1), [[63, 63, 63]]])
    out['top_corner'] = (top, 64)                                          # the upper lattice line and the clip
    dup = out['plane_tilted'][0][:600]
    out['duplicates'] = (np.concatenate([dup, dup[::3], dup[:50]]), 64)
    g = np.arange(100)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing='ij'))
    out['res100'] = (np.stack([x, y, (x + 2 * y) // 3], 1), 100)           # not a multiple of W for k = 3, 4
    for points, _ in out.values():
        points.setflags(write=False)
    return out


def hausdorff_condition(points, decoded, k, what):
    """What the definition implies, in integers: a decoded voxel lies in the closed cube of an occupied leaf, which holds an input
    point, and every leaf emits a voxel: both directed squared distances are at most 3 W^2."""
    W = 1 << k
    points, decoded = np.asarray(points, np.int64), np.asarray(decoded, np.int64)
    for a, b in ((points, decoded), (decoded, points)):
        _, idx = cKDTree(b).query(a)
        assert (((a - b[idx]) ** 2).sum(1) <= 3 * W * W).all(), what


KS = (2, 3, 4)
