"""A conventional surface-model (triangle soup class) geometry codec that runs on any voxelised cloud: the second rate-distortion
baseline of the experiment loop, beside the octree anchor (anchor_octree.py).

  python -m pcc_geo_cnn_v2_amd.anchor_surface encode in.ply out.bin --resolution 1024 --node_log2 3 [--device gpu|host]
  python -m pcc_geo_cnn_v2_amd.anchor_surface decode out.bin out.ply [--device gpu|host]

It is NOT G-PCC and not trisoup-conformant: its streams are not TMC13 streams and its numbers are not comparable with published
G-PCC trisoup numbers.  It is the same class of codec as the "G-PCC trisoup" curve of the paper -- code the occupied blocks with an
octree, one vertex per block edge the surface crosses, rebuild the surface as a triangle fan per block and voxelise it -- with nothing
external to install.  DESIGN.md §4.16 holds the normative definition (integers only) and its limits; include/pcc_geo.h "surface anchor"
the native entry points.

    encode(points, resolution, node_log2, device='gpu') -> bytes        decode(data, device='gpu') -> (M,3) int32 points

In short, with k = node_log2 in [2, 6] and W = 2^k: leaves are the distinct p >> k in Morton order; every leaf has 12 edges (lattice
corner c, axis a), the edge list is the distinct morton(c) << 2 | a, ascending; an edge has a vertex where input points lie in the
3 x 3 column around it, at the rounded mean offset t.  A leaf with m >= 3 vertices is rebuilt as the fan of m triangles around the
vertex centroid, each rasterised along all three axes; the vertices themselves are always emitted, the leaf centre where there is
none.  Stream: 'PCSA', version (1), resolution (uint32), k (uint8), leaves, edges, vertices, distinct input points, octree_len
(uint32), little endian; then octree_len bytes, a complete octree anchor stream of the leaf coordinates (lossless, resolution
ceil(resolution / W)); then the vertex payload: per edge its flag and behind a set flag the k bits of t, through the octree anchor's
binary coder.

device='gpu' finds leaves, edges and vertices (encoder) and rasterises (decoder) in HIP (csrc/surface_anchor.hip); device='host' does
the same in numpy below.  Both give the same bytes and the same decoded arrays; the entropy coder is the same host C++ either way.
A damaged stream raises AnchorStreamError from checks on the host; nothing malformed reaches the device.
"""
import argparse
import struct
import sys

import numpy as np

from . import anchor_octree as A
from .anchor_octree import AnchorStreamError, check_device, check_points, check_resolution, morton, unmorton

MAGIC, VERSION = b'PCSA', 1
HEADER = struct.Struct('<4sBIBIIIII')
NODE_LOG2 = (2, 6)
DEVICES = A.DEVICES
_NO_EDGE = np.uint64(1 << 62)


# ---- contract
def check_node_log2(k):
    if k != int(k) or not NODE_LOG2[0] <= int(k) <= NODE_LOG2[1]:
        raise ValueError(f'anchor_surface: node_log2 {k!r} outside [{NODE_LOG2[0]}, {NODE_LOG2[1]}]')
    return int(k)


def _check(points, resolution, node_log2):
    p, resolution, k = check_points(points), check_resolution(resolution), check_node_log2(node_log2)
    if int(p.max()) >= resolution:
        raise ValueError(f'anchor_surface: coordinates must lie in [0, resolution = {resolution})')
    if len(p) >= (1 << 31) // 3:
        raise ValueError('anchor_surface: at most (2^31 - 1) / 3 points')
    return p, resolution, k


def blocks_resolution(resolution, k):
    return -(-resolution // (1 << k))


def _axes(a):
    """The two other axes, ascending."""
    return (1 if a == 0 else 0), (1 if a == 2 else 2)


# ---- the numpy host path
def leaves_host(p, k):
    """(n,3) points -> (Morton keys of the distinct points, leaf keys), both ascending."""
    pkeys = np.unique(morton(p[:, 0], p[:, 1], p[:, 2]))
    return pkeys, np.unique(pkeys >> np.uint64(3 * k))


def edges_host(leaf_keys):
    b = unmorton(leaf_keys)
    keys = []
    for e in range(12):
        a = e >> 2
        u, v = _axes(a)
        c = b.copy()
        c[:, u] += e >> 1 & 1
        c[:, v] += e & 1
        keys.append(morton(c[:, 0], c[:, 1], c[:, 2]) << np.uint64(2) | np.uint64(a))
    return np.unique(np.concatenate(keys))


def vertices_host(pkeys, k, edge_keys):
    """-> (flags, t) per edge, uint8."""
    W = 1 << k
    p = unmorton(pkeys)
    rem = p & (W - 1)
    line = np.where(rem <= 1, p >> k, np.where(rem == W - 1, (p >> k) + 1, -1))          # the lattice line within 1, per coordinate
    total, count = np.zeros(len(edge_keys), np.int64), np.zeros(len(edge_keys), np.int64)
    for a in range(3):
        u, v = _axes(a)
        near = (line[:, u] >= 0) & (line[:, v] >= 0)
        c = line[near]
        c[:, a] = p[near, a] >> k
        idx = np.searchsorted(edge_keys, morton(c[:, 0], c[:, 1], c[:, 2]) << np.uint64(2) | np.uint64(a))
        assert (idx < len(edge_keys)).all() and (edge_keys[idx] == (morton(c[:, 0], c[:, 1], c[:, 2]) << np.uint64(2) | np.uint64(a))).all()
        np.add.at(total, idx, rem[near, a])
        np.add.at(count, idx, 1)
    flags = count > 0
    t = np.where(flags, (2 * total + count) // np.maximum(2 * count, 1), 0)
    return flags.astype(np.uint8), t.astype(np.uint8)


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def _half(x, y):
    return np.where((y > 0) | ((y == 0) & (x > 0)), 0, np.where((y < 0) | ((y == 0) & (x < 0)), 1, 2))


def _fans(r, m):
    """Vertices (L,12,3) in edge order (the first m of each row count), m >= 3 -> (G (L,3), B, C (L,12,3)): the m-scaled triangles
    (G, B[j], C[j]), j < m."""
    n = len(r)
    valid = np.arange(12)[None, :] < m[:, None]
    r = r * valid[:, :, None]
    G = r.sum(1)
    d = (m[:, None, None] * r - G[:, None, :]) * valid[:, :, None]
    ad = np.argmin((d * d).sum(1), axis=1)                                 # the first minimum: ties to the lowest axis
    pu, pv = np.where(ad == 0, 1, 0), np.where(ad == 2, 1, 2)
    rows = np.arange(n)[:, None]
    x, y = d[rows, np.arange(12)[None, :], pu[:, None]], d[rows, np.arange(12)[None, :], pv[:, None]]
    h, nrm = _half(x, y), x * x + y * y
    xi, yi, xj, yj = x[:, :, None], y[:, :, None], x[:, None, :], y[:, None, :]
    cr = _cross(xi, yi, xj, yj)
    i, j = np.arange(12)[None, :, None], np.arange(12)[None, None, :]
    before = np.where(h[:, :, None] != h[:, None, :], h[:, :, None] < h[:, None, :],
                      np.where(cr != 0, cr > 0, np.where(nrm[:, :, None] != nrm[:, None, :], nrm[:, :, None] < nrm[:, None, :], i < j)))
    before &= valid[:, :, None] & valid[:, None, :] & (i != j)
    rank = before.sum(1)                                                   # how many come before j
    order = np.argsort(np.where(valid, rank, 99), axis=1, kind='stable')
    nxt = np.where(np.arange(12)[None, :] + 1 == m[:, None], 0, np.minimum(np.arange(12)[None, :] + 1, 11))
    B = m[:, None, None] * r[rows, order]
    C = m[:, None, None] * r[rows, np.take_along_axis(order, nxt, 1)]
    return G, B, C


def _raster(G, B, C, m, W):
    """-> (leaf row, voxel (.,3)) of every sample inside a triangle, all three axes."""
    S = W + 1
    grid = np.arange(S)
    tri = np.arange(12)[None, :] < m[:, None]
    rows_out, vox_out = [], []
    for q in range(3):
        u, v = _axes(q)
        Au, Av, Aq = (G[:, None, ax] + 0 * B[:, :, 0] for ax in (u, v, q))
        Bu, Bv, Bq, Cu, Cv, Cq = B[:, :, u], B[:, :, v], B[:, :, q], C[:, :, u], C[:, :, v], C[:, :, q]
        area2 = _cross(Bu - Au, Bv - Av, Cu - Au, Cv - Av)
        swap = area2 < 0
        Bu, Cu, Bv, Cv, Bq, Cq = (np.where(swap, Cu, Bu), np.where(swap, Bu, Cu), np.where(swap, Cv, Bv), np.where(swap, Bv, Cv),
                                  np.where(swap, Cq, Bq), np.where(swap, Bq, Cq))
        Pu = (m[:, None] * grid[None, :])[:, None, :, None]
        Pv = (m[:, None] * grid[None, :])[:, None, None, :]
        e = lambda a: a[:, :, None, None]
        la = _cross(e(Cu - Bu), e(Cv - Bv), Pu - e(Bu), Pv - e(Bv))
        lb = _cross(e(Au - Cu), e(Av - Cv), Pu - e(Cu), Pv - e(Cv))
        lc = _cross(e(Bu - Au), e(Bv - Av), Pu - e(Au), Pv - e(Av))
        inside = (la >= 0) & (lb >= 0) & (lc >= 0) & e(tri & (area2 != 0))
        l, t, i, j = np.nonzero(inside)
        la, lb, lc = la[l, t, i, j], lb[l, t, i, j], lc[l, t, i, j]
        lam, mm = la + lb + lc, m[l]
        h = (2 * (la * Aq[l, t] + lb * Bq[l, t] + lc * Cq[l, t]) + mm * lam) // (2 * mm * lam)
        vox = np.empty((len(l), 3), np.int64)
        vox[:, q], vox[:, u], vox[:, v] = h, i, j
        rows_out.append(l)
        vox_out.append(vox)
    return np.concatenate(rows_out), np.concatenate(vox_out)


def reconstruct_host(leaf_keys, edge_keys, flags, t, k, resolution, chunk_elements=1 << 21):
    """Leaves, the edge list and its vertices -> the decoded (n,3) int32 cloud in Morton order."""
    W = 1 << k
    b = unmorton(leaf_keys)
    n = len(b)
    idx, r = np.empty((n, 12), np.int64), np.zeros((n, 12, 3), np.int64)
    for e in range(12):
        a = e >> 2
        u, v = _axes(a)
        c = b.copy()
        c[:, u] += e >> 1 & 1
        c[:, v] += e & 1
        idx[:, e] = np.searchsorted(edge_keys, morton(c[:, 0], c[:, 1], c[:, 2]) << np.uint64(2) | np.uint64(a))
        r[:, e, u], r[:, e, v], r[:, e, a] = (e >> 1 & 1) * W, (e & 1) * W, t[idx[:, e]]
    f = flags[idx] > 0
    order = np.argsort(np.where(f, idx, np.int64(1) << 62), axis=1, kind='stable')           # flagged edges first, in edge-key order
    r = np.take_along_axis(r, order[:, :, None], 1)
    m = f.sum(1)
    origin = b * W
    out = [origin[m == 0] + W // 2]
    l, e = np.nonzero(np.arange(12)[None, :] < m[:, None])
    out.append(origin[l] + r[l, e])
    fan = np.flatnonzero(m >= 3)
    step = max(1, chunk_elements // (12 * (W + 1) ** 2))
    for s in range(0, len(fan), step):
        sel = fan[s:s + step]
        G, B, C = _fans(r[sel], m[sel])
        l, vox = _raster(G, B, C, m[sel], W)
        out.append(origin[sel][l] + vox)
    p = np.minimum(np.concatenate(out), resolution - 1)
    return unmorton(np.unique(morton(p[:, 0], p[:, 1], p[:, 2]))).astype(np.int32)


# ---- the codec
def _ctx(ctx):
    from . import ops
    return ctx if ctx is not None else ops.get_context()


def _model(p, k, device, ctx):
    """-> (distinct points, leaf keys, edge keys, flags, t), numpy."""
    from . import ops
    if device == 'gpu':
        ctx = _ctx(ctx)
        pkeys, leaves = ops.surface_leaves(ctx, np.ascontiguousarray(p, dtype=np.int32), k)
        edges = ops.surface_edges(ctx, leaves)
        flags, t = ops.surface_vertices(ctx, pkeys, k, edges)
        return int(pkeys.shape[0]), leaves.cpu().numpy().view(np.uint64), edges.cpu().numpy().view(np.uint64), flags, t
    pkeys, leaves = leaves_host(p, k)
    edges = edges_host(leaves)
    flags, t = vertices_host(pkeys, k, edges)
    return len(pkeys), leaves, edges, flags, t


def vertices(points, resolution, node_log2, device='gpu', ctx=None):
    """What the encoder hands its coder: (leaf keys, edge keys, flags, t) -- tests and the timing tool."""
    check_device(device)
    p, resolution, k = _check(points, resolution, node_log2)
    return _model(p, k, device, ctx)[1:]


def surface_points(leaf_keys, edge_keys, flags, t, resolution, node_log2, device='gpu', ctx=None, return_counts=False):
    """What the decoder does behind its coder: leaves, edge list and vertices -> the decoded cloud.  return_counts (device='gpu'):
    -> (cloud, pos, total) of ops.surface_reconstruct, the count pass's numbers per leaf."""
    import torch
    from . import ops
    check_device(device)
    resolution, k = check_resolution(resolution), check_node_log2(node_log2)
    leaf_keys, edge_keys = np.ascontiguousarray(leaf_keys, np.uint64), np.ascontiguousarray(edge_keys, np.uint64)
    if device == 'host':
        if return_counts:
            raise ValueError('anchor_surface: the host path has no count pass')
        return reconstruct_host(leaf_keys, edge_keys, np.asarray(flags), np.asarray(t), k, resolution)
    ctx = _ctx(ctx)
    dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a.view(np.int64)).to(ctx.device)
    return ops.surface_reconstruct(ctx, dev(leaf_keys), dev(edge_keys), flags, t, k, resolution, return_counts=return_counts)


def encode(points, resolution, node_log2, device='gpu', ctx=None):
    """See the module docstring."""
    from . import ops
    check_device(device)
    p, resolution, k = _check(points, resolution, node_log2)
    octree = A.encode(p >> k, blocks_resolution(resolution, k), (1, 1), device, ctx)
    ndistinct, leaves, edges, flags, t = _model(p, k, device, ctx)
    assert A.read_header(octree)['points'] == len(leaves)
    payload = ops.surface_encode_vertices(edges, flags, t, k)
    return HEADER.pack(MAGIC, VERSION, resolution, k, len(leaves), len(edges), int(flags.sum()), ndistinct, len(octree)) + octree + payload


def reconstruct(points, resolution, node_log2):
    """The cloud a decoder returns for encode(points, resolution, node_log2): the encoder's own reconstruction, without coding (numpy)."""
    p, resolution, k = _check(points, resolution, node_log2)
    _, leaves, edges, flags, t = _model(p, k, 'host', None)
    return reconstruct_host(leaves, edges, flags, t, k, resolution)


def read_header(data):
    """-> dict(resolution, node_log2, leaves, edges, vertices, points, octree_len) of a stream; AnchorStreamError for anything that is
    not one."""
    data = bytes(data)
    if len(data) < HEADER.size:
        raise AnchorStreamError(f'anchor_surface: {len(data)} bytes are shorter than the header')
    magic, version, resolution, k, leaves, edges, nvert, npoints, octree_len = HEADER.unpack_from(data)
    if magic != MAGIC:
        raise AnchorStreamError(f'anchor_surface: magic {magic!r}, not {MAGIC!r}')
    if version != VERSION:
        raise AnchorStreamError(f'anchor_surface: stream version {version}, this decoder reads {VERSION}')
    if not NODE_LOG2[0] <= k <= NODE_LOG2[1]:
        raise AnchorStreamError(f'anchor_surface: node_log2 {k} outside [{NODE_LOG2[0]}, {NODE_LOG2[1]}]')
    if not 1 <= resolution <= A.COORD_LIMIT:
        raise AnchorStreamError(f'anchor_surface: resolution {resolution} outside [1, {A.COORD_LIMIT}]')
    if not (1 <= leaves < (1 << 31) // 12 and leaves <= edges <= 12 * leaves and nvert <= edges and 1 <= npoints < 1 << 31):
        raise AnchorStreamError(f'anchor_surface: header counts out of range: {leaves} leaves, {edges} edges, {nvert} vertices, {npoints} points')
    if octree_len > len(data) - HEADER.size:
        raise AnchorStreamError(f'anchor_surface: the block stream of {octree_len} bytes runs past the end')
    return dict(resolution=resolution, node_log2=k, leaves=leaves, edges=edges, vertices=nvert, points=npoints, octree_len=octree_len)


def decode(data, device='gpu', ctx=None):
    import torch
    from . import _lib, ops
    check_device(device)
    data = bytes(data)
    h = read_header(data)
    k, resolution = h['node_log2'], h['resolution']
    octree = data[HEADER.size:HEADER.size + h['octree_len']]
    hb = A.read_header(octree)
    if hb['resolution'] != blocks_resolution(resolution, k) or hb['num'] != hb['den'] or hb['points'] != h['leaves']:
        raise AnchorStreamError(f"anchor_surface: the block stream holds {hb['points']} points at resolution {hb['resolution']}, scale "
                                f"{hb['num']}/{hb['den']}; the header wants {h['leaves']} at {blocks_resolution(resolution, k)}, lossless")
    if device == 'gpu':
        ctx = _ctx(ctx)
    b = A.decode(octree, device, ctx).astype(np.int64)
    leaves = morton(b[:, 0], b[:, 1], b[:, 2])
    if device == 'gpu':
        leaves_d = torch.from_numpy(leaves.view(np.int64)).to(ctx.device)
        edges_d = ops.surface_edges(ctx, leaves_d)
        edges = edges_d.cpu().numpy().view(np.uint64)
    else:
        edges = edges_host(leaves)
    if len(edges) != h['edges']:
        raise AnchorStreamError(f"anchor_surface: the leaves have {len(edges)} edges, the header says {h['edges']}")
    payload = data[HEADER.size + h['octree_len']:]
    try:
        flags, t, nflags, consumed = ops.surface_decode_vertices(payload, edges, k)
    except _lib.PccError as e:
        raise AnchorStreamError(f'anchor_surface: damaged stream: {e}') from None
    if nflags != h['vertices']:
        raise AnchorStreamError(f"anchor_surface: decoded {nflags} vertices, the header says {h['vertices']}")
    if consumed != len(payload):
        raise AnchorStreamError(f'anchor_surface: {len(payload) - consumed} bytes left behind the last edge')
    if device == 'gpu':
        return ops.surface_reconstruct(ctx, leaves_d, edges_d, flags, t, k, resolution)
    return reconstruct_host(leaves, edges, flags, t, k, resolution)


def build_parser():
    p = argparse.ArgumentParser(prog='anchor_surface', description='Surface anchor codec: a conventional triangle-soup class geometry baseline '
                                'for any voxelised cloud.  Not G-PCC, not trisoup-conformant.', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = p.add_subparsers(dest='command', required=True)
    e = sub.add_parser('encode', help='PLY -> stream')
    e.add_argument('input_pc')
    e.add_argument('output')
    e.add_argument('--resolution', type=int, required=True, help='Size of the voxel grid (1024 for a vox10 cloud)')
    e.add_argument('--node_log2', type=int, required=True, help='log2 of the block edge, 2 .. 6: larger blocks, lower rate')
    d = sub.add_parser('decode', help='stream -> PLY')
    d.add_argument('input')
    d.add_argument('output_pc')
    for s in (e, d):
        s.add_argument('--device', choices=DEVICES, default='gpu', help='Where the surface model is fitted and rasterised')
    return p


def main(argv=None):
    from .utils import pc_io
    a = build_parser().parse_args(argv)
    if a.device == 'gpu':
        from . import want_hw_queues
        want_hw_queues()
    if a.command == 'encode':
        data = encode(pc_io.load_pc(a.input_pc), a.resolution, a.node_log2, a.device)
        with open(a.output, 'wb') as f:
            f.write(data)
    else:
        with open(a.input, 'rb') as f:
            pts = decode(f.read(), a.device)
        pc_io.write_df(a.output_pc, pc_io.pa_to_df(pts))
    return 0


if __name__ == '__main__':
    sys.exit(main())
