"""The anchor codecs' operators: octree (anchor_octree.py), surface (anchor_surface.py) and colour (anchor_color.py) -- include/pcc_geo.h
"octree anchor", "surface anchor", "colour anchor"."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _ptr, _workspace


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _encode_bytes(name, args, *caps):
    """The host payload encoder `name` of the ABI, name(*args, out, cap, &n) -> the n bytes it wrote; a capacity it answers with
    PCC_ERR_SPACE is followed by the next of `caps`."""
    n = C.c_int64()
    for cap in caps:
        out = np.empty(cap, np.uint8)
        rc = getattr(L.lib(), name)(*args, out.ctypes.data, out.size, C.byref(n))
        if rc != L.PCC_ERR_SPACE:
            break
    L.check(rc, name)
    return out[:n.value].tobytes()


# ---------------------------------------------------------------------------------------------
# octree anchor (include/pcc_geo.h "octree anchor"; the codec is anchor_octree.py)
# ---------------------------------------------------------------------------------------------
def anchor_code_bits(models, bits):
    """The anchor's binary range coder on raw decisions: models (n) in [0, 2048), bits (n) in {0, 1} -> bytes (host)."""
    m, b = np.ascontiguousarray(models, dtype=np.uint16), _u8(bits)
    assert m.ndim == 1 and m.shape == b.shape, 'anchor_code_bits: models and bits must be 1-d and of one length'
    return _encode_bytes('pcc_anchor_code_bits', (m.ctypes.data, b.ctypes.data, m.size), 2 * m.size + 16)


def anchor_decode_bits(data, models):
    m = np.ascontiguousarray(models, dtype=np.uint16)
    buf = np.frombuffer(bytes(data), np.uint8)
    out = np.empty(m.size, np.uint8)
    L.check(L.lib().pcc_anchor_decode_bits(buf.ctypes.data if buf.size else None, buf.size, m.ctypes.data, m.size, out.ctypes.data),
            'pcc_anchor_decode_bits')
    return out


def anchor_encode_nodes(occ, n6, no_context=False):
    """All occupancy bytes of a tree (breadth first) with their neighbour masks -> the payload bytes (host)."""
    occ, n6 = _u8(occ), _u8(n6)
    assert occ.ndim == 1 and occ.shape == n6.shape, 'anchor_encode_nodes: occ and n6 must be 1-d and of one length'
    return _encode_bytes('pcc_anchor_encode', (occ.ctypes.data, n6.ctypes.data, occ.size, L.PCC_ANCHOR_NO_CONTEXT if no_context else 0),
                         2 * occ.size + 16)


class AnchorDecoder:
    """The host decoder of one payload: level(n6) returns the occupancy bytes of the next level.  A payload that ends early raises
    PccError."""

    def __init__(self, payload, no_context=False):
        self._data = np.frombuffer(bytes(payload), np.uint8)          # kept alive: the C state points into it
        self._state = np.zeros(L.lib().pcc_anchor_decoder_bytes() + 8, np.uint8)
        L.check(L.lib().pcc_anchor_decoder_init(self._state.ctypes.data, self._data.ctypes.data if self._data.size else None, self._data.size,
                                                L.PCC_ANCHOR_NO_CONTEXT if no_context else 0), 'pcc_anchor_decoder_init')

    def level(self, n6):
        n6 = _u8(n6)
        occ = np.empty(n6.size, np.uint8)
        L.check(L.lib().pcc_anchor_decode_level(self._state.ctypes.data, n6.ctypes.data, n6.size, occ.ctypes.data), 'pcc_anchor_decode_level')
        return occ

    @property
    def consumed(self):
        return int(L.lib().pcc_anchor_decoder_consumed(self._state.ctypes.data))

    def __len__(self):
        return int(self._data.size)


def anchor_tree_launch(ctx, points, num, den, depth):
    """Enqueues the tree of anchor_octree.encode for an int32 (n,3) numpy cloud already checked by the caller; returns the pinned
    host buffer the result is being copied into and a function that waits for it and returns (counts[depth + 1], occ, n6): the nodes
    per level with the leaves last, and the bytes of all levels, breadth first.  Nothing is read back before that one copy."""
    lib, dev = L.lib(), ctx.device
    n, depth = int(points.shape[0]), int(depth)
    cap = int(lib.pcc_anchor_tree_capacity(n, depth))
    if cap <= 0:
        raise L.PccError(f'anchor_tree: {n} points at depth {depth} are outside the contract')
    hdr_bytes = 8 * L.PCC_ANCHOR_HDR_WORDS
    pts_d = torch.from_numpy(points).to(dev, non_blocking=True)
    out = torch.empty((hdr_bytes + 2 * cap,), dtype=torch.uint8, device=dev)
    ws = _workspace(ctx, lambda: lib.pcc_anchor_tree_workspace_bytes(n))
    base = out.data_ptr()
    L.check(lib.pcc_anchor_tree(ctx.handle, _ptr(pts_d), n, int(num), int(den), depth, C.c_void_p(base), C.c_void_p(base + hdr_bytes),
                                C.c_void_p(base + hdr_bytes + cap), _ptr(ws), ctx.stream), 'pcc_anchor_tree')
    cache = ctx.cache('anchor_pin')                     # one launch in flight per context: the pinned landing buffer is reused
    pin = cache.get('pin')
    if pin is None or pin.numel() < out.numel():
        cache['pin'] = pin = torch.empty((out.numel(),), dtype=torch.uint8, pin_memory=True)
    host = pin[:out.numel()]
    host.copy_(out, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    alive = (pts_d, out, ws)

    def finish():
        assert alive
        done.synchronize()                  # pts_d, out and ws stay alive until here
        raw = host.numpy()
        counts = raw[:hdr_bytes].view(np.int64)[:depth + 1].copy()
        offs = [int(lib.pcc_anchor_tree_level_offset(n, l)) for l in range(depth + 1)]
        for l in range(depth):
            if not 1 <= counts[l] <= offs[l + 1] - offs[l]:
                raise L.PccError(f'anchor_tree: level {l} reports {counts[l]} nodes for a slot of {offs[l + 1] - offs[l]}')
        occ = np.concatenate([raw[hdr_bytes + offs[l]:hdr_bytes + offs[l] + counts[l]] for l in range(depth)])
        n6 = np.concatenate([raw[hdr_bytes + cap + offs[l]:hdr_bytes + cap + offs[l] + counts[l]] for l in range(depth)])
        return counts, occ, n6
    return finish


def anchor_tree(ctx, points, num, den, depth):
    return anchor_tree_launch(ctx, points, num, den, depth)()


def anchor_expand(ctx, parents, occ, child_level, want_n6=True):
    """One decoder step on the device: parents (device uint64 keys of a level, ascending; None for the root), occ (numpy uint8, the
    level's decoded bytes) -> (child keys on the device, their n6 as numpy or None).  One copy in, one copy out."""
    dev = ctx.device
    occ = _u8(occ)
    if parents is None:
        parents = torch.zeros((1,), dtype=torch.int64, device=dev)
    npar = int(parents.shape[0])
    assert occ.shape == (npar,), 'anchor_expand: one occupancy byte per parent'
    nch = int(np.unpackbits(occ).sum())
    occ_d = torch.from_numpy(occ).to(dev)
    children = torch.empty((nch,), dtype=torch.int64, device=dev)
    n6 = torch.empty((nch,), dtype=torch.uint8, device=dev) if want_n6 else None
    ws = _workspace(ctx, lambda: L.lib().pcc_anchor_expand_workspace_bytes(npar))
    L.check(L.lib().pcc_anchor_expand(ctx.handle, _ptr(parents), _ptr(occ_d), npar, int(child_level), _ptr(children), nch, _ptr(n6), _ptr(ws),
                                      ctx.stream), 'pcc_anchor_expand')
    return children, (n6.cpu().numpy() if want_n6 else None)


def anchor_points(ctx, keys, num, den, resolution):
    """Leaf keys (device) -> the decoded (n,3) int32 points (numpy), in key order."""
    n = int(keys.shape[0])
    pts = torch.empty((n, 3), dtype=torch.int32, device=ctx.device)
    L.check(L.lib().pcc_anchor_points(ctx.handle, _ptr(keys), n, int(num), int(den), int(resolution), _ptr(pts), ctx.stream), 'pcc_anchor_points')
    return pts.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# surface anchor (include/pcc_geo.h "surface anchor"; the codec is anchor_surface.py)
# ---------------------------------------------------------------------------------------------
def surface_encode_vertices(edge_keys, flags, t, k):
    """The vertex payload: edge keys (n) uint64, flags (n) in {0, 1}, t (n) in [0, 2^k) -> bytes (host)."""
    keys, flags, t = np.ascontiguousarray(edge_keys, dtype=np.uint64), _u8(flags), _u8(t)
    assert keys.ndim == 1 and keys.shape == flags.shape == t.shape, 'surface_encode_vertices: one flag and one t per edge'
    return _encode_bytes('pcc_surface_encode_vertices', (keys.ctypes.data, flags.ctypes.data, t.ctypes.data, keys.size, int(k)),
                         8 * keys.size + 16)


def surface_decode_vertices(data, edge_keys, k):
    """-> (flags, t, set flags, bytes read) of a vertex payload over the given edge list (host); PccError when it ends early."""
    keys = np.ascontiguousarray(edge_keys, dtype=np.uint64)
    buf = np.frombuffer(bytes(data), np.uint8)
    flags, t = np.zeros(keys.size, np.uint8), np.zeros(keys.size, np.uint8)
    nflags, consumed = C.c_int64(), C.c_int64()
    L.check(L.lib().pcc_surface_decode_vertices(buf.ctypes.data if buf.size else None, buf.size, keys.ctypes.data, keys.size, int(k), flags.ctypes.data,
                                                t.ctypes.data, C.byref(nflags), C.byref(consumed)), 'pcc_surface_decode_vertices')
    return flags, t, nflags.value, consumed.value


def _surface_ws(ctx, name, n):
    nbytes = getattr(L.lib(), f'pcc_surface_{name}_workspace_bytes')(int(n))
    return _workspace(ctx, nbytes, f'surface_{name}: a count of {n} is outside the contract')


def _surface_hdr(ctx):
    return torch.zeros((L.PCC_SURFACE_HDR_WORDS,), dtype=torch.int64, device=ctx.device)


def surface_leaves(ctx, points, k):
    """int32 (n,3) numpy cloud already checked by the caller -> (Morton keys of its distinct points, leaf keys), device int64, ascending."""
    n = int(points.shape[0])
    pts_d = torch.from_numpy(points).to(ctx.device)
    pkeys = torch.empty((n,), dtype=torch.int64, device=ctx.device)
    leaves = torch.empty((n,), dtype=torch.int64, device=ctx.device)
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'leaves', n)
    L.check(L.lib().pcc_surface_leaves(ctx.handle, _ptr(pts_d), n, int(k), _ptr(hdr), _ptr(pkeys), _ptr(leaves), _ptr(ws), ctx.stream),
            'pcc_surface_leaves')
    ndistinct, nleaves = (int(v) for v in hdr.cpu()[:2])
    if not 1 <= nleaves <= ndistinct <= n:
        raise L.PccError(f'surface_leaves: {ndistinct} distinct points and {nleaves} leaves from {n} points')
    return pkeys[:ndistinct], leaves[:nleaves]


def surface_edges(ctx, leaf_keys):
    """Leaf keys (device int64, ascending) -> the edge list (device int64, ascending)."""
    n = int(leaf_keys.shape[0])
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'edges', n)
    edges = torch.empty((12 * n,), dtype=torch.int64, device=ctx.device)
    L.check(L.lib().pcc_surface_edges(ctx.handle, _ptr(leaf_keys), n, _ptr(hdr), _ptr(edges), _ptr(ws), ctx.stream), 'pcc_surface_edges')
    nedges = int(hdr.cpu()[0])
    if not 1 <= nedges <= 12 * n:
        raise L.PccError(f'surface_edges: {nedges} edges from {n} leaves')
    return edges[:nedges]


def surface_vertices(ctx, pkeys, k, edge_keys):
    """Distinct point keys and the edge list (device) -> (flags, t) per edge, numpy uint8."""
    n, nedges = int(pkeys.shape[0]), int(edge_keys.shape[0])
    out = torch.empty((2, nedges), dtype=torch.uint8, device=ctx.device)
    ws = _surface_ws(ctx, 'vertices', n)
    L.check(L.lib().pcc_surface_vertices(ctx.handle, _ptr(pkeys), n, int(k), _ptr(edge_keys), nedges, _ptr(out[0]), _ptr(out[1]), _ptr(ws),
                                         ctx.stream), 'pcc_surface_vertices')
    out = out.cpu().numpy()
    return out[0], out[1]


def surface_reconstruct(ctx, leaf_keys, edge_keys, flags, t, k, resolution, return_counts=False):
    """Leaves, edge list (device int64) and the vertices (numpy uint8 per edge) -> the decoded (n,3) int32 cloud (numpy), in Morton order.
    return_counts: -> (cloud, pos, total) with the count pass's pos (numpy int64: the first voxel of each leaf, before the clip and the
    final unique) and its total."""
    dev = ctx.device
    nleaves, nedges = int(leaf_keys.shape[0]), int(edge_keys.shape[0])
    flags, t = _u8(flags), _u8(t)
    assert flags.shape == t.shape == (nedges,), 'surface_reconstruct: one flag and one t per edge'
    ft = torch.from_numpy(np.stack([flags, t])).to(dev)
    pos = torch.empty((nleaves,), dtype=torch.int64, device=dev)
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'count', nleaves)
    L.check(L.lib().pcc_surface_count(ctx.handle, _ptr(leaf_keys), nleaves, _ptr(edge_keys), _ptr(ft[0]), _ptr(ft[1]), nedges, int(k), _ptr(pos),
                                      _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_surface_count')
    total = int(hdr.cpu()[0])
    if not nleaves <= total < 1 << 31:
        raise L.PccError(f'surface_reconstruct: {total} voxels from {nleaves} leaves')
    pts = torch.empty((total, 3), dtype=torch.int32, device=dev)
    ws = _surface_ws(ctx, 'reconstruct', total)
    L.check(L.lib().pcc_surface_reconstruct(ctx.handle, _ptr(leaf_keys), nleaves, _ptr(edge_keys), _ptr(ft[0]), _ptr(ft[1]), nedges, int(k),
                                            int(resolution), _ptr(pos), total, _ptr(pts), _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_surface_reconstruct')
    n = int(hdr.cpu()[0])
    if not 1 <= n <= total:
        raise L.PccError(f'surface_reconstruct: {n} distinct voxels of {total}')
    out = pts[:n].cpu().numpy()
    return (out, pos.cpu().numpy(), total) if return_counts else out


# ---------------------------------------------------------------------------------------------
# colour anchor (include/pcc_geo.h "colour anchor"; the codec is anchor_color.py)
# ---------------------------------------------------------------------------------------------
def _color_counts(counts):
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    assert counts.ndim == 1 and counts.size <= 63, 'colour anchor: one count per step, at most 63 steps'
    return counts


def color_anchor_encode_coefficients(coef, counts):
    """Coefficients (n,3) int16 in coding order and the per-step counts -> the payload bytes (host)."""
    coef, counts = np.ascontiguousarray(coef, dtype=np.int16), _color_counts(counts)
    assert coef.ndim == 2 and coef.shape[1] == 3, 'color_anchor_encode_coefficients: coefficients must be (n, 3)'
    n = coef.shape[0]                        # 48 bytes a coefficient always fit; the first try spares the memory
    return _encode_bytes('pcc_color_anchor_encode', (coef.ctypes.data, n, counts.ctypes.data, counts.size), 6 * n + 16, 48 * n + 16)


def color_anchor_decode_coefficients(data, counts, ncoef):
    """-> (coefficients (ncoef,3) int16, bytes read) of a payload (host); PccError when it is damaged or ends early."""
    counts = _color_counts(counts)
    buf = np.frombuffer(bytes(data), np.uint8)
    coef = np.zeros((int(ncoef), 3), np.int16)
    consumed = C.c_int64()
    L.check(L.lib().pcc_color_anchor_decode(buf.ctypes.data if buf.size else None, buf.size, counts.ctypes.data, counts.size, coef.ctypes.data,
                                            int(ncoef), C.byref(consumed)), 'pcc_color_anchor_decode')
    return coef, consumed.value


def _color_ws(ctx, n):
    return _workspace(ctx, L.lib().pcc_color_anchor_workspace_bytes(int(n)), f'color_anchor: {n} points are outside the contract')


def _color_hdr(raw, n):
    hdr = raw[:8 * L.PCC_COLOR_HDR_WORDS].view(np.int64)
    counts, dups = hdr[:64].copy(), int(hdr[64])
    if dups == 0 and (counts.min() < 0 or int(counts.sum()) != n - 1):
        raise L.PccError(f'color_anchor: the per-step counts sum to {int(counts.sum())} for {n} points')
    return counts, dups, hdr[65:68].copy()


def color_anchor_plan(ctx, points, depth):
    """int32 (n,3) numpy cloud already checked by the caller -> (the planned workspace for color_anchor_inverse (device), per-step
    counts int64[64], number of adjacent equal keys: nonzero = duplicate positions).  One copy back."""
    n = int(points.shape[0])
    pts_d = torch.from_numpy(points).to(ctx.device)
    hdr = torch.empty((L.PCC_COLOR_HDR_WORDS,), dtype=torch.int64, device=ctx.device)
    ws = _color_ws(ctx, n)
    L.check(L.lib().pcc_color_anchor_plan(ctx.handle, _ptr(pts_d), n, int(depth), _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_color_anchor_plan')
    counts, dups, _ = _color_hdr(hdr.cpu().numpy().view(np.uint8), n)
    return ws, counts, dups


def color_anchor_transform(ctx, points, colors, depth, qstep):
    """Plan and forward transform of an int32 (n,3) cloud and its uint8 (n,3) colours, both already checked by the caller ->
    (counts int64[64], adjacent equal keys, DC int64[3], coefficients (n - 1, 3) int16 in coding order).  Both calls are enqueued
    before the one copy back."""
    lib, dev = L.lib(), ctx.device
    n = int(points.shape[0])
    hdr_bytes = 8 * L.PCC_COLOR_HDR_WORDS
    pts_d, col_d = torch.from_numpy(points).to(dev), torch.from_numpy(colors).to(dev)
    out = torch.empty((hdr_bytes + 6 * (n - 1),), dtype=torch.uint8, device=dev)
    ws = _color_ws(ctx, n)
    base = out.data_ptr()
    L.check(lib.pcc_color_anchor_plan(ctx.handle, _ptr(pts_d), n, int(depth), C.c_void_p(base), _ptr(ws), ctx.stream), 'pcc_color_anchor_plan')
    L.check(lib.pcc_color_anchor_forward(ctx.handle, _ptr(col_d), n, int(depth), int(qstep), C.c_void_p(base),
                                         C.c_void_p(base + hdr_bytes) if n > 1 else None, _ptr(ws), ctx.stream), 'pcc_color_anchor_forward')
    raw = out.cpu().numpy()
    counts, dups, dc = _color_hdr(raw, n)
    return counts, dups, dc, raw[hdr_bytes:].view(np.int16).reshape(n - 1, 3).copy()


def color_anchor_inverse(ctx, plan, coef, dc, n, depth, qstep):
    """A workspace color_anchor_plan filled for the same n points, coefficients (n - 1, 3) int16 in coding order and the DC triple ->
    the (n,3) uint8 colours (numpy) in the row order of the planned points."""
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    assert coef.shape == (n - 1, 3), 'color_anchor_inverse: one coefficient triple per point but the first'
    coef_d = torch.from_numpy(coef).to(ctx.device) if n > 1 else None
    dc = np.ascontiguousarray(dc, dtype=np.int32)
    assert dc.shape == (3,), 'color_anchor_inverse: the DC is a triple'
    out = torch.empty((n, 3), dtype=torch.uint8, device=ctx.device)
    L.check(L.lib().pcc_color_anchor_inverse(ctx.handle, _ptr(coef_d), dc.ctypes.data, int(n), int(depth), int(qstep), _ptr(out), _ptr(plan),
                                             ctx.stream), 'pcc_color_anchor_inverse')
    return out.cpu().numpy()
