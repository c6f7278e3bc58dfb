"""A conventional transform codec for the colours of a voxelised cloud: the attribute baseline of the experiment loop, beside the two
geometry anchors (anchor_octree.py, anchor_surface.py).

  python -m pcc_geo_cnn_v2_amd.anchor_color encode coloured.ply out.bin --qstep 8 [--device gpu|host]
  python -m pcc_geo_cnn_v2_amd.anchor_color decode out.bin geometry.ply out.ply [--device gpu|host]

It is NOT G-PCC and not RAHT-conformant: its streams are not TMC13 streams and its numbers are not comparable with published G-PCC
attribute numbers.  It is the same class of codec as G-PCC's RAHT (region-adaptive hierarchical transform) -- a weighted Haar
transform along the binary Morton tree of the geometry, uniform quantisation scaled by the weights, context-coded coefficients -- with
nothing external to install.  It is an open-loop integer lifting transform, not orthonormal, and it uses one step Q for luma and
chroma.  The decoder needs the geometry the encoder had.  DESIGN.md §4.17 holds the normative definition and the limits;
include/pcc_geo.h "colour anchor" the native entry points.

    encode(points, colors, qstep, device='gpu') -> bytes        decode(data, points, device='gpu') -> (N,3) uint8 colours

In short (integers only, // and >> floor): points are N pairwise distinct integer positions in [0, 2^21), colors (N,3) uint8 RGB, Q =
qstep in 1 .. 255 (1 is lossless).  Values are YCoCg-R triples.  Leaves are the points in ascending Morton order over D =
bit_length(max coordinate) bits.  Leaf i >= 1 owns one coefficient at step s = the highest bit of key[i - 1] ^ key[i]; with base =
key[i] >> (s + 1) << (s + 1), p0 = lower_bound(keys, base), p1 = lower_bound(keys, base + 2^(s + 1)), wL = i - p0, wR = p1 - i,
w = wL + wR, the encoder goes through the steps ascending: h = val[i] - val[p0], val[p0] += (wR h) // w; val[0] ends as the DC.
c = sgn(h) ((2 |h| + step) // (2 step)) with step = max(1, isqrt((Q Q w) // (wL wR))).  The decoder starts from the DC and goes through
the steps descending: aL = val[p0] - (wR c step) // w, val[p0] = aL, val[i] = aL + c step; then RGB, clipped.  Stream: the 17 bytes
'PCCA', version (1), Q, D (uint8), N (uint32), DC (three int16), little endian, then the payload of the octree anchor's binary coder
over the coefficients, steps descending, i ascending, channels Y, Co, Cg (binarisation: include/pcc_geo.h).

device='gpu' plans the tree and runs the transform in HIP (csrc/color_anchor.hip); device='host' does the same in numpy below, one
vector operation per step.  Both give the same bytes and the same decoded arrays; the entropy coder is the same host C++ either way.
A damaged stream raises AnchorStreamError from checks on the host; the device only sees counts derived from the geometry.
"""
import argparse
import struct
import sys

import numpy as np

from . import anchor_octree as A
from .anchor_octree import AnchorStreamError, check_device, check_points, depth_of, morton

MAGIC, VERSION = b'PCCA', 1
HEADER = struct.Struct('<4sBBBI3h')
DEVICES = A.DEVICES
STEPS = 64                                     # bins of the per-step counts (steps 0 .. 3 D - 1 <= 62 are used)
DC_RANGE = ((0, 255), (-255, 255), (-255, 255))


# ---- contract
def check_qstep(qstep):
    if isinstance(qstep, (bool, np.bool_)) or qstep != int(qstep) or not 1 <= int(qstep) <= 255:
        raise ValueError(f'anchor_color: qstep {qstep!r} outside [1, 255]')
    return int(qstep)


def check_colors(colors, n):
    c = np.asarray(colors)
    if c.dtype != np.uint8:
        raise ValueError(f'anchor_color: colors must be uint8, got {c.dtype}')
    if c.shape != (n, 3):
        raise ValueError(f'anchor_color: colors must be ({n}, 3), one RGB triple per point, got {c.shape}')
    return np.ascontiguousarray(c)


def _refuse_duplicates(dups):
    if dups:
        raise ValueError(f'anchor_color: the positions must be pairwise distinct ({int(dups)} adjacent equal keys)')


# ---- colour space
def rgb_to_ycocg(rgb):
    c = np.asarray(rgb).astype(np.int64)
    co = c[:, 0] - c[:, 2]
    t = c[:, 2] + (co >> 1)
    cg = c[:, 1] - t
    return np.stack([t + (cg >> 1), co, cg], axis=1)


def ycocg_to_rgb(val):
    t = val[:, 0] - (val[:, 2] >> 1)
    g = val[:, 2] + t
    b = t - (val[:, 1] >> 1)
    return np.clip(np.stack([b + val[:, 1], g, b], axis=1), 0, 255).astype(np.uint8)


# ---- the numpy host path
def _top_bit(x):
    """Index of the highest set bit of every (nonzero) uint64."""
    x = x.copy()
    d = np.zeros(len(x), np.int64)
    for shift in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(shift)) != 0
        d += shift * m
        x = np.where(m, x >> np.uint64(shift), x)
    return d


def _isqrt(x):
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r -= r * r > x
    r += (r + 1) * (r + 1) <= x
    return r


class HostPlan:
    """The tree of a cloud: rows (leaf -> the caller's row), keys, the leaves ordered by step and the per-step counts."""

    def __init__(self, p):
        keys = morton(p[:, 0], p[:, 1], p[:, 2])
        self.n, self.depth = len(p), depth_of(p.max())
        self.rows = np.argsort(keys, kind='stable')
        self.keys = keys[self.rows]
        x = self.keys[1:] ^ self.keys[:-1]
        _refuse_duplicates(int((x == 0).sum()))
        d = _top_bit(x)
        self.order = np.argsort(d, kind='stable') + 1
        self.counts = np.bincount(d, minlength=STEPS).astype(np.int64)
        self.off = np.concatenate(([0], np.cumsum(self.counts)))

    def step(self, s, q):
        """-> (i, p0, wR, w, quantiser step, first place in coding order) of the leaves of step s, i ascending."""
        i = self.order[self.off[s]:self.off[s + 1]]
        base = (self.keys[i] >> np.uint64(s + 1)) << np.uint64(s + 1)
        p0 = np.searchsorted(self.keys, base)
        p1 = np.searchsorted(self.keys, base + (np.uint64(1) << np.uint64(s + 1)))
        wl, wr = i - p0, p1 - i
        w = wl + wr
        return i, p0, wr, w, np.maximum(1, _isqrt((q * q * w) // (wl * wr))), self.n - 1 - self.off[s + 1]


def forward_host(plan, colors, q):
    """-> (DC triple, coefficients (N - 1, 3) int16 in coding order)."""
    val = rgb_to_ycocg(colors[plan.rows])
    coef = np.zeros((plan.n - 1, 3), np.int16)
    for s in range(3 * plan.depth):
        if plan.counts[s] == 0:
            continue
        i, p0, wr, w, step, pos = plan.step(s, q)
        h = val[i] - val[p0]
        val[p0] += (wr[:, None] * h) // w[:, None]
        coef[pos:pos + len(i)] = np.sign(h) * ((2 * np.abs(h) + step[:, None]) // (2 * step[:, None]))
    return val[0].copy(), coef


def inverse_host(plan, dc, coef, q):
    """-> (N,3) uint8 colours in the caller's row order."""
    val = np.zeros((plan.n, 3), np.int64)
    val[0] = dc
    coef = np.asarray(coef).astype(np.int64)
    for s in range(3 * plan.depth - 1, -1, -1):
        if plan.counts[s] == 0:
            continue
        i, p0, wr, w, step, pos = plan.step(s, q)
        h = coef[pos:pos + len(i)] * step[:, None]
        left = val[p0] - (wr[:, None] * h) // w[:, None]
        val[p0] = left
        val[i] = left + h
    out = np.empty((plan.n, 3), np.uint8)
    out[plan.rows] = ycocg_to_rgb(val)
    return out


# ---- the codec
def _ctx(ctx):
    from . import ops
    return ctx if ctx is not None else ops.get_context()


def _forward(p, colors, q, device, ctx):
    """-> (depth, counts[STEPS], DC, coefficients)."""
    from . import ops
    if device == 'host':
        plan = HostPlan(p)
        dc, coef = forward_host(plan, colors, q)
        return plan.depth, plan.counts, dc, coef
    depth = depth_of(p.max())
    counts, dups, dc, coef = ops.color_anchor_transform(_ctx(ctx), np.ascontiguousarray(p, dtype=np.int32), colors, depth, q)
    _refuse_duplicates(dups)
    return depth, counts, dc, coef


def coefficients(points, colors, qstep, device='gpu', ctx=None):
    """What the encoder hands its coder: (per-step counts int64[64], DC int64[3], coefficients (N - 1, 3) int16 in coding order) --
    tests and the timing tool."""
    check_device(device)
    p, q = check_points(points), check_qstep(qstep)
    _, counts, dc, coef = _forward(p, check_colors(colors, len(p)), q, device, ctx)
    return counts, np.asarray(dc, np.int64), coef


def encode(points, colors, qstep, device='gpu', ctx=None):
    """See the module docstring."""
    from . import ops
    check_device(device)
    p, q = check_points(points), check_qstep(qstep)
    if len(p) >= 1 << 31:
        raise ValueError('anchor_color: at most 2^31 - 1 points')
    depth, counts, dc, coef = _forward(p, check_colors(colors, len(p)), q, device, ctx)
    assert int(counts.sum()) == len(p) - 1 and not counts[3 * depth:].any(), 'anchor_color: the per-step counts do not add up'
    return HEADER.pack(MAGIC, VERSION, q, depth, len(p), *(int(v) for v in dc)) + ops.color_anchor_encode_coefficients(coef, counts[:3 * depth])


def reconstruct(points, colors, qstep):
    """The colours a decoder returns for encode(points, colors, qstep): the encoder's own reconstruction, without coding (numpy)."""
    p, q = check_points(points), check_qstep(qstep)
    plan = HostPlan(p)
    dc, coef = forward_host(plan, check_colors(colors, len(p)), q)
    return inverse_host(plan, dc, coef, q)


def read_header(data):
    """-> dict(qstep, depth, points, dc) of a stream; AnchorStreamError for anything that is not one."""
    data = bytes(data)
    if len(data) < HEADER.size:
        raise AnchorStreamError(f'anchor_color: {len(data)} bytes are shorter than the header')
    magic, version, q, depth, n, *dc = HEADER.unpack_from(data)
    if magic != MAGIC:
        raise AnchorStreamError(f'anchor_color: magic {magic!r}, not {MAGIC!r}')
    if version != VERSION:
        raise AnchorStreamError(f'anchor_color: stream version {version}, this decoder reads {VERSION}')
    if q == 0:
        raise AnchorStreamError('anchor_color: qstep 0')
    if not (1 <= depth <= 21 and 1 <= n < 1 << 31):
        raise AnchorStreamError(f'anchor_color: header fields out of range: depth {depth}, {n} points')
    if not all(lo <= v <= hi for v, (lo, hi) in zip(dc, DC_RANGE)):
        raise AnchorStreamError(f'anchor_color: DC {tuple(dc)} outside Y [0, 255], Co, Cg [-255, 255]')
    return dict(qstep=q, depth=depth, points=n, dc=tuple(dc))


def decode(data, points, device='gpu', ctx=None):
    """The colours of `points` (the geometry the encoder had, in any row order), one row per row of `points`."""
    from . import _lib, ops
    check_device(device)
    data = bytes(data)
    h = read_header(data)
    p = check_points(points)
    depth = depth_of(p.max())
    if (depth, len(p)) != (h['depth'], h['points']):
        raise AnchorStreamError(f"anchor_color: the stream is for {h['points']} points of depth {h['depth']}, the geometry has {len(p)} "
                                f'of depth {depth}')
    q = h['qstep']
    if device == 'gpu':
        ctx = _ctx(ctx)
        plan, counts, dups = ops.color_anchor_plan(ctx, np.ascontiguousarray(p, dtype=np.int32), depth)
        _refuse_duplicates(dups)
    else:
        plan = HostPlan(p)
        counts = plan.counts
    payload = data[HEADER.size:]
    try:
        coef, consumed = ops.color_anchor_decode_coefficients(payload, counts[:3 * depth], len(p) - 1)
    except _lib.PccError as e:
        raise AnchorStreamError(f'anchor_color: damaged stream: {e}') from None
    if consumed != len(payload):
        raise AnchorStreamError(f'anchor_color: {len(payload) - consumed} bytes left behind the last coefficient')
    if device == 'gpu':
        return ops.color_anchor_inverse(ctx, plan, coef, h['dc'], len(p), depth, q)
    return inverse_host(plan, np.array(h['dc'], np.int64), coef, q)


def build_parser():
    p = argparse.ArgumentParser(prog='anchor_color', description='Colour anchor codec: a conventional transform baseline for the colours of any '
                                'voxelised cloud.  Not G-PCC, not RAHT-conformant.', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = p.add_subparsers(dest='command', required=True)
    e = sub.add_parser('encode', help='coloured PLY -> colour stream')
    e.add_argument('input_pc', help='A PLY with red, green and blue')
    e.add_argument('output')
    e.add_argument('--qstep', type=int, required=True, help='Quantiser step, 1 .. 255; 1 is lossless')
    d = sub.add_parser('decode', help='colour stream + geometry -> coloured PLY')
    d.add_argument('input')
    d.add_argument('geometry_pc', help='The PLY whose positions the encoder had (its own colours, if any, are ignored)')
    d.add_argument('output_pc')
    for s in (e, d):
        s.add_argument('--device', choices=DEVICES, default='gpu', help='Where the tree is planned and the transform runs')
    return p


def main(argv=None):
    from .utils import pc_io
    a = build_parser().parse_args(argv)
    if a.device == 'gpu':
        from . import want_hw_queues
        want_hw_queues()
    if a.command == 'encode':
        data = encode(pc_io.load_pc(a.input_pc), pc_io.load_colors(a.input_pc), a.qstep, a.device)
        with open(a.output, 'wb') as f:
            f.write(data)
    else:
        pts = pc_io.load_pc(a.geometry_pc)
        with open(a.input, 'rb') as f:
            colors = decode(f.read(), pts, a.device)
        pc_io.write_df(a.output_pc, pc_io.pa_to_df(np.concatenate([np.asarray(pts, np.float64), colors], axis=1)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
