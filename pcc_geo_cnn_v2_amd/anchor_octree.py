"""A conventional octree geometry codec that runs on any voxelised cloud: the rate-distortion baseline of the experiment loop.

  python -m pcc_geo_cnn_v2_amd.anchor_octree encode in.ply out.bin --resolution 1024 --scale 1/2 [--device gpu|host]
  python -m pcc_geo_cnn_v2_amd.anchor_octree decode out.bin out.ply [--device gpu|host]

It is NOT G-PCC: its streams are not TMC13 streams and its numbers are not comparable with published G-PCC numbers.  It is the
same class of codec as the "G-PCC octree" curve of the paper -- quantise, prune, code the occupancy bytes of the octree with
neighbour-dependent contexts -- with nothing external to install (include/pcc_geo.h "octree anchor").

    encode(points, resolution, scale=(num, den), device='gpu') -> bytes        decode(data, device='gpu') -> (M,3) int32 points

Quantisation, integer exact: q = (2 p num + den) // (2 den) per coordinate, duplicates merged; the decoder returns
min((2 q den + num) // (2 num), resolution - 1), in the Morton order of q.  num == den is lossless.  Tree: depth D =
bit_length(max q) (at least 1), breadth first, the nodes of a level in this repository's Morton order (x << 2 | y << 1 | z);
occupancy bit c of a node = child c = 4 dx + 2 dy + dz.  Contexts and coder: include/pcc_geo.h.  Stream: the 22 bytes
'PCOA', version (1), resolution, num, den (uint32), D (uint8), number of quantised points (uint32), little endian, then the
payload of the range coder.

device='gpu' builds the tree and its contexts (encoder) or expands the levels (decoder) in HIP (csrc/octree_anchor.hip);
device='host' does the same in numpy below.  Both give the same bytes and the same decoded arrays; the entropy coder is the same
host C++ either way (csrc/anchor_coder.cpp).  A damaged stream raises AnchorStreamError from checks on the host; nothing malformed
reaches the device.
"""
import argparse
import struct
import sys
from fractions import Fraction

import numpy as np

MAGIC, VERSION = b'PCOA', 1
HEADER = struct.Struct('<4sBIIIBI')
COORD_LIMIT = 1 << 21
DEVICES = ('gpu', 'host')


class AnchorStreamError(ValueError):
    """A stream that is not one of this codec's, or is cut or damaged."""


# ---- contract
def check_points(points):
    """-> (n,3) int64.  Refuses an empty cloud, non-integer values and coordinates outside [0, 2^21)."""
    a = np.asarray(points)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError(f'anchor_octree: points must be (N, 3) with N >= 1, got {a.shape}')
    if a.shape[0] >= 1 << 31:
        raise ValueError('anchor_octree: at most 2^31 - 1 points')
    if a.dtype.kind == 'f':
        if not np.isfinite(a).all() or not np.array_equal(a, np.round(a)):
            raise ValueError('anchor_octree: coordinates must be integers (a voxelised cloud)')
    elif a.dtype.kind not in 'iu':
        raise ValueError(f'anchor_octree: unsupported dtype {a.dtype}')
    if (a < 0).any() or (a >= COORD_LIMIT).any():
        raise ValueError(f'anchor_octree: coordinates must lie in [0, {COORD_LIMIT})')
    return a.astype(np.int64)


def check_scale(scale):
    """(num, den), 'num/den', a Fraction or 1 -> (num, den) as given (not reduced), 0 < num <= den < 2^31."""
    if isinstance(scale, str):
        parts = scale.split('/')
        scale = (int(parts[0]), int(parts[1]) if len(parts) > 1 else 1) if len(parts) <= 2 else None
    elif isinstance(scale, Fraction):
        scale = (scale.numerator, scale.denominator)
    elif isinstance(scale, (int, np.integer)):
        scale = (int(scale), 1)
    try:
        num, den = scale
        ok = num == int(num) and den == int(den)
    except (TypeError, ValueError):
        ok = False
    if not ok or not 0 < int(num) <= int(den) < 1 << 31:
        raise ValueError(f'anchor_octree: scale {scale!r}: need integers num / den with 0 < num <= den < 2^31')
    return int(num), int(den)


def check_resolution(resolution):
    if resolution != int(resolution) or not 1 <= int(resolution) <= COORD_LIMIT:
        raise ValueError(f'anchor_octree: resolution {resolution!r} outside [1, {COORD_LIMIT}]')
    return int(resolution)


def check_device(device):
    if device not in DEVICES:
        raise ValueError(f'anchor_octree: device must be one of {DEVICES}, got {device!r}')


def quantise(p, num, den):
    return (2 * np.asarray(p, np.int64) * num + den) // (2 * den)


def dequantise(q, num, den, resolution):
    return np.minimum((2 * np.asarray(q, np.int64) * den + num) // (2 * num), resolution - 1)


# ---- Morton keys (cell_index.h's order)
_SPREAD = ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249))


def _spread3(v):
    x = np.asarray(v).astype(np.uint64)
    for s, m in _SPREAD:
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def _compact3(k):
    x = np.asarray(k, np.uint64) & np.uint64(0x1249249249249249)
    for s, m in ((2, 0x10c30c30c30c30c3), (4, 0x100f00f00f00f00f), (8, 0x1f0000ff0000ff), (16, 0x1f00000000ffff), (32, 0x1fffff)):
        x = (x | (x >> np.uint64(s))) & np.uint64(m)
    return x.astype(np.int64)


def morton(x, y, z):
    return (_spread3(x) << np.uint64(2)) | (_spread3(y) << np.uint64(1)) | _spread3(z)


def unmorton(keys):
    k = np.asarray(keys, np.uint64)
    return np.stack([_compact3(k >> np.uint64(2)), _compact3(k >> np.uint64(1)), _compact3(k)], axis=1)


def depth_of(qmax):
    return max(1, int(qmax).bit_length())


# ---- the numpy host path
def n6_host(keys, level):
    """Face-neighbour mask of every node of one level (keys ascending): bit 0 / 1 = -x / +x, 2 / 3 = -y / +y, 4 / 5 = -z / +z."""
    xyz = unmorton(keys)
    out = np.zeros(len(keys), np.uint8)
    top = (1 << level) - 1
    for f in range(6):
        c = xyz.copy()
        c[:, f >> 1] += 1 if f & 1 else -1
        inside = (c[:, f >> 1] >= 0) & (c[:, f >> 1] <= top)
        c = np.clip(c, 0, top)
        nk = morton(c[:, 0], c[:, 1], c[:, 2])
        pos = np.minimum(np.searchsorted(keys, nk), len(keys) - 1)
        out |= ((inside & (keys[pos] == nk)).astype(np.uint8) << np.uint8(f))
    return out


def tree_host(q, depth):
    """(n,3) quantised points -> (counts[depth + 1], occ, n6): nodes per level with the leaves last, bytes of all levels breadth first."""
    keys = np.unique(morton(q[:, 0], q[:, 1], q[:, 2]))
    counts, occ, n6 = np.zeros(depth + 1, np.int64), [None] * depth, [None] * depth
    counts[depth] = len(keys)
    for level in range(depth - 1, -1, -1):
        parent = keys >> np.uint64(3)
        start = np.flatnonzero(np.concatenate(([True], parent[1:] != parent[:-1])))
        occ[level] = np.bitwise_or.reduceat((np.uint8(1) << (keys & np.uint64(7)).astype(np.uint8)), start)
        keys = parent[start]
        counts[level] = len(keys)
        n6[level] = n6_host(keys, level)
    return counts, np.concatenate(occ), np.concatenate(n6)


def expand_host(parents, occ):
    """Child keys of one level, ascending."""
    bits = np.unpackbits(occ[:, None], axis=1, bitorder='little')
    idx, child = np.nonzero(bits)
    return (parents[idx] << np.uint64(3)) | child.astype(np.uint64)


# ---- the codec
def _ctx(ctx):
    from . import ops
    return ctx if ctx is not None else ops.get_context()


def encode_launch(points, resolution, scale=(1, 1), device='gpu', ctx=None, no_context=False):
    """encode() in two halves: everything up to the enqueued device work and its one copy back, then a function that waits, runs
    the host coder and returns the bytes.  With device='host' the first half does the numpy tree."""
    from . import ops
    check_device(device)
    p, resolution = check_points(points), check_resolution(resolution)
    num, den = check_scale(scale)
    depth = depth_of(quantise(p.max(), num, den))
    if device == 'gpu':
        pending = ops.anchor_tree_launch(_ctx(ctx), np.ascontiguousarray(p, dtype=np.int32), num, den, depth)
    else:
        tree = tree_host(quantise(p, num, den), depth)
        pending = lambda: tree

    def finish():
        counts, occ, n6 = pending()
        payload = ops.anchor_encode_nodes(occ, n6, no_context=no_context)
        return HEADER.pack(MAGIC, VERSION, resolution, num, den, depth, int(counts[depth])) + payload
    return finish


def encode(points, resolution, scale=(1, 1), device='gpu', ctx=None, no_context=False):
    """See the module docstring.  no_context=True codes every byte with neighbour mask 0 (the measurement of what the contexts gain:
    such a stream decodes only with decode(..., no_context=True))."""
    return encode_launch(points, resolution, scale, device, ctx, no_context)()


def tree(points, scale=(1, 1), device='gpu', ctx=None):
    """What the encoder hands its coder: (counts[D + 1], occ, n6) -- tests and the timing tool."""
    from . import ops
    check_device(device)
    p = check_points(points)
    num, den = check_scale(scale)
    depth = depth_of(quantise(p.max(), num, den))
    if device == 'gpu':
        return ops.anchor_tree(_ctx(ctx), np.ascontiguousarray(p, dtype=np.int32), num, den, depth)
    return tree_host(quantise(p, num, den), depth)


def reconstruct(points, resolution, scale=(1, 1)):
    """The cloud a decoder returns for encode(points, resolution, scale), from the definition alone (numpy)."""
    p, resolution = check_points(points), check_resolution(resolution)
    num, den = check_scale(scale)
    q = quantise(p, num, den)
    return dequantise(unmorton(np.unique(morton(q[:, 0], q[:, 1], q[:, 2]))), num, den, resolution).astype(np.int32)


def read_header(data):
    """-> dict(resolution, num, den, depth, points) of a stream; AnchorStreamError for anything that is not one."""
    data = bytes(data)
    if len(data) < HEADER.size:
        raise AnchorStreamError(f'anchor_octree: {len(data)} bytes are shorter than the header')
    magic, version, resolution, num, den, depth, npoints = HEADER.unpack_from(data)
    if magic != MAGIC:
        raise AnchorStreamError(f'anchor_octree: magic {magic!r}, not {MAGIC!r}')
    if version != VERSION:
        raise AnchorStreamError(f'anchor_octree: stream version {version}, this decoder reads {VERSION}')
    if not (1 <= resolution <= COORD_LIMIT and 0 < num <= den < 1 << 31 and 1 <= depth <= 21 and 1 <= npoints < 1 << 31 and
            npoints <= 8 ** depth):
        raise AnchorStreamError(f'anchor_octree: header fields out of range: resolution {resolution}, scale {num}/{den}, depth {depth}, '
                                f'{npoints} points')
    return dict(resolution=resolution, num=num, den=den, depth=depth, points=npoints)


def decode(data, device='gpu', ctx=None, no_context=False):
    from . import _lib, ops
    check_device(device)
    data = bytes(data)
    h = read_header(data)
    depth, npoints = h['depth'], h['points']
    try:
        dec = ops.AnchorDecoder(data[HEADER.size:], no_context=no_context)
        keys, n6 = None, np.zeros(1, np.uint8)             # the root: one node, no neighbours
        if device == 'host':
            keys = np.zeros(1, np.uint64)
        else:
            ctx = _ctx(ctx)
        for level in range(depth):
            occ = dec.level(n6)
            nch = int(np.unpackbits(occ).sum())
            if nch > npoints:                              # every node holds a point: a level cannot outgrow the cloud
                raise AnchorStreamError(f'anchor_octree: level {level + 1} has {nch} nodes, the header says {npoints} points')
            last = level + 1 == depth
            if device == 'host':
                keys = expand_host(keys, occ)
                n6 = None if last else n6_host(keys, level + 1)
            else:
                keys, n6 = ops.anchor_expand(ctx, keys, occ, level + 1, want_n6=not last)
    except _lib.PccError as e:
        raise AnchorStreamError(f'anchor_octree: damaged stream: {e}') from None
    if int(keys.shape[0]) != npoints:
        raise AnchorStreamError(f'anchor_octree: decoded {int(keys.shape[0])} points, the header says {npoints}')
    if dec.consumed != len(dec):
        raise AnchorStreamError(f'anchor_octree: {len(dec) - dec.consumed} bytes left behind the last level')
    if device == 'host':
        return dequantise(unmorton(keys), h['num'], h['den'], h['resolution']).astype(np.int32)
    return ops.anchor_points(ctx, keys, h['num'], h['den'], h['resolution'])


def build_parser():
    p = argparse.ArgumentParser(prog='anchor_octree', description='Octree anchor codec: a conventional geometry baseline for any voxelised '
                                'cloud.  Not G-PCC: its streams are not TMC13 streams.', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = p.add_subparsers(dest='command', required=True)
    e = sub.add_parser('encode', help='PLY -> stream')
    e.add_argument('input_pc')
    e.add_argument('output')
    e.add_argument('--resolution', type=int, required=True, help='Size of the voxel grid (1024 for a vox10 cloud)')
    e.add_argument('--scale', default='1/1', help='Quantisation scale num/den, 0 < num <= den; 1/1 is lossless')
    d = sub.add_parser('decode', help='stream -> PLY')
    d.add_argument('input')
    d.add_argument('output_pc')
    for s in (e, d):
        s.add_argument('--device', choices=DEVICES, default='gpu', help='Where the tree and its contexts are computed')
    return p


def main(argv=None):
    from .utils import pc_io
    a = build_parser().parse_args(argv)
    if a.device == 'gpu':
        from . import want_hw_queues
        want_hw_queues()
    if a.command == 'encode':
        data = encode(pc_io.load_pc(a.input_pc), a.resolution, a.scale, a.device)
        with open(a.output, 'wb') as f:
            f.write(data)
    else:
        with open(a.input, 'rb') as f:
            pts = decode(f.read(), a.device)
        pc_io.write_df(a.output_pc, pc_io.pa_to_df(pts))
    return 0


if __name__ == '__main__':
    sys.exit(main())
