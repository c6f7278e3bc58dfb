"""Restatement of the octree anchor codec in pure Python and numpy, written from the specification; it shares no
code with the package: its own Morton keys (a bit loop), its own neighbour lookup (membership of linear cell ids, no binary
search), its own bit-at-a-time range coder.

Specification restated:
  quantisation   q = (2 p num + den) // (2 den); duplicates merged; decoder p = min((2 q den + num) // (2 num), resolution - 1);
  tree           D = bit_length(max q), at least 1; level l holds the distinct key >> 3 (D - l), ascending; key = per bit triple
                 x << 2 | y << 1 | z; occupancy bit c of a node = child c = 4 dx + 2 dy + dz is occupied;
  N6             bit 0 / 1 = the -x / +x face neighbour at the node's own level is occupied, 2 / 3 = -y / +y, 4 / 5 = -z / +z; outside
                 [0, 2^l) = empty;
  model rule     the byte is eight decisions, c = 0 .. 7; decision c uses model 256 t(c) + m: m = 1 at the start of a byte, then
                 m = 2 m + bit; t(c) = N6 bit (c >> 2 & 1) | N6 bit (2 + (c >> 1 & 1)) << 1 | N6 bit (4 + (c & 1)) << 2 -- the three
                 neighbours that share a face with child c's octant; after seven zeros the eighth decision is not coded;
  coder          LZMA's binary range coder: probability of a zero in 11 bits, 1024 at first, p += (2048 - p) >> 5 after a zero,
                 p -= p >> 5 after a one; 32-bit range, bound = (range >> 11) * p, normalised while below 2^24; carries through the
                 cache byte; five flush bytes; one run over all levels;
  stream         'PCOA', version 1 (uint8), resolution, num, den (uint32), D (uint8), quantised points (uint32), little endian,
                 then the payload.
"""
import struct

import numpy as np


# ---- coder
class RefEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size = 0, 0xffffffff, 0, 1
        self.out = bytearray()
        self.probs = {}
        self.carries = 0
        self.longest_pending = 0

    def _shift_low(self):
        if self.low < 0xff000000 or self.low >= 1 << 32:
            carry = self.low >> 32
            self.carries += carry
            self.longest_pending = max(self.longest_pending, self.cache_size - 1)
            self.out.append((self.cache + carry) & 0xff)
            for _ in range(self.cache_size - 1):
                self.out.append((0xff + carry) & 0xff)
            self.cache_size = 0
            self.cache = (self.low >> 24) & 0xff
        self.cache_size += 1
        self.low = (self.low & 0x00ffffff) << 8

    def encode(self, model, bit):
        p = self.probs.get(model, 1024)
        bound = (self.range >> 11) * p
        if bit == 0:
            self.range = bound
            p += (2048 - p) >> 5
        else:
            self.low += bound
            self.range -= bound
            p -= p >> 5
        self.probs[model] = p
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xffffffff
            self._shift_low()

    def finish(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


class RefDecoder:
    def __init__(self, data):
        self.data, self.pos = bytes(data), 0
        self.range, self.code = 0xffffffff, 0
        self.probs = {}
        if self._get() != 0:
            raise ValueError('first byte is not 0')
        for _ in range(4):
            self.code = self.code << 8 | self._get()

    def _get(self):
        if self.pos >= len(self.data):
            raise ValueError('the stream ends early')
        self.pos += 1
        return self.data[self.pos - 1]

    def decode(self, model):
        p = self.probs.get(model, 1024)
        bound = (self.range >> 11) * p
        if self.code < bound:
            self.range, bit = bound, 0
            p += (2048 - p) >> 5
        else:
            self.code -= bound
            self.range -= bound
            bit = 1
            p -= p >> 5
        self.probs[model] = p
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xffffffff
            self.code = ((self.code << 8) | self._get()) & 0xffffffff
        return bit


def code_bits(models, bits):
    e = RefEncoder()
    for m, b in zip(models, bits):
        e.encode(int(m), int(b))
    return e.finish(), e


def decode_bits(data, models):
    d = RefDecoder(data)
    return [d.decode(int(m)) for m in models]


# ---- tree
def quantise(p, num, den):
    return (2 * np.asarray(p, np.int64) * num + den) // (2 * den)


def dequantise(q, num, den, resolution):
    return np.minimum((2 * np.asarray(q, np.int64) * den + num) // (2 * num), resolution - 1)


def keys_of(q, depth):
    k = np.zeros(len(q), np.uint64)
    for b in range(depth):
        for a in range(3):                                   # x above y above z inside a triple
            k |= ((q[:, a].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return k


def coords_of(keys, depth):
    c = np.zeros((len(keys), 3), np.int64)
    for b in range(depth):
        for a in range(3):
            c[:, a] |= (((keys >> np.uint64(3 * b + 2 - a)) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return c


def tree(points, num, den):
    """-> (D, counts[D + 1], [occ of level l], [n6 of level l], leaf keys)."""
    q = quantise(points, num, den)
    depth = max(1, int(q.max()).bit_length())
    leaves = np.unique(keys_of(q, depth))
    counts, occs, n6s = [0] * (depth + 1), [None] * depth, [None] * depth
    counts[depth] = len(leaves)
    for level in range(depth):
        shift = np.uint64(3 * (depth - level))
        nodes = np.unique(leaves >> shift)
        counts[level] = len(nodes)
        children = np.unique(leaves >> np.uint64(3 * (depth - level - 1)))
        occ = np.zeros(len(nodes), np.int64)
        np.bitwise_or.at(occ, np.searchsorted(nodes, children >> np.uint64(3)), 1 << (children & np.uint64(7)).astype(np.int64))
        occs[level] = occ.astype(np.uint8)
        c = coords_of(nodes, max(level, 1))
        side = 1 << level
        ids = (c[:, 0] * side + c[:, 1]) * side + c[:, 2]
        n6 = np.zeros(len(nodes), np.int64)
        for f in range(6):
            d = c.copy()
            d[:, f // 2] += 1 if f % 2 else -1
            inside = (d[:, f // 2] >= 0) & (d[:, f // 2] < side)
            nid = (d[:, 0] * side + d[:, 1]) * side + d[:, 2]
            n6 |= (inside & np.isin(nid, ids)).astype(np.int64) << f
        n6s[level] = n6.astype(np.uint8)
    return depth, counts, occs, n6s, leaves


def t_of(n6, c):
    return (n6 >> (c >> 2 & 1) & 1) | (n6 >> (2 + (c >> 1 & 1)) & 1) << 1 | (n6 >> (4 + (c & 1)) & 1) << 2


def encode(points, resolution, num, den):
    depth, counts, occs, n6s, _ = tree(points, num, den)
    e = RefEncoder()
    for occ, n6 in zip(occs, n6s):
        for byte, nb in zip(occ.tolist(), n6.tolist()):
            m = 1
            for c in range(8):
                if c == 7 and m == 128:
                    break
                bit = byte >> c & 1
                e.encode(256 * t_of(nb, c) + m, bit)
                m = 2 * m + bit
    return struct.pack('<4sBIIIBI', b'PCOA', 1, resolution, num, den, depth, counts[depth]) + e.finish()


def reconstruction(points, resolution, num, den):
    """The decoded cloud as a sorted set of rows."""
    q = np.unique(quantise(points, num, den), axis=0)
    return np.unique(dequantise(q, num, den, resolution), axis=0)


def sorted_rows(a):
    a = np.asarray(a, np.int64)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


# ---- clouds
def small_clouds():
    """{name: (points, resolution)} -- the small cases of the CPU tests."""
    rng = np.random.default_rng(5)
    out = {'one_point': (np.array([[5, 0, 9]]), 16)}
    out['one_voxel'] = (np.array([[8, 8, 8], [8, 9, 8], [9, 9, 9], [9, 8, 8]]), 16)          # one voxel at scale 1/4
    g = np.arange(8)
    out['full_cube'] = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3), 8)
    top = 63
    corners = np.array([[x, y, z] for x in (0, top) for y in (0, top) for z in (0, top)])
    faces = rng.integers(0, top + 1, (120, 3))
    faces[np.arange(120), rng.integers(0, 3, 120)] = rng.choice([0, top], 120)
    out['faces_corners'] = (np.concatenate([corners, faces]), 64)
    u, v = rng.random(3000) * 100 + 10, rng.random(3000) * 100 + 10
    w = 64 + 20 * np.sin(u / 17) * np.cos(v / 23)
    out['patch'] = (np.round(np.stack([u, v, w], 1)).astype(np.int64), 128)
    return out
