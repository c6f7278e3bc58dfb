"""Restatement of the colour anchor codec in pure Python, written from the specification; it shares no code with
the package: an explicit recursive tree of nodes split one key bit at a time (not the highest-differing-bit shortcut), its own bit
loop for the Morton keys, Python integers throughout, and the bit-at-a-time range coder of tests/_anchor_ref.py.

Specification restated:
  colour space   Co = R - B, t = B + (Co >> 1), Cg = G - t, Y = t + (Cg >> 1); back: t = Y - (Cg >> 1), G = Cg + t, B = t - (Co >> 1),
                 R = B + Co;
  tree           leaves = the points by ascending key (per bit triple x << 2 | y << 1 | z over D = max(1, bit_length(max coordinate))
                 bits); a node over key bit b holds the leaves that agree above b; where both halves (bit b = 0 / 1) are occupied they
                 are its two children and the node is an inner node of step b, else it is the node over bit b - 1 of the same leaves;
  forward        bottom up: an inner node's value is aL + (wR h) // w, h = aR - aL, weights = leaf counts; the root's value is the DC;
  quantiser      step = max(1, isqrt((Q Q w) // (wL wR))), c = sgn(h) ((2 |h| + step) // (2 step));
  inverse        top down: aL = a - (wR c step) // w, aR = aL + c step; RGB clipped to [0, 255];
  coding order   steps descending, inside a step by the first leaf of the right child ascending, channels Y, Co, Cg;
  binarisation   g = 2 min(step // 3, 7) + (channel != Y); zero flag under 32 g + z (z = previous coefficient of the channel nonzero),
                 sign under 32 g + 2, v = |c|: n = bit_length(v) - 1 ones then a zero under 32 g + 3 + j, the n low bits of v MSB
                 first under 32 g + 12 + j; a ninth one is a damaged stream;
  stream         'PCCA', version 1, Q, D (uint8), N (uint32), DC (three int16), little endian, then the payload.
"""
import math
import struct
import sys

import numpy as np

from _anchor_ref import RefDecoder, RefEncoder

sys.setrecursionlimit(10000)


def key_of(p, depth):
    k = 0
    for b in range(depth):
        for a in range(3):
            k |= ((int(p[a]) >> b) & 1) << (3 * b + 2 - a)
    return k


def to_ycocg(rgb):
    r, g, b = (int(v) for v in rgb)
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    return [t + (cg >> 1), co, cg]


def to_rgb(val):
    y, co, cg = val
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    return [min(255, max(0, v)) for v in (b + co, g, b)]


class Node:
    def __init__(self, first, weight, step=None, left=None, right=None):
        self.first, self.weight, self.step, self.left, self.right = first, weight, step, left, right
        self.val, self.coef = None, None


def build(keys, lo, hi, bit):
    """The node of leaves lo .. hi - 1, which agree above `bit`."""
    if hi - lo == 1:
        return Node(lo, 1)
    assert bit >= 0, 'duplicate positions'
    split = lo
    while split < hi and not (keys[split] >> bit) & 1:
        split += 1
    if split == lo or split == hi:
        return build(keys, lo, hi, bit - 1)
    return Node(lo, hi - lo, bit, build(keys, lo, split, bit - 1), build(keys, split, hi, bit - 1))


def qstep_of(q, wl, wr):
    return max(1, math.isqrt((q * q * (wl + wr)) // (wl * wr)))


def analyse(node, leaf_vals, q):
    if node.step is None:
        node.val = list(leaf_vals[node.first])
        return
    analyse(node.left, leaf_vals, q)
    analyse(node.right, leaf_vals, q)
    wl, wr = node.left.weight, node.right.weight
    step = qstep_of(q, wl, wr)
    node.val, node.coef = [], []
    for al, ar in zip(node.left.val, node.right.val):
        h = ar - al
        node.val.append(al + (wr * h) // (wl + wr))
        mag = (2 * abs(h) + step) // (2 * step)
        node.coef.append(-mag if h < 0 else mag)


def synthesise(node, val, q, leaf_vals):
    if node.step is None:
        leaf_vals[node.first] = val
        return
    wl, wr = node.left.weight, node.right.weight
    step = qstep_of(q, wl, wr)
    left, right = [], []
    for a, c in zip(val, node.coef):
        h = c * step
        left.append(a - (wr * h) // (wl + wr))
        right.append(left[-1] + h)
    synthesise(node.left, left, q, leaf_vals)
    synthesise(node.right, right, q, leaf_vals)


def inner_nodes(root):
    """In coding order."""
    out, stack = [], [root]
    while stack:
        n = stack.pop()
        if n.step is not None:
            out.append(n)
            stack += [n.left, n.right]
    return sorted(out, key=lambda n: (-n.step, n.right.first))


def tree_of(points):
    pts = [[int(v) for v in p] for p in np.asarray(points)]
    depth = max(1, max(max(p) for p in pts).bit_length())
    keys = [key_of(p, depth) for p in pts]
    rows = sorted(range(len(pts)), key=lambda r: keys[r])
    skeys = [keys[r] for r in rows]
    return depth, rows, build(skeys, 0, len(rows), 3 * depth - 1)


def group(step, ch):
    return 2 * min(step // 3, 7) + (ch != 0)


def code_coefficients(items):
    """items: [(step, (cY, cCo, cCg))] in coding order -> bytes."""
    e = RefEncoder()
    prev = [0, 0, 0]
    for step, triple in items:
        for ch, c in enumerate(triple):
            m, v = 32 * group(step, ch), abs(c)
            e.encode(m + prev[ch], int(v != 0))
            prev[ch] = int(v != 0)
            if v == 0:
                continue
            e.encode(m + 2, int(c < 0))
            n = v.bit_length() - 1
            assert n <= 8
            for j in range(n):
                e.encode(m + 3 + j, 1)
            e.encode(m + 3 + n, 0)
            for j in range(n):
                e.encode(m + 12 + j, v >> (n - 1 - j) & 1)
    return e.finish()


def decode_coefficients(data, steps):
    """steps: the step of every coefficient in coding order -> ([(cY, cCo, cCg)], bytes read)."""
    d = RefDecoder(data)
    prev = [0, 0, 0]
    out = []
    for step in steps:
        triple = []
        for ch in range(3):
            m, c = 32 * group(step, ch), 0
            prev[ch] = d.decode(m + prev[ch])
            if prev[ch]:
                neg, n = d.decode(m + 2), 0
                while d.decode(m + 3 + n):
                    n += 1
                    if n > 8:
                        raise ValueError('a ninth one-bit')
                v = 1
                for j in range(n):
                    v = 2 * v + d.decode(m + 12 + j)
                c = -v if neg else v
            triple.append(c)
        out.append(tuple(triple))
    return out, d.pos


def encode(points, colors, q):
    depth, rows, root = tree_of(points)
    analyse(root, [to_ycocg(colors[r]) for r in rows], q)
    nodes = inner_nodes(root)
    return struct.pack('<4sBBBI3h', b'PCCA', 1, q, depth, len(rows), *root.val) + code_coefficients([(n.step, n.coef) for n in nodes])


def coefficients(points, colors, q):
    """-> (per-step counts [64], DC, [(cY, cCo, cCg)] in coding order)."""
    _, rows, root = tree_of(points)
    analyse(root, [to_ycocg(colors[r]) for r in rows], q)
    nodes = inner_nodes(root)
    counts = [0] * 64
    for n in nodes:
        counts[n.step] += 1
    return counts, root.val, [tuple(n.coef) for n in nodes]


def decode(data, points):
    magic, version, q, depth, n, *dc = struct.unpack_from('<4sBBBI3h', data)
    assert (magic, version) == (b'PCCA', 1)
    d, rows, root = tree_of(points)
    assert (d, len(rows)) == (depth, n)
    nodes = inner_nodes(root)
    coefs, used = decode_coefficients(data[17:], [nd.step for nd in nodes])
    assert used == len(data) - 17
    for nd, c in zip(nodes, coefs):
        nd.coef = c
    leaf_vals = [None] * n
    synthesise(root, dc, q, leaf_vals)
    out = np.zeros((n, 3), np.uint8)
    for leaf, r in enumerate(rows):
        out[r] = to_rgb(leaf_vals[leaf])
    return out


# ---- clouds
def shell(res=64, seed=3):
    """About 5 000 distinct voxels of a sphere shell in a res^3 grid."""
    g = np.arange(res)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    r = np.sqrt((x - res / 2 + 0.5) ** 2 + (y - res / 2 + 0.5) ** 2 + (z - res / 2 + 0.5) ** 2)
    pts = np.argwhere(np.abs(r - res * 0.32) < 0.5)
    return np.random.default_rng(seed).permutation(pts)


def smooth_colors(points, scale=64.0):
    p = np.asarray(points, np.float64) / scale
    c = np.stack([128 + 100 * np.sin(3 * p[:, 0] + p[:, 1]), 128 + 100 * np.cos(2 * p[:, 1] - p[:, 2]), 128 + 100 * np.sin(p[:, 0] + 2 * p[:, 2])], 1)
    return np.clip(np.round(c), 0, 255).astype(np.uint8)


def random_colors(n, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def alternating_colors(points):
    """(0,0,0) and (255,255,255) alternating in Morton order: h = +-510 and negative numerators that do not divide."""
    pts = np.asarray(points)
    depth = max(1, int(pts.max()).bit_length())
    order = sorted(range(len(pts)), key=lambda r: key_of(pts[r], depth))
    c = np.zeros((len(pts), 3), np.uint8)
    c[order[1::2]] = 255
    return c


def small_cases():
    """{name: (points, colours)} -- the small cases of the CPU tests."""
    rng = np.random.default_rng(11)
    top = (1 << 21) - 1
    g = np.arange(2)
    out = {
        'n1': np.array([[5, 0, 9]]),
        'n2': np.array([[5, 0, 9], [5, 1, 9]]),
        'n3': np.array([[7, 7, 7], [0, 0, 0], [3, 4, 5]]),
        'cell2': np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3),
        'line_x': np.stack([np.arange(0, 33, 3), np.full(11, 4), np.full(11, 9)], 1),
        'line_y': np.stack([np.full(11, 4), np.arange(0, 33, 3), np.full(11, 9)], 1),
        'line_z': np.stack([np.full(11, 4), np.full(11, 9), np.arange(0, 33, 3)], 1),
        'depth1': np.array([[0, 0, 1], [1, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1]]),
        'top': np.array([[top, top, top], [top, 0, top - 1], [0, top, 0], [top - 1, top, top], [0, 0, 0], [top, top, top - 1], [1 << 20, 3, top]]),
    }
    return {k: (v, rng.integers(0, 256, (len(v), 3)).astype(np.uint8)) for k, v in out.items()}
