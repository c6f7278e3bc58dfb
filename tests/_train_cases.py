"""Shared cases of the training-gradient tests: the conv geometries of c1, c2, c3 and c3p, small-integer data on which every
gradient is exact in fp32, the grids that reach partial voxel tiles, uneven slices and non-cubic address arithmetic, and their
float64 references.

Exactness: with integer weights, x and dout of magnitude <= 2 every product and every partial sum of a gradient element is an
integer, and below 2^24 as long as the element's sum of |terms| is (test_train_cpu.py asserts it per case).  Any fp32 summation order,
slice split or MFMA chain then gives the float64 value bit for bit."""
import functools

import numpy as np
import torch

import _train_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType


def _key(prefix, i, l):
    return (l.cin, l.cout, l.k, l.stride, int(l.transposed), int(l.relu), int(l.bias is not None), int(prefix == 'analysis' and i == 0))


@functools.lru_cache(maxsize=None)
def _walk():
    """(geometries, (geometry, input grid) pairs at training resolutions 16 and 32) of the conv layers of c1, c2, c3 and c3p."""
    geoms, grids = set(), set()
    for cfg in ('c1', 'c2', 'c3', 'c3p'):
        m = ModelConfigType[cfg].build()
        m.compress([1, 1, 64, 64, 64])
        for prefix, tr, _ in m._transforms():
            layers = [c.layer for c in tr.conv_layers()]
            geoms.update(_key(prefix, i, l) for i, l in enumerate(layers))
            for res in (16, 32):
                D = res if prefix == 'analysis' else (res // 8 if prefix in ('synthesis', 'hyper_analysis') else res // 16)
                for i, l in enumerate(layers):
                    grids.add((_key(prefix, i, l), D))
                    D = ops.conv_out_shape(l, (1, D, D, D, l.cin))[1]
    return sorted(geoms), sorted(grids)


def _geometries():
    """Distinct (cin, cout, k, stride, transposed, relu, bias, first) of the conv layers of c1, c2, c3, c3p; `first`: the layer
    reads the network input (no input gradient needed)."""
    return _walk()[0]


GEOMS = _geometries()
SEED = 7                  # of the integer cases


def geom_id(g):
    return f'{g[0]}-{g[1]}-k{g[2]}s{g[3]}{"T" if g[4] else ""}'


def case_id(case):
    g, n, dims = case[:3]
    return f'{geom_id(g)}{"" if g[5] else "-lin"}-n{n}-{"x".join(map(str, dims))}'


def _layer(g, rng):
    cin, cout, k, s, tr, relu, bias, _ = g
    shape = (k, k, k) + ((cout, cin) if tr else (cin, cout))
    w = rng.uniform(-1, 1, shape).astype(np.float32) / np.sqrt(k ** 3 * cin)
    b = rng.normal(0, .1, cout).astype(np.float32) if bias else None
    return ops.ConvLayer(w, b, s, tr, relu)


def desc(g, N, dims):
    """The layer descriptor of geometry g on an N x dims input grid."""
    cin, cout, k, s, tr, relu, bias, _ = g
    flags = (L.PCC_CONV_BIAS if bias else 0) | (L.PCC_CONV_RELU if relu else 0)
    return L.ConvDesc(N, *dims, cin, cout, k, s, tr, flags, L.PCC_IMPL_AUTO, 0, 0)


def int_case(g, N, dims, seed):
    """(layer, x, dout) of geometry g on an N x dims input grid: weights, bias and dout float32 integers of {-2 .. 2}, x the ReLU of
    such integers (three fifths zeros)."""
    cin, cout, k, s, tr, relu, bias, _ = g
    rng = np.random.default_rng(seed)
    shape = (k, k, k) + ((cout, cin) if tr else (cin, cout))
    w = rng.integers(-2, 3, shape).astype(np.float32)
    b = rng.integers(-2, 3, cout).astype(np.float32) if bias else None
    layer = ops.ConvLayer(w, b, s, tr, relu)
    x = np.maximum(rng.integers(-2, 3, (N,) + tuple(dims) + (cin,)), 0).astype(np.float32)
    dout = rng.integers(-2, 3, ops.conv_out_shape(layer, x.shape)).astype(np.float32)
    return layer, x, dout


# ---- the forward view of pcc_conv3d_wgrad (conv_wgrad.hip): u = the large grid, dz = the small one ------------------------------
def view(g):
    cin, cout, k, s, tr = g[:5]
    return (cout, cin, k, s) if tr else (cin, cout, k, s)


# voxel tile (TZ, TY, TX) of the dz grid of every entry of kMfma, by forward view (cu, cz, k, s)
TILES = {
    (16, 16, 3, 1): (2, 4, 16), (32, 32, 3, 1): (2, 4, 16), (64, 64, 3, 1): (2, 4, 16),
    (16, 32, 3, 2): (2, 4, 8), (32, 32, 3, 2): (2, 4, 8), (32, 64, 3, 2): (2, 4, 8), (64, 64, 3, 2): (2, 4, 8),
    (32, 32, 5, 2): (1, 4, 8),
}

# per entry one (N, (OD, OH, OW)) of the dz grid with more voxel tiles than slices, an uneven split of the tiles over the slices
# and a partial tile at the end of every axis
SLICE_GRIDS = {
    (16, 16, 3, 1): (2, (37, 42, 40)), (32, 32, 3, 1): (2, (37, 42, 40)), (64, 64, 3, 1): (3, (13, 22, 36)),
    (16, 32, 3, 2): (3, (17, 26, 44)), (32, 32, 3, 2): (3, (17, 26, 44)), (32, 64, 3, 2): (3, (13, 18, 44)),
    (64, 64, 3, 2): (3, (9, 18, 36)), (32, 32, 5, 2): (3, (7, 18, 20)),
}

VALU_GRID = (3, (7, 9, 11))                  # 2079 dz voxels: two full rounds of the 1024 slices and 31 left over
# three extents each, none a multiple of a tile extent above 1: on the first the input gradients take the generic kernel (no MFMA
# family has rows of 10 or 20 voxels), on the second the 4-voxel rows of the MFMA families
NONCUBIC_GRIDS = ((2, (3, 6, 10)), (2, (5, 3, 4)))


def small_dims(g, dims):
    """The dz grid of geometry g on input grid dims."""
    return tuple(dims) if g[4] else tuple(-(-n // g[3]) for n in dims)


def units(g, N, dims):
    """What pcc_conv3d_wgrad splits into slices: the voxel tiles of the dz grid (MFMA entries) or its voxels."""
    o = small_dims(g, dims)
    t = TILES.get(view(g), (1, 1, 1))
    return N * int(np.prod([-(-a // b) for a, b in zip(o, t)]))


def slices(g, N, dims):
    """(S, longest slice chain) as plan() of conv_wgrad.hip computes them, restated."""
    cu, cz, k, _ = view(g)
    n = units(g, N, dims)
    S = max(1, min(1024, 2 ** 25 // (k ** 3 * cu * cz), n))
    return S, -(-n // S) * int(np.prod(TILES.get(view(g), (1, 1, 1))))


def _input_dims(g, small, odd):
    """The input grid of geometry g whose dz grid is `small`: a forward stride-2 layer takes the odd large grid (2 O - 1, the other
    split of the SAME padding) when `odd`."""
    if g[4] or g[3] == 1:
        return tuple(small)
    return tuple(2 * o - 1 if odd else 2 * o for o in small)


def slice_cases():
    """(g, N, input dims) of every geometry with an MFMA entry on its entry's SLICE_GRIDS shape."""
    return [(g, SLICE_GRIDS[view(g)][0], _input_dims(g, SLICE_GRIDS[view(g)][1], True)) for g in GEOMS if view(g) in TILES]


def valu_cases():
    return [(g, VALU_GRID[0], _input_dims(g, VALU_GRID[1], True)) for g in GEOMS if view(g) not in TILES]


def noncubic_cases():
    """Every geometry with an input gradient on the grids of three different extents (even large grid: the dual descriptor of a
    forward stride-2 layer exists only there)."""
    return [(g, N, _input_dims(g, small, False)) for N, small in NONCUBIC_GRIDS for g in GEOMS if not g[7]]


def mixed_parity_cases():
    """Weight-gradient cases of every forward stride-2 geometry on large grids of mixed parity, dz grid (3, 6, 10): the SAME low
    padding is 0 on an even axis and 1 on an odd one (k = 3), so a padding taken from another axis shows here and nowhere else.  The
    two patterns tell every pair of axes apart."""
    N, small = NONCUBIC_GRIDS[0]
    return [(g, N, tuple(2 * o - p for o, p in zip(small, odd))) for odd in ((1, 0, 1), (0, 1, 1))
            for g in GEOMS if not g[4] and g[3] == 2]


def small_grids():
    """Distinct (g, 3, input grid) of the layers of c1, c2, c3 and c3p trained at resolutions 16 and 32, input grids of at most 8 per
    axis (the larger cubes have tests of their own)."""
    return [(g, 3, (D, D, D)) for g, D in _walk()[1] if D <= 8]


# ---- references -----------------------------------------------------------------------------------------------------------------
def grads(layer, x, dout, dtype=torch.float64, absolute=False, dx=True):
    """(dW, dB, dX or None) of sum(conv(x, w) * dout) by torch autograd on the CPU in `dtype`; `absolute`: on |x|, |w|, |dout|, the
    sum of |terms| of every gradient element."""
    f = np.abs if absolute else (lambda a: a)
    w = torch.from_numpy(f(layer.kernel)).to(dtype).requires_grad_()
    xt = torch.from_numpy(f(x)).to(dtype).requires_grad_(dx)
    gt = torch.from_numpy(f(dout)).to(dtype)
    y = (R.conv3d_transpose if layer.transposed else R.conv3d)(xt, w, layer.stride)
    (y * gt).sum().backward()
    db = gt.reshape(-1, layer.cout).sum(0)
    return w.grad.numpy(), db.numpy(), xt.grad.numpy() if dx else None


@functools.lru_cache(maxsize=None)
def int_reference(g, N, dims, seed):
    """float64 (dW, dB, dX) of int_case(g, N, dims, seed); dX is None for a first layer.  Shared between tests: do not write to it."""
    layer, x, dout = int_case(g, N, dims, seed)
    return grads(layer, x, dout, dx=not g[7])
