"""Inputs with a dynamic range INSIDE a block for the two-piece fp16 conv kernels (tests/test_f16s_model_cpu.py, tests/test_dynamic_range_gpu.py).

Every launch holds block 0 = the case and (N = 2) block 1 = a unit Gaussian neighbour.  Block 0 starts as a ReLU-sparse Gaussian
(about half zeros); the case then raises the voxels at x, y = 15..16 of one plane (the part of that 2 x 2 patch that lies on the grid:
the corner of four 16 x 16 workgroup tiles at W = 32, a tile edge at 16) or one channel by 2^R, thins the block out, or shrinks it
until the clamp of the pre-scale engages.  Weights are fan-in scaled Gaussians (max |U| near 2^-2), 2^-4 times that for tiny_block, so
that an unclamped s su would leave fp32's range there.  Models and references are computed once per case and shared (lru_cache); the
arrays are read-only."""
import functools

import numpy as np

import _f16s_model as M

CASES = ['gauss', 'hot_voxel_12', 'hot_voxel_20', 'hot_channel_12', 'hot_channel_20', 'sparse_bias', 'tiny_block']
BIAS_FREE = ['gauss', 'hot_voxel_12', 'hot_voxel_20', 'hot_channel_12', 'hot_channel_20']
HOT_Z = 2


def _geoms():
    g = []
    for C in (16, 32, 64):
        for i, case in enumerate(CASES):
            # transposed and forward alternate over the cases, residual on for half of them
            g.append(dict(family='wino', case=case, shape=(2, 5, 16, 32, C), cout=C, transposed=i % 2 == 0, res=(i // 2) % 2 == 0))
    g.append(dict(family='wino', case='hot_voxel_20', shape=(1, 32, 16, 16, 16), cout=16, transposed=True, res=True))
    for shape, cout in (((2, 5, 16, 16, 32), 16), ((2, 3, 16, 16, 64), 32)):
        for case in CASES:
            g.append(dict(family='tr2m', case=case, shape=shape, cout=cout, transposed=True, res=False))
    g.append(dict(family='tr2m', case='hot_voxel_20', shape=(1, 16, 16, 16, 32), cout=16, transposed=True, res=False))
    return g


GEOMS = _geoms()


def geom_id(g):
    return '{}-{}-{}-c{}'.format(g['family'], g['case'], 'x'.join(map(str, g['shape'][:4])), g['shape'][4])


IDS = [geom_id(g) for g in GEOMS]


def make_inputs(g, seed):
    """the inputs of one geometry dict (family, case, shape, cout, transposed, res; 'stride' where the family name does not say it); also the
    generator of the dense cases of the three-piece bf16 kernels (tests/_impulse_cases.py), which add 'tiny_60': block 0 scaled by 2^-60"""
    N, D, H, W, C = g['shape']
    case, cout = g['case'], g['cout']
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D, H, W, C)).astype(np.float32)
    b0 = np.maximum(x[0], 0)                                   # ReLU-sparse: about half zeros
    hot = np.zeros((D, H, W), bool)
    z0 = min(HOT_Z, D - 1)
    if case.startswith('hot_voxel'):
        R = int(case.rsplit('_', 1)[1])
        py, px = (15 if H >= 16 else H // 2 - 1), (15 if W >= 16 else W // 2 - 1)      # grids below 16: the middle 2 x 2 patch
        b0[z0, py:py + 2, px:px + 2, :] = (np.abs(x[0, z0, py:py + 2, px:px + 2, :]) + np.float32(0.5)) * np.float32(2.0 ** R)
        hot[z0, py:py + 2, px:px + 2] = True
    elif case.startswith('hot_channel'):
        b0[..., 3] *= np.float32(2.0 ** int(case.rsplit('_', 1)[1]))
    elif case == 'sparse_bias':
        b0[rng.random(b0.shape) < 0.8] = 0                     # 50 % x 20 % survive: 90 % zeros
    elif case == 'tiny_block':
        b0 = b0 * np.float32(2.0 ** -100)
    elif case == 'tiny_60':
        b0 = b0 * np.float32(2.0 ** -60)
    x[0] = b0
    stride = g.get('stride', 2 if g['family'] == 'tr2m' else 1)
    wshape = (3, 3, 3, cout, C) if g['transposed'] else (3, 3, 3, C, cout)
    fan = 27 * C / (8 if stride == 2 else 1)
    w = (rng.standard_normal(wshape) / np.sqrt(fan)).astype(np.float32)
    if case == 'tiny_block':
        w *= np.float32(2.0 ** -4)                             # small weights: without its clamp s su would pass 2^128
    bias, relu = None, case != 'gauss'
    if case == 'sparse_bias':
        bias = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        relu = True
    elif case in ('tiny_block', 'tiny_60'):
        bias = rng.uniform(-1, 1, cout).astype(np.float32)
    oshape = (N, D * stride, H * stride, W * stride, cout)
    res = rng.standard_normal(oshape).astype(np.float32) if g['res'] else None
    if res is not None and case == 'tiny_block':
        res[0] *= np.float32(2.0 ** -100)
    if res is not None and case == 'tiny_60':
        res[0] *= np.float32(2.0 ** -60)
    for a in (x, w, bias, res):
        if a is not None:
            a.setflags(write=False)
    return dict(g, x=x, w=w, bias=bias, relu=relu, res=res, stride=stride, hot=hot)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    return make_inputs(GEOMS[i], 1000 + i)


def inputs(i):
    return _inputs(i)


def run_model(inp, pieces=2, mutate=None, x=None):
    x = inp['x'] if x is None else x
    if inp['family'] == 'wino':
        return M.wino_model(x, inp['w'], inp['transposed'], inp['bias'], inp['relu'], inp['res'], pieces=pieces, mutate=mutate)
    return M.tr2m_model(x, inp['w'], inp['bias'], inp['relu'], pieces=pieces, mutate=mutate)


@functools.lru_cache(maxsize=None)
def model(i, pieces=2):
    return run_model(_inputs(i), pieces)


@functools.lru_cache(maxsize=None)
def reference(i):
    inp = _inputs(i)
    return M.direct_conv(inp['x'], inp['w'], inp['transposed'], inp['stride'], inp['bias'], inp['relu'], inp['res'])


def far_mask(i):
    """Outputs of block 0 that no hot voxel reaches through the kernel's own arithmetic: Winograd: the 4 x 4 input patch of the
    output's 2 x 2 tile holds no hot voxel on any plane; march: no tap of the output reads one.  Without hot voxels: every output."""
    inp = _inputs(i)
    N, D, H, W, C = inp['shape']
    hot2 = inp['hot'].any(axis=0)
    if inp['family'] == 'wino':
        hp = np.zeros((H + 2, W + 2), bool)
        hp[1:-1, 1:-1] = hot2
        tile = np.zeros((H // 2, W // 2), bool)
        for dy in range(4):
            for dx in range(4):
                tile |= hp[dy:dy + H:2, dx:dx + W:2]
        far = ~np.repeat(np.repeat(tile, 2, 0), 2, 1)
        return np.broadcast_to(far[None, :, :, None], (D, H, W, inp['cout']))
    reach = np.zeros((2 * H + 2, 2 * W + 2), bool)
    for ky in range(3):
        for kx in range(3):
            reach[ky:ky + 2 * H:2, kx:kx + 2 * W:2] |= hot2
    far = ~reach[:2 * H, :2 * W]
    return np.broadcast_to(far[None, :, :, None], (2 * D, 2 * H, 2 * W, inp['cout']))


def far_ratio(i, got0):
    """max |got - exact| / T over the far outputs of block 0 with T > 0"""
    v, t = reference(i)
    far = far_mask(i) & (t[0] > 0)
    return float((np.abs(np.asarray(got0, np.float64) - v[0])[far] / t[0][far]).max())
