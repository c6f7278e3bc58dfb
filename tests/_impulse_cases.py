"""Inputs for the three-piece bf16 conv kernels (tests/test_bf16x3_model_cpu.py, tests/test_bf16x3_gpu.py).

IMPULSE cases.  A lattice of impulses, one nonzero channel per nonzero voxel, 3 voxels apart for the k3 stride-1 layers and 2 apart for the
stride-2 transposed ones, so that no output of a direct kernel reads two nonzero inputs: every output is ONE product x . w, i.e. six piece
products in three accumulating MFMAs, and the accumulation bound of the suite (c n 2^-24 A with n = 6) is an order of magnitude below what
a lost piece costs.  The weights are dense full-mantissa values, so the same launch checks the index of every element of the packed weight
image.  A geometry runs several launches: lattice origins (0,0,0), (1,1,1), (2,2,2) (two origins for stride 2), so that every coordinate of
every axis carries an impulse in some launch, with impulse number j on channel (j + launch) mod Cin; where the grid is too small for these
to put every input channel on a voxel whose 27 taps all land inside the grid, further launches repeat the origins with the channel
offset that puts the first missing channel on the first such voxel.  tests/test_bf16x3_model_cpu.py asserts the coverage from the inputs.
Values: the first impulses of a launch are SPECIALS (both signs, also scaled by 2^+-60), the rest g 2^e with g standard normal and e uniform
in [-30, 30]; weights: Gaussian / sqrt(fan-in) times a power of two per input channel in [-10, 10].  Variants: 'full' = bias + ReLU (+ residual
where the family takes one), 'bare'.

DENSE cases.  The generators of tests/_dynamic_range_cases.py (block 0 = the case, block 1 = a Gaussian neighbour) with 'tiny_60' (block 0
scaled by 2^-60) in place of tiny_block: these kernels have no pre-scale to clamp.

Models and references are computed once per case and shared (lru_cache); the arrays are read-only."""
import functools

import numpy as np

import _bf16x3_model as B
import _dynamic_range_cases as DC
import _f16s_model as F

# kernel -> (model family, prefix of the routed family's name, impl, numerics switches, prefixes the exact-fp32 control may route to, its impl)
KERNELS = {
    'split16': ('direct', 'conv_k3s1_split (', 'SPLIT', {}, ('conv_fwd (exact',), 'MFMA'),
    'split16_sw': ('direct', 'conv_k3s1_split (', 'SPLIT', {'split_mfma16': True}, ('conv_fwd (exact',), 'MFMA'),
    'split32': ('direct', 'conv_k3s1_split32', 'SPLIT', {}, ('conv_fwd (exact',), 'MFMA'),
    'split32_sw': ('direct', 'conv_k3s1_split32', 'SPLIT', {'split_mfma32': True}, ('conv_fwd (exact',), 'MFMA'),
    'tr2_split': ('tr2', 'conv_tr2_split', 'AUTO', {'no_f16s': True}, ('conv_tr2 (exact', 'conv_tr2m (z march, exact'), 'AUTO'),
    'tr2m_bf16': ('tr2', 'conv_tr2m_bf16', 'AUTO', {'no_f16s': True}, ('conv_tr2m (z march, exact',), 'AUTO'),
    'wino_bf16': ('wino', 'conv16_wino_bf16', 'WINOGRAD', {'no_f16s': True}, ('conv16_wino (',), 'WINOGRAD'),
}


def _g(kernel, shape, cout, transposed=False):
    return dict(kernel=kernel, family=KERNELS[kernel][0], shape=shape, cout=cout, transposed=transposed or KERNELS[kernel][0] == 'tr2',
                stride=2 if KERNELS[kernel][0] == 'tr2' else 1)


GEOMS = [
    _g('split16', (1, 9, 16, 16, 64), 64), _g('split16', (1, 9, 8, 8, 64), 64, True), _g('split16_sw', (1, 9, 16, 16, 32), 32),
    _g('split16', (1, 7, 11, 16, 64), 64, True),                       # odd D / H: partial tiles
    _g('split32', (1, 9, 16, 16, 32), 32, True), _g('split32', (1, 6, 16, 32, 32), 32), _g('split32_sw', (1, 9, 16, 16, 64), 64),
    _g('split32', (1, 7, 11, 16, 32), 32),                             # partial tiles
    _g('tr2_split', (1, 5, 8, 8, 64), 64), _g('tr2_split', (1, 5, 16, 16, 64), 64), _g('tr2_split', (1, 5, 8, 8, 64), 32),
    _g('tr2_split', (1, 5, 7, 16, 64), 32),                            # partial tiles
    _g('tr2m_bf16', (1, 5, 16, 16, 32), 16), _g('tr2m_bf16', (1, 16, 16, 16, 32), 16),      # the second: two z slabs
    _g('wino_bf16', (1, 6, 16, 16, 16), 16), _g('wino_bf16', (1, 6, 16, 16, 16), 16, True),
]
VARIANTS = ('full', 'bare')


def geom_id(g):
    return '{}-{}-{}to{}{}'.format(g['kernel'], 'x'.join(map(str, g['shape'][:4])), g['shape'][4], g['cout'], '-tr' if g['transposed'] and g['stride'] == 1 else '')


IDS = [geom_id(g) for g in GEOMS]
ORIGINS = {1: (0, 1, 2), 2: (0, 1)}
SPACING = {1: 3, 2: 2}


def _specials():
    base = [1.5,                                               # bf16-representable: m = l = 0
            1 + 2.0 ** -7 + 2.0 ** -12,                         # l = 0
            1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8,           # ties of the first split: to even downwards, to even upwards (negative m)
            1 + 2.0 ** -10 + 2.0 ** -18, 1 + 2.0 ** -10 * (1 + 2.0 ** -7 + 2.0 ** -8),      # ties of the second split, both ways
            1 + 2.0 ** -7 - 2.0 ** -20, 2 - 2.0 ** -23]         # h rounds up (to the next binade in the second): negative m
    v = [s * b * sc for sc in (1.0, 2.0 ** 60, 2.0 ** -60) for b in base for s in (1.0, -1.0)]
    a = np.array(v, np.float32)
    assert np.array_equal(a.astype(np.float64), np.array(v)), 'a special is not an fp32 value'
    return a


SPECIALS = _specials()


def lattice(dims, stride, origin):
    """(n, 3) voxel coordinates in raster order and which of them have every tap of the kernel inside the grid (stride 1: an interior voxel;
    stride 2: out[2 i + k], k = 0, 1, 2, inside 2 dims: i <= dim - 2)"""
    ax = [np.arange(origin, n, SPACING[stride]) for n in dims]
    zz, yy, xx = np.meshgrid(*ax, indexing='ij')
    s = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1)
    hi = np.array(dims) - 2
    inner = (s <= hi).all(axis=1) & ((s >= 1).all(axis=1) if stride == 1 else True)
    return s, inner


@functools.lru_cache(maxsize=None)
def plan(gi):
    """[(origin, channel offset)] of the launches of geometry gi"""
    g = GEOMS[gi]
    dims, C, stride = g['shape'][1:4], g['shape'][4], g['stride']
    origins = ORIGINS[stride]

    def covers(o, c):
        _, inner = lattice(dims, stride, o)
        return {int((j + c) % C) for j in np.flatnonzero(inner)}
    out = [(o, l) for l, o in enumerate(origins)]
    have = set().union(*[covers(o, c) for o, c in out])
    while len(have) < C:
        o = origins[len(out) % len(origins)]
        first = min(set(range(C)) - have)
        c = int((first - np.flatnonzero(lattice(dims, stride, o)[1])[0]) % C)
        out.append((o, c))
        have |= covers(o, c)
        assert len(out) <= 24, 'the grid is too small for this many channels'
    return tuple(out)


@functools.lru_cache(maxsize=None)
def layer_inputs(gi, variant):
    """weights, bias, ReLU and residual of (geometry, variant): shared by its launches"""
    g = GEOMS[gi]
    N, D, H, W, C = g['shape']
    cout, s = g['cout'], g['stride']
    rng = np.random.default_rng(7000 + gi)
    scale = np.ldexp(np.float32(1), rng.integers(-10, 11, C)).astype(np.float32)
    fan = 27 * C / (8 if s == 2 else 1)
    if g['transposed']:
        w = (rng.standard_normal((3, 3, 3, cout, C)) / np.sqrt(fan)).astype(np.float32) * scale
    else:
        w = (rng.standard_normal((3, 3, 3, C, cout)) / np.sqrt(fan)).astype(np.float32) * scale[:, None]
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((N, D * s, H * s, W * s, cout)).astype(np.float32)
    full = variant == 'full'
    out = dict(g, w=w, bias=bias if full else None, relu=full, res=res if full and g['family'] != 'tr2' else None)
    for a in (w, bias, res):
        a.setflags(write=False)
    return out


def _specials_before(gi, l):
    g = GEOMS[gi]
    return sum(min(len(SPECIALS), len(lattice(g['shape'][1:4], g['stride'], o)[0]) // 2) for o, _ in plan(gi)[:l])


@functools.lru_cache(maxsize=16)
def launch_x(gi, l):
    g = GEOMS[gi]
    N, D, H, W, C = g['shape']
    o, coff = plan(gi)[l]
    sites, _ = lattice((D, H, W), g['stride'], o)
    rng = np.random.default_rng(9000 + 100 * gi + l)
    n = len(sites)
    gv = rng.standard_normal(n).astype(np.float32)
    gv[gv == 0] = 1
    v = np.ldexp(gv, rng.integers(-30, 31, n)).astype(np.float32)
    # the first half of the sites (at most) take specials; a launch goes on in the list where the launches before it stopped, so that
    # every special reaches every geometry (asserted in tests/test_bf16x3_model_cpu.py)
    ns = min(len(SPECIALS), n // 2)
    v[:ns] = SPECIALS[(np.arange(ns) + _specials_before(gi, l)) % len(SPECIALS)]
    x = np.zeros((N, D, H, W, C), np.float32)
    x[0, sites[:, 0], sites[:, 1], sites[:, 2], (np.arange(n) + coff) % C] = v
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=16)
def model(gi, variant, l, pieces=3):
    p = layer_inputs(gi, variant)
    return B.run(p['family'], launch_x(gi, l), p['w'], p['transposed'], p['bias'], p['relu'], p['res'], pieces=pieces, three_step=bool(pieces))


def mutated(gi, variant, l, mutate):
    p = layer_inputs(gi, variant)
    return B.run(p['family'], launch_x(gi, l), p['w'], p['transposed'], p['bias'], p['relu'], p['res'], mutate=mutate, lean=True)


@functools.lru_cache(maxsize=16)
def reference(gi, variant, l):
    p = layer_inputs(gi, variant)
    return F.direct_conv(launch_x(gi, l), p['w'], p['transposed'], p['stride'], p['bias'], p['relu'], p['res'])[0]


def untouched(gi, variant):
    """what an output that no impulse reaches must hold, bit for bit: relu(bias) (+ residual), each one fp32 operation on exact zeros"""
    p = layer_inputs(gi, variant)
    N, D, H, W, _ = p['shape']
    s = p['stride']
    v = np.zeros((N, D * s, H * s, W * s, p['cout']), np.float32)
    if p['bias'] is not None:
        v = v + p['bias']
    if p['relu']:
        v = np.maximum(v, np.float32(0))
    if p['res'] is not None:
        v = v + p['res']
    return v


# ---- dense dynamic-range cases
DENSE_CASES = ['gauss', 'hot_voxel_12', 'hot_voxel_20', 'hot_channel_20', 'sparse_bias', 'tiny_60']
BIAS_FREE = ['gauss', 'hot_voxel_12', 'hot_voxel_20', 'hot_channel_20']
_DENSE_SHAPES = [('split32', (2, 5, 16, 16, 32), 32), ('split16', (2, 5, 16, 16, 64), 64), ('tr2m_bf16', (2, 5, 16, 16, 32), 16),
                 ('split16', (2, 4, 8, 8, 64), 64), ('tr2_split', (2, 4, 8, 8, 64), 64), ('wino_bf16', (2, 5, 16, 16, 16), 16)]


def _dense():
    out = []
    for kernel, shape, cout in _DENSE_SHAPES:
        for i, case in enumerate(DENSE_CASES):
            g = _g(kernel, shape, cout, i % 2 == 0)
            out.append(dict(g, case=case, res=g['family'] != 'tr2' and (i // 2) % 2 == 0))
    return out


DENSE = _dense()
DENSE_IDS = ['{}-{}-{}-c{}'.format(g['kernel'], g['case'], 'x'.join(map(str, g['shape'][:4])), g['shape'][4]) for g in DENSE]


@functools.lru_cache(maxsize=None)
def dense_inputs(i):
    return DC.make_inputs(DENSE[i], 5000 + i)


def dense_run(inp, pieces=3, mutate=None, lean=False):
    return B.run(inp['family'], inp['x'], inp['w'], inp['transposed'], inp['bias'], inp['relu'], inp['res'], pieces=pieces, mutate=mutate, lean=lean)


@functools.lru_cache(maxsize=None)
def dense_model(i, pieces=3):
    return dense_run(dense_inputs(i), pieces)


@functools.lru_cache(maxsize=None)
def dense_reference(i):
    inp = dense_inputs(i)
    return F.direct_conv(inp['x'], inp['w'], inp['transposed'], inp['stride'], inp['bias'], inp['relu'], inp['res'])


def reach(family, hot):
    """(D, H, W) voxel mask -> the outputs that read a marked voxel through the kernel's own arithmetic: direct: any of the 27 taps; stride 2:
    out[2 i + k]; Winograd: the 4 x 4 patch of the output's 2 x 2 tile on the three planes around it"""
    D, H, W = hot.shape
    if family == 'tr2':
        r = np.zeros((2 * D + 2, 2 * H + 2, 2 * W + 2), bool)
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    r[kz:kz + 2 * D:2, ky:ky + 2 * H:2, kx:kx + 2 * W:2] |= hot
        return r[:2 * D, :2 * H, :2 * W]
    hp = np.zeros((D + 2, H + 2, W + 2), bool)
    hp[1:-1, 1:-1, 1:-1] = hot
    if family == 'direct':
        r = np.zeros((D, H, W), bool)
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    r |= hp[kz:kz + D, ky:ky + H, kx:kx + W]
        return r
    hz = hp[0:D] | hp[1:D + 1] | hp[2:D + 2]
    tile = np.zeros((D, H // 2, W // 2), bool)
    for dy in range(4):
        for dx in range(4):
            tile |= hz[:, dy:dy + H:2, dx:dx + W:2]
    return np.repeat(np.repeat(tile, 2, 1), 2, 2)


def dense_far_ratio(i, got0):
    """max |got - exact| / T over the outputs of block 0 that no hot voxel reaches (every output where the case has none), T > 0"""
    inp = dense_inputs(i)
    v, t = dense_reference(i)
    far = ~reach(inp['family'], inp['hot'])[..., None] & (t[0] > 0)
    return float((np.abs(np.asarray(got0, np.float64) - v[0])[far] / t[0][far]).max())
