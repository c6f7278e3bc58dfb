"""Boundary catalogue and numpy restatements for pcc_threshold_compact and pcc_voxelize (include/pcc_geo.h, csrc/elementwise.hip).
Nothing here touches the GPU or imports from the kernels' side; tests/test_compact_cases_cpu.py holds the restatements against the
oracle's C loops and model_types.sparse_to_dense, tests/test_compact_gpu.py holds the kernels against the restatements.

    argwhere_ref: np.argwhere((np.clip(x, 0, 1) if clip else x) > np.float32(thr)).astype(np.float32)
    voxelize_ref: a plain loop that drops every point outside [0,B) x [0,D) x [0,H) x [0,W)

The compaction kernel works on chunks of 4096 voxels (one workgroup), in 4 passes of 1024 (256 threads x 4 voxels), with float4 loads
when D*H*W is a multiple of 4: the shapes and the hit patterns sit on those seams.  A block is (name, x (D,H,W) float32, thr) with thr
the threshold as the caller has it (a float64 off np.linspace, or an out-of-contract value); the kernel gets np.float32(thr).
"""
from collections import namedtuple

import numpy as np

CHUNK, PASS = 4096, 1024
SHAPES = ((1, 1, 1), (1, 1, 3), (5, 7, 3), (3, 11, 31), (12, 12, 12), (4, 31, 33), (16, 16, 16), (4, 25, 41), (3, 37, 37), (17, 16, 16),
          (20, 20, 20), (33, 32, 32))
LINSPACE = np.linspace(0, 1.0, 256)                       # the reference's thresholds (float64)
VALUE_THRS = (LINSPACE[0], LINSPACE[1], LINSPACE[254], LINSPACE[255])
BAD_THRS = (-0.5, -np.inf, np.inf, np.nan)                # out of contract: the kernel still has to equal the numpy expression
f32 = np.float32
SPECIALS = np.array([np.nan, -np.inf, np.inf, -0.0, 1e-45, np.nextafter(f32(1.17549435e-38), f32(0)), np.finfo(np.float32).max, 1.0,
                     np.nextafter(f32(1), f32(2)), 3.0, -3.0], np.float32)

Block = namedtuple('Block', 'name x thr')


def shape_id(dhw):
    return 'x'.join(map(str, dhw))


# ---- restatements ----------------------------------------------------------------------------------------------------------
def argwhere_ref(x, thr, clip):
    """x (D,H,W) float32 -> float32 (count, 3) rows in C order; the compare is float32 against the float32-rounded threshold"""
    x = np.asarray(x, np.float32)
    assert x.ndim == 3
    with np.errstate(invalid='ignore'):
        return np.argwhere((np.clip(x, 0, 1) if clip else x) > np.float32(thr)).astype(np.float32)


def launch_ref(blocks, clip, one=argwhere_ref):
    """the rows of every block of a launch: block b under its own thr[b]"""
    return [one(b.x, b.thr, clip) for b in blocks]


def voxelize_ref(pts, block_of, B, D, H, W):
    """pts (n,3) int, block_of (n,) int or None (everything into block 0) -> dense (B,D,H,W) float32 of {0,1}"""
    dense = np.zeros((B, D, H, W), np.float32)
    pts = np.asarray(pts).tolist()                                          # Python ints: no wrap-around anywhere
    blocks = [0] * len(pts) if block_of is None else np.asarray(block_of).tolist()
    for (x, y, z), b in zip(pts, blocks):
        if 0 <= b < B and 0 <= x < D and 0 <= y < H and 0 <= z < W:
            dense[b, x, y, z] = 1.0
    return dense


# ---- threshold compaction: the blocks of one launch ------------------------------------------------------------------------
def _from_mask(mask, thr, rng):
    """values with exactly `mask` above float32(thr): hits in (thr, 1.3], the rest in [-0.3, thr] (some of them equal to thr)"""
    t = f32(thr)
    u = rng.random(mask.shape).astype(np.float32)
    hi = np.maximum(t + (f32(1.3) - t) * u, np.nextafter(t, f32(np.inf)))
    lo = np.minimum(f32(-0.3) + (t + f32(0.3)) * u, t)
    lo[rng.random(mask.shape) < 0.02] = t
    return np.where(mask, hi, lo).astype(np.float32)


def _planted(n, rng):
    """flat float32 arrays that together hold every value of SPECIALS over a uniform [-0.3, 1.3) background; the first one holds NaN.
    The first and the last voxel carry a special where the block has room."""
    out = []
    for lo in range(0, len(SPECIALS), max(n, 1)):
        sp = SPECIALS[lo:lo + n]
        x = (rng.random(n) * 1.6 - 0.3).astype(np.float32)
        at = rng.choice(n, len(sp), replace=False)
        if n >= 2 * len(SPECIALS):
            at = rng.choice(np.arange(1, n - 1), len(sp), replace=False)
            at[0], at[2] = 0, n - 1                                       # NaN in the first voxel, +inf in the last
        x[at] = sp
        out.append(x)
    return out


def patterns(dhw):
    """name -> boolean hit mask (D,H,W): the positions a compaction kernel can get wrong"""
    D, H, W = dhw
    n = D * H * W
    rng = np.random.default_rng(7000 + n)
    i = np.arange(n)
    d, h, w = np.unravel_index(i, dhw)

    def at(*idx):
        m = np.zeros(n, bool)
        m[[j for j in idx if 0 <= j < n]] = True
        return m
    out = {'none': np.zeros(n, bool), 'all': np.ones(n, bool), 'first': at(0), 'last': at(n - 1)}
    if n > CHUNK - 1:
        out['chunk-seams'] = at(CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK)
    if n > 255:
        out['thread-seams'] = at(255, 256, *range(PASS - 5, PASS + 5))
    if -(-n // CHUNK) >= 3:
        out['middle-chunk'] = (i >= CHUNK) & (i < 2 * CHUNK)
    for e in range(4):
        out[f'lane{e}'] = i % 4 == e
    out['checkerboard'] = (d + h + w) % 2 == 1
    for pct in (1, 50, 99):
        out[f'random{pct}'] = rng.random(n) < pct / 100
    return {k: m.reshape(dhw) for k, m in out.items()}


def _build(dhw):
    D, H, W = dhw
    n = D * H * W
    rng = np.random.default_rng(9000 + n)
    blocks = []
    for j, (name, mask) in enumerate(patterns(dhw).items()):
        thr = LINSPACE[(37 * j + 5) % 254 + 1]                          # a threshold of its own per block
        blocks.append(Block(name, _from_mask(mask, thr, rng), thr))
    for thr in VALUE_THRS:
        t = f32(thr)
        tag = f'thr{int(np.flatnonzero(LINSPACE == thr)[0])}'
        blocks.append(Block(f'equal-{tag}', np.full(dhw, t, np.float32), thr))
        up = rng.random(dhw) < 0.5
        if n > 1:
            up.flat[0], up.flat[n - 1] = True, False
        blocks.append(Block(f'ulp-{tag}', np.where(up, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))).astype(np.float32), thr))
        blocks += [Block(f'special{k}-{tag}', x.reshape(dhw), thr) for k, x in enumerate(_planted(n, rng))]
    for thr in BAD_THRS:
        blocks.append(Block(f'special0-bad{thr}', _planted(n, rng)[0].reshape(dhw), thr))
        blocks.append(Block(f'uniform-bad{thr}', (rng.random(dhw) * 1.6 - 0.3).astype(np.float32), thr))
    assert len({b.name for b in blocks}) == len(blocks)
    return blocks


def _build_256():
    """B = 256 blocks of (5,7,3): block t under LINSPACE[t], its values at, one ulp above and one ulp below that threshold"""
    dhw = (5, 7, 3)
    rng = np.random.default_rng(256)
    blocks = []
    for t, thr in enumerate(LINSPACE):
        v = f32(thr)
        pick = rng.integers(0, 3, dhw)
        pick.flat[:3] = (0, 1, 2)
        x = np.choose(pick, [v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))]).astype(np.float32)
        blocks.append(Block(f'thr{t}', x, thr))
    return blocks


ALL_256 = 'all256'
LAUNCHES = tuple(shape_id(s) for s in SHAPES) + (ALL_256,)
_SHAPE_OF = {shape_id(s): s for s in SHAPES}
_SHAPE_OF[ALL_256] = (5, 7, 3)
_BLOCKS, _REFS = {}, {}


def launch(name):
    """(dhw, blocks) of a launch of the catalogue, built once"""
    if name not in _BLOCKS:
        _BLOCKS[name] = _build_256() if name == ALL_256 else _build(_SHAPE_OF[name])
    return _SHAPE_OF[name], _BLOCKS[name]


def refs(name, clip):
    """argwhere_ref of every block of a launch, computed once and shared: do not write into the arrays"""
    key = (name, bool(clip))
    if key not in _REFS:
        _REFS[key] = launch_ref(launch(name)[1], clip)
    return _REFS[key]


def stacked(blocks):
    """(x (B,D,H,W) float32, thr (B,) float32) as the kernel takes them"""
    return np.stack([b.x for b in blocks]).astype(np.float32), np.array([f32(b.thr) for b in blocks], np.float32)


def cap_case():
    """(17,16,16), clip = 1: blocks of mixed counts, among them the out-of-contract ones, and the caps to run them under"""
    name = shape_id((17, 16, 16))
    dhw, blocks = launch(name)
    keep = ('none', 'chunk-seams', 'random1', 'random50', 'random99', 'special0-bad-0.5', 'special0-bad-inf')
    picked = [b for b in blocks if b.name in keep]
    assert len(picked) == len(keep)
    counts = [len(r) for r in launch_ref(picked, 1)]
    n = int(np.prod(dhw))
    caps = sorted({0, 1, min(c for c in counts if c), max(counts) - 1, max(counts), n, n + 5})
    assert len(caps) == 7                                                 # smallest count 2, largest D*H*W - 1: no two caps coincide
    return dhw, picked, caps


# ---- voxelise --------------------------------------------------------------------------------------------------------------
GRIDS = ((5, 7, 3), (16, 16, 16), (64, 64, 64))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
VoxCase = namedtuple('VoxCase', 'name pts block_of B dhw in_range')


def _vox(name, pts, block_of, B, dhw, in_range):
    pts = np.asarray(pts, np.int32).reshape(-1, 3)
    return VoxCase(name, pts, None if block_of is None else np.asarray(block_of, np.int32).reshape(-1), B, dhw, in_range)


def voxel_cases(dhw):
    D, H, W = dhw
    rng = np.random.default_rng(5000 + D * H * W)
    ext = np.array(dhw)
    inside = lambda n: rng.integers(0, ext, (n, 3))
    g = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij'), -1).reshape(-1, 3)
    cases = [_vox(f'axis{a}', [[(ext[c] - 1) if c == a else 0 for c in range(3)]], [1], 2, dhw, True) for a in range(3)]
    cases.append(_vox('corners', [[x, y, z] for x in (0, D - 1) for y in (0, H - 1) for z in (0, W - 1)], np.arange(8) % 2, 2, dhw, True))
    cases.append(_vox('faces', g[((g == 0) | (g == ext - 1)).any(1)], None, 1, dhw, True))
    cases.append(_vox('repeat', np.tile(inside(1), (1000, 1)), np.zeros(1000), 1, dhw, True))
    bad = []
    for a in range(3):
        for v in (-1, int(ext[a]), I32_MIN, I32_MAX):
            p = inside(1)[0]
            p = p.astype(np.int64)
            p[a] = v
            bad.append(p)
    good = inside(20)
    cases.append(_vox('coordinates-outside', np.concatenate([good[:10], np.array(bad), good[10:]]), rng.integers(0, 2, 32), 2, dhw, False))
    bof = np.array([0, -1, 1, 3, 2, I32_MAX, 0, I32_MIN, 2])
    cases.append(_vox('block-outside', inside(len(bof)), bof, 3, dhw, False))
    cases.append(_vox('no-block-of-B1', inside(40), None, 1, dhw, True))
    cases.append(_vox('no-block-of-B3', inside(40), None, 3, dhw, True))
    cases.append(_vox('no-points', np.zeros((0, 3)), np.zeros(0), 2, dhw, True))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def voxel_grid_pass_case(num_cu):
    """num_cu * 8 * 256 + 5 random points into 4 blocks of 16^3: a few points past one pass of the kernel's largest grid.  So many
    points fill the planes they fall into, so they stay out of the plane z = 15: the first 5 and the last 5 points own a voxel each there."""
    n = num_cu * 8 * 256 + 5
    rng = np.random.default_rng(n)
    pts = rng.integers(0, (16, 16, 15), (n, 3))
    own = np.concatenate([np.arange(5), np.arange(n - 5, n)])
    pts[own] = np.stack([np.arange(10), 15 - np.arange(10), np.full(10, 15)], -1)
    return _vox(f'grid-pass-{num_cu}cu', pts, rng.integers(0, 4, n), 4, (16, 16, 16), True)
