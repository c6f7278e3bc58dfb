"""Plain numpy restatement of what the fused quantise / index / pack kernels compute (pcc_quantize_pack, pcc_index_pack,
pcc_unpack_dequantize, pcc_symbols_pack; csrc/elementwise.hip), and the boundary-value input sets their tests share.  The
yardstick of tests/test_pack_fused_gpu.py; tests/test_pack_ref_cpu.py holds it against the oracle's C loops bit for bit.  Nothing
is imported from the package.

Arithmetic.  Everything is float32, one rounding per operation, as the C expressions of the header are:
    mode 0 (tfc 1.3):  q = floor(v + (0.5 - m))      mode 1:  q = rint(v - m)  (half to even)      sym = int32(q), deq = q + m
    row(s) = (L-1) - #{j < L-1 : s' <= tab[j]},  s' = s if s >= tab[0] else tab[0]     (any comparison with NaN is false)
Stream order.  A block's (vox, C) tensor leaves as (C, vox) when channels_first, as it is otherwise; narrowing is the C cast
(two's-complement wrap).  Tile maxima: entry (n * vtiles + vt) * ctiles + ct = max |sym| over voxels [64 vt, 64 vt + 64) x
channels [64 ct, 64 ct + 64) of block n.
"""
import numpy as np

F32 = np.float32
TILE = 64
FLOOR_HALF, HALF_EVEN = 0, 1

# (N, D, H, W, C): the smallest shape that reaches each branch of k_symbols_pack / k_symbols_unpack
SHAPES = [
    (2, 4, 4, 4, 64),    # whole 64 x 64 tile: vector load + vector store
    (2, 2, 2, 2, 64),    # 8 voxels: fewer than a tile
    (2, 5, 3, 7, 64),    # 105 voxels: one whole tile with vox % 4 != 0 (scalar store) + a partial tile
    (2, 4, 4, 4, 32),    # F = 32 of c1 / c2 / c3
    (1, 4, 4, 8, 96),    # two channel tiles (64 + 32) x two voxel tiles
    (2, 4, 4, 4, 66),    # C % 4 != 0: scalar load, vector store, and a 2-channel tail tile
    (3, 5, 3, 7, 24),    # both dimensions partial
]


def shape_id(shape):
    return 'x'.join(str(v) for v in shape)


# ---- the operations ---------------------------------------------------------------------------------------------------------
def _medians(medians, shape, channels):
    if medians is None:
        return F32(0)
    m = np.asarray(medians, F32)
    if channels is None:
        return m                                               # broadcasts over the last axis
    return m[np.arange(int(np.prod(shape))) % channels].reshape(shape)


def quantize(v, medians=None, mode=FLOOR_HALF, channels=None):
    """(sym int32, deq float32).  channels: channel count when it is not v's last axis (element i has channel i % channels)."""
    v = np.asarray(v, F32)
    m = _medians(medians, v.shape, channels)
    if mode == FLOOR_HALF:
        hm = (F32(0.5) - m).astype(F32)
        q = np.floor((v + hm).astype(F32)).astype(F32)
    else:
        q = np.rint((v - m).astype(F32)).astype(F32)
    return q.astype(np.int32), (q + m).astype(F32)


def dequantize(sym, medians=None, channels=None):
    sym = np.asarray(sym, np.int32)
    return (sym.astype(F32) + _medians(medians, sym.shape, channels)).astype(F32)


def scale_index(sigma, table):
    """the literal count, chunked so that the (n, L-1) comparison matrix stays small"""
    tab = np.asarray(table, F32).ravel()
    s = np.asarray(sigma, F32).ravel().copy()
    with np.errstate(invalid='ignore'):
        s[~(s >= tab[0])] = tab[0]
        idx = np.empty(s.shape, np.int32)
        for lo in range(0, s.size, 1 << 16):
            c = s[lo:lo + (1 << 16)]
            idx[lo:lo + c.size] = (len(tab) - 1) - (c[:, None] <= tab[None, :-1]).sum(1)
    return idx.reshape(np.shape(sigma))


def to_stream(sym, channels_first, dtype):
    """(N, ..., C) int32 -> stream order, narrowed by the C cast.  uint8 is for CDF rows: non-negative values only."""
    sym = np.asarray(sym, np.int32)
    if np.dtype(dtype) == np.uint8:
        assert sym.min() >= 0
    out = np.ascontiguousarray(np.moveaxis(sym, -1, 1)) if channels_first else sym
    return out.astype(dtype)                                   # numpy's integer astype wraps like the C cast


def from_stream(packed, ndhwc_shape, channels_first):
    """inverse of to_stream, widened to int32"""
    packed = np.asarray(packed)
    if channels_first:
        n, c = ndhwc_shape[0], ndhwc_shape[-1]
        packed = np.moveaxis(packed.reshape((n, c) + tuple(ndhwc_shape[1:-1])), 1, -1)
    return np.ascontiguousarray(packed.reshape(ndhwc_shape)).astype(np.int32)


def tiles(shape):
    """(entry, n, voxel slice, channel slice) of every 64 x 64 tile of an (N, ..., C) tensor, in tile_max order"""
    n_blocks, c = shape[0], shape[-1]
    vox = int(np.prod(shape[1:-1]))
    vtiles, ctiles = -(-vox // TILE), -(-c // TILE)
    for n in range(n_blocks):
        for vt in range(vtiles):
            for ct in range(ctiles):
                yield ((n * vtiles + vt) * ctiles + ct, n, slice(vt * TILE, min(vox, vt * TILE + TILE)),
                       slice(ct * TILE, min(c, ct * TILE + TILE)))


def tile_max(sym):
    sym = np.asarray(sym, np.int32)
    s3 = np.abs(sym.astype(np.int64)).reshape(sym.shape[0], -1, sym.shape[-1])
    out = [int(s3[n, vs, cs].max()) for _, n, vs, cs in tiles(sym.shape)]
    return np.asarray(out, np.int32)


# ---- boundary-value inputs --------------------------------------------------------------------------------------------------
def _plant(a, always, rotating, add=None, rng=None, marker=None):
    """Writes `always` into every tile of a (N, ..., C), and as many of `rotating` as fit beside them in three quarters of the
    tile (a different stretch of that list in every tile when it is longer), at random places of the tile.  add = (flags of
    `always`, flags of `rotating`, base (C,)): a flagged value is planted as base[channel] + value.  marker(t): one more value
    for tile t alone."""
    a3 = a.reshape(a.shape[0], -1, a.shape[-1])
    always, rotating = np.asarray(always, F32), np.asarray(rotating, F32)
    fa, fr, base = add if add is not None else (np.zeros(len(always), bool), np.zeros(len(rotating), bool), None)
    for t, n, vs, cs in tiles(a.shape):
        vv, cc = np.meshgrid(np.arange(vs.start, vs.stop), np.arange(cs.start, cs.stop), indexing='ij')
        order = rng.permutation(vv.size)
        vv, cc = vv.ravel()[order], cc.ravel()[order]
        k = max(0, min(len(rotating), (3 * vv.size) // 4 - len(always) - 1))
        pick = (t * k + np.arange(k)) % max(len(rotating), 1)
        own = np.asarray([] if marker is None else [marker(t)], F32)
        vals = np.concatenate([always, rotating[pick], own])
        flags = np.concatenate([fa, fr[pick], np.zeros(len(own), bool)])
        assert len(vals) <= vv.size
        vv, cc = vv[:len(vals)], cc[:len(vals)]
        if base is not None:
            vals = np.where(flags, (base[cc] + vals).astype(F32), vals).astype(F32)
        a3[n, vv, cc] = vals
    return a


def medians_of(kind, channels, seed=0):
    """None, 'dyadic' (multiples of 1/8: v - m and v + (0.5 - m) are exact, so planted ties are ties) or 'random' N(0, 0.3)"""
    rng = np.random.default_rng([11, seed, channels])
    if kind is None:
        return None
    if kind == 'dyadic':
        return (rng.integers(-8, 9, channels) / 8).astype(F32)
    assert kind == 'random'
    return rng.normal(0, 0.3, channels).astype(F32)


def quant_values(shape, medians, int16_run):
    """N(0, 3) with, in every tile: m + k + 0.5 for k in -32..31, 0.49999997, -0.0 and -- for the runs that narrow to int16 --
    +-32767.4 (the last values that fit, or just do not, depending on the median) and +-40000 (wrap).  One value of a magnitude
    of its own per tile, +-(50000 + 1000 t), makes every tile's max|symbol| differ from every other's, so that a tile maximum
    stored at another tile's entry shows."""
    rng = np.random.default_rng([12, int(int16_run)] + list(shape))
    v = (rng.standard_normal(shape) * 3).astype(F32)
    const = [0.49999997, -0.0] + ([32767.4, -32767.4, 40000.0, -40000.0] if int16_run else [])
    ties = np.arange(-32, 32) + 0.5
    always = np.concatenate([ties, const])
    flags = np.concatenate([np.ones(len(ties), bool), np.zeros(len(const), bool)])
    base = np.zeros(shape[-1], F32) if medians is None else np.asarray(medians, F32)
    return _plant(v, always, [], add=(flags, np.zeros(0, bool), base), rng=rng, marker=lambda t: (50000 + 1000 * t) * (-1) ** t)


def scale_tables():
    """name -> float32 table.  'desc' and 'shuffled' are not ascending: they take the literal count inside pcc_index_pack too."""
    ref = np.exp(np.linspace(np.log(0.11), np.log(256), 64)).astype(F32)        # model_types.py:318,324 of the reference
    rng = np.random.default_rng(13)
    return {
        'ref64': ref,
        'L1': np.array([0.5], F32),
        'L2': np.array([0.11, 3.0], F32),
        'asc256': np.exp(np.linspace(np.log(0.05), np.log(500), 256)).astype(F32),
        'runs': np.repeat(np.exp(np.linspace(np.log(0.11), np.log(256), 16)), 4).astype(F32),
        'desc': ref[::-1].copy(),
        'shuffled': ref[rng.permutation(64)],
    }


SIGMA_SPECIALS = np.array([0.0, -1.0, np.inf, np.nan], F32)


def sigma_values(shape, table):
    """log-uniform over [0.01, 600] with, in every tile, 0, -1, +inf and NaN, and every table value and its two float32
    neighbours (as many as fit: a different stretch of that list in every tile when the tile is smaller than the list)."""
    rng = np.random.default_rng([14, len(table)] + list(shape))
    s = np.exp(rng.uniform(np.log(0.01), np.log(600), shape)).astype(F32)
    tab = np.asarray(table, F32)
    near = np.stack([tab, np.nextafter(tab, F32(np.inf)), np.nextafter(tab, F32(-np.inf))], 1).ravel()
    return _plant(s, SIGMA_SPECIALS, near, rng=rng)


def stream_values(shape, dtype, seed=0):
    """symbols as the host coder hands them back, NDHWC int32, with the extremes of `dtype` planted in every tile"""
    rng = np.random.default_rng([15, seed] + list(shape))
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        x, ext = rng.integers(0, 200, shape), [255, 0]
    elif dtype == np.int16:
        x, ext = rng.integers(-3000, 3000, shape), [32767, -32767, -32768]
    else:
        x, ext = rng.integers(-30000, 30000, shape), [70000, -70000]
    x = x.astype(np.int32)
    x3 = x.reshape(shape[0], -1, shape[-1])
    for t, n, vs, cs in tiles(shape):
        cells = rng.permutation((vs.stop - vs.start) * (cs.stop - cs.start))[:len(ext)]
        x3[n, vs.start + cells // (cs.stop - cs.start), cs.start + cells % (cs.stop - cs.start)] = ext
    return x
