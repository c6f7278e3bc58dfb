"""The fixed-threshold occupancy decision on the host (tests/test_thr_fuse_gpu.py, tests/test_thr_ref_cpu.py): what the last synthesis
layer's threshold-fusing epilogue (csrc/conv_edge.hip, pcc_thr_fuse) and the compaction behind it must return for an x_hat, computed
with numpy alone -- never with another GPU kernel; the thresholds that sit on the decision's boundaries; and the (resolution, batch)
cases that reach each instantiation of conv_cout1_mfma_kernel<IN16, T, true> through the codec graph.

The decision: voxel (z, y, x) of block b is occupied when v > thr[b], compared in float32, where v = clip(x_hat, 0, 1) on the encoder
side and v = x_hat on the decoder side (the reference's model_types.py:202,209 and :232-234).

Importing this module needs numpy only."""
import numpy as np

import _direct_cases as DC

PREFILL = 0x55555555          # what the tests fill the compaction scratch with before a call


def pack_words(sel):
    """Occupancy of one block, any shape with a multiple of 32 voxels, C order (z, y, x) -> uint32 words: bit i of word j is voxel
    32 j + i."""
    flat = np.ascontiguousarray(sel, dtype=bool).reshape(-1)
    assert flat.size % 32 == 0
    return np.packbits(flat, bitorder='little').view('<u4').astype(np.uint32)


def unpack_words(words, shape):
    """The inverse of pack_words, written without packbits: voxel n is bit n % 32 of word n // 32."""
    words = np.asarray(words, np.uint32)
    n = np.arange(int(np.prod(shape)))
    return ((words[n // 32] >> (n % 32).astype(np.uint32)) & 1).astype(bool).reshape(shape)


def value(x_hat, clip):
    """What the threshold is compared with: the encoder clips, the decoder does not."""
    x_hat = np.asarray(x_hat, np.float32)
    return np.clip(x_hat, np.float32(0), np.float32(1)) if clip else x_hat


def reference(x_hat, thr, clip):
    """x_hat: (D, H, W) float32 of one block; thr: its threshold.  -> (rows float32 (count, 3) in (z, y, x) order as np.argwhere gives
    them, count, mask words or None when the block has no whole number of words)."""
    v = value(x_hat, clip)
    assert v.dtype == np.float32 and v.ndim == 3
    sel = v > np.float32(thr)
    rows = np.argwhere(sel).astype(np.float32)
    return rows, int(rows.shape[0]), (pack_words(sel) if sel.size % 32 == 0 else None)


# ---- thresholds on the boundaries of the decision -------------------------------------------------------------------------------------
GRID = np.linspace(0, 1.0, 256)      # the product's own thresholds (CompressionModel.thresholds), as float64; the product casts to float32
RANK = (1, 2)                        # the drawn threshold: the distinct value at rank len * 1 // 2 of the block's values inside (0, 1)
RECIPES = ['drawn', 0.0, -0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(0))),
           float(np.float32(GRID[0])), float(np.float32(GRID[1])), float(np.float32(GRID[128])), float(np.float32(GRID[254])),
           float(np.float32(GRID[255])), -1.0, float('inf')]
# no subnormal and no NaN threshold: the product never forms one, and their compare depends on the denormal mode


def drawn(x_hat):
    """A value of the block itself, strictly inside (0, 1) and normal: at least one voxel equals it and must not be selected."""
    x = np.asarray(x_hat, np.float32).reshape(-1)
    inside = np.unique(x[(x > np.finfo(np.float32).tiny) & (x < 1)])
    assert inside.size >= 3, 'the block has no three distinct values inside (0, 1)'
    return np.float32(inside[inside.size * RANK[0] // RANK[1]])


def threshold_sets(x_hat):
    """x_hat: (B, D, H, W) of one call.  -> [(thr float32 (B,), recipe per block)]: the recipes cycled over the blocks, call after call,
    until every recipe has had a block; with B >= len(RECIPES) that is one call."""
    B = x_hat.shape[0]
    sets, start = [], 0
    while start < len(RECIPES):
        recipes = [RECIPES[(start + b) % len(RECIPES)] for b in range(B)]
        thr = np.array([drawn(x_hat[b]) if r == 'drawn' else np.float32(r) for b, r in enumerate(recipes)], np.float32)
        sets.append((thr, recipes))
        start += B
    return sets


# ---- the cases: which (resolution, batch) launches which instantiation -----------------------------------------------------------------
def _case(cid, res, batch, T, zsp, sides=('enc', 'dec')):
    return dict(id=cid, res=res, batch=batch, T=T, zsp=zsp, sides=sides)


def cases(num_cu):
    """The batches follow the CU count, as the windowed rows of tests/_direct_cases.py do: 64, 32, 16 and 2 at 256 CUs."""
    return [
        _case('t16-r16', 16, 2, 16, 1), _case('t16-r32', 32, 5, 16, 1), _case('t16-r64', 64, 3, 16, 1),
        _case('t32-zsp1', 64, num_cu // 4, 32, 1), _case('t32-zsp2', 64, num_cu // 8, 32, 2), _case('t32-zsp4', 64, num_cu // 16, 32, 4),
        _case('t32-zsp8', 128, num_cu // 128, 32, 8),
        # W = 8 is no multiple of 16: the layer cannot fuse (conv_edge.hip:517) and the stand-alone kernels decide.  The hyperprior encoder
        # needs edges that are multiples of 16 (network.hip:481), so only the decoder's main phase (:569: multiples of 8) gets there.
        _case('nofuse-r8', 8, len(RECIPES), 16, 1, sides=('dec',)),
    ]


CASE_IDS = [c['id'] for c in cases(DC.CPU_NUM_CU)]


def last_layer(case, precision, num_cu):
    """DC.select on the 16 -> 1 layer as the codec graph launches it with a threshold: fp16 input in the fp16 precision when the last
    SynthesisBlock stores fp16 (csrc/network.hip:249-261 block_stores_fp16: its stride-1 layers run on a grid of 16-multiples; :287-293:
    the block then hands the 16 -> 1 layer an fp16 tensor), dense output, pcc_thr_fuse given (network.hip:382-385)."""
    res = case['res']
    in16 = precision == 'fp16' and res % 16 == 0
    desc = dict(geo=(case['batch'], res, res, res, 16, 1, 3, 1, 1), impl='AUTO', relu=True)
    flags = dict(f16=precision == 'fp16', in16=in16, out16=False, res=False, clip=False, thr=True)
    return DC.select(desc, flags, {}, num_cu)


def kernel_name(case, precision):
    in16 = precision == 'fp16' and case['res'] % 16 == 0
    fused = case['res'] % 16 == 0
    return 'conv_cout1_mfma_kernel<%s,%d,%s>' % ('true' if in16 else 'false', case['T'], 'true' if fused else 'false')


def explain(what, block, thr, recipe, v, got_sel, want_sel, limit=5):
    """Names the block, the first voxels on which two occupancy arrays differ and their values."""
    bad = np.argwhere(got_sel != want_sel)
    lines = [f'{what}: block {block} (threshold {thr!r}, recipe {recipe!r}): {len(bad)} of {want_sel.size} voxels decided wrongly']
    for idx in bad[:limit]:
        z, y, x = (int(i) for i in idx)
        lines.append(f'  voxel (z={z}, y={y}, x={x}): value {v[z, y, x]!r} ({"=" if v[z, y, x] == thr else ("<" if v[z, y, x] < thr else ">")} '
                     f'threshold): got {bool(got_sel[z, y, x])}, want {bool(want_sel[z, y, x])}')
    return '\n'.join(lines)
