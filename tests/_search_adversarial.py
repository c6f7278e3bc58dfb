"""Adversarial blocks for the per-block threshold search (csrc/search_d1.hip, csrc/search_d2.hip) and a brute-force reference that evaluates every
DISTINCT level set once.

The search is exact by design (integer squared distances in uint16 grids, uint8 levels, packed sort keys, a linear-time envelope with
cross-multiplied comparisons), so it can only be wrong on a particular line of a particular shape.  Every case here is built for one
such line and is as small as that line allows.  A case is `Case(name, family, shape, blocks, x_hat, thr, clip, props)`:
    blocks : one float64 (n, 6) array per block, xyz + unit normals from a seeded generator.  The D1 and `pick` engines take the normals
             as float32, the `mean` engine as float64; the references promote exactly as the product path does;
    x_hat  : float32 (B, D, H, W), built from an integer level grid (`field_from_levels`) wherever the case is about geometry;
    props  : what the case claims about itself (tests/test_search_adversarial_cpu.py asserts each claim without a GPU).

The reference is the arithmetic the suite already trusts -- `oracle.search_tallies_lowest_index` (D1 and `pick` D2) and
`_search_ties_ref.brute_tallies` / `slot_bounds` (`mean`) -- called with ONE threshold per distinct level set; the row is repeated for the
thresholds that share the set (`level_groups`; that the grouping is right is asserted from `x_hat > thr[t]` itself by the CPU test).
Nothing of the kernels' side is used: no model_opt.d*_tallies_gpu, no host_threshold_stats_pruned.

Size cap: every level set holds at most MAX_SET voxels and every block at most MAX_ROWS rows, so that one brute-force pass stays
below 0.2 s."""
import dataclasses
import functools
import itertools

import numpy as np

import _search_ties_ref as S
import _ties_ref as R

MAX_SET, MAX_ROWS = 20000, 512
T256 = np.linspace(0, 1.0, 256).astype(np.float32)        # the product's thresholds, as the engines receive them


# ---- chunk sizes: thresholds resident at a time ---------------------------------------------------------------------------------------
def d1_chunk(B, nvox):
    """chunk_thresholds(B, nvox) of csrc/search_common.h: two uint16 grids per (block, threshold) within 1 GiB, in [8, 256]."""
    return int(min(256, max(8, (1 << 30) // (B * nvox * 2 * 2))))


def d2_chunk(B, nvox, npts):
    """d2_layout(...).TC of csrc/search_d2.hip: 3 bytes per voxel and 32 bytes per row within 1 GiB, in [4, 64]."""
    return int(min(64, max(4, (1 << 30) // (B * nvox * 3 + npts * 32 + 1))))


def ties_chunk(B, D, H, W):
    """The one chunk size the library exports."""
    from pcc_geo_cnn_v2_amd import _lib
    return int(_lib.lib().pcc_d12_search_ties_chunk(B, D, H, W))


# ---- levels ---------------------------------------------------------------------------------------------------------------------------
def level_value(thr, k):
    """A float32 with exactly k thresholds strictly below it: 0 for k = 0, else the float32 just above thr[k - 1]."""
    return np.float32(0) if k == 0 else np.nextafter(np.float32(thr[k - 1]), np.float32(np.inf))


def field_from_levels(lev, thr=T256):
    table = np.array([level_value(thr, k) for k in range(len(thr))], np.float32)
    return table[np.asarray(lev)]


def levels_of(x_hat, thr, clip):
    """k(v) = #{t : x[v] > thr[t]} in float32, x = clip(x_hat, 0, 1) under `clip`; NaN compares false everywhere: level 0."""
    x = np.asarray(x_hat, np.float32)
    if clip:
        x = np.clip(x, 0, 1)
    lev = np.searchsorted(np.asarray(thr, np.float32), x, side='left')
    lev[np.isnan(x)] = 0
    return lev


def level_groups(x_hat, thr, clip):
    """(tcount, [(lo, hi)]): the thresholds lo <= t < hi share one level set; the groups cover 0 <= t < tcount = the largest level."""
    present = np.unique(levels_of(x_hat, thr, clip))
    present = present[present > 0]
    edges = [0] + [int(p) for p in present]
    return edges[-1], list(zip(edges[:-1], edges[1:]))


def paint(shape, *layers):
    """Integer level grid: every (voxels (n, 3), level) layer written in turn (later layers win)."""
    lev = np.zeros(shape, np.int64)
    for vox, level in layers:
        vox = np.asarray(vox, np.int64).reshape(-1, 3)
        lev[tuple(vox.T)] = level
    return lev


# ---- small helpers --------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    family: str
    shape: tuple
    blocks: list
    x_hat: np.ndarray
    thr: np.ndarray
    clip: bool
    props: dict


def _rows(a, seed):
    a = np.unique(np.asarray(a, np.int64).reshape(-1, 3), axis=0)
    return np.hstack([a.astype(np.float64), R.unit_normals(len(a), seed)])


def _scatter(shape, n, seed, lo=None, hi=None):
    """n distinct voxels of the box [lo, hi) (default: the whole grid), seeded, in row-major order."""
    lo = np.zeros(3, np.int64) if lo is None else np.asarray(lo)
    hi = np.asarray(shape) if hi is None else np.asarray(hi)
    ext = hi - lo
    flat = np.sort(np.random.default_rng(seed).choice(int(np.prod(ext)), size=n, replace=False))
    return np.stack(np.unravel_index(flat, ext), 1).astype(np.int64) + lo


def _grid(*axes):
    return np.stack(np.meshgrid(*[np.atleast_1d(a) for a in axes], indexing='ij'), -1).reshape(-1, 3).astype(np.int64)


def _one(name, family, shape, a, lev, seed, **props):
    return Case(name, family, tuple(shape), [_rows(a, seed)], field_from_levels(lev)[None], T256, True, props)


# ---- the families ---------------------------------------------------------------------------------------------------------------------
def _far_corners():
    """128^3, one block.  d^2 = 3 * 127^2 = 48387 is the largest value the uint16 grids carry (kInf = 65535).  The level set loses one
    voxel between the last threshold of the first D1 chunk and the first of the second (one 128^3 block: chunks of 128)."""
    sh, n = (128, 128, 128), 127
    c = d1_chunk(1, 128 ** 3)
    face = _grid(n, np.arange(128), np.arange(128))
    s = np.r_[np.arange(0, n, 7), n]
    spec = [('far_point', [[0, 0, 0]], [[n, n, n]], [[n, n, n - 1]], 3 * n * n),
            ('far_point_reversed', [[n, n, n]], [[0, 0, 0]], [[0, 0, 1]], 3 * n * n),
            # a corner (0, y, z) sees the face straight ahead: 127^2 is this pairing's largest distance
            ('far_corners_to_face', _grid([0, n], [0, n], [0, n]), face, [[n - 1, 64, 64]], n * n),
            ('far_face_to_corner', _grid(n, s, s), [[0, 0, 0]], [[0, 0, 1]], 3 * n * n)]
    return [_one(nm, 'far', sh, a, paint(sh, (main, c + 4), (extra, c)), 100 + i, max_d2=d2, changes=[c])
            for i, (nm, a, main, extra, d2) in enumerate(spec)]


def _empty_lines_and_planes():
    """32^3: level sets confined to one line / one plane / one voxel, rows of A in the corners and scattered: the nearest decoded voxel
    lies across many empty lines and planes (kInf, kNo8, kNo16 and the k < 0 path of every pass)."""
    sh, r = (32, 32, 32), np.arange(32)
    sets = {'line_z': _grid(5, 7, r), 'line_y': _grid(5, r, 7), 'line_x': _grid(r, 5, 7), 'plane_x': _grid(20, r, r),
            'plane_y': _grid(r, 20, r), 'plane_z': _grid(r, r, 20), 'single_voxel': _grid(29, 2, 30)}
    a = np.vstack([_grid([0, 31], [0, 31], [0, 31]), _scatter(sh, 24, 7)])
    return [_one(f'empty_{nm}', 'empty', sh, a, paint(sh, (v, 40), (v[1::2], 90)), 200 + i) for i, (nm, v) in enumerate(sets.items())]


def _mask_words():
    """(4, 128, 128): lines of two 64-bit mask words.  The set columns sit in one word (or at its edges), the rows of A in the other:
    zdist<2>'s cross-word branches, k_edt_zy<2, 128>."""
    sh = (4, 128, 128)
    spec = [('z63', [63], [(64, 128)]), ('z64', [64], [(0, 64)]), ('z0_127', [0, 127], [(40, 90)]), ('z63_64', [63, 64], [(0, 10), (118, 128)])]
    out = []
    for i, (nm, zs, ranges) in enumerate(spec):
        a = np.vstack([_scatter(sh, 48 // len(ranges), 300 + 10 * i + j, lo=(0, 0, lo), hi=(4, 128, hi)) for j, (lo, hi) in enumerate(ranges)])
        lev = paint(sh, (_grid([0, 3], np.arange(0, 128, 5), zs), 60), (_grid([0, 3], np.arange(0, 128, 10), zs), 120))
        out.append(_one(f'maskword_{nm}', 'maskword', sh, a, lev, 310 + i, columns=zs))
    return out


def _envelopes():
    """(2, H, 64) for H = 128 and 64 (k_edt_zy<1, 128> and <1, 64>): what the lower envelope of the y pass can get wrong."""
    out = []
    for H in (128, 64):
        sh, y = (2, H, 64), np.arange(H)
        c = (H - 1) ** 2 // 63 + 1
        col = lambda z: np.stack([np.zeros(H, np.int64), y, z], 1)
        z0 = 20
        equal_two = [[0, 10, z0], [0, 20, z0 + 10]]                        # (p - 10)^2 = 10^2 + (p - 20)^2 at p = 20: the take-over test meets equality
        equal_three = [[1, 10, z0], [1, 20, z0 + 10], [1, 30, z0]]         # all three parabolas meet at p = 20: the pop test meets equality
        sets = {'full_plane': (_grid(0, y, np.arange(64)), _grid(0, y[::2], np.arange(64))),
                'diagonal': (col(y * 64 // H), col(y * 64 // H)[::3]),
                'parabola': (col(y * y // c), col(y * y // c)[::3]),
                'parabola_mirrored': (col(63 - y * y // c), col(63 - y * y // c)[::3]),
                'comb': (_grid(0, y[::7], [3, 40]), _grid(0, y[::14], [3, 40])),
                'equal_parabolas': (np.array(equal_two + equal_three), np.array(equal_two + equal_three[:2]))}
        for i, (nm, (low, high)) in enumerate(sets.items()):
            a = np.vstack([_scatter(sh, 300, 400 + H + i), [[0, 20, z0], [1, 20, z0]]])
            out.append(_one(f'envelope{H}_{nm}', 'envelope', sh, a, paint(sh, (low, 70), (high, 140)), 420 + H + i,
                            **({'equal_rows': [[0, 20, z0], [1, 20, z0]]} if nm == 'equal_parabolas' else {})))
    return out


def _ties():
    """16^3 and 32^3: equidistant nearest voxels everywhere.  Lattices (eight equidistant neighbours per row; every decoded voxel
    chosen by several rows; at 32^3 the rows fill one octant of the grid, which keeps them within the row cap), and rows exactly midway between two decoded voxels along every axis and diagonal: the per-pass "smaller
    coordinate wins" must compose to the lowest (x, y, z); two rows choosing one decoded voxel; a decoded voxel chosen by nobody."""
    out = []
    for i, (R_, a_ax, b_ax) in enumerate([(16, np.arange(1, 16, 2), np.arange(0, 16, 2)), (16, np.arange(0, 16, 2), np.arange(1, 16, 2)),
                                          (32, np.arange(1, 16, 2), np.arange(0, 32, 2)), (32, np.arange(0, 16, 2), np.arange(1, 32, 2))]):
        sh = (R_,) * 3
        b = _grid(b_ax, b_ax, b_ax)
        lev = paint(sh, (b, 100), (b[(b[:, 0] // 2) % 2 == 0], 200))
        out.append(_one(f'ties{R_}_{"odd" if a_ax[0] else "even"}_rows', 'ties', sh, _grid(a_ax, a_ax, a_ax), lev, 500 + i))
    sh = (32, 32, 32)
    dirs = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]       # 13 directions, one of each +/- pair
    centres = _grid(*[np.arange(4, 32, 8)] * 3)
    a, b = [], []
    for c, d in zip(centres, dirs):
        a.append(c)
        b += [c - d, c + d]
    shared, orphan = centres[13], centres[14]
    a += [shared - (0, 0, 1), shared + (0, 0, 1)]
    b.append(shared)
    out.append(_one('ties32_midway', 'ties', sh, a, paint(sh, (b, 150), ([orphan], 80)), 510, orphan=orphan.tolist(), shared=shared.tolist()))
    return out


def _levels():
    """16^3: the float32 comparisons that make the levels.  x_hat equal to a threshold is not selected, the next float32 is."""
    sh = (16, 16, 16)
    a = _scatter(sh, 40, 600)
    pos = _scatter(sh, 512, 601)
    up = np.nextafter(T256, np.float32(np.inf))
    every = np.zeros(sh, np.float32)
    every[tuple(pos.T)] = np.concatenate([T256, up])
    expect = np.concatenate([np.arange(256), np.minimum(np.arange(256) + 1, 255)])      # (the float32 above 1.0 clips back to 1.0)
    special = np.zeros(sh, np.float32)
    vals = np.array([-1, 2, np.inf, -np.inf, np.nan, 0.5, 0.25], np.float32)
    special[tuple(pos[:7].T)] = vals
    mk = lambda nm, x, seed, **p: Case(nm, 'levels', sh, [_rows(a, seed)], x[None], T256, True, p)
    both = Case('levels_empty_beside_full', 'levels', sh, [_rows(a, 605), _rows(_scatter(sh, 30, 606), 607)],
                np.stack([np.zeros(sh, np.float32), every]), T256, True, dict(tcounts=[0, 255]))
    return [mk('levels_at_and_above_every_threshold', every, 602, voxels=pos, expect=expect, populated=255),
            mk('levels_all_one', np.ones(sh, np.float32), 603, tcounts=[255]),
            mk('levels_specials', special, 604, voxels=pos[:7], expect=np.array([0, 255, 255, 0, 0, 128, 64])), both]


def _chunks():
    """The level set changes exactly between the last threshold of a chunk and the first of the next, and nowhere within two
    thresholds of that.  16^3: the chunks of the two D2 engines; five 64^3 blocks: the D1 chunk (204 thresholds)."""
    sh = (16, 16, 16)
    a = _scatter(sh, 30, 700)
    sizes = {ties_chunk(1, *sh), d2_chunk(1, 16 ** 3, len(a))}
    cuts = sorted({k * c for c in sizes for k in range(1, 256 // c + 1) if k * c <= 250})
    assert cuts and all(q - p > 2 for p, q in zip(cuts, cuts[1:])), cuts
    vox = _scatter(sh, len(cuts) + 3, 701)
    lev = paint(sh, *[(vox[i], c) for i, c in enumerate(cuts)], (vox[len(cuts):], cuts[-1] + 5))
    out = [_one('chunk_d2_16', 'chunk', sh, a, lev, 702, changes=cuts)]
    sh, B = (64, 64, 64), 5
    c = d1_chunk(B, 64 ** 3)
    assert 3 <= c <= 249, c
    blocks, xs = [], []
    for b in range(B):
        vox = _scatter(sh, 60, 710 + b)
        blocks.append(_rows(_scatter(sh, 40, 720 + b), 730 + b))
        xs.append(field_from_levels(paint(sh, (vox[:30], c), (vox[30:], c + 6))))
    out.append(Case('chunk_d1_five_64', 'chunk', sh, blocks, np.stack(xs), T256, True, dict(changes=[c])))
    return out


def _non_cubic():
    """Random points and a blurred x_hat (the recipe of tests/test_threshold_search_gpu._case) on grids with three different edges:
    the index decoding with W and W * H.  (8, 24, 16) takes the fused z/y kernel, (6, 10, 12) the two-kernel form (W % 16 != 0)."""
    from scipy.ndimage import gaussian_filter
    out = []
    for i, sh in enumerate([(8, 24, 16), (6, 10, 12)]):
        rng = np.random.default_rng(800 + i)
        a = np.unique(np.stack([rng.integers(0, s, 60) for s in sh], 1), axis=0)
        dense = np.zeros(sh, np.float32)
        dense[tuple(a.T)] = 1
        x = (gaussian_filter(dense, 0.7) * 2.5 + rng.normal(0, 0.02, sh)).astype(np.float32)
        out.append(Case('noncubic_%dx%dx%d' % sh, 'noncubic', sh, [_rows(a, 810 + i)], x[None], T256, True, {}))
    return out


def _level_256():
    """256 thresholds and a voxel above the last one: level 256, which the uint8 level grid cannot hold (include/pcc_geo.h).  Legal
    arguments; the product cannot produce them (clip and thresholds up to 1.0)."""
    sh = (16, 16, 16)
    a, vox = _scatter(sh, 20, 900), _scatter(sh, 12, 901)
    x = field_from_levels(paint(sh, (vox, 200)))
    x[tuple(vox[:3].T)] = 1.5
    low = np.linspace(0, 0.9, 256).astype(np.float32)
    y = np.zeros(sh, np.float32)
    y[tuple(vox.T)] = 0.5
    y[tuple(vox[:3].T)] = 0.95
    quiet = field_from_levels(paint(sh, (vox, 200)))
    return [Case('level256_unclipped', 'level256', sh, [_rows(a, 902), _rows(a, 903)], np.stack([quiet, x]), T256, False, dict(blocks=[1])),
            Case('level256_thresholds_end_below_one', 'level256', sh, [_rows(a, 904)], y[None], low, True, dict(blocks=[0]))]


@functools.lru_cache(None)
def catalogue():
    """name -> Case, every family."""
    cases = (_far_corners() + _empty_lines_and_planes() + _mask_words() + _envelopes() + _ties() + _levels() + _chunks() + _non_cubic()
             + _level_256())
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


def names(family=None, reference=True):
    """Case names; reference=True leaves out the level-256 cases, for which no statistics are defined at t = 255."""
    return [n for n, c in catalogue().items() if (family is None or c.family == family) and not (reference and c.family == 'level256')]


# ---- the deduplicating references -----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def reference_pick(name, b):
    """(tcount, float64 (tcount, 5)) of block b: rows (|B_t|, d1_sum_AB, d1_sum_BA, d2_sum_AB, d2_sum_BA) under the lowest-(x, y, z)
    rule, one call of oracle.search_tallies_lowest_index per distinct level set."""
    from oracle import oracle as O
    case = catalogue()[name]
    assert case.clip, 'the restatements clip'
    tcount, groups = level_groups(case.x_hat[b], case.thr, case.clip)
    rows = np.zeros((tcount, 5), np.float64)
    for lo, hi in groups:
        row = O.search_tallies_lowest_index(case.blocks[b], case.x_hat[b], case.thr[lo:lo + 1])
        assert row.shape == (1, 5) and row[0, 0] <= MAX_SET and len(case.blocks[b]) <= MAX_ROWS
        rows[lo:hi] = row[0]
    rows.setflags(write=False)
    return tcount, rows


@functools.lru_cache(None)
def reference_mean(name, b):
    """(tcount, [(lo, hi, ref, (b_AB, b_BA), pairs)]) of block b under the tie-averaged rule: `_ties_ref.tally_ref` and
    `_search_ties_ref.slot_bounds` of every distinct level set (through brute_tallies), and the number of (row, tied voxel) pairs of
    the A -> B direction."""
    case = catalogue()[name]
    assert case.clip, 'the restatements clip'
    tcount, groups = level_groups(case.x_hat[b], case.thr, case.clip)
    out = []
    for lo, hi in groups:
        (ref, bounds), = S.brute_tallies(case.blocks[b], case.x_hat[b], case.thr[lo:lo + 1])
        b_t, = S.level_sets(case.x_hat[b], case.thr[lo:lo + 1])
        assert len(b_t) <= MAX_SET and len(case.blocks[b]) <= MAX_ROWS
        pairs = len(R.tie_sets(b_t, case.blocks[b][:, :3].astype(np.int64))[0])
        out.append((lo, hi, ref, bounds, pairs))
    return tcount, out


def chunk_pairs(name, chunk):
    """Largest number of tie pairs any chunk of `chunk` thresholds holds, all blocks together: what the `mean` engine reports."""
    case = catalogue()[name]
    per_t = np.zeros(len(case.thr) + chunk, np.int64)
    for b in range(len(case.blocks)):
        for lo, hi, _, _, pairs in reference_mean(name, b)[1]:
            per_t[lo:hi] += pairs
    return int(max(per_t[t0:t0 + chunk].sum() for t0 in range(0, len(case.thr), chunk)))
