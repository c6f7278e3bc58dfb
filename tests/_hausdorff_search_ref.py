"""Brute-force reference of the nine-slot search tallies: for one block and every candidate decoded set, the five
sums of oracle.search_tallies_lowest_index -- the same expressions, the same tie rule (lowest (x, y, z)) -- and beside them the
maxima of the very per-point terms those sums add.  O(|A| |B|) distance matrices: small cases only."""
import numpy as np

N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA = range(9)


def random_block(rng, shape, n_points, fill, normals=False):
    """(block float64 (n, 3 or 6), x_hat float32 `shape`): n distinct random points (with unit-free random normals that float32 holds
    exactly) and scores in (0.03, 0.99) on a random `fill` fraction of the voxels, 0 elsewhere."""
    shape = tuple(shape)
    flat = rng.choice(int(np.prod(shape)), size=n_points, replace=False)
    pts = np.stack(np.unravel_index(np.sort(flat), shape), axis=1).astype(np.float64)
    if normals:
        pts = np.hstack([pts, rng.standard_normal((n_points, 3)).astype(np.float32).astype(np.float64)])
    x_hat = np.where(rng.random(shape) < fill, rng.uniform(0.03, 0.99, shape), 0.0).astype(np.float32)
    return pts, x_hat


def level_sets(x_hat, thresholds):
    """the leading non-empty level sets {x_hat > thr[t]} as float64 (n, 3) arrays in np.argwhere (lexicographic) order; float32 compare"""
    out = []
    for t in thresholds:
        b = np.argwhere(np.asarray(x_hat, np.float32) > np.float32(t)).astype(np.float64)
        if len(b) == 0:
            break
        out.append(b)
    return out


def pair_row(block, b):
    """(float64[9], tie_free) of original rows `block` against the decoded set b (lexicographic order)."""
    blk = np.asarray(block)
    a = blk[:, :3].astype(np.float64)
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)                     # exact integers in float64
    a_order = np.lexsort((a[:, 2], a[:, 1], a[:, 0]))
    to_b = d.argmin(axis=1)                                                # first minimum = lowest (x, y, z)
    to_a = a_order[d[a_order].argmin(axis=0)]
    free = bool(((d == d.min(axis=1, keepdims=True)).sum(axis=1) == 1).all() and ((d == d.min(axis=0, keepdims=True)).sum(axis=0) == 1).all())
    row = np.zeros(9, np.float64)
    t_ab, t_ba = d.min(axis=1), d.min(axis=0)
    row[[N_B, D1_AB, D1_BA, H1_AB, H1_BA]] = len(b), t_ab.sum(), t_ba.sum(), t_ab.max(), t_ba.max()
    if blk.shape[1] >= 6:
        n_a = blk[:, 3:6].astype(np.float32).astype(np.float64)
        cnt = np.bincount(to_b, minlength=len(b)).astype(np.float64)
        acc = np.zeros((len(b), 3))
        np.add.at(acc, to_b, n_a)                                          # ascending point order
        orphan = cnt == 0
        acc[orphan] = n_a[to_a[orphan]]
        cnt[orphan] = 1
        n_b = acc / cnt[:, None]
        e_ab = ((((a - b[to_b]) * n_b[to_b]).sum(1)) ** 2)
        e_ba = ((((b - a[to_a]) * n_a[to_a]).sum(1)) ** 2)
        row[[D2_AB, D2_BA, H2_AB, H2_BA]] = e_ab.sum(), e_ba.sum(), e_ab.max(), e_ba.max()
    return row, free


def brute_tallies(block, x_hat, thresholds=None, tie_free_only=False, sets=None):
    """float64[T, 9] over the leading non-empty level sets of x_hat (or over the decoded sets `sets`, each in lexicographic order).
    tie_free_only: None when a point of any set has two equidistant nearest neighbours."""
    rows = []
    for b in (level_sets(x_hat, thresholds) if sets is None else sets):
        row, free = pair_row(block, np.asarray(b, np.float64))
        if tie_free_only and not free:
            return None
        rows.append(row)
    return np.array(rows, np.float64).reshape(-1, 9)
