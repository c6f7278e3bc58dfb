"""numpy / scipy restatement of the GPU cloud colours (include/pcc_geo.h "cloud colours") for the colour tests.

ordered_ref: per query, the candidates of a cKDTree k-query in (exact squared distance, row) order; a query whose list might not
hold every point at the distance it needs falls back to an exact query_ball_point (as _metrics_ref.nearest_ref does).
map_ref: the rank-th row of that order and its colour.  terms_ref / tally_ref: the mean colour of the whole equidistant nearest set
and the float64 BT.709 terms in the operation order of the header.  Plus the coloured test cloud pairs."""
import numpy as np
from scipy.spatial import cKDTree

import _metrics_ref as MR

BT709 = ((0.2126, 0.7152, 0.0722), (-0.1146, -0.3854, 0.5), (0.5, -0.4542, -0.0458))


def ordered_ref(points, queries, need, extra=16):
    """(dist, rows, exact): dist / rows (nq, extra) the candidates of each query sorted by (d2, row); exact = {query: (dist, rows)}
    for the queries whose list might not hold every point at the distance of its `need`-th pair: their whole ball, sorted."""
    p, q = np.asarray(points, np.int64), np.asarray(queries, np.int64)
    extra = min(extra, len(p))
    tree = cKDTree(p.astype(np.float64))
    _, cand = tree.query(q.astype(np.float64), k=extra)
    cand = cand.reshape(len(q), extra)
    d2 = ((p[cand] - q[:, None, :]) ** 2).sum(-1)                                  # exact
    order = np.lexsort((cand, d2), axis=-1)
    rows, dist = np.take_along_axis(cand, order, 1), np.take_along_axis(d2, order, 1)
    limit = dist[:, min(need, extra) - 1]
    # complete when a farther point is in the list (every point at `limit` is then in it too) or the list is the whole cloud
    exact = {}
    for i in np.nonzero((dist[:, -1] == limit) & (extra < len(p)))[0]:
        nb = np.asarray(tree.query_ball_point(q[i].astype(np.float64), np.sqrt(float(limit[i])) * (1 + 1e-12) + 1e-9), np.int64)
        dn = ((p[nb] - q[i]) ** 2).sum(-1)
        o = np.lexsort((nb, dn))
        exact[i] = (dn[o], nb[o])
    return dist, rows, exact


def map_ref(points, colors, queries, rank):
    """(colours uint8 (nq,3), rows int64 (nq,)): the rank-th point of each query's (d2, row) order."""
    _, rows, exact = ordered_ref(points, queries, rank)
    r = rows[:, rank - 1].astype(np.int64)
    for i, (_, rr) in exact.items():
        r[i] = rr[rank - 1]
    return np.asarray(colors, np.uint8)[r].reshape(-1, 3), r


def terms_ref(points, colors, queries, q_colors):
    """(nq,3) float64 (eY^2, eU^2, eV^2): each query's colour against the mean colour of every point at its smallest distance."""
    col = np.asarray(colors, np.int64)
    dist, rows, exact = ordered_ref(points, queries, 1)
    tie = dist == dist[:, :1]
    sums = (col[rows] * tie[..., None]).sum(1)                                      # exact integers
    count = tie.sum(1)
    for i, (dn, rr) in exact.items():
        t = rr[dn == dn[0]]
        sums[i], count[i] = col[t].sum(0), len(t)
    mean = sums.astype(np.float64) / count[:, None].astype(np.float64)
    d = np.asarray(q_colors, np.float64) - mean
    out = np.empty_like(d)
    for k, (w0, w1, w2) in enumerate(BT709):
        e = (w0 * d[:, 0] + w1 * d[:, 1]) + w2 * d[:, 2]
        out[:, k] = e * e
    return out


def tally_ref(a, ca, b, cb):
    """float64[6]: the Y, U, V sums of A against B, then of B against A."""
    return np.concatenate([terms_ref(b, cb, a, ca).sum(0), terms_ref(a, ca, b, cb).sum(0)])


def random_colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def color_pairs(with_shell=True):
    """{name: (A, colours of A, B, colours of B)}: original A, decoded B, random colours."""
    geo = MR.cloud_pairs(with_shell=False)
    rng = np.random.default_rng(21)
    out = {}
    out['uniform'] = geo['uniform']
    out['lattice_sublattice'] = geo['lattice_sublattice']
    out['sublattice_lattice'] = geo['sublattice_lattice']
    base = rng.integers(0, 40, (600, 3))
    dup = np.concatenate([base, base[:300], base[:100], base[:5].repeat(20, 0)])
    out['duplicates_in_a'] = (MR._shuffled(dup, 12), np.clip(base + rng.integers(-1, 2, base.shape), 0, MR.TOP))
    out['far_queries'] = (rng.integers(500000, 500020, (2000, 3)), geo['corners_vs_cluster'][1])
    out['two_points'] = (np.array([[10, 10, 10], [13, 10, 10]]), rng.integers(0, 32, (300, 3)))
    if with_shell:
        from _normals_ref import shell
        s, _ = shell(1024, radius=0.2, half_width=0.5)
        s = s.astype(np.int64)
        keep = rng.random(len(s)) < 0.8
        moved = s[keep] + rng.integers(-1, 2, (int(keep.sum()), 3)) * (rng.random((int(keep.sum()), 1)) < 0.3)
        out['shell_perturbed'] = (s, MR._shuffled(np.clip(moved, 0, 1023), 13))
    res = {}
    for i, (k, (a, b)) in enumerate(sorted(out.items())):
        a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
        res[k] = (a, random_colors(len(a), 100 + i), b, random_colors(len(b), 200 + i))
    return res
