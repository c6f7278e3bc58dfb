"""numpy / scipy restatement of the point-normal definition (include/pcc_geo.h "point normals") for the normals tests.

knn_ref: the k-th squared distance from cKDTree, then every point within that exact integer radius, sorted by (squared distance,
row index), first k_eff kept.  scatter_ref: M = k_eff sum q q^T - (sum q)(sum q)^T in int64.  Plus the test clouds."""
import numpy as np
from scipy.spatial import cKDTree


def knn_ref(points, k):
    p = np.asarray(points, np.int64)
    n = len(p)
    keff = min(k, n)
    tree = cKDTree(p.astype(np.float64))
    extra = min(n, keff + 24)
    _, cand = tree.query(p.astype(np.float64), k=extra)
    cand = cand.reshape(n, extra)
    d2 = ((p[cand] - p[:, None, :]) ** 2).sum(-1)                      # exact
    # cKDTree's order can only be off between EQUAL float distances; the exact k-th distance is the k-th smallest exact d2
    d2s = np.sort(d2, axis=1)
    kth = d2s[:, keff - 1]
    out = np.empty((n, keff), np.int64)
    # rows whose candidate list provably holds every point within the k-th distance: its largest d2 exceeds the k-th
    complete = (d2s[:, -1] > kth) | (extra == n)
    rows = np.nonzero(complete)[0]
    if len(rows):
        dd, cc = d2[rows], cand[rows]
        order = np.lexsort((cc, dd), axis=1)
        out[rows] = np.take_along_axis(cc, order, 1)[:, :keff]
    for i in np.nonzero(~complete)[0]:                                  # heavy ties: the exact ball
        r = np.sqrt(float(kth[i])) * (1 + 1e-12) + 1e-9
        nb = np.asarray(tree.query_ball_point(p[i].astype(np.float64), r), np.int64)
        dn = ((p[nb] - p[i]) ** 2).sum(-1)
        nb, dn = nb[dn <= kth[i]], dn[dn <= kth[i]]
        out[i] = nb[np.lexsort((nb, dn))][:keff]
    return out


def scatter_ref(points, knn):
    p = np.asarray(points, np.int64)
    q = p[knn] - p[:, None, :]                                          # (n, k, 3)
    s = q.sum(1)
    S = np.einsum('nka,nkb->nab', q, q)
    return knn.shape[1] * S - s[:, :, None] * s[:, None, :]


def normals_check(points, normals, knn, viewpoint=None):
    """The assertions of the definition on (points, normals, exact neighbour rows): eigenvector where the eigen-gap is clear, a
    minimal Rayleigh quotient elsewhere, unit norm, orientation.  Returns the number of well-separated points."""
    p = np.asarray(points, np.int64)
    n = np.asarray(normals, np.float64)
    M = scatter_ref(p, knn)
    zero = ~M.reshape(len(p), -1).any(1)
    assert np.array_equal(normals[zero], np.tile(np.float32([0, 0, 1]), (int(zero.sum()), 1)))
    Mf = M[~zero].astype(np.float64)
    nn = n[~zero]
    lam, vec = np.linalg.eigh(Mf)
    assert np.all(np.abs(np.linalg.norm(nn, axis=1) - 1) < 1e-6)
    sep = lam[:, 1] - lam[:, 0] > 1e-6 * lam[:, 2]
    dots = np.abs((nn[sep] * vec[sep, :, 0]).sum(1))
    assert np.all(dots >= 1 - 1e-6), np.sort(dots)[:5]
    rq = np.einsum('na,nab,nb->n', nn, Mf, nn)
    assert np.all(rq <= lam[:, 0] + 1e-6 * lam[:, 2] + 1e-9 * np.abs(lam[:, 2])), 'Rayleigh quotient above the smallest eigenvalue'
    o = p.sum(0) / len(p) if viewpoint is None else np.asarray(viewpoint, np.float64)
    rel = p[~zero] - o
    side = (nn * rel).sum(1)
    tol = 1e-6 * np.linalg.norm(rel, axis=1) + 1e-12
    assert np.all(side >= -tol), f'{int((side < -tol).sum())} normals point towards the reference point'
    return int(sep.sum())


# ---- test clouds ---------------------------------------------------------------------------------------------------------
def shell(res, radius=0.37, half_width=0.7, seed=0):
    """Voxelised sphere shell: the voxels within half_width of a sphere of radius radius * res (tests/test_cli_gpu.py::_cloud at
    any resolution, built column by column so that 1024^3 stays cheap).  Returns (int32 points, centre)."""
    rng = np.random.default_rng(seed)
    c = res / 2 - 0.3 + rng.random(3) * 0.5
    r = radius * res
    ax = np.arange(res)
    x, y = (a.ravel() for a in np.meshgrid(ax, ax, indexing='ij'))
    dxy2 = (x - c[0]) ** 2 + (y - c[1]) ** 2
    keep = dxy2 < (r + half_width) ** 2
    x, y, dxy2 = x[keep], y[keep], dxy2[keep]
    hi = np.sqrt((r + half_width) ** 2 - dxy2)
    lo = np.sqrt(np.maximum((r - half_width) ** 2 - dxy2, 0))
    pts = []
    for sign in (-1, 1):                                                # the two caps of each column
        a = np.floor(c[2] + sign * np.where(sign < 0, hi, lo)).astype(np.int64) - 1
        b = np.ceil(c[2] + sign * np.where(sign < 0, lo, hi)).astype(np.int64) + 1
        cnt = np.maximum(b - a + 1, 0)
        col = np.repeat(np.arange(len(x)), cnt)
        z = np.repeat(a, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        pts.append(np.stack([x[col], y[col], z], 1))
    g = np.unique(np.concatenate(pts), axis=0)
    g = g[(g[:, 2] >= 0) & (g[:, 2] < res)]
    d = np.linalg.norm(g - c, axis=1)
    return g[np.abs(d - r) < half_width].astype(np.int32), c
