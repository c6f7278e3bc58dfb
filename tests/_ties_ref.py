"""Brute-force numpy restatement of the tie-averaged point-to-plane (D2) tally (DESIGN.md "Tie-averaged D2"): the yardstick of the
host path (pc_metric.tie_mean_tally) and of the GPU engine (pcc_cloud_distortion_ties) alike.  All-pairs exact integer distances in
chunks, no KD-tree, nothing imported from the package.

Definition.  A = original cloud with float64 normals n_A, B = decoded cloud, integer points in [0, 2^21).  T_B(a) = all rows of B
at the smallest squared distance from a, T_A(b) the same the other way.  votes(b) = {a : b in T_B(a)}; n_B(b) = mean of n_A over
votes(b) (summed in increasing a) or, when empty, over T_A(b).  e(g, n) = ((g.x n.x + g.y n.y) + g.z n.z)^2.  t(a) = mean of
e(a - b, n_B(b)) over T_B(a); t(b) = mean of e(b - a, n_A[a]) over T_A(b).  Tally float64[9] = N_B, D1_AB, D1_BA, D2_AB, D2_BA,
H1_AB, H1_BA, H2_AB, H2_BA: sums and maxima of the squared distances (exact) and of the terms t.

Rounding bound (derived in DESIGN.md, restated at `bounds`).  u = 2^-53.  Every implementation may add the members of one tie or
vote set, and the per-point terms, in its own order; whatever the order, to first order in u
    |computed D2 - exact D2| <= (2 V + 7 + C + D(n)) u M        |computed H2 - exact H2| <= (2 V + 7 + C) u Q
with C the largest tie set, V the largest set a decoded normal averages (votes or orphan tie set), D(n) the deepest chain of
additions a term of the tally of n points can run through, M the sum and Q the maximum over the points of the mean over the tie
set of (|g.x| m.x + |g.y| m.y + |g.z| m.z)^2, m = the mean of |n_A| over the set the normal averages (M >= the D2 slot: it is the
same sum with every product replaced by its magnitude).  Two computed values differ by at most twice that.
"""
import math

import numpy as np

U = 2.0 ** -53


def tie_sets(points, queries, chunk_elems=1 << 25):
    """(q, j, best): one entry per member of a tie set, q (query row) non-decreasing and j (row of `points`) increasing inside a
    query; best[q] int64 = the smallest squared distance.  The cross term q.p is taken in float64, where it is exact (coordinates
    below 2^21: products below 2^42, their sum below 2^44), and the distances are assembled and compared as int64."""
    p, q = np.asarray(points, np.int64).reshape(-1, 3), np.asarray(queries, np.int64).reshape(-1, 3)
    pf, pp = np.ascontiguousarray(p.astype(np.float64).T), (p * p).sum(1)
    step = max(1, chunk_elems // max(len(p), 1))
    qs, js, best = [], [], np.empty(len(q), np.int64)
    for lo in range(0, len(q), step):
        qc = q[lo:lo + step]
        d = (qc.astype(np.float64) @ pf).astype(np.int64)
        d *= -2
        d += pp[None, :]
        d += (qc * qc).sum(1)[:, None]
        m = d.min(1)
        best[lo:lo + step] = m
        r, c = np.nonzero(d == m[:, None])
        qs.append(r + lo)
        js.append(c)
    return np.concatenate(qs), np.concatenate(js), best


def _plane(g, n):
    p = (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2]
    return p * p


def _seg_mean(values, seg, n):
    """Mean of `values` over the entries of every segment id (seg non-decreasing), added one by one in entry order."""
    return np.bincount(seg, weights=values, minlength=n) / np.bincount(seg, minlength=n)


def tally_ref(a, b, n_a=None):
    """dict: 'tally' float64[9]; 'C' largest tie set (either direction); 'V' largest set a decoded normal averages; 'M' / 'Q' the
    magnitude sums / maxima of the module docstring per direction (AB, BA); 'n' (N_A, N_B).  D1 sums are exact Python integers
    rounded once, the D2 sums exactly rounded (math.fsum) over the float64 per-point terms."""
    a, b = np.asarray(a, np.int64).reshape(-1, 3), np.asarray(b, np.int64).reshape(-1, 3)
    qa, jb, d_ab = tie_sets(b, a)
    qb, ja, d_ba = tie_sets(a, b)
    na, nb = len(a), len(b)
    tally = np.zeros(9, np.float64)
    tally[0] = nb
    tally[1], tally[2] = float(sum(int(v) for v in d_ab)), float(sum(int(v) for v in d_ba))
    tally[5], tally[6] = d_ab.max(), d_ba.max()
    c_ab, c_ba = np.bincount(qa, minlength=na), np.bincount(qb, minlength=nb)
    out = {'tally': tally, 'C': int(max(c_ab.max(), c_ba.max())), 'V': 1, 'M': (0.0, 0.0), 'Q': (0.0, 0.0), 'n': (na, nb)}
    if n_a is None:
        return out
    n_a = np.asarray(n_a, np.float64)
    order = np.lexsort((qa, jb))                                  # by decoded row, then increasing original row
    votes = np.bincount(jb, minlength=nb)
    n_b, m_b = np.empty((nb, 3)), np.empty((nb, 3))
    orphan = votes == 0
    own = orphan[qb]
    for c in range(3):
        with np.errstate(invalid='ignore', divide='ignore'):
            n_b[:, c] = _seg_mean(n_a[qa[order], c], jb[order], nb)
            m_b[:, c] = _seg_mean(np.abs(n_a[qa[order], c]), jb[order], nb)
            n_b[orphan, c] = _seg_mean(n_a[ja[own], c], qb[own], nb)[orphan]
            m_b[orphan, c] = _seg_mean(np.abs(n_a[ja[own], c]), qb[own], nb)[orphan]
    out['V'] = int(max(votes.max(), c_ba[orphan].max() if orphan.any() else 0))
    g_ab, g_ba = (a[qa] - b[jb]).astype(np.float64), (b[qb] - a[ja]).astype(np.float64)
    t_ab, t_ba = _seg_mean(_plane(g_ab, n_b[jb]), qa, na), _seg_mean(_plane(g_ba, n_a[ja]), qb, nb)
    tally[3], tally[4] = math.fsum(t_ab), math.fsum(t_ba)
    tally[7], tally[8] = t_ab.max(), t_ba.max()
    q_ab = _seg_mean(_plane(np.abs(g_ab), m_b[jb]), qa, na)
    q_ba = _seg_mean(_plane(np.abs(g_ba), np.abs(n_a[ja])), qb, nb)
    out['M'], out['Q'] = (math.fsum(q_ab), math.fsum(q_ba)), (q_ab.max(), q_ba.max())
    return out


def all_singletons(ref):
    return ref['C'] == 1


def tally_depth(n):
    """D(n): no term of a tally of n points runs through more additions than this, in the GPU engine (per-thread strided sums of at
    most ceil(n / 2^18) terms, an 8-level tree per workgroup, at most 4 partials per thread and another 8-level tree: at most
    20 + ceil(n / 2^18)) or in numpy's pairwise sum (blocks of at most 128 terms in 8 interleaved accumulators plus a tail of at most
    7, combined in 3 levels, then one level per halving: at most 26 + ceil(log2 n))."""
    return 26 + math.ceil(math.log2(max(n, 2))) + math.ceil(n / (1 << 18))


def bounds(ref, pair=True):
    """float64[9] of allowed |difference| per slot between two computed tallies of the input of `ref` (pair=False: between one
    computed tally and the exact value): 0 for N_B and the D1 / H1 slots, the module docstring's expressions for D2 / H2."""
    k = 2 * ref['V'] + 7 + ref['C']
    f = (2.0 if pair else 1.0) * U
    out = np.zeros(9, np.float64)
    na, nb = ref['n']
    out[3], out[4] = f * (k + tally_depth(na)) * ref['M'][0], f * (k + tally_depth(nb)) * ref['M'][1]
    out[7], out[8] = f * k * ref['Q'][0], f * k * ref['Q'][1]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def shell(radius, centre=None):
    """Voxelised sphere shell: every integer point whose distance from the centre rounds to `radius`."""
    r = int(radius)
    c = r + 2 if centre is None else centre
    g = np.arange(-r - 1, r + 2)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    d = np.sqrt(x * x + y * y + z * z)
    keep = np.abs(d - r) < 0.5
    return (np.stack([x[keep], y[keep], z[keep]], 1) + c).astype(np.int32)


def radial_normals(points, centre):
    v = np.asarray(points, np.float64) - centre
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def cases():
    """name -> (A, B, n_A): the inputs the issue names.  shell: a voxelised shell against its 1-voxel-eroded copy (tie-heavy);
    sparse: random sparse clouds; duplicates: repeated rows in both clouds; single_b: B is one point; faces: a centre point against
    its 6 face neighbours (one tie set of six)."""
    rng = np.random.default_rng(7)
    out = {}
    a = shell(12, 16)
    out['shell'] = (a, shell(11, 16), radial_normals(a, 16))
    a, b = rng.integers(0, 1 << 12, (700, 3)).astype(np.int32), rng.integers(0, 1 << 12, (500, 3)).astype(np.int32)
    out['sparse'] = (a, b, unit_normals(len(a), 1))
    a, b = rng.integers(0, 12, (300, 3)).astype(np.int32), rng.integers(0, 12, (200, 3)).astype(np.int32)
    a, b = np.vstack([a, a[::3], a[:40]]), np.vstack([b, b[::2]])
    out['duplicates'] = (a, b, unit_normals(len(a), 2))
    a = rng.integers(0, 40, (400, 3)).astype(np.int32)
    out['single_b'] = (a, np.array([[20, 20, 20]], np.int32), unit_normals(len(a), 3))
    faces = np.array([[9, 10, 10], [11, 10, 10], [10, 9, 10], [10, 11, 10], [10, 10, 9], [10, 10, 11]], np.int32)
    out['faces'] = (np.array([[10, 10, 10]], np.int32), faces, unit_normals(1, 4))
    out['faces_swapped'] = (faces, np.array([[10, 10, 10]], np.int32), unit_normals(6, 5))
    return out


def singleton_case():
    """Clouds whose tie sets are all singletons (asserted by the tests with tie_sets): points on distinct multiples of a large stride
    with small distinct offsets in B."""
    rng = np.random.default_rng(11)
    a = (rng.permutation(600)[:400, None] * 997 + rng.integers(0, 5, (400, 3)) * np.array([1, 7, 31])).astype(np.int32)
    b = (a[:350] + rng.integers(-3, 4, (350, 3)) * np.array([1, 2, 5])).astype(np.int32)
    b = np.clip(b, 0, (1 << 21) - 1)
    return a, b, unit_normals(len(a), 6)
