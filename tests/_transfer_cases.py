"""Fixtures and the brute-force restatement of the colour transfer (include/pcc_geo.h "cloud colours", DESIGN.md 4.9 "Colour
transfer"), shared by tests/test_transfer_cpu.py and tests/test_transfer_gpu.py.  Every case is (A, colours of A, B): integer
coordinates in [0, 2^21), at most 50 000 points a side."""
import numpy as np

TOP = (1 << 21) - 1


def colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def sphere_shell(res):
    """The voxelised sphere shell of radius 0.45 res around the centre of a res^3 grid."""
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).reshape(-1, 3)
    r = np.sqrt(((g - res / 2) ** 2).sum(1))
    return g[np.abs(r - 0.45 * res) < 0.5].astype(np.int64)


def decoded_variants(a, res, seed):
    """{name: B}: what a decoder makes of A -- a 60 % subset, a +-1 jitter, coordinates floored to even (duplicates dropped)."""
    rng = np.random.default_rng(seed)
    return {'subset': a[rng.random(len(a)) < 0.6],
            'jitter': np.clip(a + rng.integers(-1, 2, a.shape), 0, res - 1),
            'even': np.unique(a & ~1, axis=0)}


def benefit_fixtures(seed=7):
    """{name: (A, colours, B)}: the six cases of the benefit condition -- shells in 32^3 and 64^3 with a white-noise texture."""
    out = {}
    for res in (32, 64):
        a = sphere_shell(res)
        ca = colors(len(a), seed + res)
        for name, b in decoded_variants(a, res, seed + 2 * res).items():
            out[f'shell{res}_{name}'] = (a, ca, b)
    return out


def _shell9():
    """All integer points with |x|^2 = 9: 6 of (+-3, 0, 0) and 24 of (+-1, +-2, +-2) -- 30 equidistant points."""
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij'), -1).reshape(-1, 3)
    s = g[(g ** 2).sum(1) == 9]
    assert len(s) == 30
    return s


def cases():
    """{name: (A, colours of A, B)}."""
    rng = np.random.default_rng(11)
    out = {}
    few = np.array([[5, 5, 5], [5, 6, 5], [9, 9, 9], [5, 5, 5], [40, 2, 7]])
    out['na1'] = (np.array([[6, 5, 5]]), colors(1, 1), few)                               # one voter, a tie of two, three fall back
    out['nb1'] = (few, colors(len(few), 2), np.array([[7, 7, 7]]))
    out['na1_nb1'] = (np.array([[0, 0, 0]]), colors(1, 3), np.array([[TOP, TOP, TOP]]))
    ident = np.unique(rng.integers(0, 40, (700, 3)), axis=0)
    out['identity'] = (ident, colors(len(ident), 4), ident.copy())
    # an A point in the middle of 30 equidistant B points (more than any register tie list), other A points elsewhere
    centre = np.array([100, 100, 100])
    a = np.concatenate([centre[None], centre + [[40, 0, 0], [0, 41, 1], [3, 0, 1]]])
    out['large_tie_set'] = (a, colors(len(a), 5), np.concatenate([centre + _shell9(), centre[None] + [[60, 60, 60]]]))
    out['rounding'] = (np.array([[10, 10, 10], [12, 10, 10]]), np.array([[0, 0, 1], [1, 0, 2]], np.uint8), np.array([[11, 10, 10]]))
    # B rows far from every A point: they collect no vote and fall back
    a = np.unique(rng.integers(0, 24, (300, 3)), axis=0)
    far = np.concatenate([a[::3] + [0, 0, 1], rng.integers(1 << 20, 1 << 21, (50, 3)), [[TOP, 0, 0]]])
    out['fallback_far'] = (a, colors(len(a), 6), far)
    a = sphere_shell(32)
    out['fallback_jitter'] = (a, colors(len(a), 7), decoded_variants(a, 32, 8)['jitter'])
    # duplicate positions in B (and in A)
    a = rng.integers(0, 12, (900, 3))
    b = rng.integers(0, 12, (400, 3))
    out['duplicates'] = (a, colors(len(a), 9), np.concatenate([b, b[:150], b[:20]]))
    # the corners of the domain, and points spread over all of it: many index cells, long searches
    corners = np.array([[x, y, z] for x in (0, TOP) for y in (0, TOP) for z in (0, TOP)])
    a = np.concatenate([corners, rng.integers(0, 1 << 21, (3000, 3))])
    b = np.concatenate([corners[::-1], [[0, 0, 1], [TOP, TOP, TOP - 1]], rng.integers(0, 1 << 21, (2000, 3))])
    out['domain_edges'] = (a, colors(len(a), 10), b)
    a = np.unique(rng.integers(0, 4, (60, 3)), axis=0) + [1000, 2000, 3000]
    out['single_cell'] = (a, colors(len(a), 12), np.unique(rng.integers(0, 4, (40, 3)), axis=0) + [1000, 2000, 3000])
    a = rng.integers(0, 256, (20000, 3))
    b = np.clip(a[rng.permutation(len(a))[:15000]] + rng.integers(-1, 2, (15000, 3)), 0, 255)
    out['random256'] = (a, colors(len(a), 13), b)
    # every vote of a 40 000-point A on one decoded point: the accumulators under the most contention there is
    a = rng.integers(0, 64, (40000, 3))
    out['many_voters'] = (a, np.full((len(a), 3), 255, np.uint8) - (np.arange(len(a))[:, None] % 3 == 0), np.array([[31, 33, 30]]))
    return {k: (np.asarray(a, np.int64), np.asarray(c, np.uint8), np.asarray(b, np.int64)) for k, (a, c, b) in out.items()}


def _tie_sets(src, dst, chunk=512):
    """All-pairs exact distances: (rows of src, rows of dst) of every pair in which dst is at the smallest squared distance from
    src.  |s|^2 + |d|^2 - 2 s.d in float64 is exact here: integers, every product and partial sum below 2^45."""
    rs, rd = [], []
    s, d = src.astype(np.float64), dst.astype(np.float64)
    s2, d2n = (s * s).sum(1), (d * d).sum(1)
    for lo in range(0, len(src), chunk):
        d2 = (s2[lo:lo + chunk, None] + d2n[None, :]) - 2.0 * (s[lo:lo + chunk] @ d.T)
        i, j = np.nonzero(d2 == d2.min(1, keepdims=True))
        rs.append(i + lo)
        rd.append(j)
    return np.concatenate(rs), np.concatenate(rd)


def transfer_brute(a, ca, b):
    """(colours uint8[N_B,3], votes int64[N_B]) by the rule as the header states it, O(N_A N_B)."""
    a, b, ca = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(ca, np.int64)
    sums, votes = np.zeros((len(b), 3), np.int64), np.zeros(len(b), np.int64)
    ia, jb = _tie_sets(a, b)
    np.add.at(sums, jb, ca[ia])
    np.add.at(votes, jb, 1)
    n = votes.copy()
    orphans = np.nonzero(votes == 0)[0]
    if len(orphans):
        ib, ja = _tie_sets(b[orphans], a)
        np.add.at(sums, orphans[ib], ca[ja])
        np.add.at(n, orphans[ib], 1)
    out = (2 * sums + n[:, None]) // (2 * n[:, None])
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), votes
