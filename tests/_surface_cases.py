"""Adversarial vertex sets and point clouds for the surface anchor codec, for tests/test_surface_cases_cpu.py (the
numpy host path) and tests/test_surface_cases_gpu.py (csrc/surface_anchor.hip).  Needs numpy and tests/_surface_ref.py only; every
draw has a fixed seed.  The expected results are the restatement's, computed once per case (`reference`, `near_reference`).

A decoder case is a `Case`: (leaves, edges, flags, ts, k, resolution) as R.reconstruction takes them, the same as uint64 / uint8
arrays for the package, and one tag per leaf.  Inputs stay inside the contract: the edge list is the sorted complete one of the
leaves, t < W, flags in {0, 1}, t = 0 without a flag.

  patterns(k, mode)   one isolated leaf per pattern p of flagged edges, at the even lattice coordinates (2 (p >> 8), 2 (p >> 4 & 15),
                      2 (p & 15)): no two leaves share an edge.  Bit e of p is edge e = 4 a + 2 du + dv (R.leaf_edges, the kernel's
                      lane).  t per mode: 'zero', 'top' (W - 1), 'ends' (0 or W - 1), 'rand'.  k = 2, 3 take all 4096 patterns.  The
                      restatement's cost grows with W^2, so from k = 4 on the patterns are thinned by a fixed rule (`pattern_subset`):
                      T = the multiples of 13 (0 and 4095 are two) and every pattern with m <= 1 or m >= 11 vertices, ascending: 340
                      patterns with every m = 0 .. 12; mode number j takes T[j::4] and the patterns 0 and 4095, so the four modes of
                      one k cover T between them.
  shared(k, n, tmode, clipped)   the first n leaves, in Morton order, of the 3 x 3 x 3 block, all edges flagged: faces and edges
                      shared; n in SHARED_SIZES has every residue mod 4 (the partial last workgroup of the four-leaf layout).  The t of
                      an edge does not depend on n.  Resolution 3 W - 1, or 2 W + 1 where the clip folds the top layer onto a plane.
  searched_leaves(k)  the literals of SEARCHED, isolated, scaled to W: configurations from an exhaustive search (below).
  near_sets(k)        encoder clouds: a lattice around every near-set boundary, 81 one-point clouds, rounding runs.

SEARCHED comes from an exhaustive search over every choice of m edges and every t, m <= 5 at k = 2 and m <= 4 at k = 3.  Each literal
is (name, k it was found at, ((edge, t), ...), note); at a larger k every t is multiplied by W / W_found, which multiplies every d_i by
the same factor: halves, zero cross products, equal norms and spread ties all survive.

The norm rule (same half plane, cross product 0, different norms: the smaller norm first) fires in the searched space -- in 36, 36
and 6 configurations with m = 3, 4, 5 at k = 2 and in 108 and 84 with m = 3, 4 at k = 3 -- and the literals 'norm_*' are such
leaves, but in none of them does reversing the rule change the leaf's voxels; the same holds for the few pattern leaves that fire it
(3 at k = 2, 6 at k = 3, none above).  So RULES has no mutant for it: the literals stay, but no test here can tell a kernel that
ranks them the other way.  The search
found three-way ties of the dominant axis, leaves with an area2 == 0 triangle in each projection and vertices at the centroid's
projection (half 2); for the first, literals where taking the last axis changes the voxels were chosen.
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import _surface_ref as R

KS = (2, 3, 4, 5, 6)
MODES = ('zero', 'top', 'ends', 'rand')
SHARED_SIZES = (1, 2, 3, 5, 6, 27)
SHARED_TMODES = ('rand', 'ends')
RULES = ('index', 'dom_last', 'drop_last', 'skip_dom', 'no_swap', 'open', 'floor', 'half_down')

Case = namedtuple('Case', 'name leaves edges flags ts k resolution leaf_keys edge_keys flags8 t8 tags')
Cloud = namedtuple('Cloud', 'name points resolution axis offsets')


def popcount(p):
    return bin(p).count('1')


def _case(name, leaves, vertex, k, resolution, tags):
    """Leaves in any order and {edge key: t} of the flagged edges -> Case, leaves and edges in their coded order."""
    order = sorted(range(len(leaves)), key=lambda i: R.morton(leaves[i]))
    leaves = [tuple(leaves[i]) for i in order]
    edges = R.edge_list(leaves)
    assert set(vertex) <= set(e[0] for e in edges) and all(0 <= t < 1 << k for t in vertex.values()), name
    flags = [1 if key in vertex else 0 for key, _, _ in edges]
    ts = [vertex.get(key, 0) for key, _, _ in edges]
    arrays = (np.array([R.morton(b) for b in leaves], np.uint64), np.array([e[0] for e in edges], np.uint64), np.array(flags, np.uint8),
              np.array(ts, np.uint8))
    for a in arrays:
        a.setflags(write=False)
    return Case(name, leaves, edges, flags, ts, k, resolution, *arrays, [tags[i] for i in order])


def leaf_vertices(case):
    """-> per leaf the vertices relative to its origin, in edge-key order: what R.reconstruction hands R.leaf_voxels."""
    W = 1 << case.k
    where = {key: n for n, (key, _, _) in enumerate(case.edges)}
    for b in case.leaves:
        mine = []
        for key, c, a in R.leaf_edges(b):
            n = where[key]
            if case.flags[n]:
                r = [W * (c[x] - b[x]) for x in range(3)]
                r[a] += case.ts[n]
                mine.append((n, r))
        yield [r for _, r in sorted(mine)]


# ---- patterns --------------------------------------------------------------------------------------------------------------------
def pattern_subset(k, mode):
    if k <= 3:
        return list(range(4096))
    T = [p for p in range(4096) if p % 13 == 0 or popcount(p) <= 1 or popcount(p) >= 11]
    return sorted(set(T[MODES.index(mode)::4]) | {0, 4095})


def _pattern_ts(k, mode):
    """(4096, 12): the t of every edge of every pattern, whether flagged or not: a subset draws what the whole set draws."""
    W = 1 << k
    rng = np.random.default_rng(4160 + 10 * k + MODES.index(mode))
    if mode == 'zero':
        return np.zeros((4096, 12), np.int64)
    if mode == 'top':
        return np.full((4096, 12), W - 1)
    if mode == 'ends':
        return rng.integers(0, 2, (4096, 12)) * (W - 1)
    return rng.integers(0, W, (4096, 12))


def _isolated(i):
    return (2 * (i >> 8), 2 * (i >> 4 & 15), 2 * (i & 15))


@functools.lru_cache(maxsize=None)
def patterns(k, mode):
    tt = _pattern_ts(k, mode)
    leaves, vertex, tags = [], {}, []
    for p in pattern_subset(k, mode):
        leaves.append(_isolated(p))
        tags.append(p)
        for e, (key, _, _) in enumerate(R.leaf_edges(leaves[-1])):
            if p >> e & 1:
                vertex[key] = int(tt[p, e])
    return _case(f'patterns-k{k}-{mode}', leaves, vertex, k, 32 << k, tags)


# ---- shared faces ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared(k, n, tmode, clipped):
    W = 1 << k
    block = sorted(((x, y, z) for x in range(3) for y in range(3) for z in range(3)), key=R.morton)
    rng = np.random.default_rng(4170 + 10 * k + SHARED_TMODES.index(tmode))
    every = R.edge_list(block)
    draw = rng.integers(0, W, len(every)) if tmode == 'rand' else rng.integers(0, 2, len(every)) * (W - 1)
    t_of = {key: int(t) for (key, _, _), t in zip(every, draw)}
    leaves = block[:n]
    vertex = {key: t_of[key] for key, _, _ in R.edge_list(leaves)}
    return _case(f'shared-k{k}-n{n}-{tmode}-{"clipped" if clipped else "open"}', leaves, vertex, k, 2 * W + 1 if clipped else 3 * W - 1,
                 list(range(n)))


# ---- literals from the exhaustive search ---------------------------------------------------------------------------------------
SEARCHED = (
    ('norm_m3', 2, ((0, 0), (1, 0), (8, 1)), 'norm rule: three vertices on one line, two on one side of the centroid; every triangle is flat'),
    ('norm_m4', 2, ((0, 0), (1, 0), (5, 0), (8, 1)), 'norm rule beside a coincident pair'),
    ('norm_m5', 2, ((0, 0), (2, 0), (4, 3), (8, 0), (9, 0)), 'norm rule at m = 5, the only shape of it there (6 configurations)'),
    ('norm_k3', 3, ((0, 0), (1, 0), (4, 0), (8, 3)), 'norm rule with an odd t: not a scaled k = 2 leaf'),
    ('dom3_m4', 2, ((0, 0), (1, 0), (2, 0), (6, 0)), 'three-way tie of the dominant axis; taking the last axis changes the voxels'),
    ('dom3_m5', 2, ((0, 0), (1, 0), (2, 0), (4, 2), (6, 0)), 'three-way tie of the dominant axis at m = 5; the last axis changes the voxels'),
    ('dom3_k3', 3, ((0, 6), (1, 7), (4, 3), (9, 3)), 'three-way tie of the dominant axis away from the corners'),
    ('area0_each_m3', 2, ((0, 0), (8, 0), (9, 1)), 'a triangle with area2 == 0 in each of the three projections'),
    ('area0_each_m4', 2, ((0, 0), (1, 0), (4, 0), (10, 1)), 'the same at m = 4'),
    ('area0_each_m5', 2, ((0, 0), (1, 0), (2, 0), (5, 0), (10, 1)), 'the same at m = 5'),
    ('half2_m3', 2, ((0, 0), (1, 0), (8, 2)), 'a vertex at the projection of the centroid (half 2), on a line'),
    ('half2_m5', 2, ((0, 0), (2, 0), (4, 2), (8, 0), (9, 0)), 'a vertex at the projection of the centroid among five'),
)


def searched():
    return SEARCHED


@functools.lru_cache(maxsize=None)
def searched_leaves(k):
    leaves, vertex, tags = [], {}, []
    for i, (name, found_at, verts, _) in enumerate(SEARCHED):
        if found_at > k:
            continue
        leaves.append(_isolated(i))
        tags.append(name)
        keys = R.leaf_edges(leaves[-1])
        for e, t in verts:
            vertex[keys[e][0]] = t << (k - found_at)
    return _case(f'searched-k{k}', leaves, vertex, k, 32 << k, tags)


# ---- the restatement's results, once per case ------------------------------------------------------------------------------------
FAMILIES = {'patterns': patterns, 'shared': shared, 'searched': searched_leaves}


def decoder_cases(k):
    """(family, args) of every decoder case at k."""
    return ([('searched', (k,))] + [('shared', (k, n, tmode, clipped)) for tmode in SHARED_TMODES for n in SHARED_SIZES for clipped in (False, True)]
            + [('patterns', (k, mode)) for mode in MODES])


@functools.lru_cache(maxsize=None)
def reference(family, args):
    """-> (case, dict(decoded, counts per leaf before the clip, clipped = voxels the clip moved)): computed once, shared, read only."""
    case = FAMILIES[family](*args)
    decoded, leafwise = R.reconstruction(case.leaves, case.edges, case.flags, case.ts, case.k, case.resolution, per_leaf=True)
    decoded.setflags(write=False)
    W = 1 << case.k
    clipped = sum(1 for b, rel in zip(case.leaves, leafwise) for vox in rel if max(W * b[x] + vox[x] for x in range(3)) > case.resolution - 1)
    counts = np.array([len(rel) for rel in leafwise], np.int64)
    counts.setflags(write=False)
    return case, dict(decoded=decoded, counts=counts, clipped=clipped)


# ---- what a leaf exercises, and the mutants ------------------------------------------------------------------------------------
def _fan(rs, rule=None):
    """-> (G, spread, dom, xy, angular order) of a leaf with m >= 3 vertices, as R.leaf_voxels has them; `rule` names a mutation."""
    m = len(rs)
    G = [sum(r[a] for r in rs) for a in range(3)]
    d = [[m * r[a] - G[a] for a in range(3)] for r in rs]
    spread = [sum(di[a] ** 2 for di in d) for a in range(3)]
    dom = 2 - spread[::-1].index(min(spread)) if rule == 'dom_last' else spread.index(min(spread))
    pu, pv = R.others(dom)
    xy = [(di[pu], di[pv]) for di in d]

    def compare(i, j):
        hi, hj = R.half(*xy[i]), R.half(*xy[j])
        if hi != hj:
            return -1 if hi < hj else 1
        cr = R.cross(xy[i][0], xy[i][1], xy[j][0], xy[j][1])
        if cr != 0:
            return -1 if cr > 0 else 1
        ni, nj = xy[i][0] ** 2 + xy[i][1] ** 2, xy[j][0] ** 2 + xy[j][1] ** 2
        if ni != nj:
            return (-1 if ni < nj else 1) * (-1 if rule == 'norm' else 1)
        return (-1 if i < j else 1 if i > j else 0) * (-1 if rule == 'index' else 1)

    return G, spread, dom, xy, sorted(range(m), key=functools.cmp_to_key(compare))


def mutant_voxels(rs, W, rule=None):
    """R.leaf_voxels with one rule of the definition changed, by name (RULES, and 'norm'); None changes nothing."""
    m = len(rs)
    if m == 0:
        return {(W // 2, W // 2, W // 2)}
    out = set(tuple(r) for r in rs)
    if m < 3:
        return out
    G, _, dom, _, s = _fan(rs, rule)
    for j in range(m - 1 if rule == 'drop_last' else m):
        A, B, C = G, [m * v for v in rs[s[j]]], [m * v for v in rs[s[(j + 1) % m]]]
        for q in range(3):
            if rule == 'skip_dom' and q == dom:
                continue
            u, v = R.others(q)
            Bq, Cq = B, C
            area2 = R.cross(Bq[u] - A[u], Bq[v] - A[v], Cq[u] - A[u], Cq[v] - A[v])
            if area2 == 0:
                continue
            if area2 < 0 and rule != 'no_swap':
                Bq, Cq = C, B
            for i in range(W + 1):
                for jj in range(W + 1):
                    Pu, Pv = m * i, m * jj
                    la = R.cross(Cq[u] - Bq[u], Cq[v] - Bq[v], Pu - Bq[u], Pv - Bq[v])
                    lb = R.cross(A[u] - Cq[u], A[v] - Cq[v], Pu - Cq[u], Pv - Cq[v])
                    lc = R.cross(Bq[u] - A[u], Bq[v] - A[v], Pu - A[u], Pv - A[v])
                    if min(la, lb, lc) < 0 or (rule == 'open' and min(la, lb, lc) == 0):
                        continue
                    lam = la + lb + lc                                     # = area2 > 0: without the swap a sum < 0 never gets here
                    num = la * A[q] + lb * Bq[q] + lc * Cq[q]
                    if rule == 'floor':
                        h = num // (m * lam)
                    elif rule == 'half_down':
                        h = -((m * lam - 2 * num) // (2 * m * lam))
                    else:
                        h = (2 * num + m * lam) // (2 * m * lam)
                    vox = [0, 0, 0]
                    vox[q], vox[u], vox[v] = h, i, jj
                    out.add(tuple(vox))
    return out


EVENTS = ('coincident', 'index', 'norm', 'half2', 'dom2', 'dom3', 'area0', 'area0_each')


def leaf_events(rs):
    """-> the set of EVENTS a leaf shows.  coincident: two vertices at one point; index / norm: a pair of vertices that the index / the
    norm rule orders (every pair counts: the kernel compares all of them); half2: a vertex at the centroid's projection; dom2 / dom3:
    two / three axes share the least spread; area0: a fan triangle with area2 == 0 in a projection; area0_each: one in each."""
    m = len(rs)
    found = set()
    if len(set(tuple(r) for r in rs)) < m:
        found.add('coincident')
    if m < 3:
        return found
    G, spread, _, xy, s = _fan(rs)
    ties = spread.count(min(spread))
    if ties > 1:
        found.add('dom2' if ties == 2 else 'dom3')
    if (0, 0) in xy:
        found.add('half2')
    halves, norms = [R.half(*p) for p in xy], [p[0] ** 2 + p[1] ** 2 for p in xy]
    for i in range(m):
        for j in range(i + 1, m):
            if halves[i] == halves[j] and xy[i][0] * xy[j][1] == xy[i][1] * xy[j][0]:
                found.add('index' if norms[i] == norms[j] else 'norm')
    flat = set()
    for j in range(m):
        B, C = [m * v for v in rs[s[j]]], [m * v for v in rs[s[(j + 1) % m]]]
        for q in range(3):
            u, v = R.others(q)
            if R.cross(B[u] - G[u], B[v] - G[v], C[u] - G[u], C[v] - G[v]) == 0:
                flat.add(q)
    if flat:
        found.add('area0')
    if len(flat) == 3:
        found.add('area0_each')
    return found


@functools.lru_cache(maxsize=None)
def census(k):
    """-> ({m: leaves}, {event: leaves}, {residue of the leaf count mod 4: cases}) over every decoder case at k."""
    by_m, by_event, residues = {}, {e: 0 for e in EVENTS}, {}
    for family, args in decoder_cases(k):
        case = FAMILIES[family](*args)
        residues[len(case.leaves) % 4] = residues.get(len(case.leaves) % 4, 0) + 1
        for rs in leaf_vertices(case):
            by_m[len(rs)] = by_m.get(len(rs), 0) + 1
            for e in leaf_events(rs):
                by_event[e] += 1
    return by_m, by_event, residues


# ---- encoder clouds --------------------------------------------------------------------------------------------------------------
def _edge_points(W, a, triples):
    """(off, eu, ev) around the interior edge (corner (1, 1, 1), axis a) -> points."""
    u, v = R.others(a)
    pts = np.zeros((len(triples), 3), np.int64)
    for n, (off, eu, ev) in enumerate(triples):
        pts[n, a], pts[n, u], pts[n, v] = W + off, W + eu, W + ev
    return pts


def rounding_runs(W):
    """{name: [(off, eu, ev)]}: runs on one edge.  A mean that ends in .5 needs an even count; the three-point runs sit a third off."""
    return {'two_low': [(0, 0, 0), (1, 0, 0)], 'two_high': [(W - 2, 0, 0), (W - 1, 0, 0)], 'two_columns': [(1, -1, 0), (2, 1, 0)],
            'two_far_apart': [(0, 0, -1), (W - 1, 0, 1)], 'three_down': [(0, 0, 0), (0, 1, 0), (1, 0, 0)], 'three_up': [(0, 0, 0), (1, 1, 0), (1, 0, 0)],
            'three_top': [(W - 1, 0, 0), (W - 1, -1, 1), (W - 2, 0, 0)], 'four_half': [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1)],
            'full_run': [(off, eu, ev) for off in range(W) for eu in (-1, 0, 1) for ev in (-1, 0, 1)]}


def rounded_mean(offsets):
    """-> (t by the definition, whether the mean ends in exactly .5) in exact fractions."""
    mean = Fraction(sum(offsets), len(offsets))
    return math.floor(mean + Fraction(1, 2)), mean.denominator == 2


@functools.lru_cache(maxsize=None)
def near_sets(k):
    """-> tuple of Cloud(name, points, resolution, axis, offsets): axis and the run's offsets where the cloud is one run on the interior
    edge (corner (1, 1, 1), axis); a point of it at an end of the edge is near edges of the other axes as well."""
    W = 1 << k
    res = 3 * W - 1
    axis = sorted(set(v for c in range(3) for v in (W * c - 1, W * c, W * c + 1, W * c + 2, W * c + W // 2, W * c + W - 2) if 0 <= v < res))
    full = np.array([(x, y, z) for x in axis for y in axis for z in axis], np.int64)
    keep = np.random.default_rng(4180 + k).random(len(full)) < 0.15
    out = [Cloud('lattice_full', full, res, None, None), Cloud('lattice_15', full[keep], res, None, None)]
    for a in range(3):
        for eu in (-1, 0, 1):
            for ev in (-1, 0, 1):
                for off in (0, 1, W - 1):
                    out.append(Cloud(f'one_a{a}_u{eu}_v{ev}_off{off}', _edge_points(W, a, [(off, eu, ev)]), res, a, (off,)))
        for name, triples in rounding_runs(W).items():
            out.append(Cloud(f'{name}_a{a}', _edge_points(W, a, triples), res, a, tuple(t[0] for t in triples)))
    for c in out:
        c.points.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def near_reference(k, name):
    cloud = {c.name: c for c in near_sets(k)}[name]
    return R.coded_points(cloud.points, cloud.resolution, k)
