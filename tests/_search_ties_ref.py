"""Yardsticks of the tie-averaged threshold search (DESIGN.md 4.6 "search_ties mean"), on top of the brute-force tally of
tests/_ties_ref.py.  Nothing here is imported from the package.

Rounding bound of one (block, threshold) pair.  DESIGN.md 4.8.1 with the pair's own C, V, M (`_ties_ref.tally_ref`) and the
summation depth of the SEARCH engines instead of the whole-cloud one.  The host restatement sums its per-point terms with numpy's
pairwise sum: at most 26 + ceil(log2 n) additions on the path of a term.  The GPU search sums them in k_d2_ab's / k_d2_ba's form:
thread k of a 256-thread workgroup adds elements k, k + 256, ... of an array of L elements one by one, then an 8-level tree.  A -> B:
L = N_A (one element per row).  B -> A: L = the grid's voxel count, but only the voxels of B_t are non-zero and adding a zero is
exact, so a term runs through at most min(N_B, ceil(L / 256)) + 8 inexact additions.  Hence
    D_AB = max(26 + ceil(log2 N_A), 8 + ceil(N_A / 256))        D_BA = max(26 + ceil(log2 N_B), 8 + min(N_B, ceil(nvox / 256)))
and two computed values of a D2 slot differ by at most 2 u (2V + 7 + C + D) M.

Carried through the metric formulas (pc_metric.metrics_table; b_AB, b_BA = the slot bounds): the sums are the slots themselves;
mse_AB = sum_AB / N_A and mse_BA = sum_BA / N_B add one rounding each (u |value|); max() is 1-Lipschitz in each argument and exact;
sum_mean adds one addition and an exact halving.  The final operations' own roundings enter as 4 u |value| (at most two per value,
two values compared)."""
import math

import numpy as np

import _ties_ref as R

U = R.U


def depth_ab(n_a):
    return max(26 + math.ceil(math.log2(max(n_a, 2))), 8 + math.ceil(n_a / 256))


def depth_ba(n_b, nvox):
    return max(26 + math.ceil(math.log2(max(n_b, 2))), 8 + min(n_b, math.ceil(nvox / 256)))


def slot_bounds(ref, nvox):
    """(b_AB, b_BA): allowed |difference| of the D2_AB / D2_BA slots between two computed tallies of the pair behind `ref`."""
    k = 2 * ref['V'] + 7 + ref['C']
    n_a, n_b = ref['n']
    return 2 * U * (k + depth_ab(n_a)) * ref['M'][0], 2 * U * (k + depth_ba(n_b, nvox)) * ref['M'][1]


def metric_bound(name, b_ab, b_ba, n_a, n_b, value):
    """Allowed |difference| of metric `name` (a d2_* optimisation metric) between two computed tallies, see the module docstring."""
    stem = name.split('_', 1)[1]
    core = {'sum_AB': b_ab, 'sum_BA': b_ba, 'sum_max': max(b_ab, b_ba), 'sum_mean': (b_ab + b_ba) / 2, 'mse_AB': b_ab / n_a,
            'mse_BA': b_ba / n_b, 'mse': max(b_ab / n_a, b_ba / n_b)}[stem]
    return core + 4 * U * abs(value)


def level_sets(x_hat, thresholds):
    """[B_t int64 (n, 3)] for t = 0, 1, ... while non-empty: {v : clip(x_hat, 0, 1)[v] > float32(thresholds[t])} in argwhere order."""
    xh = np.clip(np.asarray(x_hat, np.float32), 0, 1)
    out = []
    for t in thresholds:
        b = np.argwhere(xh > np.float32(t))
        if len(b) == 0:
            break
        out.append(b.astype(np.int64))
    return out


def brute_tallies(block, x_hat, thresholds):
    """Per level set: (`_ties_ref.tally_ref` dict, (b_AB, b_BA)) of the block's rows (xyz + float64 normals) against B_t."""
    a, n = np.asarray(block)[:, :3].astype(np.int64), np.asarray(block)[:, 3:6].astype(np.float64)
    out = []
    for b in level_sets(x_hat, thresholds):
        ref = R.tally_ref(a, b, n)
        out.append((ref, slot_bounds(ref, int(np.prod(np.asarray(x_hat).shape)))))
    return out


def decisions(n_a, tallies, guard_tally, peak, metrics, max_deltas, table_fn, eligible_fn):
    """The search's choices restated step by step: [(name, pool, column, k, guard)] per (max_delta, metric), k = first minimum of
    the metric over the pool (index into pool)."""
    table, guard = table_fn(n_a, tallies, peak), table_fn(n_a, guard_tally, peak)
    everything = np.arange(len(tallies))
    out = []
    for d in max_deltas:
        pool = everything
        if d is not None:
            ok = everything[eligible_fn(tallies[:, 0], n_a, d)]
            pool = ok if len(ok) else everything
        for m in metrics:
            col = table[m][pool]
            out.append((f'{m}_{d}', pool, col, int(np.argmin(col)), float(guard[m])))
    return out


def metric_bounds(n_a, tallies, brute, names, table_fn, peak):
    """{metric: float64[T]}: allowed |difference| between two computed values of the metric at every level set (`brute`: brute_tallies)."""
    table = table_fn(n_a, tallies, peak)
    return {m: np.array([metric_bound(m, *brute[t][1], n_a, tallies[t, 0], table[m][t]) for t in range(len(tallies))]) for m in names}


def gap_failures(n_a, tallies, guard_tally, brute, peak, metrics, max_deltas, table_fn, eligible_fn):
    """The precondition of the exact-decision test, from HOST data only: per (max_delta, metric) the runner-up gap of the host
    restatement's minimum and its distance from the guard must exceed 2 beta (beta = the largest metric bound over the pool).  Level
    sets with the same voxel count are the same set (the sets are nested): they give the same bits on either engine and 'first
    minimum' takes the first of them, so they are no runners-up.  Returns [(name, t, gap, guard gap, 2 beta)] of the violations."""
    beta = metric_bounds(n_a, tallies, brute, metrics, table_fn, peak)
    bad = []
    for nm, pool, col, k, gv in decisions(n_a, tallies, guard_tally, peak, metrics, max_deltas, table_fn, eligible_fn):
        b = float(beta[nm.rsplit('_', 1)[0]][pool].max())
        other = tallies[pool, 0] != tallies[pool[k], 0]
        gap = float((col[other] - col[k]).min()) if other.any() else np.inf
        if not (gap > 2 * b and abs(col[k] - gv) > 2 * b):
            bad.append((nm, int(pool[k]), gap, abs(col[k] - gv), 2 * b))
    return bad


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def field(points, shape, seed, sharp=1.0, noise=0.02, floor=0.06):
    """A decoder-like occupancy estimate: the blurred occupancy of `points` plus seeded noise, minus a floor so that far voxels are
    exactly 0 after the clip (the level sets stay near the surface: the brute force stays cheap)."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    dense = np.zeros(shape, np.float32)
    dense[tuple(np.asarray(points)[:, :3].astype(int).T)] = 1
    return (gaussian_filter(dense, sharp) * 2.5 + rng.normal(0, noise, shape) - floor).astype(np.float32)


def blocks_32():
    """Three blocks on a 32^3 grid: a voxelised shell with radial normals (tie-heavy), a shell whose rows partly repeat with other
    normals (several rows in one voxel), a sparse random block.  Returns ([block float64 (n, 6)], x_hat float32 (3, 32, 32, 32))."""
    rng = np.random.default_rng(21)
    a0 = R.shell(11, 16)
    b0 = np.hstack([a0, R.radial_normals(a0, 16)])
    a1 = R.shell(6, 15)
    a1 = np.vstack([a1, a1[::4], a1[:30]])
    b1 = np.hstack([a1, R.unit_normals(len(a1), 31)])
    a2 = np.unique(rng.integers(3, 29, (220, 3)), axis=0)
    b2 = np.hstack([a2, R.unit_normals(len(a2), 32)])
    blocks = [b.astype(np.float64) for b in (b0, b1, b2)]
    x_hat = np.stack([field(b, (32, 32, 32), 40 + i, sharp=(1.0, 0.8, 0.7)[i]) for i, b in enumerate(blocks)])
    return blocks, x_hat


def blocks_odd():
    """Two blocks on a (20, 24, 12) grid (no axis a multiple of 16: the unfused distance-transform passes)."""
    rng = np.random.default_rng(22)
    shape = (20, 24, 12)
    out = []
    for n, seed in ((300, 51), (90, 52)):
        a = np.unique(np.stack([rng.integers(1, s - 1, n) for s in shape], 1), axis=0)
        out.append(np.hstack([a, R.unit_normals(len(a), seed)]).astype(np.float64))
    x_hat = np.stack([field(b, shape, 60 + i, sharp=0.9) for i, b in enumerate(out)])
    return out, x_hat
