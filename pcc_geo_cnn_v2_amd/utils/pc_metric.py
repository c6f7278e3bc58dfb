"""Point-to-point (D1) and point-to-plane (D2) distortion between an original cloud A and a decoded cloud B.

Same numbers as /root/reference/src/utils/pc_metric.py:76-138 (pinned by tests/golden/model_opt*.npz and select_best.npz, which
the reference's own module produced), organised differently: the KD-trees are only asked for nearest-neighbour INDICES
(`nearest`), the distortion is reduced to a five-number tally per cloud pair (`pair_tally`), and every derived quantity
(sum / mse / psnr, per direction and symmetric) comes from one table builder (`metrics_table`) that also works on whole arrays
of tallies -- the threshold search (model_opt.py) evaluates all thresholds of a block with one call, the GPU search feeds it
exact integer sums, and the multi-GPU path (sharding.py) all-reduces the tally before building the table.  `compute_metrics`
is the single-process, one-candidate case of `cloud_metrics_batch`.

Conventions: `to_b[i]` = index (into B) of the nearest decoded point of original point i; `to_a[j]` = index (into A) of the
nearest original point of decoded point j.  Arithmetic runs in whatever dtype numpy promotes the operands to, like the
reference (float32 PLY points against float64 departitioned blocks -> float64).
"""
import numpy as np
from scipy.spatial import cKDTree

GROUPS = ('d1', 'd2')
_OPT_STEMS = ('sum_AB', 'sum_BA', 'sum_max', 'sum_mean', 'mse_AB', 'mse_BA', 'mse')
# psnr is not offered for optimisation: it is monotone in mse (pc_metric.py:55)
avail_opt_metrics = [f'{g}_{stem}' for g in GROUPS for stem in _OPT_STEMS]      # the reference's order (pc_metric.py:57-58): --help and assertion texts print it

# slots of a tally vector (float64[5]); additive over disjoint parts of B (B->A terms) and of A (A->B terms)
N_B, D1_AB, D1_BA, D2_AB, D2_BA = range(5)
_TALLY_SLOTS = {'d1': (D1_AB, D1_BA), 'd2': (D2_AB, D2_BA)}
# the Hausdorff slots of a 9-slot tally (float64[9] = the five above + these): per-direction maxima of the per-point D1 / D2 terms
H1_AB, H1_BA, H2_AB, H2_BA = range(5, 9)
_HAUSDORFF_SLOTS = {'d1': (H1_AB, H1_BA), 'd2': (H2_AB, H2_BA)}


# new: the worst-point objectives of the per-block search, kept apart so that the reference's list above stays as it is
_HAUSDORFF_STEMS = ('hausdorff_AB', 'hausdorff_BA', 'hausdorff')
hausdorff_opt_metrics = [f'{g}_{stem}' for g in GROUPS for stem in _HAUSDORFF_STEMS]


def wants_hausdorff(opt_metrics):
    """Whether one of the opt metrics is a Hausdorff one: the search then carries 9-slot tallies (the maxima beside the sums)."""
    return any(m in hausdorff_opt_metrics for m in (opt_metrics or ()))


def validate_opt_metrics(opt_metrics, with_normals=False):
    unknown = [m for m in opt_metrics if m not in avail_opt_metrics and m not in hausdorff_opt_metrics]
    assert not unknown, f'{unknown[0] if unknown else None} not found in {avail_opt_metrics}'
    needs_normals = [m for m in opt_metrics if m.split('_', 1)[0] == 'd2']
    assert with_normals or not needs_normals, f'{needs_normals[0] if needs_normals else None} not available without normals'


def estimate_normals(ctx, points, k=16, viewpoint=None, return_knn=False):
    """Normals for the D2 terms when the cloud comes without a normals file: ops.estimate_normals (HIP, include/pcc_geo.h
    "point normals"), re-exported beside the metric code that consumes them.  Oriented away from the centroid (or `viewpoint`),
    so that transfer_normals' averages do not cancel."""
    from .. import ops
    return ops.estimate_normals(ctx, points, k=k, viewpoint=viewpoint, return_knn=return_knn)


def psnr(mse, max_energy):
    with np.errstate(divide='ignore'):
        return 10 * np.log10(max_energy / mse)


def nearest(tree, queries):
    """Index of the nearest tree point for every query point.  Large clouds use all cores (the reference always does,
    pc_metric.py:80-81); for the small per-block queries of the threshold search the thread start-up dominates."""
    if len(queries) == 0:
        return np.zeros(0, np.int64)
    return tree.query(queries, workers=-1 if max(tree.n, len(queries)) > 200000 else 1)[1]


def point_gap(src, dst, link):
    """Residual vectors src[i] - dst[link[i]]."""
    return src - dst[link]


def squared_norms(gap):
    return (gap ** 2).sum(axis=1)


def plane_error(gap, normals):
    """Sum over points of the squared projection of the residual on the normal."""
    return (((gap * normals).sum(axis=1)) ** 2).sum()


def transfer_normals(a_normals, to_a, to_b, a_mask=None):
    """Normals for the decoded points (pc_metric.py:8-25): decoded point j gets the mean normal of the original points that
    have j as THEIR nearest decoded point (restricted to `a_mask` when given); a decoded point nobody points to takes the
    normal of its own nearest original point.  bincount accumulates in index order, i.e. in the order of the reference's loop."""
    n_b = len(to_a)
    src, link = (a_normals, to_b) if a_mask is None else (a_normals[a_mask], to_b[a_mask])
    votes = np.bincount(link, minlength=n_b).astype(np.float64)
    acc = np.stack([np.bincount(link, weights=src[:, c], minlength=n_b) for c in range(src.shape[1])], axis=1)
    orphan = votes == 0
    acc[orphan] += a_normals[to_a[orphan]]
    votes[orphan] = 1
    return acc / votes[:, None]


def pair_tally(a, b, to_b, to_a, a_normals=None, a_mask=None):
    """float64[5] tally (N_B, D1_AB, D1_BA, D2_AB, D2_BA) of the pair (A, B).  `a_mask` limits the A->B terms to a subset of
    the original points (the multi-GPU path: the points whose nearest decoded point lives on this rank)."""
    tally = np.zeros(5, np.float64)
    tally[N_B] = len(b)
    if len(b) == 0:
        return tally
    gap_ab, gap_ba = point_gap(a, b, to_b), point_gap(b, a, to_a)
    if a_mask is not None:
        gap_ab = gap_ab[a_mask]
    tally[D1_AB] = squared_norms(gap_ab).sum()
    tally[D1_BA] = squared_norms(gap_ba).sum()
    if a_normals is not None:
        b_normals = transfer_normals(a_normals, to_a, to_b, a_mask)
        tally[D2_AB] = plane_error(gap_ab, b_normals[to_b if a_mask is None else to_b[a_mask]])
        tally[D2_BA] = plane_error(gap_ba, a_normals[to_a])
    return tally


def pair_tally_hausdorff(a, b, to_b, to_a, a_normals=None):
    """float64[9]: pair_tally's five slots plus the Hausdorff maxima, np.max over the per-point terms pair_tally sums (H1_AB, H1_BA and,
    with normals, H2_AB, H2_BA).  B must not be empty."""
    tally = np.zeros(9, np.float64)
    tally[:5] = pair_tally(a, b, to_b, to_a, a_normals)
    gap_ab, gap_ba = point_gap(a, b, to_b), point_gap(b, a, to_a)
    tally[H1_AB], tally[H1_BA] = squared_norms(gap_ab).max(), squared_norms(gap_ba).max()
    if a_normals is not None:
        b_normals = transfer_normals(a_normals, to_a, to_b)
        tally[H2_AB] = (((gap_ab * b_normals[to_b]).sum(axis=1)) ** 2).max()
        tally[H2_BA] = (((gap_ba * a_normals[to_a]).sum(axis=1)) ** 2).max()
    return tally


def metrics_table(n_a, tally, peak, groups=GROUPS):
    """The reference's metric dictionary (pc_metric.py:83-137) from tallies.  `tally` is float64[5] (-> scalars) or
    float64[T, 5] (-> arrays over T candidate clouds).  An empty B gives mse_BA = nan / psnr nan -- callers guard that.
    A 9-slot tally (float64[9] / float64[T, 9]) also gives the three Hausdorff columns of every group, hausdorff_table's values."""
    tally = np.asarray(tally, np.float64)
    n_b = tally[..., N_B]
    energy = 3 * peak * peak
    out = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for g in groups:
            s_ab, s_ba = (tally[..., k] for k in _TALLY_SLOTS[g])
            per_dir = {'AB': (s_ab, s_ab / n_a), 'BA': (s_ba, s_ba / n_b)}
            out[f'{g}_sum_AB'], out[f'{g}_sum_BA'] = s_ab, s_ba
            out[f'{g}_sum_max'] = np.maximum(s_ab, s_ba)
            out[f'{g}_sum_mean'] = (s_ab + s_ba) / 2
            for d, (_, mse) in per_dir.items():
                out[f'{g}_mse_{d}'] = mse
            out[f'{g}_mse'] = np.maximum(per_dir['AB'][1], per_dir['BA'][1])
            for d, (_, mse) in per_dir.items():
                out[f'{g}_psnr_{d}'] = psnr(mse, energy)
            out[f'{g}_psnr'] = np.minimum(out[f'{g}_psnr_AB'], out[f'{g}_psnr_BA'])
            if tally.shape[-1] == 9:
                h_ab, h_ba = (tally[..., k] for k in _HAUSDORFF_SLOTS[g])
                out[f'{g}_hausdorff_AB'], out[f'{g}_hausdorff_BA'], out[f'{g}_hausdorff'] = h_ab, h_ba, np.maximum(h_ab, h_ba)
    return out


class SingleProcess:
    """The world-size-1 communicator of `cloud_metrics_batch` (sharding.RankGroup is the torch.distributed one)."""
    rank, world = 0, 1

    def claim(self, sq_dist_ab, have_points):
        """Per candidate cloud: which original points have their globally nearest decoded point on this rank -- all of them
        here (None = no decoded point anywhere)."""
        return [np.ones(len(d), bool) if h else None for d, h in zip(sq_dist_ab, have_points)]

    def total(self, tallies):
        return tallies


def cloud_metrics_batch(p1, p2_locals, r, p1_n=None, t1=None, comm=None, partial=False, ties='pick'):
    """D1 (and, with normals `p1_n`, D2) metrics between the original cloud p1 (replicated on every rank) and each of several
    candidate decoded clouds, candidate m = union over ranks of `p2_locals[m]`.  Returns one reference-style dictionary per
    candidate (None where the decoded cloud is empty on every rank).  Two collectives for ALL candidates (one MIN, one SUM),
    none in a single process.  Exact for D1 in any world size (squared distances between integer points are integers; A->B is
    a MIN over ranks, B->A a SUM).  D2 across ranks: see sharding.RankGroup.claim.  ties='mean' (single process only): the D2
    slots come from tie_mean_tally, the tie-averaged rule of DESIGN.md "Tie-averaged D2"; D1 is the same either way."""
    comm = comm or SingleProcess()
    check_ties(ties, comm.world)
    tree_a = t1 if t1 is not None else cKDTree(p1, balanced_tree=False)
    links = []
    for p2 in p2_locals:
        p2 = np.asarray(p2).reshape(-1, 3)
        if len(p2):
            to_b = nearest(cKDTree(p2, balanced_tree=False), p1)
            links.append((p2, to_b, nearest(tree_a, p2), squared_norms(point_gap(p1, p2, to_b))))
        else:
            links.append((p2, np.zeros(len(p1), np.int64), np.zeros(0, np.int64), np.full(len(p1), np.inf)))
    owned = comm.claim([x[3] for x in links], [len(x[0]) > 0 for x in links])
    tallies = np.zeros((len(links), 5), np.float64)
    for m, ((p2, to_b, to_a, _), mine) in enumerate(zip(links, owned)):
        if mine is not None:
            tallies[m] = pair_tally(p1, p2, to_b, to_a, p1_n, None if mine.all() else mine)
            if ties == 'mean' and p1_n is not None:
                tallies[m, [D2_AB, D2_BA]] = tie_mean_tally(p1, p2, p1_n, tree_a)[[D2_AB, D2_BA]]
    if partial:     # the caller sums the per-rank tallies itself (they ride in a collective it issues anyway) and finishes with finish_metrics
        return tallies, [o is not None for o in owned]
    return finish_metrics(len(p1), comm.total(tallies), [o is not None for o in owned], r, p1_n is not None)


def finish_metrics(n_a, tallies, have, r, with_normals):
    """Reference-style metric dictionaries from the (globally summed) tallies of cloud_metrics_batch(..., partial=True)."""
    groups = GROUPS if with_normals else GROUPS[:1]
    return [metrics_table(n_a, tallies[m], r, groups) if have[m] else None for m in range(len(tallies))]


def compute_metrics(p1, p2, r, p1_n=None, t1=None):
    """The reference's entry point (pc_metric.py:76): metrics of decoded cloud p2 against original p1, peak value r."""
    assert len(p2), 'compute_metrics: empty decoded cloud'
    return cloud_metrics_batch(p1, [p2], r, p1_n, t1)[0]


# ---- Hausdorff terms and the GPU engine (include/pcc_geo.h "cloud metrics") ------------------------------------------------------
def hausdorff_table(tally, peak, with_normals=False):
    """pc_error's --hausdorff keys from 9-slot tallies: per group, '{g}_hausdorff_AB' / '_BA' (largest per-point squared error in
    each direction), '{g}_hausdorff' (the larger of the two) and '{g}_hausdorff_psnr' = 10 log10(3 peak^2 / {g}_hausdorff).  d2
    keys only with_normals.  Works on float64[9] (-> scalars) and float64[T, 9] (-> arrays)."""
    tally = np.asarray(tally, np.float64)
    out = {}
    for g in (GROUPS if with_normals else GROUPS[:1]):
        h_ab, h_ba = (tally[..., k] for k in _HAUSDORFF_SLOTS[g])
        out[f'{g}_hausdorff_AB'], out[f'{g}_hausdorff_BA'] = h_ab, h_ba
        out[f'{g}_hausdorff'] = np.maximum(h_ab, h_ba)
        out[f'{g}_hausdorff_psnr'] = psnr(out[f'{g}_hausdorff'], 3 * peak * peak)
    return out


def cloud_tally_host(p1, p2, p1_n=None, t1=None, ties='pick'):
    """Host restatement of the 9-slot tally with the KD-tree links of cloud_metrics_batch: pair_tally's five slots plus the
    Hausdorff maxima (np.max over the per-point terms pair_tally sums).  p2 must not be empty.  ties='mean': tie_mean_tally."""
    check_ties(ties)
    p2 = np.asarray(p2).reshape(-1, 3)
    assert len(p2), 'cloud_tally_host: empty decoded cloud'
    tree_a = t1 if t1 is not None else cKDTree(p1, balanced_tree=False)
    if ties == 'mean':
        return tie_mean_tally(p1, p2, p1_n, tree_a)
    to_b, to_a = nearest(cKDTree(p2, balanced_tree=False), p1), nearest(tree_a, p2)
    return pair_tally_hausdorff(p1, p2, to_b, to_a, p1_n)


def cloud_tallies_gpu(ctx, p1, p2_list, p1_n=None, index_a=None, ties='pick'):
    """9-slot tallies of every candidate decoded cloud against p1 on the GPU (ops.cloud_distortion): one float64[9] per candidate,
    None for an empty one.  The original cloud's index is built once (or `index_a` is reused) and every candidate is queued
    before the one host copy.  Neighbour ties go to the lowest row (include/pcc_geo.h "cloud metrics"): D1 and the D1 Hausdorff
    terms equal the host path's whenever its float64 sums are exact; D2 may differ where cKDTree picks another equidistant point.
    ties='mean': D2 averages over all equidistant points (DESIGN.md "Tie-averaged D2") and agrees with the host path's 'mean' up to
    float64 rounding.  Every candidate runs with the default pair capacity and its status rides in the one host copy; a candidate
    that reported more pairs than that is run once more with the exact number."""
    import torch
    from .. import ops
    check_ties(ties)
    clouds = [np.asarray(p2).reshape(-1, 3) for p2 in p2_list]
    live = [m for m, p2 in enumerate(clouds) if len(p2)]
    out = [None] * len(clouds)
    if not live:
        return out
    if index_a is None:
        index_a = ops.CloudIndex(ctx, np.asarray(p1)[:, :3])
    if ties == 'mean' and p1_n is not None:
        runs = [ops.cloud_distortion_launch(ctx, index_a, clouds[m], p1_n, ties='mean') for m in live]
        dev = [t for t, _ in runs]
        for k, (pairs, over) in enumerate(torch.stack([st for _, st in runs]).cpu().tolist()):
            if over:
                dev[k] = torch.from_numpy(ops.cloud_distortion(ctx, None, clouds[live[k]], p1_n, index_a=index_a, ties='mean',
                                                               max_pairs=pairs)).to(dev[k].device)
    else:
        dev = [ops.cloud_distortion_launch(ctx, index_a, clouds[m], p1_n) for m in live]
    host = torch.stack(dev).cpu().numpy()
    for m, t in zip(live, host):
        out[m] = t
    return out


def cloud_metrics_batch_gpu(ctx, p1, p2_list, r, p1_n=None, index_a=None, ties='pick'):
    """cloud_metrics_batch's single-process result computed on the GPU: one reference-style dictionary per candidate decoded cloud
    (None for an empty one), D1 and, with normals p1_n, D2.  Points are integer coordinates in [0, 2^21).  ties: cloud_tallies_gpu."""
    n_a = index_a.n if index_a is not None else len(p1)
    groups = GROUPS if p1_n is not None else GROUPS[:1]
    return [None if t is None else metrics_table(n_a, t[:5], r, groups) for t in cloud_tallies_gpu(ctx, p1, p2_list, p1_n, index_a, ties)]


# ---- tie-averaged D2 (DESIGN.md "Tie-averaged D2"; include/pcc_geo.h pcc_cloud_distortion_ties) ----------------------------------
TIES = ('pick', 'mean')     # pick: one neighbour per point (whichever the engine returns); mean: all equidistant nearest points


def check_ties(ties, world=1):
    """The tie rules of the D2 terms; 'mean' runs in one process (its tie sets are not sharded)."""
    if ties not in TIES:
        raise AssertionError(f'ties must be one of {TIES}, got {ties!r}')
    if ties == 'mean' and world > 1:
        raise AssertionError(f"ties 'mean' is single-process only (world size {world}): the sharded metric path picks one "
                             'neighbour per point, drop the flag or run on one GPU')


def tie_pairs(points, queries, tree=None, k=8):
    """All equidistant nearest points: (q, j, best) with one entry of q (query row, non-decreasing) and j (row of `points`) per member
    of a query's tie set -- every j at the smallest squared distance best[q] (int64[nq], exact: integer coordinates below 2^21).  The
    KD-tree proposes k candidates per query and distances are recomputed in integers; a query whose k candidates all tie takes its
    set from a ball query instead."""
    p, q = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    pi, qi = p.astype(np.int64), q.astype(np.int64)
    k = min(k, len(p))
    tree = tree if tree is not None else cKDTree(p, balanced_tree=False)
    _, cand = tree.query(q, k=k, workers=-1 if max(len(p), len(q)) > 200000 else 1)
    cand = cand.reshape(len(q), k)
    d2 = ((pi[cand] - qi[:, None, :]) ** 2).sum(-1)
    best = d2.min(1)
    tie = d2 == best[:, None]
    incomplete = np.nonzero(tie.all(1) & (k < len(p)))[0]
    tie[incomplete] = False
    rows, cols = np.nonzero(tie)
    qs, js = [rows], [cand[rows, cols]]
    if len(incomplete):
        balls = tree.query_ball_point(q[incomplete], np.sqrt(best[incomplete].astype(np.float64)) * (1 + 1e-12) + 1e-9)
        for i, nb in zip(incomplete, balls):
            nb = np.sort(np.asarray(nb, np.int64))
            nb = nb[((pi[nb] - qi[i]) ** 2).sum(-1) == best[i]]
            qs.append(np.full(len(nb), i, np.int64))
            js.append(nb)
        qs, js = np.concatenate(qs), np.concatenate(js)
        order = np.argsort(qs, kind='stable')
        return qs[order], js[order], best
    return qs[0], js[0], best


def plane_terms(gap, normals):
    """Per-point squared projection ((g.x n.x + g.y n.y) + g.z n.z)^2, every operation rounded: plane_error's terms."""
    return ((gap * normals).sum(axis=1)) ** 2


def tie_mean_tally(p1, p2, p1_n=None, t1=None):
    """The 9-slot tally under ties = 'mean' on the host (the definition of DESIGN.md "Tie-averaged D2", which the GPU engine's
    pcc_cloud_distortion_ties restates): the normal of a decoded point is the mean normal of the original points that have it in
    their tie set (bincount: summed in increasing original row), or of its own tie set when nobody does; each point's term is the
    mean plane term over its tie set.  With singleton tie sets every operation is pair_tally's: the same bits."""
    a, b = np.asarray(p1, np.float64)[:, :3], np.asarray(p2, np.float64).reshape(-1, 3)
    assert len(b), 'tie_mean_tally: empty decoded cloud'
    qa, jb, d_ab = tie_pairs(b, a)
    qb, ja, d_ba = tie_pairs(a, b, t1)
    tally = np.zeros(9, np.float64)
    tally[N_B] = len(b)
    tally[D1_AB], tally[D1_BA] = d_ab.astype(np.float64).sum(), d_ba.astype(np.float64).sum()
    tally[H1_AB], tally[H1_BA] = d_ab.max(), d_ba.max()
    if p1_n is None:
        return tally
    n_a = np.asarray(p1_n, np.float64)
    votes = np.bincount(jb, minlength=len(b)).astype(np.float64)
    acc = np.stack([np.bincount(jb, weights=n_a[qa, c], minlength=len(b)) for c in range(3)], axis=1)
    orphan = votes == 0
    if orphan.any():
        own = orphan[qb]
        acc[orphan] = np.stack([np.bincount(qb[own], weights=n_a[ja[own], c], minlength=len(b)) for c in range(3)], axis=1)[orphan]
        votes[orphan] = np.bincount(qb[own], minlength=len(b))[orphan]
    n_b = acc / votes[:, None]
    t_ab = np.bincount(qa, weights=plane_terms(a[qa] - b[jb], n_b[jb]), minlength=len(a)) / np.bincount(qa, minlength=len(a))
    t_ba = np.bincount(qb, weights=plane_terms(b[qb] - a[ja], n_a[ja]), minlength=len(b)) / np.bincount(qb, minlength=len(b))
    tally[D2_AB], tally[D2_BA] = t_ab.sum(), t_ba.sum()
    tally[H2_AB], tally[H2_BA] = t_ab.max(), t_ba.max()
    return tally


# ---- colour distortion (include/pcc_geo.h "cloud colours") -------------------------------------------------------------------
COLOR_KEYS = ('y', 'u', 'v')
# BT.709 RGB -> YUV rows; each term is evaluated as ((w0 dR + w1 dG) + w2 dB), every operation rounded
BT709 = ((0.2126, 0.7152, 0.0722), (-0.1146, -0.3854, 0.5), (0.5, -0.4542, -0.0458))


def color_table(tally, n_a, n_b):
    """pc_error's colour keys from 6-slot colour tallies (ops.cloud_color_distortion / color_tally_host): per channel c of y, u, v,
    '{c}_mse' = max(A->B sum / n_a, B->A sum / n_b) and '{c}_psnr' = psnr(mse, 255^2).  Works on float64[6] (-> scalars) and
    float64[T, 6] (-> arrays)."""
    tally = np.asarray(tally, np.float64)
    out = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for c, k in enumerate(COLOR_KEYS):
            out[f'{k}_mse'] = np.maximum(tally[..., c] / n_a, tally[..., 3 + c] / n_b)
        for k in COLOR_KEYS:
            out[f'{k}_psnr'] = psnr(out[f'{k}_mse'], 255 ** 2)
    return out


def yuv_terms(c_q, mean):
    """(n,3) float64 squared BT.709 errors of colours c_q against mean colours, in the operation order of the GPU engine."""
    d = np.asarray(c_q, np.float64) - mean
    out = np.empty_like(d)
    for k, (w0, w1, w2) in enumerate(BT709):
        e = (w0 * d[:, 0] + w1 * d[:, 1]) + w2 * d[:, 2]
        out[:, k] = e * e
    return out


def tie_mean_colors(points, colors, queries, k=16):
    """(nq,3) float64 mean colour of ALL points at the smallest squared distance from each query (exact integer sums over the
    equidistant set, divided once).  Coordinates are integers: distances are recomputed exactly from the candidates of a k-nearest
    query, and a query whose candidates all lie at that distance takes the equidistant set from an exact ball query."""
    p, q = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    col = np.asarray(colors, np.int64)
    k = min(k, len(p))
    tree = cKDTree(p, balanced_tree=False)
    _, cand = tree.query(q, k=k, workers=-1 if max(len(p), len(q)) > 200000 else 1)
    cand = cand.reshape(len(q), k)
    d2 = ((p[cand] - q[:, None, :]) ** 2).sum(-1)                     # exact: integer coordinates below 2^21
    best = d2.min(1)
    tie = d2 == best[:, None]
    sums = (col[cand] * tie[..., None]).sum(1)
    count = tie.sum(1)
    incomplete = np.nonzero(tie.all(1) & (k < len(p)))[0]
    if len(incomplete):
        balls = tree.query_ball_point(q[incomplete], np.sqrt(best[incomplete]) * (1 + 1e-12) + 1e-9)
        for i, nb in zip(incomplete, balls):
            nb = np.asarray(nb, np.int64)
            nb = nb[((p[nb] - q[i]) ** 2).sum(-1) == best[i]]
            sums[i], count[i] = col[nb].sum(0), len(nb)
    return sums.astype(np.float64) / count[:, None].astype(np.float64)


def transfer_colors_host(points, colors, queries):
    """Host restatement of ops.transfer_colors (include/pcc_geo.h "cloud colours", DESIGN.md §4.9 "Colour transfer"): (colours
    uint8[nq,3], votes int64[nq]).  Every row of `points` votes for all rows of `queries` in its tie set (tie_pairs: the exact
    equidistant nearest set, ball query included); a query row takes the exact integer sums of its voters' colours, or, with no
    voter, of its own tie set in `points`; colour = (2 S + n) // (2 n), the mean rounded half up.  votes is 0 where a row fell back."""
    p, q = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    col = np.asarray(colors, np.int64).reshape(-1, 3)
    assert len(p) and len(q) and len(col) == len(p), 'transfer_colors_host: empty cloud or colours that do not match the points'
    nq = len(q)
    qa, jb, _ = tie_pairs(q, p)                                   # original row qa votes for query row jb
    # bincount adds in float64: exact, every sum is an integer below 255 * 2^31 < 2^53
    gather = lambda to, frm, n: np.stack([np.bincount(to, weights=col[frm, c], minlength=n) for c in range(3)], axis=1).astype(np.int64)
    votes = np.bincount(jb, minlength=nq).astype(np.int64)
    sums = gather(jb, qa, nq)
    count = votes.copy()
    rows = np.nonzero(votes == 0)[0]
    if len(rows):
        qb, ja, _ = tie_pairs(p, q[rows])                         # query row rows[qb] against its own tie set ja
        sums[rows] = gather(qb, ja, len(rows))
        count[rows] = np.bincount(qb, minlength=len(rows))
    out = (2 * sums + count[:, None]) // (2 * count[:, None])
    return out.astype(np.uint8), votes


def color_tally_host(p1, c1, p2, c2):
    """Host restatement of the colour tally of ops.cloud_color_distortion (scipy KD-trees): float64[6] = the sums of eY^2, eU^2,
    eV^2 of every original point against the mean colour of its equidistant nearest decoded points, then the same for the decoded
    points against the original.  p1, p2: integer coordinates; c1, c2: (n,3) colours in 0..255; neither cloud may be empty."""
    assert len(p1) and len(p2), 'color_tally_host: empty cloud'
    tally = np.zeros(6, np.float64)
    tally[:3] = yuv_terms(c1, tie_mean_colors(p2, c2, p1)).sum(0)
    tally[3:] = yuv_terms(c2, tie_mean_colors(p1, c1, p2)).sum(0)
    return tally
