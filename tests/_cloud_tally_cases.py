"""The cases behind tests/golden/cloud_tally_bits.json: the bits of the whole-cloud distortion tallies (ops.cloud_distortion under both
tie rules, ops.cloud_color_distortion) and of the D2 threshold searches (ops.d12_threshold_stats, ops.d12_threshold_stats_ties).

The other GPU tests compare these sums with host restatements to 1e-12 or a rounding bound, which a changed summation order passes.
Here every output is recorded: float64 tallies and int64 status words as the hex of their bytes, arrays (links, per-threshold
columns) as a blake2b-128 digest of theirs.  tests/golden/make_cloud_tally_bits.py writes the file, tests/test_cloud_tally_bits_gpu.py
recomputes and compares; both call the run_* functions below, so a case is stated once.

Inputs: every pair of _metrics_ref.cloud_pairs() and _ties_ref.cases(), every pair of _color_ref.color_pairs(), and one pair above
256 * 1024 points a side (LARGE): below that size every thread of the tally adds at most one point, so neither its grid-stride loop
nor the cap on its grid is exercised.  Search: two 16^3 and two 32^3 blocks of the adversarial catalogue, 256 thresholds (four chunks
of the tie-averaged engine, which holds at most 64), and one tie-averaged call whose capacity overflows in exactly one chunk."""
import functools
import os

import numpy as np
import torch

import _bits_ref as BR
import _color_ref as CR
import _metrics_ref as MR
import _search_adversarial as SA
import _search_ties_ref as S
import _ties_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cloud_tally_bits.json')
LARGE, LARGE_EDGE = 'lattice_box_67', 67         # 67^3 = 300763 points > 256 * 1024 = 262144
OVERFLOW = 'shell'                               # the _ties_ref case whose `mean` tally is also recorded one pair short
SEARCH = {'blocks16': ('ties16_odd_rows', 'chunk_d2_16'), 'blocks32': ('ties32_odd_rows', 'ties32_midway')}
SEARCH_OVERFLOW = 'blocks16'


def hexbytes(a):
    return np.ascontiguousarray(a).tobytes().hex()


@functools.lru_cache(None)
def large_pair():
    """A filled box of LARGE_EDGE^3 voxels against its copy shifted by one voxel along every axis, both in a seeded row order."""
    g = np.arange(LARGE_EDGE)
    box = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + 100
    assert len(box) > 256 * 1024
    return MR._shuffled(box, 31).astype(np.int32), MR._shuffled(box + 1, 32).astype(np.int32)


PAIR_NAMES = ('cluster_vs_corners', 'corners_vs_cluster', 'duplicates_in_b', 'lattice_sublattice', 'shell_perturbed', 'single_a', 'single_b',
              'single_both', 'sublattice_lattice', 'two_far_clusters', 'uniform')                      # _metrics_ref.cloud_pairs()
TIE_NAMES = ('duplicates', 'faces', 'faces_swapped', 'shell', 'single_b', 'sparse')                    # _ties_ref.cases()
COLOR_PAIR_NAMES = ('duplicates_in_a', 'far_queries', 'lattice_sublattice', 'shell_perturbed', 'sublattice_lattice', 'two_points',
                    'uniform')                                                                         # _color_ref.color_pairs()
CLOUD_NAMES = sorted(['pairs.' + n for n in PAIR_NAMES] + ['ties.' + n for n in TIE_NAMES] + [LARGE])
COLOR_NAMES = sorted(COLOR_PAIR_NAMES + (LARGE,))


@functools.lru_cache(None)
def _pairs(module, with_shell):
    """cloud_pairs() / color_pairs() of a restatement module, checked against the names above.  The 1024^3 shell takes seconds to
    make and cloud_pairs() draws it last, so only the case that is the shell pays for it there; color_pairs() seeds its colours by
    the place in the sorted names and is always taken whole."""
    out = MR.cloud_pairs(with_shell) if module == 'metrics' else CR.color_pairs(with_shell)
    names = PAIR_NAMES if module == 'metrics' else COLOR_PAIR_NAMES
    assert sorted(out) == sorted(n for n in names if with_shell or n != 'shell_perturbed'), sorted(out)
    return out


@functools.lru_cache(None)
def cloud_case(name):
    """(A, B, normals of A): seeded unit normals where the source gives none."""
    if name == LARGE:
        a, b = large_pair()
        return a, b, TR.unit_normals(len(a), 33)
    source, key = name.split('.')
    if source == 'ties':
        assert sorted(TR.cases()) == sorted(TIE_NAMES)
        return TR.cases()[key]
    a, b = _pairs('metrics', key == 'shell_perturbed')[key]
    return a, b, MR.unit_normals(len(a), 40 + PAIR_NAMES.index(key))


@functools.lru_cache(None)
def color_case(name):
    """(A, colours of A, B, colours of B)"""
    if name == LARGE:
        a, b = large_pair()
        return a, CR.random_colors(len(a), 34), b, CR.random_colors(len(b), 35)
    return _pairs('color', True)[name]


def _tally_record(out, mean):
    rec = dict(tally=hexbytes(out[0].cpu().numpy()), to_b=BR.digest(out[1].cpu().numpy()), to_a=BR.digest(out[2].cpu().numpy()))
    if mean:
        rec['status'] = hexbytes(out[3].cpu().numpy())
    return rec


def run_cloud(ctx, name):
    """{rule_slots: {tally, to_b, to_a[, status]}} for rule in pick / mean, with normals (d2) and without (d1).  A `mean` call that
    needs more pairs than the default capacity takes the documented second run with the count the first one reported.  OVERFLOW adds
    'mean_d2_one_pair_short': the same call with max_pairs one below that count (D2 / H2 slots NaN, status says so)."""
    from pcc_geo_cnn_v2_amd import ops
    a, b, nrm = cloud_case(name)
    index_a = ops.CloudIndex(ctx, a)
    rec = {}
    for ties in ('pick', 'mean'):
        for slots, n in (('d2', nrm), ('d1', None)):
            out = ops.cloud_distortion_launch(ctx, index_a, b, n, links=True, ties=ties)
            if ties == 'mean':
                pairs, over = (int(v) for v in out[3].cpu())
                if over:
                    out = ops.cloud_distortion_launch(ctx, index_a, b, n, links=True, ties=ties, max_pairs=pairs)
                if slots == 'd2' and name == 'ties.' + OVERFLOW:
                    short = ops.cloud_distortion_launch(ctx, index_a, b, n, links=True, ties=ties, max_pairs=pairs - 1)
                    rec['mean_d2_one_pair_short'] = _tally_record(short, True)
            rec[f'{ties}_{slots}'] = _tally_record(out, ties == 'mean')
    return rec


def run_color(ctx, name):
    from pcc_geo_cnn_v2_amd import ops
    a, ca, b, cb = color_case(name)
    return dict(tally=hexbytes(ops.cloud_color_distortion(ctx, a, ca, b, cb)))


# ---- the searches ----------------------------------------------------------------------------------------------------------------------
def search_args(ctx, key, normals):
    """The blocks of SEARCH[key] as one call: (x_hat, thr, pts, block_of, block_start, normals) on the device, normals in the dtype
    the engine takes (tests/test_search_adversarial_gpu._args)."""
    cases = [SA.catalogue()[n] for n in SEARCH[key]]
    assert all(len(c.blocks) == 1 and c.shape == cases[0].shape and c.clip for c in cases)
    blocks = [c.blocks[0] for c in cases]
    sizes = [len(b) for b in blocks]
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(ctx.device)
    return (up(np.concatenate([c.x_hat for c in cases])), up(SA.T256), up(np.concatenate([b[:, :3] for b in blocks]).astype(np.int32)),
            up(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)), up(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)),
            up(np.concatenate([b[:, 3:] for b in blocks]).astype(normals)))


@functools.lru_cache(None)
def one_chunk_overflow_capacity(key=SEARCH_OVERFLOW):
    """(capacity, chunk, pairs per chunk): one pair below the fullest chunk of the call's thresholds, which every other chunk fits
    in (asserted).  The pair counts are the brute force's (_ties_ref.tie_sets over every distinct level set), not the engine's."""
    names = SEARCH[key]
    shape = SA.catalogue()[names[0]].shape
    chunk = SA.ties_chunk(len(names), *shape)
    per_t = np.zeros(len(SA.T256) + chunk, np.int64)
    for n in names:
        case = SA.catalogue()[n]
        rows = case.blocks[0][:, :3].astype(np.int64)
        for lo, hi in SA.level_groups(case.x_hat[0], case.thr, case.clip)[1]:
            b_t, = S.level_sets(case.x_hat[0], case.thr[lo:lo + 1])
            per_t[lo:hi] += len(TR.tie_sets(b_t, rows)[0])
    per_chunk = [int(per_t[t0:t0 + chunk].sum()) for t0 in range(0, len(SA.T256), chunk)]
    assert len(per_chunk) > 1, 'the call must span more than one chunk of thresholds'
    top, second = sorted(per_chunk)[-1], sorted(per_chunk)[-2]
    assert second < top - 1, per_chunk
    return top - 1, chunk, per_chunk


def _search_record(res):
    names = ('s_ab', 's_ba', 'n_b', 'tcount', 'd2_ab', 'd2_ba')
    return {k: BR.digest(v) for k, v in zip(names, res)}


def run_search(ctx, key):
    """{pick, mean[, mean_one_chunk_overflows]}: the six outputs of either engine as digests, the tie-averaged engine's status
    (largest pair count of a chunk, overflowed) as two integers."""
    from pcc_geo_cnn_v2_amd import ops
    rec = {'pick': _search_record(ops.d12_threshold_stats(ctx, *search_args(ctx, key, np.float32)))}
    args = search_args(ctx, key, np.float64)
    out = ops.d12_threshold_stats_ties(ctx, *args, return_status=True)
    pairs, over = out[-1]
    if over:
        out = ops.d12_threshold_stats_ties(ctx, *args, max_pairs=pairs, return_status=True)
    rec['mean'] = dict(_search_record(out[:6]), status=[int(out[-1][0]), int(out[-1][1])])
    if key == SEARCH_OVERFLOW:
        cap, _, per_chunk = one_chunk_overflow_capacity(key)
        assert pairs == max(per_chunk), (pairs, per_chunk)
        out = ops.d12_threshold_stats_ties(ctx, *args, max_pairs=cap, return_status=True)
        rec['mean_one_chunk_overflows'] = dict(_search_record(out[:6]), status=[int(out[-1][0]), int(out[-1][1])], max_pairs=cap)
    return rec
