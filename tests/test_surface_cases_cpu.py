"""The surface anchor catalogue (tests/_surface_cases.py) without a GPU: the numpy host path against the restatement on every case,
the catalogue against what it claims to hold, and mutated restatements against the catalogue: a rule of DESIGN.md §4.16 that no
leaf of the catalogue notices would be a rule the GPU test does not test."""
import numpy as np
import pytest

import _surface_cases as C
import _surface_ref as R
from pcc_geo_cnn_v2_amd import anchor_surface as S

DECODER = [(k, family, args) for k in C.KS for family, args in C.decoder_cases(k)]
ids = lambda cases: ['-'.join(map(str, (family,) + args)) for _, family, args in cases]


@pytest.mark.parametrize('k,family,args', DECODER, ids=ids(DECODER))
def test_host_reconstruction_equals_the_restatement(k, family, args):
    case, ref = C.reference(family, args)
    got = S.surface_points(case.leaf_keys, case.edge_keys, case.flags8, case.t8, case.resolution, k, device='host')
    assert got.dtype == np.int32 and np.array_equal(got, ref['decoded'])
    assert len(ref['counts']) == len(case.leaves) and ref['counts'].min() >= 1


@pytest.mark.parametrize('k', C.KS)
def test_host_encoder_equals_the_restatement_on_the_near_sets(k):
    for cloud in C.near_sets(k):
        ref = C.near_reference(k, cloud.name)
        got = S.vertices(cloud.points, cloud.resolution, k, device='host')
        for a, key in zip(got, ('leaf_keys', 'edge_keys', 'flags', 't')):
            assert np.array_equal(a, ref[key]), (cloud.name, key)
        assert S.encode(cloud.points, cloud.resolution, k, device='host') == ref['stream'], cloud.name
        assert np.array_equal(S.reconstruct(cloud.points, cloud.resolution, k), ref['decoded']), cloud.name
        assert np.array_equal(S.surface_points(ref['leaf_keys'], ref['edge_keys'], ref['flags'], ref['t'], cloud.resolution, k, device='host'),
                              ref['decoded']), cloud.name


# ---- the catalogue is what it claims
def test_the_pattern_subsets_follow_their_rule():
    for k in C.KS:
        union = set()
        for mode in C.MODES:
            case = C.patterns(k, mode)
            assert sorted(case.tags) == C.pattern_subset(k, mode) and len(set(case.leaves)) == len(case.leaves)
            assert len(case.edges) == 12 * len(case.leaves)                                # isolated: no edge belongs to two leaves
            assert {0, 4095} <= set(case.tags)
            vertices = dict(zip(case.tags, C.leaf_vertices(case)))
            assert all(len(rs) == C.popcount(p) for p, rs in vertices.items())
            assert len(vertices[4095]) == 12
            union |= set(case.tags)
        assert len(union) == (4096 if k <= 3 else 340) and {C.popcount(p) for p in union} == set(range(13))
    # bit e of the pattern is edge e: pattern 1 << e alone puts its vertex on edge e = 4 a + 2 du + dv
    case = C.patterns(3, 'top')
    for p, rs in zip(case.tags, C.leaf_vertices(case)):
        if C.popcount(p) == 1:
            e = p.bit_length() - 1
            a, (u, v) = e >> 2, R.others(e >> 2)
            want = [0, 0, 0]
            want[a], want[u], want[v] = 7, 8 * (e >> 1 & 1), 8 * (e & 1)
            assert rs == [want], p


@pytest.mark.parametrize('k', C.KS)
def test_the_catalogue_holds_what_it_claims(k):
    by_m, by_event, residues = C.census(k)
    print(f'k = {k}: leaves per m {sorted(by_m.items())}; leaves per event {by_event}; cases per residue {sorted(residues.items())}')
    assert set(by_m) == set(range(13)) and by_m[12] == 4 + 4 * sum(C.SHARED_SIZES)
    for event in ('coincident', 'index', 'dom2', 'dom3', 'area0', 'area0_each', 'half2', 'norm'):
        assert by_event[event] >= 1, event
    assert set(residues) == {0, 1, 2, 3}
    moved = {(n, clipped): C.reference('shared', (k, n, 'rand', clipped))[1]['clipped'] for n in (6, 27) for clipped in (False, True)}
    assert moved[6, True] == 0 and moved[27, True] > moved[27, False] > 0
    whole, folded = (C.reference('shared', (k, 27, 'rand', clipped))[1] for clipped in (False, True))
    assert np.array_equal(whole['counts'], folded['counts']) and len(folded['decoded']) < len(whole['decoded'])     # the clip merged voxels


def test_the_searched_literals_show_what_their_names_say():
    assert len({name for name, *_ in C.searched()}) == len(C.searched())
    for k in C.KS:
        case = C.searched_leaves(k)
        assert len(case.leaves) == sum(found_at <= k for _, found_at, _, _ in C.searched())
        for name, rs in zip(case.tags, C.leaf_vertices(case)):
            events = C.leaf_events(rs)
            assert name.rsplit('_', 1)[0] in events, (k, name, events)
            if name.startswith('norm'):                                    # the rule fires; reversing it changes no voxel (module docstring)
                assert C.mutant_voxels(rs, 1 << k, 'norm') == R.leaf_voxels(rs, 1 << k), (k, name)


@pytest.mark.parametrize('k', C.KS)
def test_the_near_sets_reach_the_boundaries(k):
    W = 1 << k
    flagged = unflagged = rounded_up = 0
    for cloud in C.near_sets(k):
        ref = C.near_reference(k, cloud.name)
        flagged += int(ref['flags'].sum())
        unflagged += int((ref['flags'] == 0).sum())
        if cloud.offsets is not None:                                      # one run on one edge: its vertex sits at the rounded mean
            t, half_way = C.rounded_mean(cloud.offsets)
            n = int(np.searchsorted(ref['edge_keys'], np.uint64(R.morton((1, 1, 1)) << 2 | cloud.axis)))
            assert ref['edges'][n][1:] == ((1, 1, 1), cloud.axis) and ref['flags'][n] == 1 and ref['t'][n] == t, cloud.name
            rounded_up += half_way
    lattice = C.near_reference(k, 'lattice_full')
    assert len(lattice['leaves']) == 27 and 0 < lattice['flags'].sum() < len(lattice['flags'])
    print(f'k = {k}: {flagged} flagged and {unflagged} unflagged edges, {rounded_up} runs whose mean ends in .5')
    assert flagged and unflagged and rounded_up == 3 * 6
    assert C.rounded_mean(C.near_sets(k)[-1].offsets) == (W // 2, True) and len(C.near_sets(k)[-1].points) == 9 * W


# ---- sensitivity
def _catalogue_leaves(k):
    """The catalogue's leaves at k, the cheap and the telling ones first."""
    for family, args in [('searched', (k,)), ('patterns', (k, 'rand')), ('patterns', (k, 'ends')), ('shared', (k, 27, 'rand', False)),
                         ('patterns', (k, 'zero')), ('patterns', (k, 'top'))]:
        case = C.FAMILIES[family](*args)
        for tag, rs in zip(case.tags, C.leaf_vertices(case)):
            if len(rs) >= 3:
                yield case.name, tag, rs


def test_the_unmutated_copy_is_the_restatement():
    """mutant_voxels tries every sample of [0, W]^2, R.leaf_voxels those in the triangle's box: the shortcut its docstring names."""
    for k in (2, 3, 4):
        case = C.searched_leaves(k)
        for rs in list(C.leaf_vertices(case)) + list(C.leaf_vertices(C.shared(k, 3, 'rand', False))):
            assert C.mutant_voxels(rs, 1 << k) == R.leaf_voxels(rs, 1 << k)


@pytest.mark.parametrize('k', C.KS)
@pytest.mark.parametrize('rule', C.RULES)
def test_a_mutated_rule_changes_a_catalogue_leaf(rule, k):
    for name, tag, rs in _catalogue_leaves(k):
        if C.mutant_voxels(rs, 1 << k, rule) != R.leaf_voxels(rs, 1 << k):
            print(f'{rule} at k = {k}: first seen by {name} leaf {tag}')
            return
    pytest.fail(f'no leaf of the catalogue at k = {k} notices the mutant {rule!r}')
