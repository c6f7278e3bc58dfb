"""GPU: the recorded bits of the whole-cloud distortion tallies (both tie rules, with and without normals, links included), of the
colour tally and of the two D2 threshold searches (tests/golden/cloud_tally_bits.json; cases: tests/_cloud_tally_cases.py).

Every number these engines report is a sum in a fixed order: per-thread strided sums over a grid fixed by the sizes, a fixed tree per
workgroup, a fixed tree over the partials.  The other tests compare the sums with host restatements to a tolerance, which any
order passes; these compare bytes, so that an edit which claims to leave the order alone is held to it.  If a change of order is
intended, regenerate with tests/golden/make_cloud_tally_bits.py and say so: reported metrics change in their last bits."""
import json

import pytest

import _cloud_tally_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with open(TC.GOLDEN) as fh:
        return json.load(fh)


def _flat(rec, prefix=''):
    out = {}
    for k, v in rec.items():
        out.update(_flat(v, f'{prefix}{k}.') if isinstance(v, dict) else {prefix + k: v})
    return out


def _compare(what, got, want):
    got, want = _flat(got), _flat(want)
    assert sorted(got) == sorted(want), f'{what}: the recorded entries are {sorted(want)}, computed {sorted(got)}'
    bad = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not bad, (f'{what}: the bits differ from tests/golden/cloud_tally_bits.json in {sorted(bad)} (recorded, computed): {bad}.  '
                     'A sum changed its order, or a tie rule its pick')


@pytest.mark.parametrize('name', TC.CLOUD_NAMES)
def test_cloud_distortion_bits(ctx, golden, name):
    _compare(f'cloud_distortion {name}', TC.run_cloud(ctx, name), golden['cloud'][name])


@pytest.mark.parametrize('name', TC.COLOR_NAMES)
def test_cloud_color_distortion_bits(ctx, golden, name):
    _compare(f'cloud_color_distortion {name}', TC.run_color(ctx, name), golden['color'][name])


@pytest.mark.parametrize('key', sorted(TC.SEARCH))
def test_threshold_search_d2_bits(ctx, golden, key):
    _compare(f'd12_threshold_stats {key}', TC.run_search(ctx, key), golden['search'][key])
