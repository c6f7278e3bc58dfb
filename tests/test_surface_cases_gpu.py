"""GPU: csrc/surface_anchor.hip on the catalogue of tests/_surface_cases.py, against the restatement in tests/_surface_ref.py.
k_raster<K, WRITE> on every pattern of flagged edges, on coincident and tied vertices, on leaves that share faces, in both thread
layouts (k <= 3 and k >= 4) and with a partial last workgroup; the count pass leaf by leaf, which the decoder's final unique cannot
hide; k_pairs and k_fit on every boundary of the near set.  Every input is inside the contract.  Every test runs under its own time
limit (a watchdog that ends the process: a stuck kernel must not keep the card)."""
import faulthandler

import numpy as np
import pytest

import _surface_cases as C
from pcc_geo_cnn_v2_amd import anchor_surface as S

pytestmark = pytest.mark.gpu
STEP_LIMIT = 300          # seconds per test
DECODER = [(k, family, args) for k in C.KS for family, args in C.decoder_cases(k)]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize('k,family,args', DECODER, ids=['-'.join(map(str, (family,) + args)) for _, family, args in DECODER])
def test_voxels_and_per_leaf_counts_equal_the_restatement(ctx, k, family, args):
    case, ref = C.reference(family, args)
    arrays = [a.copy() for a in (case.leaf_keys, case.edge_keys, case.flags8, case.t8)]        # the catalogue's own are read only
    run = lambda **kw: S.surface_points(*arrays, case.resolution, k, device='gpu', ctx=ctx, **kw)
    got, pos, total = run(return_counts=True)
    assert got.dtype == np.int32 and got.shape == ref['decoded'].shape and np.array_equal(got, ref['decoded'])
    # the count pass, leaf by leaf: the bit map's population count and the restatement's set, both before the clip
    assert pos.dtype == np.int64 and pos.shape == (len(case.leaves),) and pos[0] == 0
    counts = np.diff(np.append(pos, total))
    wrong = np.flatnonzero(counts != ref['counts'])
    assert len(wrong) == 0, [(case.tags[i], int(counts[i]), int(ref['counts'][i])) for i in wrong[:8]]
    assert total == int(ref['counts'].sum())
    again = run()
    assert again.dtype == got.dtype and again.tobytes() == got.tobytes()                   # two calls, the same bytes


@pytest.mark.parametrize('k', C.KS)
def test_encoder_and_codec_equal_the_restatement_on_the_near_sets(ctx, k):
    for cloud in C.near_sets(k):
        ref = C.near_reference(k, cloud.name)
        got = S.vertices(cloud.points, cloud.resolution, k, device='gpu', ctx=ctx)
        for a, key in zip(got, ('leaf_keys', 'edge_keys', 'flags', 't')):
            assert a.dtype == ref[key].dtype and np.array_equal(a, ref[key]), (cloud.name, key)
        stream = S.encode(cloud.points, cloud.resolution, k, device='gpu', ctx=ctx)
        assert stream == ref['stream'], cloud.name
        dec = S.decode(stream, device='gpu', ctx=ctx)
        assert dec.dtype == np.int32 and np.array_equal(dec, ref['decoded']), cloud.name
