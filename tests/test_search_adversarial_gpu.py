"""GPU: the three engines of the per-block threshold search (ops.d1_threshold_stats, ops.d12_threshold_stats,
ops.d12_threshold_stats_ties) on every block of the adversarial catalogue (tests/_search_adversarial.py), against brute force over
every distinct level set: the integers exactly, the D2 sums within the tolerance (`pick`) or the derived rounding bound (`mean`) the
suite already uses.  The references are tests/_search_adversarial.reference_pick / reference_mean; nothing of the kernels' side."""
import numpy as np
import pytest
import torch

import _search_adversarial as A
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_opt, ops

pytestmark = pytest.mark.gpu
CAT = A.catalogue()


def _args(ctx, case, normals):
    """(x_hat, thr, pts, block_of, block_start, normals) on the device; `normals`: the dtype the engine takes."""
    dev = ctx.device
    sizes = [len(b) for b in case.blocks]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (up(case.x_hat), up(case.thr), up(np.concatenate([b[:, :3] for b in case.blocks]).astype(np.int32)),
            up(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)), up(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)),
            up(np.concatenate([b[:, 3:] for b in case.blocks]).astype(normals)))


def _check_d1(name, s_ab, s_ba, n_b, tcount, upto=None):
    """tcount and the three integer columns of every block equal the brute force at every t < tcount (and are zero from there on)."""
    for b in range(len(CAT[name].blocks)):
        tc, ref = A.reference_pick(name, b)
        assert tcount[b] == tc, (b, tcount[b], tc)
        n = tc if upto is None else min(tc, upto)
        for col, (got, what) in enumerate(((n_b, 'n_b'), (s_ab, 's_ab'), (s_ba, 's_ba'))):
            bad = np.flatnonzero(got[b][:n] != ref[:n, col])
            assert not len(bad), (name, what, b, int(bad[0]), int(got[b][bad[0]]), ref[bad[0], col])
            assert not got[b][tc:].any(), (name, what, b)


@pytest.mark.parametrize('z_y_passes', ['fused', 'two_kernels'])
@pytest.mark.parametrize('name', A.names())
def test_d1_integers_equal_brute_force(ctx, oracle, monkeypatch, name, z_y_passes):
    """Both forms of the z / y passes (PCC_EDT_OLD=1 selects k_edt_z + k_edt_axis; read per call), each against the reference."""
    if z_y_passes == 'two_kernels':
        monkeypatch.setenv('PCC_EDT_OLD', '1')
    else:
        monkeypatch.delenv('PCC_EDT_OLD', raising=False)
    x_hat, thr, pts, bof, _, _ = _args(ctx, CAT[name], np.float32)
    _check_d1(name, *ops.d1_threshold_stats(ctx, x_hat, thr, pts, bof, clip=CAT[name].clip))


@pytest.mark.parametrize('name', A.names())
def test_pick_engine_equals_the_lowest_index_brute_force(ctx, oracle, name):
    """D1 columns exact; D2 sums to 1e-11 (float64 sums in another order, the tolerance of
    test_d2_stats_match_the_lowest_index_restatement); a second call gives identical bits."""
    case = CAT[name]
    args = _args(ctx, case, np.float32)
    got = ops.d12_threshold_stats(ctx, *args, clip=case.clip)
    again = ops.d12_threshold_stats(ctx, *args, clip=case.clip)
    _check_d1(name, *got[:4])
    for b in range(len(case.blocks)):
        tc, ref = A.reference_pick(name, b)
        for slot, col in ((4, 3), (5, 4)):
            g = got[slot][b][:tc]
            assert np.allclose(g, ref[:, col], rtol=1e-11, atol=1e-300), (name, b, slot, np.abs(g - ref[:, col]).max())
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes()


@pytest.mark.parametrize('name', A.names())
def test_mean_engine_equals_the_tie_averaged_brute_force(ctx, oracle, name):
    """D1 columns exact; D2 sums within `_search_ties_ref.slot_bounds` of the level set; the reported pair count is the largest
    per-chunk count of the brute force.  A case that needs more pairs than the default capacity takes the documented second run."""
    case = CAT[name]
    args = _args(ctx, case, np.float64)
    out = ops.d12_threshold_stats_ties(ctx, *args, clip=case.clip, return_status=True)
    pairs, over = out[-1]
    if over:
        out = ops.d12_threshold_stats_ties(ctx, *args, clip=case.clip, max_pairs=pairs, return_status=True)
        assert out[-1] == (pairs, False)
    assert pairs == A.chunk_pairs(name, A.ties_chunk(len(case.blocks), *case.shape))
    _check_d1(name, *out[:4])
    for b in range(len(case.blocks)):
        for lo, hi, ref, (b_ab, b_ba), _ in A.reference_mean(name, b)[1]:
            for slot, col, bound in ((4, 3, b_ab), (5, 4, b_ba)):
                d = np.abs(out[slot][b][lo:hi] - ref['tally'][col]).max()
                assert d <= bound, (name, b, lo, slot, d, bound)


@pytest.mark.parametrize('engine', ['d1', 'pick', 'mean'])
@pytest.mark.parametrize('name', A.names('level256', reference=False))
def test_level_256_is_reported_and_threshold_255_left_out(ctx, oracle, name, engine):
    """tcount[b] == 256 says that block b held a voxel above all 256 thresholds: a level the uint8 grid cannot hold.  The wrappers raise
    PccError naming the block; the engines leave t = 255 out, so every sum at [b][255] is zero, and the other blocks and (where the
    restatements apply: under clip) the thresholds below 255 are computed as ever.
    Before the fix this failed: no error, and at t = 255 all transforms were empty -- s_ab[b][255] = 65535 * |A| (the kInf sentinel per
    row; 1310700 for the 20 rows of these cases), n_b = s_ba = 0, and the D2 engines keyed every row on voxel 0."""
    case = CAT[name]
    f32, f64 = _args(ctx, case, np.float32), _args(ctx, case, np.float64)
    call = {'d1': lambda: ops.d1_threshold_stats(ctx, *f32[:4], clip=case.clip),
            'pick': lambda: ops.d12_threshold_stats(ctx, *f32, clip=case.clip),
            'mean': lambda: ops.d12_threshold_stats_ties(ctx, *f64, clip=case.clip)}[engine]
    with pytest.raises(L.PccError, match='level 256') as e:
        call()
    assert e.value.blocks == case.props['blocks'] and all(f'{b}' in str(e.value) for b in e.value.blocks)
    res = e.value.results
    s_ab, s_ba, n_b, tcount = res[:4]
    for b in range(len(case.blocks)):
        assert (tcount[b] == 256) == (b in case.props['blocks'])
        if tcount[b] == 256:
            print(f'{name} {engine} block {b}: s_ab[255] = {s_ab[b][255]} for {len(case.blocks[b])} rows')
            assert all(r[b][255] == 0 for r in res[:3] + res[4:])
            assert n_b[b][254] > 0 and s_ab[b][254] > 0
    if case.clip:
        _check_d1(name, *res[:4], upto=255)
    else:                                         # the block beside the reported one is an ordinary block
        quiet = [b for b in range(len(case.blocks)) if b not in case.props['blocks']]
        assert quiet and all(0 < tcount[b] < 256 and n_b[b][tcount[b] - 1] > 0 and s_ab[b][tcount[b] - 1] > 0 for b in quiet)


def test_the_products_search_takes_infinities_and_nan(ctx):
    """compute_optimal_thresholds_gpu clips and searches linspace(0, 1, 256): +inf becomes level 255, NaN and -inf level 0, so the
    level-256 error cannot be raised from there; the decisions are the host search's."""
    rng = np.random.default_rng(11)
    thresholds = np.linspace(0, 1.0, 256)
    blocks, xs = [], []
    for n in (60, 200):
        a = np.unique(rng.integers(0, 16, (n, 3)), axis=0).astype(np.float64)
        x = np.zeros((16, 16, 16), np.float32)
        x[tuple(a.astype(int).T)] = rng.uniform(0.2, 1.0, len(a)).astype(np.float32)
        near = np.clip(a.astype(int) + rng.integers(-1, 2, a.shape), 0, 15)
        x[tuple(near[::3].T)] = rng.uniform(0.0, 0.6, len(near[::3])).astype(np.float32)
        x[tuple(a[:4].astype(int).T)] = np.array([np.inf, np.nan, -np.inf, 3.0], np.float32)
        blocks.append(a)
        xs.append(x)
    mets, deltas = ['d1_mse', 'd1_sum_mean', 'd1_sum_max'], [np.inf, 2.0]
    names, best = model_opt.compute_optimal_thresholds_gpu(ctx, blocks, torch.from_numpy(np.stack(xs)).to(ctx.device), thresholds, 16, mets, deltas)
    for b, x, bt in zip(blocks, xs, best):
        hn, hb = model_opt.compute_optimal_thresholds(b, np.clip(x, 0, 1), thresholds, 16, opt_metrics=mets, max_deltas=deltas)
        assert hn == names and hb == bt
