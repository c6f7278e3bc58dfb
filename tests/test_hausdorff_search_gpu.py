"""GPU: the Hausdorff forms of the search statistics (pcc_d1/d12_threshold/count_stats_hausdorff) against brute force
and the host restatement -- never against the code under test.  D1 maxima are integers: np.array_equal.  Every shape is the smallest that
reaches its code path (fused z/y kernel, two-kernel fall-back, two-word lines, level 256, a second chunk of thresholds)."""
import gzip
import json

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter
from scipy.spatial import cKDTree

import _count_search_ref as CR
import _hausdorff_search_ref as R
import _topk_ref as T
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_opt as MO
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.utils import pc_metric as PM

pytestmark = pytest.mark.gpu
# the last synthesis layer of the end-to-end case: x_hat = relu(E2E_GAIN * (its output under scaled_weights) + E2E_BIAS).  Under scaled_weights
# alone a third of a 64^3 block sits above 1 (every level set ~90 k voxels, 255 KD-trees of that size per block on the host); scaled like this
# about 1 % of the voxels is positive, graded between 0 and 1, and the host reference of all 8 blocks takes seconds
E2E_GAIN, E2E_BIAS = 0.01, -0.8
D2_RTOL = 1e-11      # tests/test_threshold_search_gpu.py:132, the per-block tolerance of the D2 sums against the same restatement


def _block(rng, shape, npts, sharp=0.9, gain=2.5, normals=True):
    """npts distinct points (+ float32 normals) and a blurred, noisy occupancy as x_hat: nested level sets that thin out towards 1"""
    shape = tuple(shape)
    flat = np.sort(rng.choice(int(np.prod(shape)), size=npts, replace=False))
    pts = np.stack(np.unravel_index(flat, shape), axis=1).astype(np.float64)
    dense = np.zeros(shape, np.float32)
    dense[tuple(pts.astype(int).T)] = 1
    x_hat = (gaussian_filter(dense, sharp) * gain + rng.normal(0, 0.02, shape)).astype(np.float32)
    if normals:
        pts = np.hstack([pts, rng.standard_normal((npts, 3)).astype(np.float32).astype(np.float64)])
    return pts, x_hat


def _device(ctx, blocks, xs, thr=None):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    sizes = [len(b) for b in blocks]
    out = dict(x_hat=dev(np.stack(xs).astype(np.float32)), pts=dev(np.concatenate([b[:, :3] for b in blocks]).astype(np.int32)),
               bof=dev(np.repeat(np.arange(len(blocks), dtype=np.int32), sizes)), start=dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)))
    if blocks[0].shape[1] >= 6:
        out['nrm'] = dev(np.concatenate([b[:, 3:6] for b in blocks]).astype(np.float32))
    if thr is not None:
        out['thr'] = dev(np.asarray(thr, np.float32))
    return out


def _check_d1(res, refs):
    """res: a hausdorff=True result tuple; refs: per block float64[T, 9] brute-force rows.  Every live (b, t) equal, zeros from tcount on."""
    tcount, h1_ab, h1_ba = res[3], res[-2] if len(res) == 6 else res[6], res[-1] if len(res) == 6 else res[7]
    assert h1_ab.shape == h1_ba.shape == (len(refs), 256) and h1_ab.dtype == np.int64
    for b, ref in enumerate(refs):
        n = len(ref)
        assert tcount[b] == len(ref), (b, tcount[b], len(ref))
        print(f'block {b}: {n} live candidates, H1_AB {h1_ab[b, :n].min()}..{h1_ab[b, :n].max()}, H1_BA {h1_ba[b, :n].min()}..{h1_ba[b, :n].max()}')
        assert np.array_equal(h1_ab[b, :n], ref[:n, R.H1_AB]), (b, h1_ab[b, :n], ref[:n, R.H1_AB])
        assert np.array_equal(h1_ba[b, :n], ref[:n, R.H1_BA]), (b, h1_ba[b, :n], ref[:n, R.H1_BA])
        assert np.array_equal(res[0][b, :n], ref[:n, R.D1_AB]) and np.array_equal(res[1][b, :n], ref[:n, R.D1_BA]) and np.array_equal(res[2][b, :n], ref[:n, R.N_B])
        assert not h1_ab[b, n:].any() and not h1_ba[b, n:].any()


# ---- the first case: 3 blocks of 16^3 with 37, 91 and 64 points (waves of k_edt_points span two blocks), 32 thresholds ------------------
THR32 = np.linspace(0.0, 1.0, 32)


@pytest.fixture(scope='module')
def first_case():
    rng = np.random.default_rng(20)
    blocks, xs = zip(*[_block(rng, (16, 16, 16), n) for n in (37, 91, 64)])
    refs = [R.brute_tallies(b, np.clip(x, 0, 1), THR32) for b, x in zip(blocks, xs)]
    assert all(len(r) >= 8 for r in refs) and len({len(r) for r in refs}) > 1      # blocks with different numbers of live thresholds
    return list(blocks), list(xs), refs


def test_d1_fused_kernel_three_blocks(ctx, first_case):
    blocks, xs, refs = first_case
    d = _device(ctx, blocks, xs, THR32)
    res = ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], hausdorff=True)
    assert len(res) == 6
    _check_d1(res, refs)
    again = ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], hausdorff=True)
    assert all(np.array_equal(x, y) for x, y in zip(res, again))                                  # determinism
    plain = ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'])
    assert len(plain) == 4 and all(np.array_equal(x, y) for x, y in zip(plain, res))              # the plain call: unchanged outputs


@pytest.mark.parametrize('shape,npts', [((8, 12, 20), 29), ((4, 16, 128), 45)], ids=['fallback-8x12x20', 'two-words-4x16x128'])
def test_d1_other_transform_paths(ctx, shape, npts):
    """8x12x20: W % 16 != 0, the two-kernel z / y fall-back.  4x16x128: lines of two 64-bit words in the fused kernel (NW = 2)."""
    rng = np.random.default_rng(sum(shape))
    blk, x = _block(rng, shape, npts, normals=False)
    ref = R.brute_tallies(blk, np.clip(x, 0, 1), THR32)
    assert len(ref) >= 8
    d = _device(ctx, [blk], [x], THR32)
    _check_d1(ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], hausdorff=True), [ref])


def test_d1_level_256_is_reported_and_slot_255_stays_zero(ctx):
    """256 thresholds that end at 0.9 and a voxel at 0.95: its level is 256, tcount reports it, threshold 255 is not computed."""
    rng = np.random.default_rng(256)
    blk, x = _block(rng, (16, 16, 16), 20, sharp=1.0, gain=14.0, normals=False)
    x = np.clip(x, 0, 0.89).astype(np.float32)
    x[tuple(blk[3, :3].astype(int))] = 0.95
    thr = np.linspace(0.0, 0.9, 256)
    ref = R.brute_tallies(blk, x, thr)
    assert len(ref) == 256                                                                        # every level set is non-empty on the host
    d = _device(ctx, [blk], [x], thr)
    with pytest.raises(L.PccError, match='level 256') as e:
        ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], hausdorff=True)
    res = e.value.results
    assert len(res) == 6 and res[3][0] == 256
    assert res[4][0, 255] == 0 and res[5][0, 255] == 0 and res[0][0, 255] == 0
    res = res[:3] + (np.array([255]),) + res[4:]
    _check_d1(res, [ref[:255]])


def test_d1_128_cube_runs_two_threshold_chunks(ctx):
    """One 128^3 block: 128 thresholds are resident at a time, so 256 thresholds take two passes of the chunk loop.  About 2000
    positive voxels and 300 points; the reference queries KD-trees over the small level sets (squared distances of integer points:
    rounded back to the integers they are)."""
    rng = np.random.default_rng(128)
    shape = (128, 128, 128)
    flat = np.sort(rng.choice(128 ** 3, size=300, replace=False))
    blk = np.stack(np.unravel_index(flat, shape), axis=1).astype(np.float64)
    x = np.zeros(shape, np.float32)
    near = (blk[rng.integers(0, 300, 2000)] + rng.integers(-6, 7, (2000, 3))).clip(0, 127).astype(int)
    x[tuple(near.T)] = rng.uniform(0.02, 1.0, 2000).astype(np.float32)
    thr = np.linspace(0.0, 1.0, 256)
    tree_a = cKDTree(blk)
    ref = []
    for b in R.level_sets(x, thr):
        d_ab, d_ba = np.rint(cKDTree(b).query(blk)[0] ** 2), np.rint(tree_a.query(b)[0] ** 2)
        row = np.zeros(9)
        row[[R.N_B, R.D1_AB, R.D1_BA, R.H1_AB, R.H1_BA]] = len(b), d_ab.sum(), d_ba.sum(), d_ab.max(), d_ba.max()
        ref.append(row)
    ref = np.array(ref)
    assert 200 <= len(ref) <= 255 and 1500 <= ref[0, R.N_B] <= 2000
    d = _device(ctx, [blk], [x], thr)
    _check_d1(ops.d1_threshold_stats(ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], hausdorff=True), [ref])


# ---- count source ------------------------------------------------------------------------------------------------------------------------
def test_count_source(ctx, first_case):
    """d1_count_stats(hausdorff=True) with J = 5 counts per block against the brute force over the top-k sets of tests/_count_search_ref.py's
    decision reference (_topk_ref.select); the scores are not clipped."""
    blocks, xs, _ = first_case
    dhw = (16, 16, 16)
    rows, refs = [], []
    for blk, x in zip(blocks, xs):
        P = int(np.count_nonzero(T.keys(x)))
        row = np.array([P + 9, P, P // 2, 7, 1], np.int32)
        sets = [T.select(x, int(k), dhw)[0].astype(np.float64) for k in row]
        rows.append(row)
        refs.append(R.brute_tallies(blk, None, sets=sets))
        assert [len(s) for s in sets] == [P, P, P // 2, 7, 1]
    rows = np.stack(rows)
    d = _device(ctx, blocks, xs)
    counts = torch.from_numpy(rows)
    res = ops.d1_count_stats(ctx, d['x_hat'], counts, d['pts'], d['bof'], hausdorff=True)
    _check_d1(res, refs)
    plain = ops.d1_count_stats(ctx, d['x_hat'], counts, d['pts'], d['bof'])
    assert len(plain) == 4 and all(np.array_equal(x, y) for x, y in zip(plain, res))
    res12 = ops.d12_count_stats(ctx, d['x_hat'], counts, d['pts'], d['bof'], d['start'], d['nrm'], hausdorff=True)
    plain12 = ops.d12_count_stats(ctx, d['x_hat'], counts, d['pts'], d['bof'], d['start'], d['nrm'])
    assert len(res12) == 10 and len(plain12) == 6 and all(np.array_equal(x, y) for x, y in zip(plain12, res12))
    assert all(np.array_equal(x, y) for x, y in zip(res[4:], res12[6:8]))
    for b, ref in enumerate(refs):
        assert np.allclose(res12[8][b, :5], ref[:, R.H2_AB], rtol=D2_RTOL, atol=1e-300) and np.allclose(res12[9][b, :5], ref[:, R.H2_BA], rtol=D2_RTOL, atol=1e-300)
        assert not res12[8][b, 5:].any() and not res12[9][b, 5:].any()
    # and the decision of the count search from these tallies: the brute-force choice of _count_search_ref, restated for a maximum
    tallies = MO.count_tallies_gpu(ctx, blocks, d['x_hat'], rows, hausdorff=True)
    names, ks, idx = MO.decide_counts_from_tallies(blocks, tallies, rows, 16, ['d1_mse', 'd1_hausdorff'], [np.inf])
    for b, blk in enumerate(blocks):
        assert ks[b][0] == CR.brute_choice(blk, xs[b], rows[b], dhw, 16, ['d1_mse'], [np.inf])[1][0]
        col = np.maximum(refs[b][:, R.H1_AB], refs[b][:, R.H1_BA])
        guard = MO.mean_point_d1_tally(blk, hausdorff=True)
        j = int(np.argmin(col))
        assert ks[b][1] == (0 if col[j] > max(guard[PM.H1_AB], guard[PM.H1_BA]) else int(rows[b][j]))


# ---- D2 pick -------------------------------------------------------------------------------------------------------------------------------
def test_d2_pick_maxima(ctx, oracle, first_case):
    """The maxima of the per-point plane terms under the lowest-(x, y, z) rule.  The reference rows restate
    oracle.search_tallies_lowest_index (the reference of the existing D2 sum tests: its five sums must be THE SAME BITS as the
    reference rows', which ties the maxima to the terms those sums add).  The engine evaluates a term's dot product in its own operation
    order (numpy: products rounded, then added), so the per-term bits are not reproduced and the maxima carry the tolerance the sums
    carry there (D2_RTOL); among themselves two calls are bit-identical, and the maxima of the plain outputs' terms bound the sums."""
    blocks, xs, refs = first_case
    d = _device(ctx, blocks, xs, THR32)
    args = (ctx, d['x_hat'], d['thr'], d['pts'], d['bof'], d['start'], d['nrm'])
    res = ops.d12_threshold_stats(*args, hausdorff=True)
    assert len(res) == 10
    _check_d1(res, refs)
    for b, ref in enumerate(refs):
        assert np.array_equal(ref[:, :5], oracle.search_tallies_lowest_index(blocks[b], xs[b], THR32))
        n = len(ref)
        for got, slot in ((res[4], R.D2_AB), (res[5], R.D2_BA), (res[8], R.H2_AB), (res[9], R.H2_BA)):
            err = (np.abs(got[b, :n] - ref[:, slot]) / np.maximum(ref[:, slot], 1e-300)).max()
            print(f'block {b} slot {slot}: largest relative difference {err:.3e}')
            assert np.allclose(got[b, :n], ref[:, slot], rtol=D2_RTOL, atol=1e-300), (b, slot, err)
            assert not got[b, n:].any()
        assert (res[8][b, :n] <= res[4][b, :n]).all() and (res[9][b, :n] <= res[5][b, :n]).all()      # a maximum of non-negative terms <= their sum
        assert (res[8][b, :n] * len(blocks[b]) >= res[4][b, :n] * (1 - 1e-12)).all()
    again = ops.d12_threshold_stats(*args, hausdorff=True)
    assert all(np.array_equal(x, y) for x, y in zip(res, again))
    plain = ops.d12_threshold_stats(*args)
    assert len(plain) == 6 and all(np.array_equal(x, y) for x, y in zip(plain, res))
    # the tallies the search reads, and a decision from them against the brute-force column
    tallies = MO.d12_tallies_gpu(ctx, blocks, d['x_hat'], THR32, hausdorff=True)
    assert all(t.shape == r.shape for t, r in zip(tallies, refs))
    assert all(np.array_equal(t[:, :5], p) for t, p in zip(tallies, MO.d12_tallies_gpu(ctx, blocks, d['x_hat'], THR32)))
    names, best = MO.decide_from_tallies(blocks, tallies, len(THR32), 16, ['d1_hausdorff', 'd2_mse'], [np.inf], gpu_d2=True)
    for b, blk in enumerate(blocks):
        col = np.maximum(refs[b][:, R.H1_AB], refs[b][:, R.H1_BA])
        guard = MO.mean_point_d1_tally(blk, hausdorff=True)
        j = int(np.argmin(col))
        assert best[b][0] == (len(THR32) - 1 if col[j] > max(guard[PM.H1_AB], guard[PM.H1_BA]) else j)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_compress_blocks_with_a_hausdorff_metric(ctx, tmp_path):
    """compress_blocks on the 128^3 shell of tests/test_cli_gpu.py at octree level 1 (8 blocks of 64^3; level 0 is one block) with
    opt_metrics = ['d1_mse', 'd1_hausdorff']: the thresholds chosen for d1_hausdorff equal compute_optimal_thresholds (the host
    restatement) on every block, the stream decodes, and .enc.metric.json holds the Hausdorff keys."""
    from types import SimpleNamespace
    from test_cli_gpu import _cloud
    from test_codec_gpu import scaled_weights
    from pcc_geo_cnn_v2_amd import compress_octree as CO
    from pcc_geo_cnn_v2_amd import model_syntax
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    res, level, bs = 128, 1, 64
    pts = _cloud(res, 0).astype(np.float64)
    blocks, binstr = partition_octree(pts, [0, 0, 0], [res] * 3, level)
    assert len(blocks) > 1
    m = ModelConfigType['c3p'].build(batch_size=4)
    m.compress([1, 1, bs, bs, bs])
    w = scaled_weights(m, 2.2)
    last = max(int(k.split('/')[1]) for k in w if k.startswith('synthesis/'))
    w[f'synthesis/{last}/kernel'] = (w[f'synthesis/{last}/kernel'] * E2E_GAIN).astype(np.float32)
    w[f'synthesis/{last}/bias'] = np.array([E2E_BIAS], np.float32)
    m.set_weights(w)
    seen = {}
    inner = m.encode_block_range

    def spy(*a, **k):      # the per-metric thresholds of every block: compress_blocks keeps only the winning output's
        seen['out'] = inner(*a, **k)
        return seen['out']
    m.encode_block_range = spy
    metrics = ['d1_mse', 'd1_hausdorff']
    data_list, metadata, debug = m.compress_blocks(ctx, blocks, binstr, pts, res, level, opt_metrics=metrics, max_deltas=[np.inf], debug=True)
    _, thresholds, _, names, _ = seen['out']
    assert names == ['d1_mse_inf', 'd1_hausdorff_inf'] and len(thresholds) == len(blocks)
    sizes = []
    for b, blk in enumerate(blocks):
        x_hat = np.clip(debug[b]['x_hat'].reshape(bs, bs, bs), 0.0, 1.0)
        sizes.append(int((x_hat > 0).sum()))
        want = MO.compute_optimal_thresholds(blk, x_hat, m.thresholds, res, opt_metrics=metrics, max_deltas=[np.inf])[1]
        assert list(thresholds[b]) == want, (b, thresholds[b], want)
    print('voxels above threshold 0 per block:', sizes, 'chosen:', [list(t) for t in thresholds])
    # one d1 group -> one output; its metrics carry the Hausdorff keys of the whole cloud, equal to the host tally's
    assert len(data_list) == 1 and len(metadata) == 1
    info = metadata[0]
    want = PM.hausdorff_table(PM.cloud_tally_host(pts, info['blocks_full']), res - 1)
    for k in ('d1_hausdorff_AB', 'd1_hausdorff_BA', 'd1_hausdorff', 'd1_hausdorff_psnr'):
        assert info['metrics'][k] == want[k]
    assert info['metrics']['d1_hausdorff'] >= info['metrics']['d1_mse']
    # --metrics_device gpu: the same keys from the GPU's nine-slot tally (D1: integers, equal to the host's)
    from pcc_geo_cnn_v2_amd.model_types import select_best_per_opt_metric
    on_gpu = select_best_per_opt_metric(binstr, list(zip(*seen['out'][2])), level, names, pts, res, False, metrics_device='gpu', ctx=ctx,
                                        hausdorff=True)
    assert len(on_gpu) == 1 and on_gpu[0]['idx'] == info['idx']
    for k in ('d1_hausdorff_AB', 'd1_hausdorff_BA', 'd1_hausdorff', 'd1_hausdorff_psnr', 'd1_mse', 'd1_psnr'):
        assert on_gpu[0]['metrics'][k] == info['metrics'][k], k
    # the files of the rate point
    args = SimpleNamespace(resolution=res, octree_level=level, debug=False, opt_metrics=metrics)
    info['numerics_tag'] = model_syntax.stream_tag(ctx.numerics_tag('fp32'), m.entropy_coder)
    target = str(tmp_path / 'o.ply.bin')
    CO._write_rate_point(target, None, binstr, data_list[0], info, args, blocks, None)
    record = json.load(open(target + '.enc.metric.json'))
    assert record['d1_hausdorff'] == float(want['d1_hausdorff']) and 'd1_hausdorff_AB' in record and 'd1_psnr' in record
    # the stream decodes to the encoder's candidate
    with gzip.open(target, 'rb') as f:
        r, l, bstr, coded = model_syntax.load_compressed_file(f)
    dec = ModelConfigType['c3p'].build(batch_size=3)
    dec.decompress()
    dec.set_weights({k: v for k, v in w.items() if not k.startswith(('analysis/', 'hyper_analysis/'))})
    dec_blocks, _ = dec.decompress_blocks(ctx, coded, [bs] * 3)
    assert (r, l) == (res, level) and len(dec_blocks) == len(blocks)
    for got, ref in zip(dec_blocks, info['x_hat_list']):
        assert np.array_equal(np.asarray(got), np.asarray(ref))

