"""GPU: exact adaptive-threshold statistics (distance transforms) vs the host KD-tree path, whose results are
pinned by the reference fixtures (tests/golden/model_opt.npz)."""
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter
from scipy.spatial import cKDTree

from pcc_geo_cnn_v2_amd import model_opt, ops

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _case(rng, R, npts, sharp):
    block = np.unique(rng.integers(0, R, (npts, 3)), axis=0).astype(np.float64)
    dense = np.zeros((R, R, R), np.float32)
    dense[tuple(block.astype(int).T)] = 1
    x_hat = (gaussian_filter(dense, sharp) * 2.5 + rng.normal(0, 0.02, dense.shape)).astype(np.float32)
    return block, x_hat


def _host_stats(block, x_hat, thresholds):
    xh = np.clip(x_hat, 0, 1)
    t1 = cKDTree(block)
    out = []
    for t in thresholds:
        pa = np.argwhere(xh > np.float32(t)).astype(np.float64)
        if len(pa) == 0:
            break
        d_ab, _ = cKDTree(pa).query(block)
        d_ba, _ = t1.query(pa)
        out.append((int(round(np.sum(d_ab ** 2))), int(round(np.sum(d_ba ** 2))), len(pa)))
    return out


@pytest.mark.parametrize('R', [16, 32, 64])
def test_stats_match_kdtree_exactly(ctx, R):
    rng = np.random.default_rng(R)
    thresholds = np.linspace(0, 1.0, 256)
    blocks, xs = zip(*[_case(rng, R, n, s) for n, s in [(40, 0.7), (400, 1.0), (3, 0.5), (900, 1.5)]])
    x_hat = torch.from_numpy(np.stack(xs)).to(ctx.device)
    pts = np.concatenate(blocks).astype(np.int32)
    bof = np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(blocks)])
    s_ab, s_ba, n_b, tcount = ops.d1_threshold_stats(ctx, x_hat, torch.from_numpy(thresholds.astype(np.float32)).to(ctx.device),
                                                     torch.from_numpy(pts).to(ctx.device), torch.from_numpy(bof).to(ctx.device))
    for i, (block, xh) in enumerate(zip(blocks, xs)):
        ref = _host_stats(block, xh, thresholds)
        assert tcount[i] == len(ref)
        for t, (ab, ba, n) in enumerate(ref):
            assert (s_ab[i, t], s_ba[i, t], n_b[i, t]) == (ab, ba, n), (i, t)


def test_decisions_match_host_search_and_reference_fixtures(ctx):
    g = np.load(os.path.join(G, 'model_opt.npz'))
    thresholds = np.linspace(0, 1.0, 256)
    blocks = [g[f'm{i}_block'] for i in range(int(g['n_cases'][0]))]
    xs = np.stack([g[f'm{i}_x_hat'] for i in range(len(blocks))])
    names, best = model_opt.compute_optimal_thresholds_gpu(ctx, blocks, torch.from_numpy(xs).to(ctx.device), thresholds, 64,
                                                           ['d1_mse', 'd1_sum_mean'], [np.inf])
    for i in range(len(blocks)):
        assert names == list(g[f'm{i}_names_fixed0']) and best[i] == list(g[f'm{i}_best_fixed0'])   # == the reference's own answers
    # more metrics and max_delta filters against the host restatement
    rng = np.random.default_rng(1)
    blocks, xs = zip(*[_case(rng, 32, n, s) for n, s in [(300, 0.8), (50, 1.2), (1500, 1.0)]])
    mets, deltas = ['d1_mse', 'd1_sum_AB', 'd1_sum_BA', 'd1_mse_BA', 'd1_sum_max'], [np.inf, 2.0, 1.2]
    names, best = model_opt.compute_optimal_thresholds_gpu(ctx, list(blocks), torch.from_numpy(np.stack(xs)).to(ctx.device),
                                                           thresholds, 64, mets, deltas)
    for b, xh, bt in zip(blocks, xs, best):
        hn, hb = model_opt.compute_optimal_thresholds(b, np.clip(xh, 0, 1), thresholds, 64, opt_metrics=mets, max_deltas=deltas)
        assert hn == names and hb == bt


def test_empty_and_degenerate_blocks(ctx):
    thresholds = np.linspace(0, 1.0, 256)
    block = np.array([[3, 4, 5], [3, 4, 6]], float)
    xs = np.zeros((2, 16, 16, 16), np.float32)          # block 0: nothing above threshold 0 -> [255]
    xs[1, 8, 8, 8] = 0.9                                 # block 1: one far voxel -> mean point wins -> 255
    names, best = model_opt.compute_optimal_thresholds_gpu(ctx, [block, block], torch.from_numpy(xs).to(ctx.device), thresholds, 16)
    for b, xh, bt in zip([block, block], xs, best):
        assert model_opt.compute_optimal_thresholds(b, xh, thresholds, 16, opt_metrics=['d1_mse'], max_deltas=[np.inf])[1] == bt
    assert best[0] == [255]


def test_fortran_ordered_blocks(ctx):
    """np.argwhere returns transposed views; a concatenation of those stays column-major unless forced.  The host
    wrappers must hand the kernels row-major (n,3) points regardless."""
    rng = np.random.default_rng(7)
    thresholds = np.linspace(0, 1.0, 256)
    blocks, xs = [], []
    for n, s in [(600, 0.9), (60, 1.1)]:
        b, xh = _case(rng, 32, n, s)
        dense = np.zeros((32, 32, 32), np.uint8)
        dense[tuple(b.astype(int).T)] = 1
        bf = np.asfortranarray(np.argwhere(dense).astype(np.float64))
        assert not bf.flags['C_CONTIGUOUS']
        blocks.append(bf)
        xs.append(xh)
    names, best = model_opt.compute_optimal_thresholds_gpu(ctx, blocks, torch.from_numpy(np.stack(xs)).to(ctx.device),
                                                           thresholds, 64, ['d1_mse', 'd1_sum_mean'], [np.inf, 1.5])
    for b, xh, bt in zip(blocks, xs, best):
        hn, hb = model_opt.compute_optimal_thresholds(np.ascontiguousarray(b), np.clip(xh, 0, 1), thresholds, 64,
                                                      opt_metrics=['d1_mse', 'd1_sum_mean'], max_deltas=[np.inf, 1.5])
        assert hn == names and hb == bt


# ------------------------------------------------------------------------------------------------------------ D2 on the GPU (round 4)
def _case6(rng, R, npts, sharp):
    block, x_hat = _case(rng, R, npts, sharp)
    nrm = rng.standard_normal((len(block), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.hstack([block, nrm.astype(np.float32)]), x_hat


@pytest.mark.parametrize('R', [16, 32])
def test_d2_stats_match_the_lowest_index_restatement(ctx, oracle, R):
    """pcc_d12_threshold_stats against the brute-force restatement with the same stated tie rule (oracle.search_tallies_lowest_index):
    |B_t| and the D1 sums exactly, the D2 sums to 1e-11 (fp64 sums in another order); twice -> bit-identical."""
    rng = np.random.default_rng(100 + R)
    thresholds = np.linspace(0, 1.0, 256)
    blocks, xs = zip(*[_case6(rng, R, n, s) for n, s in [(40, 0.7), (300, 1.0), (3, 0.5), (700, 1.4)]])
    x_hat = torch.from_numpy(np.stack(xs)).to(ctx.device)
    got = model_opt.d12_tallies_gpu(ctx, list(blocks), x_hat, thresholds)
    again = model_opt.d12_tallies_gpu(ctx, list(blocks), x_hat, thresholds)
    d1 = model_opt.d1_tallies_gpu(ctx, list(blocks), x_hat, thresholds)
    for i, (blk, xh) in enumerate(zip(blocks, xs)):
        ref = oracle.search_tallies_lowest_index(blk, xh, thresholds)
        assert got[i].shape == ref.shape and len(ref) > 3
        assert np.array_equal(got[i][:, :3], ref[:, :3]) and np.array_equal(got[i][:, :3], d1[i][:, :3])
        assert np.allclose(got[i][:, 3:], ref[:, 3:], rtol=1e-11, atol=1e-300), (i, np.abs(got[i][:, 3:] / ref[:, 3:] - 1).max())
        assert np.array_equal(got[i], again[i])


def test_d2_search_against_the_reference_fixtures_and_tie_free_cases(ctx, oracle):
    """(a) tests/golden/model_opt_d2.npz (the reference's own metric dictionaries and decisions, scipy's tie pick; resolution 64):
    every d1_* number of the GPU path equals the reference's; its level sets all contain equidistant neighbours (voxel grids), so the
    d2_* numbers and decisions may differ there -- only there: (b) on random sparse cases WITHOUT ties the GPU tallies equal the
    KD-tree path's (model_opt.host_threshold_stats, the restatement those fixtures pin) to 1e-11."""
    from pcc_geo_cnn_v2_amd.utils import pc_metric as PM
    g = np.load(os.path.join(G, 'model_opt_d2.npz'), allow_pickle=True)
    thresholds = np.linspace(0, 1.0, 256)
    mets, deltas = [str(m) for m in g['opt_metrics']], [float(d) for d in g['max_deltas']]
    differing = []
    for i in range(int(g['n_cases'][0])):
        blk, xh = g[f's{i}_block'], g[f's{i}_x_hat']
        tallies = model_opt.d12_tallies_gpu(ctx, [blk], torch.from_numpy(xh[None]).to(ctx.device), thresholds)[0]
        free = oracle.tie_free(blk, xh, thresholds)
        for t in (40, 100, 160):
            if t >= len(tallies):
                continue
            table = PM.metrics_table(len(blk), tallies[t], 63)
            ref = dict(zip([str(k) for k in g[f's{i}_t{t}_keys']], g[f's{i}_t{t}_vals']))
            for k, v in ref.items():
                if k.startswith('d1_') or free[t]:
                    assert np.isclose(table[k], v, rtol=1e-6), (i, t, k, table[k], v)      # (case 2 is a float32 block: the reference rounds there)
        names, best = model_opt.decide_from_tallies([blk], [tallies], len(thresholds), 64, mets, deltas, gpu_d2=True)
        assert names == [str(n) for n in g[f's{i}_names']]
        for k, (mine, theirs) in enumerate(zip(best[0], [int(b) for b in g[f's{i}_best']])):
            assert mine == theirs or (names[k].startswith('d2_') and not all(free)), (i, names[k], mine, theirs)
            if mine != theirs:
                differing.append((i, names[k], theirs, mine))
    # not "may differ where tied" but WHICH decisions the lowest-(x,y,z) rule moves on these fixtures (reference
    # index -> GPU index; tools/d2_tie_table.py prints the table of DESIGN_HISTORY.md 3.8) -- a regression cannot hide behind `not all(free)`
    assert differing == [(0, 'd2_mse_inf', 198, 218), (0, 'd2_sum_max_inf', 198, 217), (0, 'd2_mse_2.0', 198, 218), (0, 'd2_sum_max_2.0', 198, 217),
                         (2, 'd2_sum_max_inf', 233, 232), (2, 'd2_sum_max_2.0', 233, 232)], differing
    # (b) tie-free cases: a handful of scattered points against a handful of scattered decoded voxels
    rng = np.random.default_rng(2024)
    R, kept = 16, 0
    for trial in range(400):
        a = np.unique(rng.integers(0, R, (int(rng.integers(2, 7)), 3)), axis=0).astype(np.float64)
        nr = rng.standard_normal((len(a), 3)).astype(np.float32)
        xh = np.zeros((R, R, R), np.float32)
        vox = np.unique(rng.integers(0, R, (int(rng.integers(2, 7)), 3)), axis=0)
        xh[tuple(vox.T)] = rng.uniform(0.05, 0.95, len(vox)).astype(np.float32)
        blk = np.hstack([a, nr])
        free = oracle.tie_free(blk, xh, thresholds)
        if not all(free):
            continue
        kept += 1
        got = model_opt.d12_tallies_gpu(ctx, [blk], torch.from_numpy(xh[None]).to(ctx.device), thresholds)[0]
        host, _ = model_opt.host_threshold_stats(blk, np.clip(xh, 0, 1), thresholds, normals=blk[:, 3:6])
        assert got.shape == host.shape and np.array_equal(got[:, :3], host[:, :3])
        assert np.allclose(got[:, 3:], host[:, 3:], rtol=1e-11, atol=1e-300), (trial, got[:, 3:], host[:, 3:])
    assert kept >= 20, kept


def test_gpu_d2_search_reproduces_the_reference_where_no_tie_rule_is_involved(ctx, oracle):
    """tests/golden/model_opt_d2_tiefree.npz: six sparse blocks on which the REFERENCE's compute_optimal_thresholds / compute_metrics
    (imported by make_golden.py --round5-only) never meet equidistant neighbours -- not at any level set, not in the mean-point guard.
    The GPU search (nearest-index transforms + the lexicographic guard) must give every one of the reference's 8 decisions per block and
    its metric values at EVERY level set (D1 exactly; D2 to the float32 rounding of the normals): at least these reference D2 decisions are
    pinned end to end."""
    from pcc_geo_cnn_v2_amd.utils import pc_metric as PM
    g = np.load(os.path.join(G, 'model_opt_d2_tiefree.npz'))
    thresholds = np.linspace(0, 1.0, 256)
    mets, deltas = [str(m) for m in g['opt_metrics']], [float(d) for d in g['max_deltas']]
    decided = 0
    for i in range(int(g['n_cases'][0])):
        blk, xh = g[f's{i}_block'], g[f's{i}_x_hat']
        assert all(oracle.tie_free(blk, xh, thresholds))
        tallies = model_opt.d12_tallies_gpu(ctx, [blk], torch.from_numpy(xh[None]).to(ctx.device), thresholds)[0]
        keys, want = [str(k) for k in g[f's{i}_keys']], g[f's{i}_vals']
        assert len(tallies) == len(want)
        table = PM.metrics_table(len(blk), tallies, 63)
        got = np.array([[table[k][t] for k in keys] for t in range(len(tallies))])
        d1 = [j for j, k in enumerate(keys) if k.startswith('d1_')]
        assert np.allclose(got[:, d1], want[:, d1], rtol=1e-12 if blk.dtype == np.float64 else 1e-6)        # (the float32 block: the reference rounds there)
        assert np.allclose(got, want, rtol=2e-6), (i, np.abs(got / want - 1).max())
        names, best = model_opt.decide_from_tallies([blk], [tallies], len(thresholds), 64, mets, deltas, gpu_d2=True)
        assert names == [str(n) for n in g[f's{i}_names']]
        assert best[0] == [int(b) for b in g[f's{i}_best']], (i, best[0], list(g[f's{i}_best']))
        decided += sum(n.startswith('d2_') for n in names)
    assert decided >= 36


def test_adaptive_encode_with_d2_metrics_issues_no_host_job(ctx, monkeypatch):
    """compress_blocks with ['d1_mse', 'd2_mse'] and normals (the reference's experiment, src/ev_experiment.yml:47): everything on
    the GPU with --d2_search gpu (no worker-pool job); the default KD-tree pool's decisions may differ only through ties."""
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd import init_checkpoint
    rng = np.random.default_rng(5)
    model = ModelConfigType['c3p'].build(batch_size=4)
    model.compress([1, 1, 32, 32, 32])
    model.set_weights(init_checkpoint.make_synthetic_weights('c3p', seed=3, final_bias=0.3))
    blocks = []
    for n in (500, 900, 200):
        b = np.unique(rng.integers(4, 28, (n, 3)), axis=0).astype(np.float64)
        nr = rng.standard_normal((len(b), 3)); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        blocks.append(np.hstack([b, nr]))
    model.host_search_jobs = 0
    monkeypatch.setattr(model_opt, 'D2_SEARCH', 'gpu')
    out = model.encode_block_range(ctx, blocks, 32, with_normals=True, opt_metrics=['d1_mse', 'd2_mse'], max_deltas=[np.inf])
    assert model.host_search_jobs == 0 and out[3] == ['d1_mse_inf', 'd2_mse_inf']
    monkeypatch.setattr(model_opt, 'D2_SEARCH', None)            # the default: D2 tallies from the host KD-tree pool
    host = model.encode_block_range(ctx, blocks, 32, with_normals=True, opt_metrics=['d1_mse', 'd2_mse'], max_deltas=[np.inf])
    assert model.host_search_jobs == len(blocks)
    assert out[0] == host[0] and [t[0] for t in out[1]] == [t[0] for t in host[1]]          # strings and the d1 decisions are the same


# ------------------------------------------------------------------------------------------------------------ fused z / y passes (round 6)
def _edt_case(ctx, shape):
    """Device arguments (x_hat, thr, pts, block_of) of a search on random levels with empty planes and lines and about 2 % occupancy,
    then block_start and unit float64 normals from the same generator for the D2 engines."""
    B, D, H, W = shape
    rng = np.random.default_rng(B * 1000 + W)
    x = rng.random((B, D, H, W), dtype=np.float32) ** 6                   # few voxels above the high thresholds
    x[0, : D // 2] = 0.0                                                  # empty planes and lines
    x[-1, :, :, : W // 3] *= 0.01
    pts, bof = [], []
    for b in range(B):
        p = np.argwhere(rng.random((D, H, W)) < 0.02).astype(np.int32)
        pts.append(p); bof.append(np.full(len(p), b, np.int32))
    start = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
    pts, bof = np.ascontiguousarray(np.vstack(pts)), np.concatenate(bof)          # (np.argwhere hands out a transposed view)
    nrm = rng.standard_normal((len(pts), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    thr = torch.from_numpy(np.linspace(0, 1.0, 256).astype(np.float32)).to(ctx.device)
    dev = lambda a: torch.from_numpy(a).to(ctx.device)
    return (ctx, dev(x), thr, dev(pts), dev(bof)), (dev(start), dev(nrm))


@pytest.mark.parametrize('shape', [(3, 64, 64, 64), (2, 128, 128, 128), (2, 32, 48, 80), (2, 16, 24, 40), (1, 8, 128, 64)])
def test_fused_linear_time_distance_passes_give_the_integers_of_the_two_kernel_form(ctx, shape, monkeypatch):
    """search_d1.hip k_edt_zy (round 6): the z and y passes of the squared Euclidean distance transform of every level set in one
    kernel -- bit masks for the z distances, a lower envelope of parabolas along y with exact integer cross-multiplied comparisons --
    must give the sums of the two brute-force kernels (PCC_EDT_OLD=1) bit for bit: sparse and dense level sets, empty lines and planes,
    64^3 and 128^3 blocks (one and two mask words), edges that are not powers of two, and a shape the fused kernel does not take
    (W % 16 != 0: both runs then use the old kernels).  The search these sums feed restates /root/reference/src/model_opt.py:33-73."""
    args, _ = _edt_case(ctx, shape)
    monkeypatch.delenv('PCC_EDT_OLD', raising=False)
    new = ops.d1_threshold_stats(*args)
    monkeypatch.setenv('PCC_EDT_OLD', '1')
    old = ops.d1_threshold_stats(*args)
    for a, b in zip(new, old):
        assert np.array_equal(a, b)
    assert new[3].max() > 200 and new[0].any()


@pytest.mark.parametrize('shape', [(2, 8, 16, 32), (1, 4, 80, 16), (1, 4, 8, 128)])
def test_tie_averaged_engine_gives_the_same_bits_under_either_form_of_the_distance_passes(ctx, shape, monkeypatch):
    """The tie-averaged D2 engine (search_d2.hip) takes its z / y passes from the same dispatcher as the D1 engine (search_d1.hip,
    pcc_search_edt_zy): with PCC_EDT_OLD=1 every array it returns and its status equal the fused run's -- exactly, since nothing in the
    engine uses float atomics and the kernels behind the z / y passes are the same.  One mask word with stack 64, stack 128, two words."""
    args, d2 = _edt_case(ctx, shape)
    monkeypatch.delenv('PCC_EDT_OLD', raising=False)
    new = ops.d12_threshold_stats_ties(*args, *d2, return_status=True)
    monkeypatch.setenv('PCC_EDT_OLD', '1')
    old = ops.d12_threshold_stats_ties(*args, *d2, return_status=True)
    assert new[-1] == old[-1] and not new[-1][1], (new[-1], old[-1])
    for a, b in zip(new[:-1], old[:-1]):
        assert np.array_equal(a, b)
    assert new[3].max() > 200 and np.isfinite(new[4]).all() and new[4].any() and new[5].any()
