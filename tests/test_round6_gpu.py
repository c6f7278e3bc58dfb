"""Round 6: the configs[2] bench workload (one cloud, sharded, collectives inside the clock) and the fp16-split side channel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('force_dist', [False, True])
def test_bench_configs2_runs_one_cloud_through_the_sharded_entry_points(force_dist):
    """`bench.py --workload configs2` (BASELINE.json configs[2]; /root/reference/src/compress_octree.py:97-105, decompress_octree.py:60-66):
    a labelled strong-scaling line; with a one-rank RCCL group the closing collectives really run and are accounted for."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    if force_dist:
        env.update(PCC_BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29631')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'configs2', '--steps', '2', '--warmup', '2'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['scaling'] == 'strong' and d['n_gpus'] == 1 and 'configs2' in d['metric'] and d['value'] > 0
    assert 150 < d['config']['blocks'] < 2000 and d['config']['decoded_points'] > 0 and d['config']['container_bytes_gzip'] > 0
    # a one-rank group takes the unsharded path (sharding.world_info() == (0, 1)): no collective is issued, and the line says so
    assert d['final_collectives_calls_per_step'] == 0 and d['final_collectives_ms'] == 0
    assert set(d['config']['phase_ms_per_step_rank0']) == {'encode', 'handover', 'decode'}


def _ctx():
    from pcc_geo_cnn_v2_amd import ops
    return ops.get_context(torch.device('cuda', 0))


# One layer per kernel family the route can return (csrc/conv_route.hip, pcc_conv_route): expected name prefix, (N, D, H, W, Cin, Cout,
# k, stride, transposed), flags on top of BIAS | RELU, impl, numerics switches
_F16, _IN16, _OUT16 = 16, 32, 64
FAMILY_CASES = [
    ('generic (', (1, 16, 16, 16, 16, 16, 3, 1, 0), 0, 'GENERIC', {}),
    ('generic (', (1, 7, 9, 6, 3, 5, 3, 1, 0), 0, 'AUTO', {}),
    ('conv_f16 (', (2, 16, 16, 16, 16, 16, 3, 1, 0), _F16 | _IN16, 'AUTO', {}),
    ('conv_fwd (exact fp32', (1, 16, 16, 16, 16, 32, 3, 2, 0), 0, 'AUTO', {}),
    ('conv_fwd (f16', (1, 16, 16, 16, 16, 32, 3, 2, 0), _F16, 'AUTO', {}),
    ('conv_fwd (exact fp32', (1, 32, 32, 32, 16, 16, 3, 1, 0), 0, 'MFMA', {}),
    ('conv_k3s1_split (', (4, 8, 8, 8, 64, 64, 3, 1, 1), 0, 'AUTO', {}),
    ('conv_k3s1_split32', (4, 16, 16, 16, 32, 32, 3, 1, 1), 0, 'AUTO', {}),
    ('conv_k3s1_split32', (1, 16, 16, 32, 64, 64, 3, 1, 0), 0, 'SPLIT', {'split_mfma32': True}),
    ('conv_k3s1_split (', (1, 16, 16, 16, 32, 32, 3, 1, 0), 0, 'SPLIT', {'split_mfma16': True}),
    # the 32x32x16 formulation needs W % 32 == 0 or W == 16: at W = 48 the 16x16x32 kernel runs, and is named
    ('conv_k3s1_split (', (1, 8, 16, 48, 32, 32, 3, 1, 1), 0, 'SPLIT', {}),
    ('conv_k3s1_split (', (1, 8, 16, 48, 64, 64, 3, 1, 0), 0, 'SPLIT', {'split_mfma32': True}),
    ('conv16_wino (', (1, 64, 64, 64, 16, 16, 3, 1, 1), 0, 'AUTO', {'no_split': True}),
    ('conv16_wino (', (1, 32, 32, 32, 32, 32, 3, 1, 1), 0, 'WINOGRAD', {'no_f16s': True}),
    ('conv16_wino_bf16', (1, 64, 64, 64, 16, 16, 3, 1, 1), 0, 'AUTO', {'no_f16s': True}),
    ('conv16_wino_f16s', (1, 64, 64, 64, 16, 16, 3, 1, 1), 0, 'AUTO', {}),
    ('conv16_wino_f16s', (1, 16, 16, 16, 64, 64, 3, 1, 0), 0, 'WINOGRAD', {}),
    ('conv_tr2 (', (1, 32, 32, 32, 32, 16, 3, 2, 1), 0, 'AUTO', {'no_tr2m': True}),
    ('conv_tr2 (', (1, 8, 8, 8, 32, 32, 5, 2, 1), 0, 'AUTO', {}),
    ('conv_tr2m_f16 (', (1, 32, 32, 32, 32, 16, 3, 2, 1), _F16 | _OUT16, 'AUTO', {}),
    ('conv_tr2m_f16s', (1, 32, 32, 32, 32, 16, 3, 2, 1), 0, 'AUTO', {}),
    ('conv_tr2m_f16s', (1, 32, 32, 32, 64, 32, 3, 2, 1), 0, 'MFMA', {}),
    ('conv_tr2_split', (1, 8, 8, 8, 64, 64, 3, 2, 1), 0, 'AUTO', {}),
    ('conv_tr2_split', (1, 16, 16, 16, 64, 32, 3, 2, 1), 0, 'AUTO', {'no_f16s': True}),
    ('conv_tr2m_bf16', (1, 32, 32, 32, 32, 16, 3, 2, 1), 0, 'AUTO', {'no_f16s': True}),
    ('conv_tr2m (', (1, 32, 32, 32, 32, 16, 3, 2, 1), 0, 'AUTO', {'no_split': True}),
    ('conv_cin1', (1, 32, 32, 32, 1, 16, 9, 2, 0), 0, 'AUTO', {}),
    ('conv_cout1_mfma', (1, 16, 16, 16, 16, 1, 3, 1, 1), 0, 'AUTO', {}),
    ('conv_cout1 (', (1, 16, 16, 16, 32, 1, 3, 1, 1), 0, 'AUTO', {}),
]


def test_kernel_family_names_the_round6_kernels_and_follows_the_numerics_switches():
    """pcc_conv_kernel_family (include/pcc_geo.h): the c3p layers that VERDICT r05 item 1 asked to move take the two-piece fp16 kernels by
    default, PCC_NO_F16S=1 (numerics switch no_f16s) gives round 5's kernels, PCC_NO_SPLIT=1 the exact-fp32 ones -- a function of the layer
    shape and the context only, never of the batch (encoder and decoder chunks must take the same kernel).  Every family the route can
    return is named for a layer that reaches it (FAMILY_CASES), and the name is the kernel the launcher runs."""
    import ctypes
    from pcc_geo_cnn_v2_amd import _lib as L
    ctx = _ctx()

    def fam(N, D, cin, cout, stride=1, tr=1, H=None, W=None, k=3, flags=0, impl=L.PCC_IMPL_AUTO):
        d = L.ConvDesc(N=N, D=D, H=H or D, W=W or D, Cin=cin, Cout=cout, k=k, stride=stride, transposed=tr,
                       flags=L.PCC_CONV_BIAS | L.PCC_CONV_RELU | flags, impl=impl)
        buf = ctypes.create_string_buffer(96)
        L.check(L.lib().pcc_conv_kernel_family(ctx.handle, ctypes.byref(d), buf, 96), 'pcc_conv_kernel_family')
        return buf.value.decode()
    for N in (1, 32):
        assert fam(N, 64, 16, 16).startswith('conv16_wino_f16s') and fam(N, 32, 32, 32).startswith('conv16_wino_f16s') and fam(N, 16, 64, 64).startswith('conv16_wino_f16s')
        assert fam(N, 32, 32, 16, 2).startswith('conv_tr2m_f16s') and fam(N, 8, 64, 64).startswith('conv_k3s1_split') and fam(N, 16, 32, 32).startswith('conv_k3s1_split32')
    with ctx.numerics_override(no_f16s=True):
        assert fam(32, 64, 16, 16).startswith('conv16_wino_bf16') and fam(32, 32, 32, 32).startswith('conv16_wino (') and fam(32, 16, 64, 64).startswith('conv_k3s1_split (')
        assert fam(32, 32, 32, 16, 2).startswith('conv_tr2m_bf16')
    with ctx.numerics_override(no_split=True):
        assert fam(32, 64, 16, 16).startswith('conv16_wino (') and fam(32, 32, 32, 16, 2).startswith('conv_tr2m (')
    names = set()
    for want, (N, D, H, W, cin, cout, k, stride, tr), flags, impl, switches in FAMILY_CASES:
        with ctx.numerics_override(**switches):
            got = fam(N, D, cin, cout, stride, tr, H, W, k, flags, getattr(L, 'PCC_IMPL_' + impl))
        assert got.startswith(want), (want, got, (N, D, H, W, cin, cout, k, stride, tr), flags, impl, switches)
        names.add(got)
    assert len(names) == 18, sorted(names)       # every family, each under its own name


@pytest.mark.parametrize('C,D,N', [(16, 32, 3), (32, 32, 2), (64, 16, 3)])
def test_two_piece_fp16_layers_scale_per_block_and_not_per_launch(C, D, N):
    """conv_wino_f16s.hip: the pre-scale follows the maximum of EACH 64^3 block (/root/reference/src/model_transforms.py:62-81 run block by
    block in the reference, src/model_types.py:192-212): a block's output bits do not depend on what else is in the launch -- even when a
    neighbour is 2^30 times larger or all zero -- and scaling ONE block by a power of two scales that block's output bit for bit."""
    from pcc_geo_cnn_v2_amd import ops, _lib as L
    ctx = _ctx()
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((3, 3, 3, C, C)) / np.sqrt(27 * C)).astype(np.float32)
    layer = ops.ConvLayer(w, None, 1, True, True)
    x = torch.from_numpy(rng.standard_normal((N, D, D, D, C)).astype(np.float32)).to(ctx.device)
    base = ops.conv3d(ctx, x, layer, impl=L.PCC_IMPL_WINOGRAD)
    y = x.clone()
    y[0] *= 2.0 ** 30
    y[N - 1] = 0
    got = ops.conv3d(ctx, y, layer, impl=L.PCC_IMPL_WINOGRAD)
    assert torch.equal(got[0], base[0] * 2.0 ** 30) and torch.count_nonzero(got[N - 1]) == 0
    for b in range(1, N - 1):
        assert torch.equal(got[b], base[b])
    assert torch.equal(ops.conv3d(ctx, x[1:2].contiguous(), layer, impl=L.PCC_IMPL_WINOGRAD), base[1:2])


def test_recorded_block_maxima_equal_a_reduction_over_the_tensor():
    """The side channel of the fp16-split kernels (csrc/common.h, pcc_conv_ext): inside pcc_network_forward the kernel that writes a tensor
    records max |x| per block; chained through pcc_conv3d the library reduces the tensor itself.  Both must give the same bits: the c3p
    synthesis transform through the network call == layer by layer (this is what makes encoder-side and decoder-side x_hat equal whatever
    API level a caller uses)."""
    from pcc_geo_cnn_v2_amd import ops, _lib as L
    from pcc_geo_cnn_v2_amd.model_transforms import SynthesisTransformProgressiveV2, init_transform
    ctx = _ctx()
    tr = init_transform(SynthesisTransformProgressiveV2(64, data_format='channels_last'), 64, np.random.default_rng(1))
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 8, 8, 8, 64)).astype(np.float32)).to(ctx.device)
    a = tr.forward_ndhwc(ctx, x)
    os.environ['PCC_LAYERWISE'] = '1'
    try:
        b = tr.forward_ndhwc(ctx, x)
    finally:
        del os.environ['PCC_LAYERWISE']
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize('cin,cout,D,N', [(32, 16, 16, 3), (64, 32, 8, 3)])
def test_two_piece_fp16_marches_scale_per_block_and_match_the_oracle(cin, cout, D, N):
    """conv_tr2m_f16s.hip (Conv3DTranspose k3 stride 2, /root/reference/src/model_transforms.py:78): within 8e-6 (1 + max |ref|) of the
    fp64-accumulating oracle like the bf16 kernel it replaces; a block's bits do not depend on its neighbours in the launch; scaling one
    block by a power of two scales its output bit for bit (bias-free); AUTO really takes the kernel."""
    import ctypes
    from pcc_geo_cnn_v2_amd import ops, _lib as L
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    ctx = _ctx()
    rng = np.random.default_rng(11)
    w = (rng.standard_normal((3, 3, 3, cout, cin)) / np.sqrt(27 * cin / 8)).astype(np.float32)
    layer = ops.ConvLayer(w, None, 2, True, True)
    H = 16
    xn = rng.standard_normal((N, D, H, H, cin)).astype(np.float32)
    x = torch.from_numpy(xn).to(ctx.device)
    d = layer.desc(N, D, H, H, 0, L.PCC_IMPL_AUTO, 0, 0)
    buf = ctypes.create_string_buffer(96)
    L.check(L.lib().pcc_conv_kernel_family(ctx.handle, ctypes.byref(d), buf, 96), 'pcc_conv_kernel_family')
    assert buf.value.decode().startswith('conv_tr2m_f16s')
    base = ops.conv3d(ctx, x, layer)
    ref = O.conv3d_transpose(xn[:1], w, None, 2, True)
    assert np.abs(base[:1].cpu().numpy() - ref).max() <= 8e-6 * (1 + np.abs(ref).max())
    y = x.clone()
    y[0] *= 2.0 ** -40
    y[N - 1] = 0
    got = ops.conv3d(ctx, y, layer)
    assert torch.equal(got[0], base[0] * 2.0 ** -40) and torch.count_nonzero(got[N - 1]) == 0 and torch.equal(got[1], base[1])
    assert torch.equal(ops.conv3d(ctx, x[1:2].contiguous(), layer), base[1:2])


def test_bound_pruned_d2_search_takes_the_decisions_of_the_full_kdtree_search(monkeypatch):
    """model_opt.host_threshold_stats_pruned (/root/reference/src/model_opt.py:33-73, src/utils/pc_metric.py:76-131): the
    host pool builds the A->B KD-trees only for the thresholds whose lower bound (exact B->A side, zero A->B side) does not exceed the best
    upper bound (A->B side <= max |n|^2 x the GPU's exact D1 sum).  Every decision -- d1 and d2, every max_delta -- must EQUAL the unpruned
    search's on a voxelised shell with a plausible decoder output (ties at every level set), and most trees must really be skipped."""
    import bench
    from pcc_geo_cnn_v2_amd import ops
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    ctx = _ctx()
    R, level, res = 1024, 4, 64
    rng = np.random.default_rng(0)
    u = rng.standard_normal((1_200_000, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = 200 + 6 * np.sin(9 * u[:, :1]) * np.cos(7 * u[:, 1:2]) + rng.normal(0, 0.6, (len(u), 1))
    pts, first = np.unique(np.round(u * rad + np.array([512, 500, 520])).astype(np.int64), axis=0, return_index=True)
    cloud = np.hstack([pts.astype(np.float64), u[first]])
    blocks, _ = partition_octree(cloud, [0, 0, 0], [R] * 3, level)
    blocks = blocks[::5]                                  # 40-odd blocks keep the unpruned run inside the test budget
    model = ModelConfigType['c3p'].build(batch_size=16)
    model.compress([1, 1, res, res, res])
    model.set_weights(bench.synthetic_weights(model))
    orig = model._encode_batch

    def plausible(x):                                     # the recipe of the golden fixtures: blurred occupancy x 2.2 + noise, clipped
        k = torch.exp(-torch.arange(-2, 3, device=x.device, dtype=torch.float32) ** 2 / (2 * 0.8 ** 2)); k /= k.sum()
        v = x[:, None]
        for ax in range(3):
            shape = [1, 1, 1, 1, 1]; shape[2 + ax] = 5
            pad = [0, 0, 0, 0, 0, 0]; pad[2 * (2 - ax)] = pad[2 * (2 - ax) + 1] = 2
            v = torch.nn.functional.conv3d(torch.nn.functional.pad(v, pad), k.reshape(shape))
        g = torch.Generator(device=x.device).manual_seed(int(x.sum().item()) & 0xffff)
        return (v[:, 0] * 2.2 + 0.03 * torch.randn(x.shape, device=x.device, generator=g)).clamp_(0, 1).contiguous()

    def enc(ctx_, x, debug=False, thr=None, slot=0):
        e = orig(ctx_, x, debug, thr=thr, slot=slot)
        e['x_hat'] = plausible(x)
        return e
    model._encode_batch = enc
    mets, deltas = ['d1_mse', 'd2_mse', 'd2_sum_max'], [np.inf, 2.0]
    monkeypatch.delenv('PCC_D2_NO_PRUNE', raising=False)
    model.search_trees_built = model.search_trees_total = 0
    pruned = model.encode_block_range(ctx, blocks, R, with_normals=True, opt_metrics=mets, max_deltas=deltas)[1]
    built, total = model.search_trees_built, model.search_trees_total
    monkeypatch.setenv('PCC_D2_NO_PRUNE', '1')
    full = model.encode_block_range(ctx, blocks, R, with_normals=True, opt_metrics=mets, max_deltas=deltas)[1]
    assert pruned == full
    assert total > 0 and built < 0.5 * total, (built, total)
    print(f'pruned d2 search: {built} of {total} A->B trees built ({100.0 * built / total:.1f} %), {len(blocks)} blocks, decisions equal')

