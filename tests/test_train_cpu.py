"""CPU: the training pieces that need no GPU -- tfc 1.3 entropy-model formulas, lower_bound gradients, aux targets, the exported
checkpoint's keys and tables, the train / test split, the tr_train command line, and the premises of the exact gradient tests of
test_train_gpu.py (tests/_train_cases.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_cases as T
import _train_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops, train
from pcc_geo_cnn_v2_amd.entropy_models import EntropyBottleneck as HostEB
from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CpuCtx:
    device = torch.device('cpu')


def _eb(seed=3, C=4):
    p = HostEB.init_params(C, init_scale=10, seed=seed)
    rng = np.random.default_rng(seed)
    p = {k: (v + rng.normal(0, .1, v.shape)).astype(np.float32) for k, v in p.items()}
    return p, train.EntropyBottleneck(p, torch.device('cpu'))


def test_bottleneck_likelihood_matches_tfc_formula():
    p, eb = _eb()
    rng = np.random.default_rng(0)
    y = rng.normal(0, 3, (2, 3, 3, 3, 4)).astype(np.float32)
    noise = (rng.random(y.shape) - .5).astype(np.float32)
    y_t, lik = eb(torch.from_numpy(y), torch.from_numpy(noise))
    v = (y + noise).reshape(-1, 4).T.reshape(4, 1, -1).astype(np.float64)
    ref = R.np_eb_likelihood(p, v).reshape(4, -1).T.reshape(y.shape)
    assert np.allclose(y_t.numpy(), y + noise)
    assert np.allclose(lik.detach().numpy(), ref, rtol=2e-5, atol=1e-9)


def test_gaussian_likelihood_matches_tfc_formula():
    rng = np.random.default_rng(1)
    y = rng.normal(0, 2, 1000).astype(np.float32)
    sigma = np.abs(rng.normal(0, 1, 1000)).astype(np.float32)
    sigma[:50] = 0
    noise = (rng.random(1000) - .5).astype(np.float32)
    _, lik = train.gaussian_likelihood(torch.from_numpy(y), torch.from_numpy(sigma), torch.from_numpy(noise))
    ref = R.np_gaussian_likelihood((y + noise).astype(np.float64), sigma.astype(np.float64))
    assert np.allclose(lik.numpy(), ref, rtol=1e-4, atol=1e-9)


def test_lower_bound_passes_the_gradient_only_where_it_pushes_up():
    x = torch.tensor([0.05, 0.2, 0.05, 0.11], requires_grad=True)
    y = train.lower_bound(x, 0.11)
    assert torch.equal(y.detach(), torch.tensor([0.11, 0.2, 0.11, 0.11]))
    y.backward(torch.tensor([1.0, 1.0, -1.0, 1.0]))
    assert torch.equal(x.grad, torch.tensor([0.0, 1.0, -1.0, 1.0]))


def test_aux_loss_targets_and_stop_gradient():
    p, eb = _eb(5)
    aux = eb.aux_loss()
    t = math.log(2 / 2 ** -8 - 1)
    ref = np.abs(R.np_logits_cumulative(p, p['quantiles'].astype(np.float64)) - np.array([-t, 0, t])).sum()
    assert abs(float(aux) - ref) <= 1e-5 * ref
    aux.backward()
    assert eb.params['quantiles'].grad is not None and float(eb.params['quantiles'].grad.abs().sum()) > 0
    assert all(v.grad is None for k, v in eb.params.items() if k != 'quantiles')


@pytest.mark.parametrize('cfg', ['c1', 'c2', 'c3', 'c3p'])
def test_exported_checkpoint_has_init_checkpoint_keys_and_rebuilt_tables(cfg):
    m = ModelConfigType[cfg].build(seed=4)
    m.compress([1, 1, 64, 64, 64])
    g = train.TrainGraph(m, _CpuCtx())
    with torch.no_grad():
        g.eb.params['quantiles'].add_(torch.tensor([-1., 0.5, 2.]))
        g.eb.params['bias_0'].mul_(1.5)
    w = g.export_weights()
    assert set(w) == set(make_synthetic_weights(cfg))
    p = {k.split('/', 1)[1]: v for k, v in w.items() if k.startswith('entropy_bottleneck/') and 'cdf' not in k and k != 'entropy_bottleneck/offset'}
    cdf, length, offset = HostEB(m.num_filters, params=p)._build()
    assert np.array_equal(w['entropy_bottleneck/quantized_cdf'], cdf)
    assert np.array_equal(w['entropy_bottleneck/cdf_length'], length)
    assert np.array_equal(w['entropy_bottleneck/offset'], offset)
    assert np.array_equal(w['entropy_bottleneck/quantiles'], g.eb.params['quantiles'].detach().numpy())


def test_train_test_split_by_parent_directory():
    files = ['/d/train/a.ply', '/d/test/b.ply', '/d/x/train/c.ply', '/d/other/d.ply', '/e/test/e.ply']
    tr, te = train.split_files(files)
    assert tr == ['/d/train/a.ply', '/d/x/train/c.ply'] and te == ['/d/test/b.ply', '/e/test/e.ply']


def test_save_npz_is_byte_stable_and_loadable(tmp_path):
    a = {'x/0/kernel': np.arange(6, dtype=np.float32).reshape(2, 3), 'b': np.array([1, 2], np.int32)}
    train.save_npz(str(tmp_path / 'a.npz'), a)
    train.save_npz(str(tmp_path / 'b.npz'), a)
    assert (tmp_path / 'a.npz').read_bytes() == (tmp_path / 'b.npz').read_bytes()
    with np.load(str(tmp_path / 'a.npz')) as f:
        assert set(f.files) == set(a) and all(np.array_equal(f[k], a[k]) for k in a)


def test_tr_train_help():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.tr_train', '--help'], cwd=ROOT, env=env, capture_output=True,
                       text=True, check=True)
    for flag in ('--model_config', '--resolution', '--batch_size', '--lmbda', '--alpha', '--gamma', '--max_steps', '--warm_start',
                 '--seed', '--validation_interval', '--validation_steps', '--data_format'):
        assert flag in r.stdout


# ---- the cases of the exact gradient tests (tests/_train_cases.py; the GPU assertions are in test_train_gpu.py) --------------------
INT_CASES = list(dict.fromkeys(T.slice_cases() + T.valu_cases() + T.small_grids() + T.noncubic_cases() + T.mixed_parity_cases()))


def test_every_mfma_entry_has_a_geometry_and_a_slice_grid():
    assert len(T.TILES) == 8 and set(T.SLICE_GRIDS) == set(T.TILES)
    assert {T.view(g) for g in T.GEOMS} >= set(T.TILES)
    assert {T.view(c[0]) for c in T.slice_cases()} == set(T.TILES)
    # forward and transposed layers of one entry are cases of their own, and every geometry is in one of the two slice sets
    assert len(T.slice_cases()) + len(T.valu_cases()) == len(T.GEOMS)
    assert {T.view(c[0]) for c in T.valu_cases()} == {(1, 16, 3, 2), (1, 16, 3, 1), (1, 32, 9, 2)}
    assert {c[0] for c in T.noncubic_cases()} == {g for g in T.GEOMS if not g[7]}
    mixed = T.mixed_parity_cases()
    assert {c[0] for c in mixed} == {g for g in T.GEOMS if not g[4] and g[3] == 2}
    assert {tuple(n % 2 for n in c[2]) for c in mixed} == {(1, 0, 1), (0, 1, 1)} and all(T.small_dims(c[0], c[2]) == (3, 6, 10) for c in mixed)
    grids = T.small_grids()
    assert all(max(c[2]) <= 8 and c[1] == 3 for c in grids)
    assert {c[2][0] for c in grids} == {1, 2, 4, 8}


@pytest.mark.parametrize('case', INT_CASES, ids=T.case_id)
def test_integer_cases_are_exact_in_any_float32_order(case):
    """The premise of the exact GPU tests: every gradient element's sum of |terms| is below 2^24, so all its partial sums are integers
    a float32 holds; torch's float32 conv backward on the CPU (another summation order again) already gives the float64 bits."""
    g, N, dims = case
    layer, x, dout = T.int_case(g, N, dims, T.SEED)
    for a in (layer.kernel, x, dout):
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 2
    assert np.count_nonzero(x) < .5 * x.size or x.size < 100                   # ReLU-sparse
    ref = T.int_reference(g, N, dims, T.SEED)
    tot = T.grads(layer, x, dout, absolute=True, dx=not g[7])
    f32 = T.grads(layer, x, dout, dtype=torch.float32, dx=not g[7])
    assert (ref[2] is None) == bool(g[7])
    for name, r, a, f in zip(('dW', 'dB', 'dX'), ref, tot, f32):
        if r is None:
            continue
        assert a.max() < 2 ** 24, (name, a.max())
        assert np.all(np.abs(r) <= a) and np.array_equal(r, np.rint(r)), name
        assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64), r), name


@pytest.mark.parametrize('case', T.slice_cases() + T.valu_cases(), ids=T.case_id)
def test_slice_grids_split_unevenly_and_end_in_partial_tiles(case):
    g, N, dims = case
    n = T.units(g, N, dims)
    S, chain = T.slices(g, N, dims)
    assert ops.conv_wgrad_slices(T.desc(g, N, dims)) == (S, chain)            # host-only: TILES is the library's tiling
    assert S < n and n % S != 0, (S, n)
    o = T.small_dims(g, dims)
    if T.view(g) in T.TILES:
        tile = T.TILES[T.view(g)]
        assert o == T.SLICE_GRIDS[T.view(g)][1] and N == T.SLICE_GRIDS[T.view(g)][0]
        assert chain == -(-n // S) * int(np.prod(tile))
        assert all(a % t != 0 for a, t in zip(o, tile) if t > 1), (o, tile)
    else:
        assert S == 1024 and n == N * int(np.prod(o)) and len(set(o)) == 3
    if not g[4] and g[3] == 2:
        assert all(d == 2 * a - 1 for d, a in zip(dims, o))                      # the odd large grid


def test_slice_grids_have_the_tile_and_slice_counts_of_the_plan():
    """(slices, tiles) per entry, worked out by hand from S = min(1024, 2^25 / (k^3 cu cz), tiles)."""
    want = {(16, 16, 3, 1): (1024, 1254), (32, 32, 3, 1): (1024, 1254), (64, 64, 3, 1): (303, 378), (16, 32, 3, 2): (1024, 1134),
            (32, 32, 3, 2): (1024, 1134), (32, 64, 3, 2): (606, 630), (64, 64, 3, 2): (303, 375), (32, 32, 5, 2): (262, 315)}
    for g, N, dims in T.slice_cases():
        assert (T.slices(g, N, dims)[0], T.units(g, N, dims)) == want[T.view(g)], g


@pytest.mark.parametrize('case', list({T.view(c[0]): c for c in reversed(T.slice_cases())}.values()), ids=T.case_id)
def test_reference_dw_moves_by_an_integer_with_one_edge_voxel_and_with_a_shifted_dout(case):
    """Exact equality cannot pass a kernel that drops the last column of a partial tile or misplaces dout by a voxel: either change
    moves an element of the float64 dW by at least 1."""
    g, N, dims = case
    layer, x, dout = T.int_case(g, N, dims, T.SEED)
    ref = T.int_reference(g, N, dims, T.SEED)[0]
    n, z, y, _ = np.argwhere(x[:, :, :, -1, :] != 0)[-1]                        # a voxel of the last x column, in a partial tile
    x2 = x.copy()
    x2[n, z, y, -1, :] = 0
    for what, xs, gs in (('edge voxel', x2, dout), ('shift', x, np.roll(dout, 1, axis=3))):
        diff = T.grads(layer, xs, gs, dx=False)[0] - ref
        assert np.array_equal(diff, np.rint(diff)) and np.abs(diff).max() >= 1, what


def test_dgrad_refuses_a_stride_2_conv_on_an_odd_grid():
    for dims in ((5, 6, 6), (6, 6, 7)):
        with pytest.raises(AssertionError, match='odd grid'):
            train.dgrad(None, None, L.ConvDesc(1, *dims, 16, 32, 3, 2, 0, 0, L.PCC_IMPL_AUTO, 0, 0), None, None)
