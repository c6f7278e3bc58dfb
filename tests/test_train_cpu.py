"""CPU: the training pieces that need no GPU -- tfc 1.3 entropy-model formulas, lower_bound gradients, aux targets, the exported
checkpoint's keys and tables, the train / test split and the tr_train command line."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_ref as R
from pcc_geo_cnn_v2_amd import train
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
