"""GPU: training -- weight / input gradients of every conv geometry of c1, c2, c3 and c3p against float64 autograd, determinism,
the device repack of the packed weight images, the focal-loss gradient, whole-model gradients, and tr_train end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_transforms as MT
from pcc_geo_cnn_v2_amd import ops, train
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _geometries():
    """Distinct (cin, cout, k, stride, transposed, relu, bias, first) of the conv layers of c1, c2, c3, c3p; `first`: the layer
    reads the network input (no input gradient needed)."""
    out = set()
    for cfg in ('c1', 'c2', 'c3', 'c3p'):
        m = ModelConfigType[cfg].build()
        m.compress([1, 1, 64, 64, 64])
        for prefix, tr, _ in m._transforms():
            for i, c in enumerate(tr.conv_layers()):
                l = c.layer
                out.add((l.cin, l.cout, l.k, l.stride, int(l.transposed), int(l.relu), int(l.bias is not None),
                         int(prefix == 'analysis' and i == 0)))
    return sorted(out)


GEOMS = _geometries()


@pytest.fixture(scope='module')
def pctx():
    return train.training_context(torch.device('cuda', 0))


def _layer(g, rng):
    cin, cout, k, s, tr, relu, bias, _ = g
    shape = (k, k, k) + ((cout, cin) if tr else (cin, cout))
    w = rng.uniform(-1, 1, shape).astype(np.float32) / np.sqrt(k ** 3 * cin)
    b = rng.normal(0, .1, cout).astype(np.float32) if bias else None
    return ops.ConvLayer(w, b, s, tr, relu)


def _grid(g):
    cin, cout, k, s, tr = g[:5]
    return 8 if k == 9 else 16


def _wgrad_case(pctx, g, n, D, seed):
    rng = np.random.default_rng(seed)
    layer = _layer(g, rng)
    x = np.maximum(rng.normal(0, 1, (n, D, D, D, layer.cin)), 0).astype(np.float32)      # ReLU-sparse input
    oshape = ops.conv_out_shape(layer, x.shape)
    dout = rng.normal(0, 1, oshape).astype(np.float32)
    d = layer.desc(n, D, D, D)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    dw = torch.empty(layer.kernel.shape, dtype=torch.float32, device='cuda')
    db = torch.empty(layer.cout, dtype=torch.float32, device='cuda')
    ops.conv3d_wgrad(pctx, d, xd, gd, dw, db)
    return layer, x, dout, d, dw, db


def _ref_wgrad(layer, x, dout):
    """float64 dW, dB and the sums of |terms| of every dW element (the same autograd on |x|, |dout|)."""
    res = []
    for xs, gs in ((x, dout), (np.abs(x), np.abs(dout))):
        w = torch.from_numpy(layer.kernel).double().requires_grad_()
        y = (R.conv3d_transpose if layer.transposed else R.conv3d)(torch.from_numpy(xs).double(), w, layer.stride)
        (y * torch.from_numpy(gs).double()).sum().backward()
        res.append(w.grad.numpy())
    db = dout.astype(np.float64).reshape(-1, layer.cout).sum(0)
    return res[0], res[1], db, np.abs(dout).astype(np.float64).reshape(-1, layer.cout).sum(0)


def _check_wgrad(layer, d, x, dout, dw, db):
    ref, absum, rdb, dbabs = _ref_wgrad(layer, x, dout)
    # each dW element is one fp32 FMA chain over a voxel slice (at most `chain` terms, pcc_conv_wgrad_slices) plus a fixed-order
    # sum of the S slice partials: its error is below (chain + S) * 2^-24 * sum|terms|
    S, chain = ops.conv_wgrad_slices(d)
    bound = (chain + S) * EPS * absum + 1e-30
    err = np.abs(dw.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= bound), f'wgrad: max err/bound {np.max(err / bound):.3g}'
    # bias: 1024 (or fewer) voxel slices, each summed by up to 256 lanes then across the lanes, then across the slices
    nb = int(np.prod(dout.shape[:4]))
    sb = min(nb, 1024)
    errb = np.abs(db.cpu().numpy().astype(np.float64) - rdb)
    assert np.all(errb <= (-(-nb // sb) + 256 + sb) * EPS * dbabs + 1e-30), 'bias gradient'


@pytest.mark.parametrize('g', GEOMS, ids=[f'{g[0]}-{g[1]}-k{g[2]}s{g[3]}{"T" if g[4] else ""}' for g in GEOMS])
def test_wgrad_matches_float64_autograd(pctx, g):
    layer, x, dout, d, dw, db = _wgrad_case(pctx, g, 2, _grid(g), 1)
    _check_wgrad(layer, d, x, dout, dw, db)


def test_wgrad_full_size_16_16_transposed_64(pctx):
    layer, x, dout, d, dw, db = _wgrad_case(pctx, (16, 16, 3, 1, 1, 1, 1, 0), 2, 64, 2)
    _check_wgrad(layer, d, x, dout, dw, db)


@pytest.mark.parametrize('g', [(16, 16, 3, 1, 1, 1, 1, 0), (1, 16, 3, 2, 0, 1, 1, 1), (64, 32, 3, 2, 1, 1, 1, 0)])
def test_wgrad_is_bitwise_deterministic(pctx, g):
    layer, x, dout, d, dw, db = _wgrad_case(pctx, g, 2, 32, 3)
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    ops.conv3d_wgrad(pctx, d, torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda(), dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('g', [g for g in GEOMS if not g[7]], ids=[f'{g[0]}-{g[1]}-k{g[2]}s{g[3]}{"T" if g[4] else ""}' for g in GEOMS if not g[7]])
def test_dgrad_through_the_dual_descriptor(pctx, g):
    rng = np.random.default_rng(4)
    layer = _layer(g, rng)
    D = _grid(g)
    x = np.maximum(rng.normal(0, 1, (2, D, D, D, layer.cin)), 0).astype(np.float32)
    dout = rng.normal(0, 1, ops.conv_out_shape(layer, x.shape)).astype(np.float32)
    dd = ops.dual_desc(layer.desc(2, D, D, D))
    m = ops.conv_repack_map(dd)
    wd = torch.from_numpy(layer.kernel).cuda()
    pk = None
    if m is not None:
        pk = ops.conv_repack_device(pctx, dd, torch.from_numpy(m).cuda(), wd, torch.empty(m.shape, dtype=torch.float32, device='cuda'))
    dx = torch.empty(x.shape, dtype=torch.float32, device='cuda')
    L.check(L.lib().pcc_conv3d(pctx.handle, C.byref(dd), ops._ptr(torch.from_numpy(dout).cuda()), ops._ptr(wd), ops._ptr(pk),
                               None, None, ops._ptr(dx), pctx.stream), 'dgrad')
    ref = []
    for xs, gs, ws in ((x, dout, layer.kernel), (x, np.abs(dout), np.abs(layer.kernel))):
        xt = torch.from_numpy(xs).double().requires_grad_()
        y = (R.conv3d_transpose if layer.transposed else R.conv3d)(xt, torch.from_numpy(ws).double(), layer.stride)
        (y * torch.from_numpy(gs).double()).sum().backward()
        ref.append(xt.grad.numpy())
    # one output is a sum of at most k^3 Cout products, accumulated in fp32 (any order): error <= 2 k^3 Cout 2^-24 sum|terms|
    bound = 2 * layer.k ** 3 * layer.cout * EPS * ref[1] + 1e-30
    err = np.abs(dx.cpu().numpy().astype(np.float64) - ref[0])
    assert np.all(err <= bound), f'dgrad: max err/bound {np.max(err / bound):.3g}'


# the families whose packed images are reorders of the Keras taps (the segments pcc_conv_repack_weights_device rebuilds)
TRAINING_FAMILIES = {
    'generic (reference-order fp32 FMA chain)', 'conv_fwd (exact fp32 MFMA)', 'conv_tr2 (exact fp32 MFMA)',
    'conv_tr2m (z march, exact fp32 MFMA)', 'conv_cin1 (exact fp32 MFMA)', 'conv_cout1_mfma (exact fp32 MFMA)', 'conv_cout1 (fp32 VALU)'}


def _family(ctx, d):
    buf = C.create_string_buffer(256)
    L.check(L.lib().pcc_conv_kernel_family(ctx.handle, C.byref(d), buf, 256), 'family')
    return buf.value.decode()


@pytest.mark.parametrize('cfg', ['c1', 'c2', 'c3', 'c3p'])
def test_device_repack_equals_host_pack_on_the_training_segments(pctx, cfg):
    rng = np.random.default_rng(5)
    m = ModelConfigType[cfg].build()
    m.compress([1, 1, 64, 64, 64])
    for res in (32, 64):
        for prefix, tr, cin in m._transforms():
            grid = res if prefix == 'analysis' else (res // 8 if prefix in ('synthesis', 'hyper_analysis') else res // 16)
            D = grid
            for c in tr.conv_layers():
                l = c.layer
                d = l.desc(2, D, D, D)
                for dd in (d, ops.dual_desc(d)):
                    fam = _family(pctx, dd)
                    assert fam in TRAINING_FAMILIES, fam
                    mp = ops.conv_repack_map(dd)
                    if mp is None:
                        continue
                    w = (l.kernel * rng.uniform(0.5, 1.5, l.kernel.shape) + rng.normal(0, .01, l.kernel.shape)).astype(np.float32)
                    host = np.empty(mp.shape, np.float32)
                    L.check(L.lib().pcc_conv_pack_weights(C.byref(dd), w.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p)), 'pack')
                    dev = ops.conv_repack_device(pctx, dd, torch.from_numpy(mp).cuda(), torch.from_numpy(w).cuda(),
                                                 torch.empty(mp.shape, dtype=torch.float32, device='cuda')).cpu().numpy()
                    sel = mp >= -1
                    assert sel.sum() >= w.size
                    assert np.array_equal(dev[sel].view(np.uint32), host[sel].view(np.uint32)), (cfg, prefix, fam)
                D = ops.conv_out_shape(l, (2, D, D, D, l.cin))[1]


def test_focal_gradient_matches_float64_autograd(pctx):
    rng = np.random.default_rng(6)
    n = 4096
    yt = (rng.random(n) < .3).astype(np.float32)
    yp = rng.random(n).astype(np.float32)
    special = np.array([0, 1, 1e-3, .999, 0, 1, 1e-3, .999, 5e-4, .9995, 2.0, -1.0], np.float32)
    yp[:12] = special
    yt[:12] = [1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0]
    scale = torch.tensor([0.37], dtype=torch.float32, device='cuda')
    g = ops.focal_loss_grad(pctx, torch.from_numpy(yt).cuda(), torch.from_numpy(yp).cuda(), scale, 2.0, 0.9).cpu().numpy()
    p = torch.from_numpy(yp).double().requires_grad_()
    (0.37 * R.focal_loss(torch.from_numpy(yt).double(), p, 2.0, 0.9)).backward()
    ref = p.grad.numpy()
    assert np.all(ref[[0, 4 + 1, 8, 9, 10, 11]] == 0)          # strictly outside [1e-3, 0.999]: no gradient
    assert np.all(ref[[2, 3, 6, 7]] != 0)                      # at the bounds: passed
    assert np.allclose(g, ref, rtol=1e-5, atol=1e-6), np.max(np.abs(g - ref))


def _blocks_dense(n, res, seed):
    """Planes and spherical shells, {0,1} float32 (n, res, res, res)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).astype(np.float64)
    out = np.zeros((n, res, res, res), np.float32)
    for i in range(n):
        if i % 2 == 0:
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            out[i] = np.abs((g - res / 2) @ nrm - rng.uniform(-res / 6, res / 6)) < .6
        else:
            out[i] = np.abs(np.linalg.norm(g - res / 2 - rng.uniform(-2, 2, 3), axis=-1) - rng.uniform(res / 5, res / 2.5)) < .6
    return out


@pytest.mark.parametrize('cfg', ['c1', 'c3', 'c3p'])
def test_whole_model_gradients_match_float64(pctx, cfg):
    torch.manual_seed(0)
    m = ModelConfigType[cfg].build(seed=7)
    m.compress([1, 1, 32, 32, 32])
    graph = train.TrainGraph(m, pctx)
    x = torch.from_numpy(_blocks_dense(2, 32, 8)).cuda()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(9)
    noise = [torch.rand(s, generator=gen, device='cuda') - .5 for s in graph.latent_shapes(tuple(x.shape))]
    out = graph.loss(x, noise, 1e-4 * 100)
    aux = graph.eb.aux_loss()
    params = {f'{p}/{i}/kernel': tc.weight for p, i, tc in graph.prefixed}
    params.update({f'{p}/{i}/bias': tc.bias_p for p, i, tc in graph.prefixed if tc.bias_p is not None})
    params.update({f'entropy_bottleneck/{k}': v for k, v in graph.eb.params.items()})
    (out['loss'] + aux).backward()
    loss64, aux64, leaves = R.model_loss64(graph, x, noise, 1e-4 * 100)
    (loss64 + aux64).backward()
    assert abs(float(out['loss']) - float(loss64)) <= 1e-4 * abs(float(loss64))
    # fp32 kernels against float64 over a network of up to 20 layers: every parameter's gradient within 1e-3 of its norm
    for k, leaf in leaves.items():
        got = params[k].grad
        got = np.zeros(leaf.shape) if got is None else got.detach().cpu().double().numpy()
        ref = leaf.grad.numpy() if leaf.grad is not None else np.zeros(leaf.shape)
        assert np.linalg.norm(got - ref) <= 1e-3 * np.linalg.norm(ref) + 1e-12, (k, np.linalg.norm(got - ref), np.linalg.norm(ref))


def _write_blocks(root, res, n_train, n_test, seed):
    for sub, n, s in (('train', n_train, seed), ('test', n_test, seed + 100)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for i, blk in enumerate(_blocks_dense(n, res, s)):
            pts = np.argwhere(blk > 0).astype(np.float32)
            pc_io.write_df(os.path.join(root, sub, f'b{i:03d}.ply'), pc_io.pa_to_df(pts))


def _tr_train(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.tr_train'] + [str(a) for a in args], cwd=ROOT, env=env,
                          check=True, capture_output=True, text=True, timeout=900)


def test_tr_train_lowers_validation_loss_and_its_checkpoint_codes(tmp_path):
    import json
    data = tmp_path / 'data'
    _write_blocks(str(data), 32, 16, 4, 11)
    ck = tmp_path / 'ck'
    _tr_train(str(data / '**' / '*.ply'), ck, '--model_config', 'c3p', '--resolution', 32, '--batch_size', 4, '--max_steps', 200,
              '--validation_interval', 50, '--validation_steps', 1, '--lmbda', 1e-2)
    recs = [json.loads(l) for l in open(ck / 'log.jsonl')]
    val = [r['val_loss'] for r in recs if 'val_loss' in r]
    assert len(val) >= 2 and min(val[1:]) < val[0], val
    assert (ck / 'done').exists() and (ck / 'model.npz').exists()
    # the trained checkpoint through the codec CLIs: the decoder's points equal the encoder-side reconstruction
    src = str(tmp_path / 'in.ply')
    pc_io.write_df(src, pc_io.pa_to_df(np.argwhere(_blocks_dense(1, 64, 3)[0] > 0).astype(np.float32)))
    out, dec_enc, dec = str(tmp_path / 'o' / 'in.ply.bin'), str(tmp_path / 'enc.ply'), str(tmp_path / 'dec.ply')
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, '-m'] + list(a), cwd=ROOT, env=env, check=True, capture_output=True, text=True)
    run('pcc_geo_cnn_v2_amd.compress_octree', '--input_files', src, '--output_files', out, '--dec_files', dec_enc, '--checkpoint_dir',
        str(ck), '--model_config', 'c3p', '--resolution', '64', '--octree_level', '1', '--opt_metrics', 'd1_mse', '--fixed_threshold')
    run('pcc_geo_cnn_v2_amd.decompress_octree', '--input_files', out, '--output_files', dec, '--checkpoint_dir', str(ck),
        '--model_config', 'c3p')
    a, b = pc_io.load_pc(dec_enc), pc_io.load_pc(dec)
    assert a.shape == b.shape and np.array_equal(a, b)


def test_tr_train_is_deterministic_and_resumes_to_the_same_bytes(tmp_path):
    data = tmp_path / 'data'
    _write_blocks(str(data), 16, 8, 2, 21)
    common = ['--model_config', 'c3p', '--resolution', 16, '--batch_size', 2, '--validation_interval', 3, '--validation_steps', 1,
              '--lmbda', 1e-2]
    glob_ = str(data / '**' / '*.ply')
    for name in ('a', 'b'):
        _tr_train(glob_, tmp_path / name, '--max_steps', 6, *common)
    _tr_train(glob_, tmp_path / 'c', '--max_steps', 3, *common)
    _tr_train(glob_, tmp_path / 'c', '--max_steps', 6, *common)
    a, b, c = [(tmp_path / n / 'model.npz').read_bytes() for n in 'abc']
    assert a == b and a == c
    import json
    la = [json.loads(l) for l in open(tmp_path / 'a' / 'log.jsonl') if 'loss' in l and 'val' not in l]
    lc = [json.loads(l) for l in open(tmp_path / 'c' / 'log.jsonl') if 'loss' in l and 'val' not in l]
    assert la == lc and len(la) == 6


def _trainer(ck, data, **kw):
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType as MC
    args = dict(resolution=16, batch_size=2, lmbda=1e-2, validation_interval=3, validation_steps=1, seed=42, log=None)
    args.update(kw)
    return train.Trainer(MC['c3p'].build(seed=42), str(ck), data[0], data[1], **args)


def _blocks(n, res, seed):
    return [np.argwhere(b > 0) for b in _blocks_dense(n, res, seed)]


def test_interrupted_run_resumes_from_its_last_validation_to_the_same_bytes(tmp_path):
    data = (_blocks(8, 16, 31), _blocks(2, 16, 32))
    _trainer(tmp_path / 'full', data, max_steps=8).run()
    t = _trainer(tmp_path / 'cut', data, max_steps=8)
    step_fn = t.train_step

    def failing(x):
        if t.step == 5:                   # after the validation (and saves) at step 3
            raise RuntimeError('interrupted')
        return step_fn(x)
    t.train_step = failing
    with pytest.raises(RuntimeError, match='interrupted'):
        t.run()
    assert not (tmp_path / 'cut' / 'done').exists()
    r = _trainer(tmp_path / 'cut', data, max_steps=8)
    assert r.step == 3 and r.last_val == 3
    r.run()
    for f in ('model.npz',):
        assert (tmp_path / 'full' / f).read_bytes() == (tmp_path / 'cut' / f).read_bytes()
    assert r.step == 8 and (tmp_path / 'cut' / 'done').exists()


def test_model_npz_without_train_state_is_not_overwritten(tmp_path):
    data = (_blocks(4, 16, 41), _blocks(2, 16, 42))
    ck = tmp_path / 'ck'
    ck.mkdir()
    (ck / 'model.npz').write_bytes(b'trained')
    with pytest.raises(AssertionError, match='train_state.pt'):
        _trainer(ck, data, max_steps=3)
    assert (ck / 'model.npz').read_bytes() == b'trained'


def test_early_stop_saves_the_current_model_and_resumes_stopped(tmp_path):
    data = (_blocks(4, 16, 51), _blocks(2, 16, 52))
    t = _trainer(tmp_path / 'ck', data, max_steps=100, validation_interval=1)
    vals = iter([1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    t.validate = lambda: next(vals)
    t.run()
    assert t.step == 4 and t.best_step == 0 and (tmp_path / 'ck' / 'done').exists()
    with np.load(str(tmp_path / 'ck' / 'model.npz')) as f:           # the model at the stop, not the step-0 best
        k = 'synthesis/9/kernel'
        assert np.array_equal(f[k], t.graph.export_weights()[k])
    r = _trainer(tmp_path / 'ck', data, max_steps=100, validation_interval=1)
    assert r.step == 4 and r.last_val == 4 and r.best_step == 0
