"""GPU: training -- weight / input gradients of every conv geometry of c1, c2, c3 and c3p against float64 autograd (with a bound
on Gaussian data, bit for bit on the integer cases of tests/_train_cases.py: partial tiles, uneven slices, the trainer's small grids,
non-cubic grids), the ReLU mask bitwise, packed images after in-place weight updates, determinism, the device repack of the packed weight images, the focal-loss gradient, whole-model gradients, and tr_train end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_cases as T
import _train_ref as R
from _train_cases import GEOMS, _layer
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_transforms as MT
from pcc_geo_cnn_v2_amd import ops, train
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def pctx():
    return train.training_context(torch.device('cuda', 0))


def _grid(g):
    cin, cout, k, s, tr = g[:5]
    return 8 if k == 9 else 16


def _wgrad(pctx, layer, x, dout):
    """(descriptor, dW, dB) of pcc_conv3d_wgrad on host arrays x and dout."""
    d = layer.desc(*x.shape[:4])
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    dw = torch.empty(layer.kernel.shape, dtype=torch.float32, device='cuda')
    db = torch.empty(layer.cout, dtype=torch.float32, device='cuda')
    ops.conv3d_wgrad(pctx, d, xd, gd, dw, db)
    return d, dw, db


def _gauss_case(g, n, dims, seed):
    """Layer of geometry g, ReLU-sparse Gaussian x on an n x dims grid (dims: one extent for a cube, or three) and Gaussian dout."""
    rng = np.random.default_rng(seed)
    layer = _layer(g, rng)
    dims = (dims,) * 3 if isinstance(dims, int) else tuple(dims)
    x = np.maximum(rng.normal(0, 1, (n,) + dims + (layer.cin,)), 0).astype(np.float32)      # ReLU-sparse input
    dout = rng.normal(0, 1, ops.conv_out_shape(layer, x.shape)).astype(np.float32)
    return layer, x, dout


def _wgrad_case(pctx, g, n, D, seed):
    layer, x, dout = _gauss_case(g, n, D, seed)
    d, dw, db = _wgrad(pctx, layer, x, dout)
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
    layer, x, dout = _gauss_case(g, 2, _grid(g), 4)
    _check_dgrad(layer, x, dout, _dgrad(pctx, layer, x, dout))


def _dgrad(pctx, layer, x, dout):
    """dX of host arrays: pcc_conv3d on the dual descriptor with the Keras array and its device-repacked image."""
    dd = ops.dual_desc(layer.desc(*x.shape[:4]))
    m = ops.conv_repack_map(dd)
    wd = torch.from_numpy(layer.kernel).cuda()
    pk = None
    if m is not None:
        pk = ops.conv_repack_device(pctx, dd, torch.from_numpy(m).cuda(), wd, torch.empty(m.shape, dtype=torch.float32, device='cuda'))
    dx = torch.empty(x.shape, dtype=torch.float32, device='cuda')
    L.check(L.lib().pcc_conv3d(pctx.handle, C.byref(dd), ops._ptr(torch.from_numpy(dout).cuda()), ops._ptr(wd), ops._ptr(pk),
                               None, None, ops._ptr(dx), pctx.stream), 'dgrad')
    return dx


def _check_dgrad(layer, x, dout, dx):
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


# ---- exact gradients on small integers (tests/_train_cases.py): every partial sum is an integer below 2^24, so any slice split,
#      MFMA chain or summation order gives the float64 value bit for bit
SEED = T.SEED


def _assert_exact(what, got, want64, k=None):
    """got (device float32) equals the float64 reference; dW (k given) names the first bad (tap, cu, cz)."""
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), f'{what}: the reference is not a float32'
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(~(got == want))
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        where = f'(tap {(i[0] * k + i[1]) * k + i[2]}, cu {i[3]}, cz {i[4]})' if k else str(i)
        raise AssertionError(f'{what}: {len(bad)} of {got.size} differ, first at {where}: got - want = {got[i] - want[i]:g}')


def _exact_wgrad(pctx, case):
    g, N, dims = case
    layer, x, dout = T.int_case(g, N, dims, SEED)
    d, dw, db = _wgrad(pctx, layer, x, dout)
    rdw, rdb, _ = T.int_reference(g, N, dims, SEED)
    _assert_exact('dW', dw, rdw, layer.k)
    _assert_exact('dB', db, rdb)
    return layer, x, dout, d


def _uneven_slices(case):
    """The preconditions of the slice tests: what the library plans is what TILES predicts, more units than slices, uneven split."""
    g, N, dims = case
    n = T.units(g, N, dims)
    S, chain = T.slices(g, N, dims)
    assert ops.conv_wgrad_slices(T.desc(g, N, dims)) == (S, chain)
    assert S < n and n % S != 0, (S, n)
    return S, n


@pytest.mark.parametrize('case', T.slice_cases(), ids=T.case_id)
def test_wgrad_is_exact_on_integers_with_partial_tiles_and_uneven_slices(pctx, case):
    g, N, dims = case
    S, ntiles = _uneven_slices(case)
    tile, o = T.TILES[T.view(g)], T.small_dims(g, dims)
    assert all(a % t != 0 for a, t in zip(o, tile) if t > 1), (o, tile)
    _exact_wgrad(pctx, case)


@pytest.mark.parametrize('case', T.valu_cases(), ids=T.case_id)
def test_wgrad_valu_and_bias_are_exact_with_uneven_voxel_slices(pctx, case):
    S, nvox = _uneven_slices(case)
    assert S == 1024 and nvox == case[1] * int(np.prod(T.small_dims(case[0], case[2])))
    layer, x, dout, d = _exact_wgrad(pctx, case)
    assert int(np.prod(dout.shape[:4])) % 1024 != 0            # the bias slices are uneven too


def _train_conv(layer):
    """The trainer's layer object over an ops.ConvLayer."""
    class _Conv:
        pass
    c = _Conv()
    c.layer = layer
    return train.TrainConv(c, torch.device('cuda', 0))


@pytest.mark.parametrize('case', T.small_grids(), ids=T.case_id)
def test_gradients_are_exact_on_the_small_grids_the_trainer_runs(pctx, case):
    g, N, dims = case
    layer, x, dout, d = _exact_wgrad(pctx, case)
    if g[7]:
        return
    assert _family(pctx, ops.dual_desc(d)) in TRAINING_FAMILIES
    tc = _train_conv(layer)
    xd = torch.from_numpy(x).cuda()
    dx = train.dgrad(pctx, tc, d, torch.from_numpy(dout).cuda(), xd)
    _assert_exact('dX', dx, T.int_reference(g, N, dims, SEED)[2])


@pytest.mark.parametrize('case', T.noncubic_cases(), ids=T.case_id)
def test_gradients_on_a_non_cubic_grid(pctx, case):
    g, N, dims = case
    assert len(set(dims)) == 3 and len(set(T.small_dims(g, dims))) == 3
    tile = T.TILES.get(T.view(g), (1, 1, 1))
    assert all(a % t != 0 for a, t in zip(T.small_dims(g, dims), tile) if t > 1)
    layer, x, dout, d = _exact_wgrad(pctx, case)
    assert _family(pctx, ops.dual_desc(d)) in TRAINING_FAMILIES
    _assert_exact('dX', _dgrad(pctx, layer, x, dout), T.int_reference(g, N, dims, SEED)[2])
    layer, x, dout = _gauss_case(g, N, dims, 12)
    d, dw, db = _wgrad(pctx, layer, x, dout)
    _check_wgrad(layer, d, x, dout, dw, db)
    _check_dgrad(layer, x, dout, _dgrad(pctx, layer, x, dout))


@pytest.mark.parametrize('case', T.mixed_parity_cases(), ids=T.case_id)
def test_wgrad_is_exact_on_large_grids_of_mixed_parity(pctx, case):
    assert len({n % 2 for n in case[2]}) == 2
    _exact_wgrad(pctx, case)


@pytest.mark.parametrize('n', [1, 255, 257, None], ids=['1', '255', '257', 'second-pass'])
def test_relu_backward_masks_by_act_greater_than_zero(pctx, n):
    if n is None:
        n = pctx.num_cu * 32 * 256 + 5           # a few elements past one pass of the largest grid pcc_relu_backward launches
    rng = np.random.default_rng(13)
    special = np.array([0, 0x80000000, 1, 0x80000001, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000], np.uint32)
    # +0, -0, the smallest denormal, its negative, 1, -1, inf, -inf, NaN
    act = rng.normal(0, 1, n).astype(np.float32)
    grad = rng.normal(0, 1, n).astype(np.float32)
    gspecial = np.array([np.inf, -np.inf, np.nan, -0.0, 1e-45], np.float32)
    pos = rng.permutation(n)
    if n >= 64:                                  # every act special under a finite, an inf and a NaN gradient
        k = len(special)
        for j in range(3):
            act[pos[j * k:(j + 1) * k]] = special.view(np.float32)
        grad[pos[k:2 * k]] = np.inf
        grad[pos[2 * k:3 * k]] = np.nan
        grad[pos[3 * k:3 * k + len(gspecial)]] = gspecial
        act[-1], grad[-1] = np.float32(1e-45), -np.inf           # the last element of the last pass
    else:
        act[0], grad[0] = np.float32(1e-45), np.nan
    a = act.view(np.uint32)
    keep = (a > 0) & (a <= 0x7f800000)           # act > 0 on the bits: positive, denormals and +inf included, NaN and zeros not
    assert np.array_equal(keep, act > 0)
    want = np.where(keep, grad.view(np.uint32), np.uint32(0))
    got = ops.relu_backward(pctx, torch.from_numpy(grad.copy()).cuda(), torch.from_numpy(act).cuda()).cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (f'{len(bad)} of {n} differ, first at {bad[0]}: act {a[bad[0]]:#010x} grad '
                           f'{grad.view(np.uint32)[bad[0]]:#010x} got {got[bad[0]]:#010x} want {want[bad[0]]:#010x}')


def _step(pctx, tc, x, dout):
    """One forward and backward of train.conv: (y, dX, dW), the parameter gradients cleared first."""
    tc.weight.grad = None
    xd = torch.from_numpy(x).cuda().requires_grad_()
    y = train.conv(pctx, tc, xd)
    y.backward(torch.from_numpy(dout).cuda())
    return y.detach().clone(), xd.grad.clone(), tc.weight.grad.clone()


def test_packed_images_follow_in_place_weight_updates(pctx):
    g = (16, 16, 3, 1, 1, 1, 0, 0)               # 16 -> 16 k3 s1 transposed, ReLU, no bias
    assert T.view(g) in T.TILES
    N, dims = 2, (8, 8, 8)
    layer, x, dout = T.int_case(g, N, dims, SEED)
    tc = _train_conv(layer)
    d = tc.desc(N, *dims)
    assert tc.packed(pctx, d) is not None and tc.packed(pctx, ops.dual_desc(d)) is not None      # both read a packed image
    y1, dx1, dw1 = _step(pctx, tc, x, dout)
    assert bool((y1 != 0).any()) and bool((dx1 != 0).any())
    with torch.no_grad():
        tc.weight.mul_(2)
    y2, dx2, dw2 = _step(pctx, tc, x, dout)
    assert torch.equal(y2, 2 * y1) and torch.equal(dx2, 2 * dx1) and torch.equal(dw2, dw1)
    # an optimizer step (weights no longer integers): the forward and dX are those of the new weights
    tc.weight.grad = dw2
    torch.optim.SGD([tc.weight], lr=1e-3).step()
    y3, dx3, _ = _step(pctx, tc, x, dout)
    assert not torch.equal(y3, y2)
    w = tc.weight.detach().cpu().numpy()
    assert not np.array_equal(w, 2 * layer.kernel)
    ref = [R.layer(torch.from_numpy(x).double(), torch.from_numpy(ws).double(), None, 1, True, relu).numpy()
           for ws, relu in ((w, True), (np.abs(w), False))]
    # one output is a sum of at most k^3 Cin products accumulated in fp32 (any order), the bound of the dual's dgrad
    bound = 2 * 27 * 16 * EPS * ref[1] + 1e-30
    err = np.abs(y3.cpu().numpy().astype(np.float64) - ref[0])
    assert np.all(err <= bound), f'forward after the step: max err/bound {np.max(err / bound):.3g}'
    _check_dgrad(ops.ConvLayer(w, None, 1, True, True), x, dout * (y3.cpu().numpy() > 0), dx3)      # under the mask the kernel used


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
