"""conv16_wino_f16s_kernel and conv_tr2m_f16s_kernel on inputs with a dynamic range inside a block (tests/_dynamic_range_cases.py): held, per
output, to the numpy model of their documented arithmetic (tests/_f16s_model.py) and, through the model's derived bound, to a float64
convolution; their exact-fp32 siblings run the same inputs as controls.  DESIGN.md section 4.1 states the contract and the figures."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_range_cases as DC      # noqa: E402
import _f16s_model as M                # noqa: E402

from pcc_geo_cnn_v2_amd import _lib as L      # noqa: E402
from pcc_geo_cnn_v2_amd import ops            # noqa: E402

pytestmark = pytest.mark.gpu

ALL = list(range(len(DC.GEOMS)))
# accumulation: n terms summed in fp32 in some fixed order cost at most n 2^-24 of the sum of their magnitudes per unit of c; c = 2 is
# the figure tests/test_train_gpu.py uses for MFMA chains (test_dgrad_through_the_dual_descriptor)
C_ACC = 2.0
TWO_PIECE = {'wino': 'conv16_wino_f16s', 'tr2m': 'conv_tr2m_f16s'}
EXACT = {'wino': 'conv16_wino (', 'tr2m': 'conv_tr2m ('}
EXACT_SWITCHES = {'wino': dict(no_split=True), 'tr2m': dict(no_split=True, tr2m=True)}
_LAYERS, _OUT = {}, {}


def _layer(i):
    if i not in _LAYERS:
        inp = DC.inputs(i)
        _LAYERS[i] = ops.ConvLayer(np.array(inp['w']), None if inp['bias'] is None else np.array(inp['bias']), inp['stride'], inp['transposed'], inp['relu'])
    return _LAYERS[i]


def _launch(ctx, i, want, x=None, res=None):
    """one launch through ops.conv3d with the kernel family asserted; x / res default to the case's"""
    inp = DC.inputs(i)
    layer = _layer(i)
    x = inp['x'] if x is None else x
    res = inp['res'] if res is None else res
    impl = L.PCC_IMPL_WINOGRAD if inp['family'] == 'wino' else L.PCC_IMPL_AUTO
    N, D, H, W, _ = x.shape
    d = layer.desc(N, D, H, W, L.PCC_CONV_ADD if res is not None else 0, impl)
    buf = ctypes.create_string_buffer(96)
    L.check(L.lib().pcc_conv_kernel_family(ctx.handle, ctypes.byref(d), buf, 96), 'pcc_conv_kernel_family')
    assert buf.value.decode().startswith(want), (buf.value.decode(), want)
    xt = torch.from_numpy(np.array(x, np.float32)).to(ctx.device)
    rt = None if res is None else torch.from_numpy(np.array(res, np.float32)).to(ctx.device)
    out = ops.conv3d(ctx, xt, layer, residual=rt, impl=impl)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _two_piece(ctx, i):
    if (i, 2) not in _OUT:
        _OUT[(i, 2)] = _launch(ctx, i, TWO_PIECE[DC.GEOMS[i]['family']])
    return _OUT[(i, 2)]


def _exact(ctx, i):
    if (i, None) not in _OUT:
        fam = DC.GEOMS[i]['family']
        with ctx.numerics_override(**EXACT_SWITCHES[fam]):
            _OUT[(i, None)] = _launch(ctx, i, EXACT[fam])
    return _OUT[(i, None)]


def _acc_bound(m):
    return C_ACC * m['n'] * M.U32 * m['A'] + 2.0 ** -23 * np.abs(m['value'])


def _check(got, centre, bound, what):
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - centre)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f'{what}: max |err| / bound = {ratio.max():.3f}')
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float(ratio.max()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize('i', ALL, ids=lambda i: DC.IDS[i])
def test_two_piece_kernel_matches_the_model_of_its_arithmetic(ctx, i):
    """|kernel - model| <= c n 2^-24 A + 2^-23 |model|: the kernel may differ from the model by its fp32 accumulation (n terms, A = the sum
    of their magnitudes) and the rounding of the result, by nothing else.  A flushed denormal piece, a wrong clamp or a wrong bias
    scale breaks this on hot_voxel_20 / tiny_block / sparse_bias (tests/test_f16s_model_cpu.py shows by how much)."""
    m = DC.model(i)
    _check(_two_piece(ctx, i), m['value'], _acc_bound(m), DC.IDS[i] + ' two-piece kernel against its model')


@pytest.mark.parametrize('i', ALL, ids=lambda i: DC.IDS[i])
def test_two_piece_kernel_is_within_the_derived_bound_of_float64(ctx, i):
    """|kernel - exact| <= (operand bound of the model, tests/test_f16s_model_cpu.py) + (accumulation term above)"""
    m = DC.model(i)
    ref, _ = DC.reference(i)
    _check(_two_piece(ctx, i), ref, m['bound'] + _acc_bound(m), DC.IDS[i] + ' two-piece kernel against float64')


@pytest.mark.parametrize('i', ALL, ids=lambda i: DC.IDS[i])
def test_exact_fp32_sibling_as_control(ctx, i):
    """The same inputs through conv16_wino / conv_tr2m (fp32 operands) against the fp32-operand model under the same accumulation bound,
    and the far-output figures of both kernels beside the model's."""
    m = DC.model(i, None)
    got = _exact(ctx, i)
    _check(got, m['value'], _acc_bound(m), DC.IDS[i] + ' exact kernel against the fp32-operand model')
    ref, _ = DC.reference(i)
    _check(got, ref, m['bound'] + _acc_bound(m), DC.IDS[i] + ' exact kernel against float64')
    print(f'{DC.IDS[i]}: far outputs of block 0, max err / T: two-piece kernel {DC.far_ratio(i, _two_piece(ctx, i)[0]):.2e} '
          f'(model {DC.far_ratio(i, DC.model(i)["value"][0]):.2e}), exact kernel {DC.far_ratio(i, got[0]):.2e} (model {DC.far_ratio(i, m["value"][0]):.2e})')


@pytest.mark.parametrize('i', ALL, ids=lambda i: DC.IDS[i])
def test_bits_do_not_depend_on_the_call_the_position_or_a_power_of_two(ctx, i):
    """Two calls are equal; block 0's bits are the same at n = 0, at n = 1 and alone (its pre-scale is its own); without a bias, scaling
    block 0 (and its residual) by 2^7 scales its output bit for bit."""
    inp = DC.inputs(i)
    want = TWO_PIECE[inp['family']]
    base = _two_piece(ctx, i)
    assert np.array_equal(_launch(ctx, i, want).view(np.uint32), base.view(np.uint32))
    x, res = inp['x'], inp['res']
    if x.shape[0] == 2:
        swapped = _launch(ctx, i, want, x=x[::-1], res=None if res is None else res[::-1])
        assert np.array_equal(swapped[1].view(np.uint32), base[0].view(np.uint32))
        assert np.array_equal(swapped[0].view(np.uint32), base[1].view(np.uint32))
        alone = _launch(ctx, i, want, x=x[:1], res=None if res is None else res[:1])
        assert np.array_equal(alone[0].view(np.uint32), base[0].view(np.uint32))
    if inp['case'] in DC.BIAS_FREE:
        xs = x.copy()
        xs[0] *= np.float32(2.0 ** 7)
        rs = None
        if res is not None:
            rs = res.copy()
            rs[0] *= np.float32(2.0 ** 7)
        scaled = _launch(ctx, i, want, x=xs, res=rs)
        assert np.array_equal(scaled[0].view(np.uint32), (base[0] * np.float32(2.0 ** 7)).view(np.uint32))
        assert np.array_equal(scaled[1:].view(np.uint32), base[1:].view(np.uint32))


def test_recorded_block_maxima_equal_a_reduction_under_a_hot_voxel(ctx):
    """test_recorded_block_maxima_equal_a_reduction_over_the_tensor (tests/test_round6_gpu.py) with a 2^20 range inside block 0: the c3p
    synthesis transform in one launch (maxima recorded by the producing kernels) and layer by layer (maxima reduced from the tensor)
    must give the same bits, and finite ones."""
    from pcc_geo_cnn_v2_amd.model_transforms import SynthesisTransformProgressiveV2, init_transform
    tr = init_transform(SynthesisTransformProgressiveV2(64, data_format='channels_last'), 64, np.random.default_rng(1))
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 8, 8, 8, 64)).astype(np.float32)
    x[0] = np.maximum(x[0], 0)
    x[0, 2, 3:5, 3:5, :] = (x[0, 2, 3:5, 3:5, :] + np.float32(0.5)) * np.float32(2.0 ** 20)
    xt = torch.from_numpy(x).to(ctx.device)
    a = tr.forward_ndhwc(ctx, xt)
    os.environ['PCC_LAYERWISE'] = '1'
    try:
        b = tr.forward_ndhwc(ctx, xt)
    finally:
        del os.environ['PCC_LAYERWISE']
    assert torch.equal(a, b) and torch.isfinite(a).all()
