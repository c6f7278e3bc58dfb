"""The three-piece bf16 conv kernels -- conv_k3s1_split / conv_k3s1_split32 / conv_tr2_split (csrc/conv_split.hip), conv_tr2m_bf16 and
conv16_wino_bf16 -- held, per output, to the numpy model of their documented arithmetic (tests/_bf16x3_model.py) and, through the model's
bound, to a float64 convolution: on impulse lattices, where every output of a direct kernel is ONE product and a lost piece costs ten times
the bound, and on dense inputs with a dynamic range inside a block (tests/_impulse_cases.py).  The exact-fp32 siblings run the same inputs as
controls.  tests/test_bf16x3_model_cpu.py shows what these assertions can see; DESIGN.md section 4.2 states the contract and the figures."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bf16x3_model as B              # noqa: E402
import _impulse_cases as IC            # noqa: E402

from pcc_geo_cnn_v2_amd import _lib as L      # noqa: E402
from pcc_geo_cnn_v2_amd import ops            # noqa: E402

pytestmark = pytest.mark.gpu

# accumulation: n terms summed in fp32 in some fixed order cost at most n 2^-24 of the sum of their magnitudes per unit of c; c = 2 is the
# figure of tests/test_dynamic_range_gpu.py and tests/test_train_gpu.py for MFMA chains
C_ACC = 2.0
CASES = [(gi, v) for gi in range(len(IC.GEOMS)) for v in IC.VARIANTS]
CASE_IDS = [f'{IC.IDS[gi]}-{v}' for gi, v in CASES]
DENSE = list(range(len(IC.DENSE)))
_LAYERS, _OUT = {}, {}


def _layer(key, p):
    if key not in _LAYERS:
        _LAYERS[key] = ops.ConvLayer(np.array(p['w']), None if p['bias'] is None else np.array(p['bias']), p['stride'], p['transposed'], p['relu'])
    return _LAYERS[key]


def _launch(ctx, key, p, x, res, exact=False):
    """one launch through ops.conv3d, the kernel family asserted by name; exact: the exact-fp32 sibling (no_split)"""
    _, want, impl, switches, control, control_impl = IC.KERNELS[p['kernel']]
    if exact:
        want, impl, switches = control, control_impl, dict(switches, no_split=True)
    impl = getattr(L, 'PCC_IMPL_' + impl)
    layer = _layer(key, p)
    N, D, H, W, _ = x.shape
    with ctx.numerics_override(**switches):
        d = layer.desc(N, D, H, W, L.PCC_CONV_ADD if res is not None else 0, impl)
        buf = ctypes.create_string_buffer(96)
        L.check(L.lib().pcc_conv_kernel_family(ctx.handle, ctypes.byref(d), buf, 96), 'pcc_conv_kernel_family')
        assert buf.value.decode().startswith(want), (buf.value.decode(), want)
        xt = torch.from_numpy(np.array(x, np.float32)).to(ctx.device)
        rt = None if res is None else torch.from_numpy(np.array(res, np.float32)).to(ctx.device)
        out = ops.conv3d(ctx, xt, layer, residual=rt, impl=impl)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, centre, bound, what):
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - centre)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float(ratio.max()), np.argwhere(bad)[:4].tolist())
    return float(ratio.max())


# ---- impulse lattices
def _impulse_out(ctx, gi, variant, l, exact=False):
    p = IC.layer_inputs(gi, variant)
    return _launch(ctx, ('imp', gi, variant), p, IC.launch_x(gi, l), p['res'], exact)


@pytest.mark.parametrize('gi,variant', CASES, ids=CASE_IDS)
def test_single_product_outputs_match_the_model_of_the_arithmetic(ctx, gi, variant):
    """Per output and launch: |kernel - model| <= c n 2^-24 A + 2^-23 |model| with n = 6 (+ bias, + residual) for the direct kernels: six piece
    products in three accumulating MFMAs and the rounding of the result, nothing else; |kernel - float64| <= the dropped terms + the same.
    Outputs that no impulse reaches hold relu(bias) (+ residual) bit for bit: no halo, padding or tile edge leaks."""
    worst = worst64 = 0.0
    clean = IC.untouched(gi, variant)
    for l in range(len(IC.plan(gi))):
        m = IC.model(gi, variant, l)
        got = _impulse_out(ctx, gi, variant, l)
        what = f'{IC.IDS[gi]}-{variant} launch {l}'
        worst = max(worst, _check(got, m['value'], B.acc_bound(m, C_ACC), what + ': kernel against its model'))
        worst64 = max(worst64, _check(got, IC.reference(gi, variant, l), m['bound'] + B.acc_bound(m, C_ACC), what + ': kernel against float64'))
        far = m['products'] == 0                # (a stride-1 lattice from origin 1 reaches every output of some grids: then nothing to compare)
        assert np.array_equal(got.view(np.uint32)[far], clean.view(np.uint32)[far]), what + ': an output that no impulse reaches moved'
    print(f'{IC.IDS[gi]}-{variant}: max |err| / bound = {worst:.3f} against the model, {worst64:.3f} against float64')


@pytest.mark.parametrize('gi,variant', CASES, ids=CASE_IDS)
def test_exact_fp32_sibling_on_the_same_impulses_as_control(ctx, gi, variant):
    """The same launches through the exact-fp32 family (no_split) against the fp32-operand model under the same accumulation bound: if both
    kernels missed it, the bound or the model would be wrong, not the split."""
    worst = 0.0
    for l in range(len(IC.plan(gi))):
        m = IC.model(gi, variant, l, None)
        got = _impulse_out(ctx, gi, variant, l, exact=True)
        what = f'{IC.IDS[gi]}-{variant} launch {l}: exact kernel'
        worst = max(worst, _check(got, m['value'], B.acc_bound(m, C_ACC), what + ' against the fp32-operand model'))
        _check(got, IC.reference(gi, variant, l), m['bound'] + B.acc_bound(m, C_ACC), what + ' against float64')
    print(f'{IC.IDS[gi]}-{variant}: exact-fp32 control, max |err| / bound = {worst:.3f}')


# ---- dense inputs with a dynamic range inside block 0
def _dense_launch(ctx, i, x=None, res=None, exact=False):
    inp = IC.dense_inputs(i)
    return _launch(ctx, ('dense', i), inp, inp['x'] if x is None else x, inp['res'] if res is None else res, exact)


def _dense_out(ctx, i, exact=False):
    if (i, exact) not in _OUT:
        _OUT[(i, exact)] = _dense_launch(ctx, i, exact=exact)
    return _OUT[(i, exact)]


@pytest.mark.parametrize('i', DENSE, ids=IC.DENSE_IDS)
def test_dense_outputs_match_the_model_and_float64(ctx, i):
    """the same two per-output checks with n = every nonzero piece product behind the output (tests/test_bf16x3_model_cpu.py prints why this
    alone could not see a lost piece)"""
    m = IC.dense_model(i)
    ref, _ = IC.dense_reference(i)
    got = _dense_out(ctx, i)
    r = _check(got, m['value'], B.acc_bound(m, C_ACC), IC.DENSE_IDS[i] + ': kernel against its model')
    r64 = _check(got, ref, m['bound'] + B.acc_bound(m, C_ACC), IC.DENSE_IDS[i] + ': kernel against float64')
    print(f'{IC.DENSE_IDS[i]}: max |err| / bound = {r:.3f} against the model, {r64:.3f} against float64')


@pytest.mark.parametrize('i', DENSE, ids=IC.DENSE_IDS)
def test_exact_fp32_sibling_on_dense_inputs_as_control(ctx, i):
    m = IC.dense_model(i, None)
    ref, _ = IC.dense_reference(i)
    got = _dense_out(ctx, i, exact=True)
    r = _check(got, m['value'], B.acc_bound(m, C_ACC), IC.DENSE_IDS[i] + ': exact kernel against the fp32-operand model')
    _check(got, ref, m['bound'] + B.acc_bound(m, C_ACC), IC.DENSE_IDS[i] + ': exact kernel against float64')
    print(f'{IC.DENSE_IDS[i]}: exact-fp32 control, max |err| / bound = {r:.3f}; far outputs of block 0, max err / T: three-piece kernel '
          f'{IC.dense_far_ratio(i, _dense_out(ctx, i)[0]):.2e} (model {IC.dense_far_ratio(i, IC.dense_model(i)["value"][0]):.2e}), exact kernel '
          f'{IC.dense_far_ratio(i, got[0]):.2e} (model {IC.dense_far_ratio(i, m["value"][0]):.2e})')


@pytest.mark.parametrize('i', DENSE, ids=IC.DENSE_IDS)
def test_dense_bits_do_not_depend_on_the_call_the_position_or_a_power_of_two(ctx, i):
    """Two calls are equal; block 0's bits are the same at n = 0, at n = 1 and alone; without a bias, scaling block 0 (and its residual) by 2^7
    scales its output bit for bit and leaves the neighbour's alone."""
    inp = IC.dense_inputs(i)
    base = _dense_out(ctx, i)
    assert np.array_equal(_dense_launch(ctx, i).view(np.uint32), base.view(np.uint32))
    x, res = inp['x'], inp['res']
    swapped = _dense_launch(ctx, i, x=x[::-1], res=None if res is None else res[::-1])
    assert np.array_equal(swapped[1].view(np.uint32), base[0].view(np.uint32))
    assert np.array_equal(swapped[0].view(np.uint32), base[1].view(np.uint32))
    alone = _dense_launch(ctx, i, x=x[:1], res=None if res is None else res[:1])
    assert np.array_equal(alone[0].view(np.uint32), base[0].view(np.uint32))
    if inp['case'] in IC.BIAS_FREE:
        xs = x.copy()
        xs[0] *= np.float32(2.0 ** 7)
        rs = None
        if res is not None:
            rs = res.copy()
            rs[0] *= np.float32(2.0 ** 7)
        scaled = _dense_launch(ctx, i, x=xs, res=rs)
        assert np.array_equal(scaled[0].view(np.uint32), (base[0] * np.float32(2.0 ** 7)).view(np.uint32))
        assert np.array_equal(scaled[1:].view(np.uint32), base[1:].view(np.uint32))


@pytest.mark.parametrize('i', [k for k in DENSE if IC.DENSE[k]['case'].startswith('hot_voxel')], ids=lambda i: IC.DENSE_IDS[i])
def test_a_hot_voxel_moves_no_output_it_does_not_reach(ctx, i):
    """These kernels apply no per-block scale: with the hot voxels set to 1 instead, every output that reads none of them keeps its bits."""
    inp = IC.dense_inputs(i)
    cool = inp['x'].copy()
    cool[0][inp['hot']] = 1
    got = _dense_launch(ctx, i, x=cool)
    far = ~IC.reach(inp['family'], inp['hot'])
    base = _dense_out(ctx, i)
    assert far.any() and not far.all()
    assert np.array_equal(got[0][far].view(np.uint32), base[0][far].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32))
    assert not np.array_equal(got[0][~far], base[0][~far])
