"""The case table of the recorded-bits tests (tests/test_family_bits_gpu.py, tests/test_family_bits_cpu.py) and of the generator that
records them (tests/golden/make_family_bits.py): two or three small layers per kernel family that pcc_conv_kernel_family can name, the
inputs of each (tests/_bits_ref.py: no library RNG), its launch through pcc_conv3d and its float64-accumulating oracle.

Importing this module needs numpy only; the functions that launch import torch and the package when called.
"""
import os

import numpy as np

import _bits_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'family_bits.json')

# stated tolerances of the suite (tests/test_conv_gpu.py, tests/test_round6_gpu.py): |gpu - oracle| <= tol * (1 + max |oracle|)
TOL = 2e-5            # exact fp32 kernels, and the split kernels the suite holds to the same figure
TOL_SPLIT = 8e-6      # bf16 x 3 Winograd and direct split kernels, two-piece fp16 kernels on 16 channels and the two-piece march
TOL_F16 = 4e-3        # fp16 mode against unrounded operands
TOL_F16_Q = 6e-4      # fp16 mode against the same fp16-rounded operands, fp16 output (or the fp16 partial sums of 64 channels)
TOL_F16_Q32 = 1e-5    # ... fp32 output of conv_f16 on 16 / 32 channels: only the accumulation order is left

# the 18 names of csrc/conv_route.hip, pcc_conv_kernel_family
FAMILIES = {
    'generic': 'generic (reference-order fp32 FMA chain)',
    'conv_f16': 'conv_f16 (fp16 storage, f16 MFMA)',
    'conv_fwd': 'conv_fwd (exact fp32 MFMA)',
    'conv_fwd_f16': 'conv_fwd (f16 MFMA)',
    'split16': 'conv_k3s1_split (direct, bf16 x 3, 16x16x32 MFMA)',
    'split32': 'conv_k3s1_split32 (direct, bf16 x 3, 32x32x16 MFMA)',
    'wino': 'conv16_wino (Winograd, exact fp32 MFMA)',
    'wino_bf16': 'conv16_wino_bf16 (Winograd, bf16 x 3)',
    'wino_f16s': 'conv16_wino_f16s (Winograd, fp16 x 2 under a per-block pre-scale)',
    'tr2': 'conv_tr2 (exact fp32 MFMA)',
    'tr2m_f16': 'conv_tr2m_f16 (z march, f16 MFMA)',
    'tr2m_f16s': 'conv_tr2m_f16s (z march, fp16 x 2 under a per-block pre-scale)',
    'tr2_split': 'conv_tr2_split (parity classes, bf16 x 3)',
    'tr2m_bf16': 'conv_tr2m_bf16 (z march, bf16 x 3)',
    'tr2m': 'conv_tr2m (z march, exact fp32 MFMA)',
    'cin1': 'conv_cin1 (exact fp32 MFMA)',
    'cout1_mfma': 'conv_cout1_mfma (exact fp32 MFMA)',
    'cout1': 'conv_cout1 (fp32 VALU)',
}

PLAIN = dict(bias=False, relu=False, res=False)
FULL = dict(bias=True, relu=True, res=True)
NORES = dict(bias=True, relu=True, res=False)       # families without a residual input (the stride-2 marches and parity-class tiles)


def _case(cid, fam, geo, impl='AUTO', switches=None, mode='fp32', tol=TOL, tol_q=None, ocs=0, oco=0, **epilogue):
    """geo = (N, D, H, W, Cin, Cout, k, stride, transposed).  mode: 'fp32' | 'f16' (PCC_CONV_F16, fp32 tensors) | 'in16-out16' |
    'in16-out32' (conv_f16.hip: fp16 input and residual) | 'out16' (PCC_CONV_F16 | OUT16: the fp16 hand-over of a stride-2 layer).
    ocs / oco: channel stride / offset of the output buffer (0: dense)."""
    c = dict(id=cid, family=FAMILIES[fam], geo=tuple(geo), impl=impl, switches=dict(switches or {}), mode=mode, tol=tol, tol_q=tol_q,
             ocs=ocs, oco=oco)
    c.update(epilogue)
    return c


# `a`: plain, full tiles.  `b`: bias + ReLU (+ residual where the family takes one), N = 2, odd D, a partial tile in y or z where the
# family allows one (Winograd and the marches need H, W = 0 mod 16: their partial tile is the odd D), a channel-offset output where the
# family honours one.  The families are reached as FAMILY_CASES of tests/test_round6_gpu.py reaches them (same impl, switches, flags).
# Cases that share a geometry and an epilogue share their inputs bit for bit (SENSITIVITY below compares their digests).
_W16 = (1, 4, 16, 16, 16, 16, 3, 1, 1)        # the 16-channel transposed stride-1 layer of the c3p synthesis blocks, one x-y tile
_W32 = (2, 5, 16, 32, 32, 32, 3, 1, 0)
_T16 = (1, 2, 16, 16, 32, 16, 3, 2, 1)        # Conv3DTranspose k3 stride 2, 32 -> 16
_T16B = (2, 5, 32, 16, 32, 16, 3, 2, 1)
_T32B = (2, 5, 16, 32, 64, 32, 3, 2, 1)
_S32 = (2, 5, 12, 32, 32, 32, 3, 1, 0)        # direct split kernels: partial tiles in z and y
CASES = [
    _case('generic-a', 'generic', (1, 4, 8, 8, 16, 16, 3, 1, 0), 'GENERIC', **PLAIN),
    _case('generic-b', 'generic', (2, 7, 9, 6, 3, 5, 3, 1, 0), ocs=8, oco=2, **FULL),
    _case('conv_f16-a', 'conv_f16', (1, 4, 16, 16, 16, 16, 3, 1, 0), mode='in16-out16', tol=TOL_F16, tol_q=TOL_F16_Q, **PLAIN),
    _case('conv_f16-b', 'conv_f16', _W32, mode='in16-out32', tol=TOL_F16, tol_q=TOL_F16_Q32, **FULL),
    _case('conv_f16-c', 'conv_f16', (2, 3, 16, 16, 64, 64, 3, 1, 1), mode='in16-out16', tol=TOL_F16, tol_q=TOL_F16_Q, **FULL),
    _case('conv_fwd-a', 'conv_fwd', (1, 4, 8, 16, 16, 32, 3, 2, 0), **PLAIN),
    _case('conv_fwd-b', 'conv_fwd', (2, 5, 10, 16, 16, 16, 3, 1, 0), 'MFMA', ocs=24, oco=8, **FULL),
    _case('conv_fwd_f16-a', 'conv_fwd_f16', (1, 4, 8, 16, 16, 32, 3, 2, 0), mode='f16', tol=TOL_F16, **PLAIN),
    _case('conv_fwd_f16-b', 'conv_fwd_f16', (2, 5, 10, 16, 16, 16, 3, 1, 0), mode='f16', tol=TOL_F16, ocs=24, oco=8, **FULL),
    _case('split16-a', 'split16', (1, 8, 8, 8, 64, 64, 3, 1, 1), tol=TOL_SPLIT, **PLAIN),
    _case('split16-b', 'split16', _S32, 'SPLIT', {'split_mfma16': True}, tol=TOL_SPLIT, ocs=40, oco=8, **FULL),
    _case('split32-a', 'split32', (1, 4, 16, 16, 32, 32, 3, 1, 1), tol=TOL_SPLIT, **PLAIN),
    _case('split32-b', 'split32', _S32, 'SPLIT', tol=TOL_SPLIT, ocs=40, oco=8, **FULL),
    _case('split32-c', 'split32', (2, 3, 7, 32, 64, 64, 3, 1, 0), 'SPLIT', {'split_mfma32': True}, tol=TOL_SPLIT, **FULL),
    _case('wino-a', 'wino', _W16, switches={'no_split': True}, **PLAIN),
    _case('wino-b', 'wino', _W32, 'WINOGRAD', {'no_f16s': True}, ocs=48, oco=12, **FULL),
    _case('wino_bf16-a', 'wino_bf16', _W16, switches={'no_f16s': True}, tol=TOL_SPLIT, **PLAIN),
    _case('wino_bf16-b', 'wino_bf16', (2, 5, 32, 16, 16, 16, 3, 1, 0), switches={'no_f16s': True}, tol=TOL_SPLIT, ocs=32, oco=12, **FULL),
    _case('wino_f16s-a', 'wino_f16s', _W16, tol=TOL_SPLIT, **PLAIN),
    _case('wino_f16s-b', 'wino_f16s', _W32, 'WINOGRAD', ocs=48, oco=12, **FULL),
    _case('wino_f16s-c', 'wino_f16s', (2, 3, 16, 16, 64, 64, 3, 1, 1), **FULL),
    _case('tr2-a', 'tr2', (1, 4, 4, 4, 32, 32, 5, 2, 1), **PLAIN),
    _case('tr2-b', 'tr2', _T16, switches={'no_tr2m': True}, **PLAIN),
    _case('tr2-c', 'tr2', (2, 3, 10, 16, 32, 16, 3, 2, 1), switches={'no_tr2m': True}, ocs=24, oco=8, **FULL),
    _case('tr2m_f16-a', 'tr2m_f16', _T16, mode='out16', tol=TOL_F16, tol_q=TOL_F16_Q, **PLAIN),
    _case('tr2m_f16-b', 'tr2m_f16', _T32B, mode='out16', tol=TOL_F16, tol_q=TOL_F16_Q, ocs=48, oco=8, **NORES),
    _case('tr2m_f16s-a', 'tr2m_f16s', _T16, tol=TOL_SPLIT, **PLAIN),
    _case('tr2m_f16s-b', 'tr2m_f16s', _T32B, tol=TOL_SPLIT, ocs=48, oco=8, **NORES),
    _case('tr2_split-a', 'tr2_split', (1, 8, 8, 8, 64, 64, 3, 2, 1), **PLAIN),
    _case('tr2_split-b', 'tr2_split', (2, 3, 7, 16, 64, 32, 3, 2, 1), ocs=48, oco=8, **NORES),
    _case('tr2m_bf16-a', 'tr2m_bf16', _T16, switches={'no_f16s': True}, **PLAIN),
    _case('tr2m_bf16-b', 'tr2m_bf16', _T16B, switches={'no_f16s': True}, ocs=24, oco=4, **NORES),
    _case('tr2m-a', 'tr2m', _T16, switches={'no_split': True}, **PLAIN),
    _case('tr2m-b', 'tr2m', _T16B, switches={'no_split': True}, ocs=24, oco=4, **NORES),
    _case('cin1-a', 'cin1', (1, 8, 16, 32, 1, 16, 9, 2, 0), **PLAIN),
    _case('cin1-b', 'cin1', (2, 6, 10, 32, 1, 32, 3, 2, 0), ocs=40, oco=8, **FULL),
    _case('cout1_mfma-a', 'cout1_mfma', (1, 4, 16, 16, 16, 1, 3, 1, 1), **PLAIN),
    _case('cout1_mfma-b', 'cout1_mfma', (2, 5, 10, 16, 16, 1, 3, 1, 1), **FULL),
    _case('cout1-a', 'cout1', (1, 4, 8, 8, 32, 1, 3, 1, 1), **PLAIN),
    _case('cout1-b', 'cout1', (2, 5, 6, 16, 32, 1, 3, 1, 1), **FULL),
]
BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)

# Pairs that compute the same layer on the same inputs with different arithmetic: their digests must differ (the digest sees a
# reordered sum or another operand split, and the switches switch).  Left column from the table; right column from the table or a
# variant of a table case under other switches (computed, never recorded).
SENSITIVITY = [
    ('wino_f16s-a', 'wino_bf16-a'), ('wino_f16s-a', 'wino-a'), ('wino_bf16-a', 'wino-a'),
    ('tr2m_f16s-a', 'tr2m_bf16-a'), ('tr2m_bf16-a', 'tr2m-a'), ('tr2m-a', 'tr2-b'), ('tr2m_f16s-a', 'tr2-b'),
    ('split16-b', 'split32-b'), ('wino-b', 'wino_f16s-b'),
    ('wino-b', ('wino-b', {'no_f16s': True, 'wino_per_group': True})),
]


def variant(cid, switches):
    c = dict(BY_ID[cid])
    c['switches'] = dict(switches)
    c['id'] = cid + '+' + '+'.join(sorted(switches))
    c['family'] = None           # not asserted: only the bits are compared
    return c


def geo_tag(case):
    return '.'.join(str(v) for v in case['geo'])


def inputs(case):
    """x, w (Keras layout), b or None, r or None as float32 numpy arrays; a function of the geometry and the epilogue only."""
    N, D, H, W, cin, cout, k, s, tr = case['geo']
    t = geo_tag(case)
    x = BR.tensor('x/' + t, (N, D, H, W, cin), 'act')
    w = BR.tensor('w/' + t, (k, k, k, cout, cin) if tr else (k, k, k, cin, cout), 'weight', fan_in=k ** 3 * cin)
    b = BR.tensor('b/' + t, (cout,), 'bias') if case['bias'] else None
    r = None
    if case['res']:
        o = (lambda n: n * s) if tr else (lambda n: -(-n // s))
        r = BR.tensor('r/' + t, (N, o(D), o(H), o(W), cout), 'residual')
    return x, w, b, r


def _flags(case, L):
    m = case['mode']
    f = 0
    if m != 'fp32':
        f |= L.PCC_CONV_F16
    if m.startswith('in16'):
        f |= L.PCC_CONV_IN16 | (L.PCC_CONV_RES16 if case['res'] else 0)
    if m in ('in16-out16', 'out16'):
        f |= L.PCC_CONV_OUT16
    if case['res']:
        f |= L.PCC_CONV_ADD
    if case.get('clip'):        # rows of tests/_direct_cases.py
        f |= L.PCC_CONV_CLIP01
    return f


def run(ctx, case, arrays=None):
    """Launch the case through pcc_conv3d under its switches.  Returns (family name, the WHOLE output buffer as a numpy array of its own
    dtype -- with a channel-offset output that includes the channels the kernel must leave at zero)."""
    import ctypes as C

    import torch
    from pcc_geo_cnn_v2_amd import _lib as L, ops
    N, D, H, W, cin, cout, k, s, tr = case['geo']
    x, w, b, r = arrays if arrays is not None else inputs(case)
    layer = ops.ConvLayer(w, b, s, bool(tr), case['relu'])
    m = case['mode']
    in16, out16 = m.startswith('in16'), m in ('in16-out16', 'out16')
    dev = lambda a, half: None if a is None else (torch.from_numpy(a).half() if half else torch.from_numpy(a)).to(ctx.device).contiguous()
    xd, rd = dev(x, in16), dev(r, in16)
    oshape = ops.conv_out_shape(layer, x.shape)
    out = torch.zeros(tuple(oshape[:4]) + (case['ocs'] or cout,), dtype=torch.float16 if out16 else torch.float32, device=ctx.device)
    d = layer.desc(N, D, H, W, _flags(case, L), getattr(L, 'PCC_IMPL_' + case['impl']), case['ocs'], case['oco'])
    with ctx.numerics_override(**case['switches']):
        buf = C.create_string_buffer(96)
        L.check(L.lib().pcc_conv_kernel_family(ctx.handle, C.byref(d), buf, 96), 'pcc_conv_kernel_family')
        im = layer.device_images(ctx, d)
        p = ops._ptr
        L.check(L.lib().pcc_conv3d(ctx.handle, C.byref(d), p(xd), p(im['w']), p(im['pk']), p(im['b']), p(rd), p(out), ctx.stream), 'pcc_conv3d')
        torch.cuda.synchronize()
    return buf.value.decode(), out.cpu().numpy()


def _h(a):
    return None if a is None else a.astype(np.float16).astype(np.float32)


def oracle_refs(O, case, arrays=None):
    """[(reference, tolerance, what)]: the float64-accumulating C oracle (oracle/pcc_oracle.c) on the case's operands; in the fp16
    modes also on the operands rounded to fp16 where the kernel rounds them."""
    N, D, H, W, cin, cout, k, s, tr = case['geo']
    x, w, b, r = arrays if arrays is not None else inputs(case)
    conv = O.conv3d_transpose if tr else O.conv3d

    def ref(x_, w_, r_):
        y = conv(x_, w_, b, s, case['relu']).astype(np.float64)
        return y if r_ is None else y + r_
    out = [(ref(x, w, r), case['tol'], 'float64 oracle')]
    if case['tol_q'] is not None:
        in16 = case['mode'].startswith('in16')
        out.append((ref(_h(x), _h(w), _h(r) if in16 else r), case['tol_q'], 'float64 oracle on fp16-rounded operands'))
    return out


def written(case, buf):
    """The channels of the output buffer the layer writes, and whether everything else is still zero."""
    cout = case['geo'][5]
    if not case['ocs']:
        return buf.astype(np.float64), True
    o = case['oco']
    rest = np.delete(buf, np.s_[o:o + cout], axis=-1)
    return buf[..., o:o + cout].astype(np.float64), not rest.any()


def accuracy(O, case, buf, arrays=None):
    """[(max |got - ref| / (1 + max |ref|), tolerance, what)] and whether the channels outside the layer's stayed zero."""
    got, clean = written(case, buf)
    rows = []
    for ref, tol, what in oracle_refs(O, case, arrays):
        assert got.shape == ref.shape, (got.shape, ref.shape)
        rows.append((float(np.abs(got - ref).max() / (1 + np.abs(ref).max())), tol, what))
    return rows, clean


def family_number():
    """PCC_KERNEL_FAMILY of include/pcc_geo.h, read from the header (no library needed)."""
    import re
    with open(os.path.join(ROOT, 'include', 'pcc_geo.h')) as fh:
        m = re.search(r'^#define\s+PCC_KERNEL_FAMILY\s+(\d+)', fh.read(), re.M)
    return int(m.group(1))


# ---- training kernels: pinned in their own section ("training") -- a trained checkpoint depends on them, a coded stream does not, so a
# change of their bits asks for a regeneration and a note in DESIGN.md, never for a new PCC_KERNEL_FAMILY ------------------------------
# id -> (what, (cin, cout, k, stride, transposed, relu, bias, first)) in the notation of tests/test_train_gpu.py; N = 2, D = 8
TRAINING = {
    'wgrad-mfma-16-16-k3s1T': ('wgrad', (16, 16, 3, 1, 1, 1, 1, 0)),      # Cin, Cout multiples of 16: wgrad_mfma_kernel
    'wgrad-valu-1-16-k3s2': ('wgrad', (1, 16, 3, 2, 0, 1, 1, 1)),         # Cin = 1: the VALU kernel
    'dgrad-16-16-k3s1T': ('dgrad', (16, 16, 3, 1, 1, 1, 1, 0)),           # input gradient through the dual descriptor
}
TRAIN_N, TRAIN_D = 2, 8


def training_inputs(tid):
    from pcc_geo_cnn_v2_amd import ops
    what, (cin, cout, k, s, tr, relu, bias, _) = TRAINING[tid]
    t = f'{what}/{cin}.{cout}.k{k}s{s}t{tr}'
    w = BR.tensor('w/' + t, (k, k, k, cout, cin) if tr else (k, k, k, cin, cout), 'weight', fan_in=k ** 3 * cin)
    b = BR.tensor('b/' + t, (cout,), 'bias') if bias else None
    layer = ops.ConvLayer(w, b, s, bool(tr), bool(relu))
    x = BR.tensor('x/' + t, (TRAIN_N, TRAIN_D, TRAIN_D, TRAIN_D, cin), 'act')
    dout = BR.tensor('g/' + t, ops.conv_out_shape(layer, x.shape), 'residual')
    return layer, x, dout


def run_wgrad(pctx, tid):
    """(layer, desc, x, dout, dW, dB) of pcc_conv3d_wgrad on the hash inputs (as tests/test_train_gpu.py::_wgrad_case launches it)."""
    import torch
    from pcc_geo_cnn_v2_amd import ops
    layer, x, dout = training_inputs(tid)
    d = layer.desc(TRAIN_N, TRAIN_D, TRAIN_D, TRAIN_D)
    dw = torch.empty(layer.kernel.shape, dtype=torch.float32, device='cuda')
    db = torch.empty(layer.cout, dtype=torch.float32, device='cuda')
    ops.conv3d_wgrad(pctx, d, torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda(), dw, db)
    torch.cuda.synchronize()
    return layer, d, x, dout, dw, db


def run_dgrad(pctx, tid):
    """(layer, x, dout, dX) of the input gradient: pcc_conv3d on the dual descriptor with the device-repacked weights (as
    tests/test_train_gpu.py::test_dgrad_through_the_dual_descriptor launches it)."""
    import ctypes as C

    import torch
    from pcc_geo_cnn_v2_amd import _lib as L, ops
    layer, x, dout = training_inputs(tid)
    dd = ops.dual_desc(layer.desc(TRAIN_N, TRAIN_D, TRAIN_D, TRAIN_D))
    m = ops.conv_repack_map(dd)
    wd = torch.from_numpy(layer.kernel).cuda()
    pk = None
    if m is not None:
        pk = ops.conv_repack_device(pctx, dd, torch.from_numpy(m).cuda(), wd, torch.empty(m.shape, dtype=torch.float32, device='cuda'))
    dx = torch.empty(x.shape, dtype=torch.float32, device='cuda')
    L.check(L.lib().pcc_conv3d(pctx.handle, C.byref(dd), ops._ptr(torch.from_numpy(dout).cuda()), ops._ptr(wd), ops._ptr(pk),
                               None, None, ops._ptr(dx), pctx.stream), 'dgrad')
    torch.cuda.synchronize()
    return layer, x, dout, dx


def check_dgrad(layer, x, dout, dx):
    """The bound of tests/test_train_gpu.py::test_dgrad_through_the_dual_descriptor: one output is a sum of at most k^3 Cout products
    accumulated in fp32 in any order: |error| <= 2 k^3 Cout 2^-24 sum |terms|, against float64 autograd.  Returns max error / bound."""
    import torch

    import _train_ref as R
    ref = []
    for gs, ws in ((dout, layer.kernel), (np.abs(dout), np.abs(layer.kernel))):
        xt = torch.from_numpy(x).double().requires_grad_()
        y = (R.conv3d_transpose if layer.transposed else R.conv3d)(xt, torch.from_numpy(ws).double(), layer.stride)
        (y * torch.from_numpy(gs).double()).sum().backward()
        ref.append(xt.grad.numpy())
    bound = 2 * layer.k ** 3 * layer.cout * 2.0 ** -24 * ref[1] + 1e-30
    err = np.abs(dx.cpu().numpy().astype(np.float64) - ref[0])
    return float(np.max(err / bound))
