"""Convolution layers and whole transforms (include/pcc_geo.h: pcc_conv3d, pcc_network_forward_*), and their live profiling."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _ptr


class ConvLayer:
    """Weights of one Conv3D / Conv3DTranspose (Keras layouts) + their device images."""

    def __init__(self, kernel, bias, stride, transposed, relu):
        kernel = np.ascontiguousarray(kernel, np.float32)
        self.k = int(kernel.shape[0])
        assert kernel.shape[:3] == (self.k,) * 3
        self.transposed = bool(transposed)
        if transposed:
            self.cout, self.cin = int(kernel.shape[3]), int(kernel.shape[4])
        else:
            self.cin, self.cout = int(kernel.shape[3]), int(kernel.shape[4])
        self.kernel = kernel
        self.bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
        self.stride = int(stride)
        self.relu = bool(relu)
        self._dev = {}

    def desc(self, N, D, H, W, flags=0, impl=L.PCC_IMPL_AUTO, out_cstride=0, out_coffset=0):
        f = flags | (L.PCC_CONV_BIAS if self.bias is not None else 0) | (L.PCC_CONV_RELU if self.relu else 0)
        return L.ConvDesc(N, D, H, W, self.cin, self.cout, self.k, self.stride, int(self.transposed), f, impl,
                          out_cstride, out_coffset)

    def device_images(self, ctx, d):
        key = ctx.device.index
        if key not in self._dev:
            self._dev[key] = dict(w=torch.from_numpy(self.kernel).to(ctx.device),
                                  b=None if self.bias is None else torch.from_numpy(self.bias).to(ctx.device),
                                  pk=None)
        im = self._dev[key]
        if im['pk'] is None and L.lib().pcc_conv_mfma_supported(C.byref(d)) == 1:
            n = L.lib().pcc_conv_packed_floats(C.byref(d))
            pk = np.empty(n, np.float32)
            L.check(L.lib().pcc_conv_pack_weights(C.byref(d), self.kernel.ctypes.data_as(C.c_void_p),
                                                  pk.ctypes.data_as(C.c_void_p)), 'pcc_conv_pack_weights')
            im['pk'] = torch.from_numpy(pk).to(ctx.device)
        return im


def conv_out_shape(layer, x_shape):
    N, D, H, W, _ = x_shape
    s = layer.stride
    if layer.transposed:
        return (N, D * s, H * s, W * s, layer.cout)
    o = lambda n: -(-n // s)
    return (N, o(D), o(H), o(W), layer.cout)


def conv3d(ctx, x, layer, residual=None, flags=0, impl=L.PCC_IMPL_AUTO, out=None, out_coffset=0):
    """x: (N,D,H,W,Cin) float32 contiguous on ctx.device.  Returns (N,OD,OH,OW,Cout).  flags with PCC_CONV_IN16 / OUT16 / RES16 (a
    layer of the fp16 mode as network_plan plans it): x, residual and the result are fp16 where the bits say so."""
    if flags & (L.PCC_CONV_IN16 | L.PCC_CONV_OUT16 | L.PCC_CONV_RES16):
        assert impl == L.PCC_IMPL_AUTO and out is None
        return conv3d_fp16_storage(ctx, x, layer, residual, bool(flags & L.PCC_CONV_IN16), bool(flags & L.PCC_CONV_OUT16), flags)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.device == ctx.device and x.dim() == 5
    N, D, H, W, Cin = x.shape
    assert Cin == layer.cin, f'expected {layer.cin} input channels, got {Cin}'
    oshape = conv_out_shape(layer, x.shape)
    ocs = 0
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=ctx.device)
    else:
        assert out.is_contiguous() and tuple(out.shape[:4]) == tuple(oshape[:4])
        ocs = out.shape[4]
    if residual is not None:
        flags |= L.PCC_CONV_ADD
        assert residual.is_contiguous() and tuple(residual.shape) == tuple(oshape)
    flags |= ctx.conv_flags
    d = layer.desc(N, D, H, W, flags, impl, ocs, out_coffset)
    im = layer.device_images(ctx, d)
    L.check(L.lib().pcc_conv3d(ctx.handle, C.byref(d), _ptr(x), _ptr(im['w']), _ptr(im['pk']), _ptr(im['b']),
                               _ptr(residual), _ptr(out), ctx.stream), 'pcc_conv3d')
    return out


class NetworkWeights:
    """The weights of one whole transform (src/model_transforms.py:41-158) as ONE packed device blob per GPU
    (pcc_weights_upload): Keras-layout kernel + MFMA/Winograd fragment image + bias of every conv layer."""

    def __init__(self, transform_id, filters, conv_layers):
        self.transform, self.filters = int(transform_id), int(filters)
        n = L.lib().pcc_network_num_layers(self.transform, self.filters)
        L.check(n, 'pcc_network_num_layers')
        assert n == len(conv_layers), f'transform {transform_id}: {n} layers in the library, {len(conv_layers)} in the model'
        d, role = L.ConvDesc(), C.c_int32()
        for i, cl in enumerate(conv_layers):     # the model's layers must be the reference stack the library restates
            L.check(L.lib().pcc_network_layer(self.transform, self.filters, i, C.byref(d), C.byref(role)), 'pcc_network_layer')
            got = (cl.cin, cl.cout, cl.k, cl.stride, int(cl.transposed), cl.bias is not None, cl.relu)
            want = (d.Cin, d.Cout, d.k, d.stride, d.transposed, bool(d.flags & L.PCC_CONV_BIAS), bool(d.flags & L.PCC_CONV_RELU))
            assert got == want, f'layer {i} of transform {transform_id}: model {got} != library {want}'
        self.layers = list(conv_layers)
        self._blob = {}

    def blob(self, ctx):
        key = ctx.device.index
        if key not in self._blob:
            n = len(self.layers)
            ks = (C.c_void_p * n)(*[l.kernel.ctypes.data for l in self.layers])
            bs = (C.c_void_p * n)(*[None if l.bias is None else l.bias.ctypes.data for l in self.layers])
            dev = torch.empty((L.lib().pcc_weights_blob_floats(self.transform, self.filters),), dtype=torch.float32, device=ctx.device)
            L.check(L.lib().pcc_weights_upload(ctx.handle, self.transform, self.filters, ks, bs, _ptr(dev), ctx.stream),
                    'pcc_weights_upload')
            self._blob[key] = dev
        return self._blob[key]


_FAMILY = {0: 'analysis', 2: 'analysis', 4: 'analysis', 1: 'synthesis', 3: 'synthesis', 5: 'synthesis', 6: 'hyper_a', 7: 'hyper_s'}


def network_forward(ctx, net, x, final_flags=0):
    """y = transform(x) in ONE ABI call (pcc_network_forward_{analysis,synthesis,hyper_a,hyper_s}).  x: (N,D,H,W,Cin)."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.device == ctx.device and x.dim() == 5
    N, D, H, W, _ = x.shape
    od, oh, ow, oc = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().pcc_network_out_dims(net.transform, net.filters, D, H, W, C.byref(od), C.byref(oh), C.byref(ow), C.byref(oc)),
            'pcc_network_out_dims')
    y = torch.empty((N, od.value, oh.value, ow.value, oc.value), dtype=torch.float32, device=ctx.device)
    nb = L.lib().pcc_network_workspace_bytes(net.transform, net.filters, N, D, H, W)
    ws = ctx.workspace(nb)
    fn = getattr(L.lib(), 'pcc_network_forward_' + _FAMILY[net.transform])
    L.check(fn(ctx.handle, net.transform, net.filters, _ptr(net.blob(ctx)), _ptr(x), N, D, H, W, _ptr(y), _ptr(ws), ws.numel(),
               ctx.conv_flags, final_flags, ctx.stream), 'pcc_network_forward')
    return y


def network_plan(descs, roles, x_shape, layer_flags=0, final_flags=0, numerics=0):
    """pcc_network_plan: what every layer of a stack runs with on an input of x_shape (N,D,H,W,C) -- one L.LayerPlan per layer,
    `.desc` with its input dims and flags (the fp16 storage bits of the fp16 mode included), `.record_amax` whether it is asked for
    the block maxima of its output.  descs: L.ConvDesc per layer (geometry, own flags, impl), roles: 0 | 1 | 2 as
    pcc_network_layer gives them.  Host arithmetic: needs no context and no GPU."""
    n = len(descs)
    plan = (L.LayerPlan * n)()
    N, D, H, W = x_shape[:4]
    L.check(L.lib().pcc_network_plan((L.ConvDesc * n)(*descs), (C.c_int32 * n)(*roles), n, N, D, H, W, layer_flags, final_flags,
                                     numerics, plan, None), 'pcc_network_plan')
    return list(plan)


def profile_select(ctx, transform, layer, stride=1):
    """Live HIP-event timing of one layer of one transform inside the graph calls; stride > 1 times every stride-th call only."""
    L.check(L.lib().pcc_profile_select(ctx.handle, transform, layer | (int(stride) << 16) if transform >= 0 else layer), 'pcc_profile_select')


def profile_read(ctx, cap=8192):
    ms, n = (C.c_float * cap)(), C.c_int32()
    L.check(L.lib().pcc_profile_read(ctx.handle, ms, cap, C.byref(n)), 'pcc_profile_read')
    return [ms[i] for i in range(n.value)]


def conv3d_fp16_storage(ctx, x, layer, residual=None, in16=None, out16=True, flags=0):
    """One layer of the fp16 mode with fp16 tensors in HBM (PCC_CONV_IN16 / OUT16 / RES16, include/pcc_geo.h): x fp16 (k3
    stride-1 layers, Cin = Cout in {16, 32, 64}) or fp32 (k3 stride-2 transposed layers, out16 only).  pcc_network_forward chains
    these itself in the fp16 mode; this wrapper exists for tests and for callers that chain layers by hand."""
    in16 = (x.dtype == torch.float16) if in16 is None else in16
    assert x.is_contiguous() and x.device == ctx.device and x.dim() == 5 and x.dtype == (torch.float16 if in16 else torch.float32)
    N, D, H, W, Cin = x.shape
    assert Cin == layer.cin
    oshape = conv_out_shape(layer, x.shape)
    out = torch.empty(oshape, dtype=torch.float16 if out16 else torch.float32, device=ctx.device)
    f = flags | L.PCC_CONV_F16 | (L.PCC_CONV_IN16 if in16 else 0) | (L.PCC_CONV_OUT16 if out16 else 0)
    if residual is not None:
        assert in16 and residual.dtype == torch.float16 and residual.is_contiguous() and tuple(residual.shape) == tuple(oshape)
        f |= L.PCC_CONV_ADD | L.PCC_CONV_RES16
    d = layer.desc(N, D, H, W, f)
    im = layer.device_images(ctx, d)
    L.check(L.lib().pcc_conv3d(ctx.handle, C.byref(d), _ptr(x), _ptr(im['w']), _ptr(im['pk']), _ptr(im['b']), _ptr(residual),
                               _ptr(out), ctx.stream), 'pcc_conv3d')
    return out


def mfma_supported(layer, x_shape):
    N, D, H, W, _ = x_shape
    d = layer.desc(N, D, H, W)
    return L.lib().pcc_conv_mfma_supported(C.byref(d)) == 1
