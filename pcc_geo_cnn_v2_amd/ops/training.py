"""Training and its summaries (include/pcc_geo.h): focal loss and its gradient, ReLU backward, weight gradients and the packed-image
repack, TensorFlow-bucketed histograms and occupancy scores."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _ptr, _workspace


def focal_loss(ctx, y_true, y_pred, gamma=2.0, alpha=0.9):
    """src/utils/focal_loss.py:5-12 -> 0-d float32 tensor on the device."""
    assert y_true.numel() == y_pred.numel() and y_true.is_contiguous() and y_pred.is_contiguous()
    out = torch.empty((1,), dtype=torch.float32, device=y_pred.device)
    scratch = torch.empty((L.lib().pcc_focal_scratch_floats(),), dtype=torch.float32, device=y_pred.device)
    L.check(L.lib().pcc_focal_loss(ctx.handle, _ptr(y_true), _ptr(y_pred), y_true.numel(), gamma, alpha, _ptr(out),
                                   _ptr(scratch), ctx.stream), 'pcc_focal_loss')
    return out[0]


def focal_loss_grad(ctx, y_true, y_pred, scale=None, gamma=2.0, alpha=0.9):
    """scale * d focal_loss / d y_pred (pcc_focal_loss_grad); scale: a one-element float32 device tensor (None: 1)."""
    assert y_true.numel() == y_pred.numel() and y_true.is_contiguous() and y_pred.is_contiguous()
    assert scale is None or (scale.dtype == torch.float32 and scale.numel() == 1 and scale.device == y_pred.device)
    grad = torch.empty_like(y_pred)
    L.check(L.lib().pcc_focal_loss_grad(ctx.handle, _ptr(y_true), _ptr(y_pred), y_pred.numel(), gamma, alpha,
                                        _ptr(None if scale is None else scale.contiguous()), _ptr(grad), ctx.stream),
            'pcc_focal_loss_grad')
    return grad


def relu_backward(ctx, grad, act):
    """grad *= (act > 0), in place (pcc_relu_backward)."""
    assert grad.is_contiguous() and act.is_contiguous() and grad.numel() == act.numel() and grad.dtype == act.dtype == torch.float32
    L.check(L.lib().pcc_relu_backward(ctx.handle, _ptr(grad), _ptr(act), grad.numel(), ctx.stream), 'pcc_relu_backward')
    return grad


def dual_desc(d):
    """The descriptor whose pcc_conv3d is the input gradient of layer `d` (include/pcc_geo.h, training): forward <-> transposed,
    Cin <-> Cout, on the layer's output grid, no bias / ReLU / residual."""
    od, oh, ow = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().pcc_conv_out_dims(C.byref(d), C.byref(od), C.byref(oh), C.byref(ow)), 'pcc_conv_out_dims')
    return L.ConvDesc(d.N, od.value, oh.value, ow.value, d.Cout, d.Cin, d.k, d.stride, 1 - d.transposed, 0, L.PCC_IMPL_AUTO, 0, 0)


def conv_repack_map(d):
    """int32 gather map of the packed image of `d` (pcc_conv_repack_map), or None when the MFMA path does not cover `d`."""
    if L.lib().pcc_conv_mfma_supported(C.byref(d)) != 1:
        return None
    m = np.empty(L.lib().pcc_conv_packed_floats(C.byref(d)), np.int32)
    L.check(L.lib().pcc_conv_repack_map(C.byref(d), m.ctypes.data_as(C.c_void_p)), 'pcc_conv_repack_map')
    return m


def conv_repack_device(ctx, d, map_dev, w, pk):
    """pk <- the packed image of the device Keras kernel w (pcc_conv_repack_weights_device, gather segments only)."""
    assert map_dev.dtype == torch.int32 and w.dtype == pk.dtype == torch.float32 and w.is_contiguous() and pk.is_contiguous()
    L.check(L.lib().pcc_conv_repack_weights_device(ctx.handle, C.byref(d), _ptr(map_dev), _ptr(w), _ptr(pk), ctx.stream),
            'pcc_conv_repack_weights_device')
    return pk


def conv_wgrad_slices(d):
    """(S, longest slice chain) of pcc_conv3d_wgrad on descriptor d (pcc_conv_wgrad_slices)."""
    s, n = C.c_int32(), C.c_int64()
    L.check(L.lib().pcc_conv_wgrad_slices(C.byref(d), C.byref(s), C.byref(n)), 'pcc_conv_wgrad_slices')
    return int(s.value), int(n.value)


def conv3d_wgrad(ctx, d, x, dout, dw, db=None, workspace=None):
    """dw (Keras layout) and db of layer `d` from its input x and the gradient dout of its conv output (pcc_conv3d_wgrad)."""
    assert x.is_contiguous() and dout.is_contiguous() and dw.is_contiguous()
    nbytes = L.lib().pcc_conv_wgrad_workspace_bytes(C.byref(d))
    if workspace is None or workspace.numel() < nbytes:
        workspace = _workspace(ctx, nbytes)
    L.check(L.lib().pcc_conv3d_wgrad(ctx.handle, C.byref(d), _ptr(x), _ptr(dout), _ptr(dw), _ptr(db), _ptr(workspace),
                                     workspace.numel(), ctx.stream), 'pcc_conv3d_wgrad')
    return dw, db


def histogram_limits():
    """The 1551 bucket limits as the library computes them (pcc_histogram_limits), float64."""
    lim = np.empty(L.HISTOGRAM_BUCKETS, np.float64)
    n = L.check(L.lib().pcc_histogram_limits(lim.ctypes.data_as(C.c_void_p)), 'pcc_histogram_limits')
    assert n == L.HISTOGRAM_BUCKETS
    return lim


def _f32_flat(t, what):
    assert t.dtype == torch.float32 and t.is_cuda, f'{what}: float32 device tensor expected'
    return t.detach().contiguous().reshape(-1)


def histogram_unpack(raw):
    """One pcc_histogram (its bytes as a uint8 array) -> dict(counts uint64[1551], num, nonfinite, min, max, sum, sum_squares)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    assert raw.size == C.sizeof(L.Histogram)
    counts = raw[:8 * L.HISTOGRAM_BUCKETS].view(np.uint64).copy()
    num, nonfinite = (int(v) for v in raw[8 * L.HISTOGRAM_BUCKETS:8 * L.HISTOGRAM_BUCKETS + 16].view(np.uint64))
    mn, mx, sm, sq = (float(v) for v in raw[8 * L.HISTOGRAM_BUCKETS + 16:].view(np.float64))
    return dict(counts=counts, num=num, nonfinite=nonfinite, min=mn, max=mx, sum=sm, sum_squares=sq)


def tensor_histograms_launch(ctx, tensors):
    """pcc_tensor_histogram of every tensor on the context's stream -> (len(tensors), sizeof(pcc_histogram)) uint8 on the device (the
    calls share one workspace: they are ordered on one stream)."""
    size = C.sizeof(L.Histogram)
    out = torch.empty((len(tensors), size), dtype=torch.uint8, device=ctx.device)
    ws = _workspace(ctx, L.lib().pcc_tensor_histogram_workspace_bytes())
    keep = []
    for i, t in enumerate(tensors):
        flat = _f32_flat(t, 'tensor_histogram')
        keep.append(flat)
        L.check(L.lib().pcc_tensor_histogram(ctx.handle, _ptr(flat) if flat.numel() else None, flat.numel(),
                                             C.c_void_p(out.data_ptr() + i * size), _ptr(ws), ctx.stream), 'pcc_tensor_histogram')
    return out, keep


def tensor_histograms(ctx, tensors):
    """The histograms of several tensors after ONE device-to-host copy of their results."""
    out, _keep = tensor_histograms_launch(ctx, tensors)
    raw = out.cpu().numpy()
    return [histogram_unpack(r) for r in raw]


def tensor_histogram(ctx, t):
    """TensorFlow-bucketed histogram of a float32 device tensor (pcc_tensor_histogram): dict(counts uint64[1551], num, nonfinite,
    min, max, sum, sum_squares) on the host."""
    return tensor_histograms(ctx, [t])[0]


def occupancy_scores_launch(ctx, x, x_tilde, want_quant=False):
    """pcc_occupancy_scores on the context's stream -> (5 int64 on the device: tp, tn, fp, fn, num_occupied; quantised x_tilde or None)."""
    a, b = _f32_flat(x, 'occupancy_scores'), _f32_flat(x_tilde, 'occupancy_scores')
    assert a.numel() == b.numel(), 'occupancy_scores: x and x_tilde differ in size'
    out = torch.empty((C.sizeof(L.Occupancy) // 8,), dtype=torch.int64, device=ctx.device)
    quant = torch.empty_like(b) if want_quant else None
    L.check(L.lib().pcc_occupancy_scores(ctx.handle, _ptr(a) if a.numel() else None, _ptr(b) if b.numel() else None, a.numel(),
                                         _ptr(quant), _ptr(out), ctx.stream), 'pcc_occupancy_scores')
    return out, (None if quant is None else quant.reshape(x_tilde.shape))


def occupancy_scores(ctx, x, x_tilde, want_quant=False):
    """Confusion matrix of rint(clip(x_tilde, 0, 1)) against rint(clip(x, 0, 1)) (pcc_occupancy_scores): dict(tp, tn, fp, fn,
    num_occupied) of Python ints after one device-to-host copy; with want_quant also the quantised x_tilde (float32 device tensor of
    x_tilde's shape)."""
    out, quant = occupancy_scores_launch(ctx, x, x_tilde, want_quant)
    res = dict(zip(('tp', 'tn', 'fp', 'fn', 'num_occupied'), (int(v) for v in out.cpu().numpy().view(np.uint64))))
    return (res, quant) if want_quant else res
