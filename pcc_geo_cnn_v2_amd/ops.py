"""Thin torch-facing wrappers over the C ABI (include/pcc_geo.h).

PyTorch-ROCm is plumbing only: it owns device memory (tensors) and streams; every operator below is
a hand-written HIP kernel (or the host range coder) inside libpcc_geo_hip.so.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Context:
    """One per (process, GPU).  Replaces the tf.Session of src/compress_octree.py:84-92."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise L.PccError('no ROCm device visible to PyTorch: the MI355X path cannot run (no CPU fallback)')
        self.device = torch.device('cuda', device)
        h = C.c_void_p()
        L.check(L.lib().pcc_ctx_create(device, C.byref(h)), 'pcc_ctx_create')
        self.handle = h
        self.num_cu = L.lib().pcc_ctx_num_cu(h)
        self.numerics_at_creation = self.numerics()[1]       # the PCC_* environment switches as pcc_ctx_create read them

    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def workspace(self, nbytes):
        """Activations workspace of the batched-graph entry points: one caller-owned device buffer per context, grown on
        demand.  Calls on a context are ordered on one stream, so consecutive transforms may reuse it."""
        ws = getattr(self, '_ws', None)
        if ws is None or ws.numel() < nbytes:
            self._ws = ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=self.device)
        return ws

    conv_flags = 0      # extra pcc_conv_desc.flags of every conv issued through this context (0 = the reference's fp32)

    # ---- codec numerics (include/pcc_geo.h): which kernel family computes a layer is state of the context, read once from the PCC_*
    #      environment switches at creation; encoder and decoder must agree on it (sigma-hat selects the entropy coder's rows)
    def numerics(self):
        """(kernel family of this build, PCC_NUM_* switches in effect)."""
        fam, sw = C.c_uint32(), C.c_uint32()
        L.check(L.lib().pcc_ctx_get_numerics(self.handle, C.byref(fam), C.byref(sw)), 'pcc_ctx_get_numerics')
        return int(fam.value), int(sw.value)

    def numerics_tag(self, precision='fp32'):
        """What the CLIs record beside a stream (gzip header comment and `.enc.metric.json` key `codec_numerics`) and the decoder compares.
        Switches that are documented AND tested as bit-identical (P16, COUT1_T16: launch geometry only) are masked out: they must not
        make a decoder refuse a stream."""
        fam, sw = self.numerics()
        sw &= ~(L.PCC_NUM['p16'] | L.PCC_NUM['cout1_t16'])
        return f'pcc_geo_cnn_v2_amd/k{fam}/sw{sw:04x}/{precision}'

    def set_numerics(self, **switches):
        """Replace named switches (L.PCC_NUM keys -> bool); returns the previous word.  Tests / A/B runs only: never between an
        encode and the decode of its stream."""
        _, old = self.numerics()
        new = old
        for k, v in switches.items():
            new = (new | L.PCC_NUM[k]) if v else (new & ~L.PCC_NUM[k])
        L.check(L.lib().pcc_ctx_set_numerics(self.handle, new), 'pcc_ctx_set_numerics')
        return old

    @contextlib.contextmanager
    def numerics_override(self, **switches):
        old = self.set_numerics(**switches)
        try:
            yield self
        finally:
            L.check(L.lib().pcc_ctx_set_numerics(self.handle, old), 'pcc_ctx_set_numerics')

    def view(self, conv_flags):
        """The same context (handle, device, stream, workspace) with other default conv flags -- how a model in the fp16 mode
        (PCC_CONV_F16) uses a context without changing it for anybody else."""
        if not conv_flags:
            return self
        views = self.__dict__.setdefault('_views', {})
        if conv_flags not in views:
            views[conv_flags] = _ContextView(self, conv_flags)
        return views[conv_flags]

    def close(self):
        if self.handle is not None:
            L.lib().pcc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ContextView:
    def __init__(self, base, conv_flags):
        self._base, self.conv_flags = base, conv_flags

    def __getattr__(self, name):          # handle, device, num_cu, stream, workspace, ...
        return getattr(self._base, name)

    def view(self, conv_flags):
        return self._base.view(conv_flags)


_CONTEXTS = {}


def get_context(device=None):
    """Process-wide context cache: one pcc_ctx per GPU."""
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
    device = torch.device(device)
    if device.type != 'cuda':
        raise L.PccError(f'tensor is on {device}: the codec operators only run on the MI355X (no CPU fallback)')
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _CONTEXTS:
        _CONTEXTS[idx] = Context(idx)
    return _CONTEXTS[idx]


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


# Optional live profiling of selected conv launches with HIP events on the launch stream (bench.py):
# PROFILE = {'match': callable(layer, x_shape) -> bool, 'events': [(start, end), ...]}
PROFILE = None


def conv3d(ctx, x, layer, residual=None, flags=0, impl=L.PCC_IMPL_AUTO, out=None, out_coffset=0):
    """x: (N,D,H,W,Cin) float32 contiguous on ctx.device.  Returns (N,OD,OH,OW,Cout)."""
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
    flags |= getattr(ctx, 'conv_flags', 0)
    d = layer.desc(N, D, H, W, flags, impl, ocs, out_coffset)
    im = layer.device_images(ctx, d)
    prof = PROFILE is not None and PROFILE['match'](layer, x.shape)
    if prof:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(ctx.device))
    rc = L.lib().pcc_conv3d(ctx.handle, C.byref(d), _ptr(x), _ptr(im['w']), _ptr(im['pk']), _ptr(im['b']),
                            _ptr(residual), _ptr(out), ctx.stream)
    L.check(rc, 'pcc_conv3d')
    if prof:
        e1.record(torch.cuda.current_stream(ctx.device))
        PROFILE['events'].append((e0, e1))
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
               getattr(ctx, 'conv_flags', 0), final_flags, ctx.stream), 'pcc_network_forward')
    return y


def codec_desc(ctx, version, filters, nets, medians=None, scale_table=None, round_mode=L.PCC_ROUND_FLOOR_HALF):
    """pcc_codec_desc of a model: nets = dict(analysis=, synthesis=, hyper_analysis=, hyper_synthesis=) of NetworkWeights
    (None where absent); medians / scale_table: device tensors.  Returns (desc, keepalive)."""
    d = L.CodecDesc()
    d.version, d.filters, d.round_mode = version, filters, round_mode
    d.analysis = nets['analysis'].transform if nets.get('analysis') is not None else -1
    d.synthesis = nets['synthesis'].transform
    keep = []
    for name in ('analysis', 'synthesis', 'hyper_analysis', 'hyper_synthesis'):
        net = nets.get(name)
        blob = net.blob(ctx) if net is not None else None
        keep.append(blob)
        setattr(d, 'w_' + name, None if blob is None else blob.data_ptr())
    d.medians = None if medians is None else medians.data_ptr()
    d.scale_table = None if scale_table is None else scale_table.data_ptr()
    d.scale_levels = 0 if scale_table is None else scale_table.numel()
    keep += [medians, scale_table]
    return d, keep


def usable_cores():
    """Cores this process may use: the affinity mask capped by the cgroup CPU quota (cgroup v2 cpu.max, v1 cfs_quota_us)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            quota = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            period = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return n


_ITEM = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}


class SymbolStaging:
    """What leaves the device for the host coder after one encode of B blocks, as ONE buffer: z symbols, y symbols, CDF-row
    indexes (stream order, narrow integers) and the per-tile max|symbol| of both symbol tensors.  `dev` (device uint8) is
    filled by the library (pcc_symbol_io / pcc_symbols_pack), `host` (pinned uint8) receives it in one copy; the
    attributes zsym / ysym / idx / ztm / ytm are views of `host`.  z pieces are absent for a version-1 codec."""

    def __init__(self, device, B, stream_shape_y, stream_shape_z, F, sym_dtype, idx_dtype, channels_first):
        self.sym_dtype, self.idx_dtype, self.channels_first = sym_dtype, idx_dtype, bool(channels_first)
        vy = int(np.prod(stream_shape_y[1:])) // F
        vz = int(np.prod(stream_shape_z[1:])) // F if stream_shape_z is not None else 0
        self.vy, self.vz, self.B, self.F = vy, vz, B, F
        pieces = [('ysym', stream_shape_y, sym_dtype)]
        if stream_shape_z is not None:
            pieces += [('zsym', stream_shape_z, sym_dtype), ('idx', stream_shape_y, idx_dtype)]
        pieces.append(('ytm', (L.lib().pcc_symbols_tiles(B, vy, F),), torch.int32))
        if stream_shape_z is not None:
            pieces.append(('ztm', (L.lib().pcc_symbols_tiles(B, vz, F),), torch.int32))
        off, self.layout = 0, {}
        for name, shape, dt in pieces:
            nbytes = int(np.prod(shape)) * _ITEM[dt]
            self.layout[name] = (off, nbytes, tuple(shape), dt)
            off += (nbytes + 15) // 16 * 16
        self.nbytes = off
        self.dev = torch.empty((off,), dtype=torch.uint8, device=device)
        self.host = torch.empty((off,), dtype=torch.uint8, pin_memory=True)
        for name, (o, nb, shape, dt) in self.layout.items():
            setattr(self, name, self.host[o:o + nb].view(dt).reshape(shape))

    def dev_ptr(self, name):
        return self.dev.data_ptr() + self.layout[name][0] if name in self.layout else None

    def sink(self):
        k = L.SymbolSink()
        k.zsym, k.ysym, k.idx = self.dev_ptr('zsym'), self.dev_ptr('ysym'), self.dev_ptr('idx')
        k.zsym_tile_max, k.ysym_tile_max = self.dev_ptr('ztm'), self.dev_ptr('ytm')
        k.sym_bytes, k.idx_bytes, k.channels_first = _ITEM[self.sym_dtype], _ITEM[self.idx_dtype], int(self.channels_first)
        return k

    def pack(self, ctx, ysym, zsym=None, idx=None):
        """the same packing from Python (the per-layer path, which has no pcc_codec_encode call to do it)"""
        symbols_pack(ctx, ysym, self.channels_first, self.dev_ptr('ysym'), _ITEM[self.sym_dtype], self.dev_ptr('ytm'))
        if zsym is not None:
            symbols_pack(ctx, zsym, self.channels_first, self.dev_ptr('zsym'), _ITEM[self.sym_dtype], self.dev_ptr('ztm'))
            symbols_pack(ctx, idx, self.channels_first, self.dev_ptr('idx'), _ITEM[self.idx_dtype], None)

    def copy_out(self):
        """device -> pinned host on the current stream (one copy)"""
        self.host.copy_(self.dev, non_blocking=True)


def symbols_pack(ctx, src, channels_first, dst_ptr, dst_bytes, tile_max_ptr=None):
    """(N, ..., C) int32 device tensor -> stream order, dst_bytes-wide integers at the device address dst_ptr."""
    assert src.dtype == torch.int32 and src.is_contiguous() and src.device == ctx.device
    N, Cc = src.shape[0], src.shape[-1]
    L.check(L.lib().pcc_symbols_pack(ctx.handle, _ptr(src), N, src[0].numel() // Cc, Cc, int(bool(channels_first)),
                                     C.c_void_p(dst_ptr), dst_bytes, None if tile_max_ptr is None else C.c_void_p(tile_max_ptr),
                                     ctx.stream), 'pcc_symbols_pack')


def symbols_unpack(ctx, src, ndhwc_shape, channels_first):
    """stream-order device tensor (uint8 / int16 / int32) of N blocks -> (N,D,H,W,C) int32 device tensor."""
    assert src.is_contiguous() and src.device == ctx.device and src.dtype in _ITEM
    out = torch.empty(tuple(ndhwc_shape), dtype=torch.int32, device=ctx.device)
    N, Cc = out.shape[0], out.shape[-1]
    assert src.numel() == out.numel()
    L.check(L.lib().pcc_symbols_unpack(ctx.handle, _ptr(src), _ITEM[src.dtype], N, out[0].numel() // Cc, Cc,
                                       int(bool(channels_first)), _ptr(out), ctx.stream), 'pcc_symbols_unpack')
    return out


def _out(t, shape, dtype, ref):
    """a caller-supplied output tensor (tests pass views into guarded buffers) or a fresh one"""
    if t is None:
        return torch.empty(tuple(shape), dtype=dtype, device=ref.device)
    assert t.dtype == dtype and t.is_contiguous() and t.device == ref.device and tuple(t.shape) == tuple(shape)
    return t


def quantize_pack(ctx, v, medians, mode, channels_first, dst_ptr, dst_bytes, tile_max_ptr=None, want_deq=True, sym=None, deq=None):
    """The quantiser fused with symbols_pack, as the encoder graph launches it (pcc_quantize_pack): (N, ..., C) float32 ->
    (sym int32, deq float32 or None) like quantize(), and sym in stream order as dst_bytes-wide integers at dst_ptr."""
    assert v.dtype == torch.float32 and v.is_contiguous() and v.device == ctx.device
    N, Cc = v.shape[0], v.shape[-1]
    sym = _out(sym, v.shape, torch.int32, v)
    deq = _out(deq, v.shape, torch.float32, v) if want_deq else None
    L.check(L.lib().pcc_quantize_pack(ctx.handle, _ptr(v), _ptr(medians), _ptr(sym), _ptr(deq), N, v[0].numel() // Cc, Cc, mode,
                                      int(bool(channels_first)), C.c_void_p(dst_ptr), dst_bytes,
                                      None if tile_max_ptr is None else C.c_void_p(tile_max_ptr), ctx.stream), 'pcc_quantize_pack')
    return sym, deq


def index_pack(ctx, sigma, table, channels_first, dst_ptr, dst_bytes, idx=None):
    """scale_to_index fused with symbols_pack (pcc_index_pack): (N, ..., C) float32 sigma -> idx int32 of the same shape, and idx
    in stream order as dst_bytes-wide integers at dst_ptr."""
    assert sigma.dtype == torch.float32 and sigma.is_contiguous() and sigma.device == ctx.device and table.dtype == torch.float32
    N, Cc = sigma.shape[0], sigma.shape[-1]
    idx = _out(idx, sigma.shape, torch.int32, sigma)
    L.check(L.lib().pcc_index_pack(ctx.handle, _ptr(sigma), _ptr(table), table.numel(), _ptr(idx), N, sigma[0].numel() // Cc, Cc,
                                   int(bool(channels_first)), C.c_void_p(dst_ptr), dst_bytes, ctx.stream), 'pcc_index_pack')
    return idx


def unpack_dequantize(ctx, src, ndhwc_shape, channels_first, medians=None, sym=None, deq=None):
    """symbols_unpack fused with dequantize, as the decoder graphs launch it (pcc_unpack_dequantize): stream-order device tensor
    (uint8 / int16 / int32) of N blocks -> (sym int32, deq float32), both (N,D,H,W,C)."""
    assert src.is_contiguous() and src.device == ctx.device and src.dtype in _ITEM
    sym = _out(sym, ndhwc_shape, torch.int32, src)
    deq = _out(deq, ndhwc_shape, torch.float32, src)
    N, Cc = sym.shape[0], sym.shape[-1]
    assert src.numel() == sym.numel()
    L.check(L.lib().pcc_unpack_dequantize(ctx.handle, _ptr(src), _ITEM[src.dtype], N, sym[0].numel() // Cc, Cc,
                                          int(bool(channels_first)), _ptr(sym), _ptr(medians), _ptr(deq), ctx.stream),
            'pcc_unpack_dequantize')
    return sym, deq


def codec_encode(ctx, desc, x, thr=None, cap=None, symbols_ready=None, staging=None, scratch=None):
    """The GPU part of compress() (src/model_types.py:289-293 / :379-388) for a batch of blocks in ONE ABI call.
    x: (N,D,H,W) float32.  Returns dict of device tensors (NDHWC); with `thr` (N,) float32 also the encoder-side point
    lists xyz / counts of the clipped x_hat (fixed-threshold policy).  symbols_ready: a torch.cuda.Event that has been
    recorded once (so that its handle exists); the library re-records it when the symbols are final.  staging: a
    SymbolStaging whose device buffer the library fills (stream order, narrow integers) before that event."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.device == ctx.device
    N, D, H, W = x.shape
    F, dev = desc.filters, ctx.device
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)
    ys, zs = (N, D // 8, H // 8, W // 8, F), (N, D // 16, H // 16, W // 16, F)
    t = dict(y=f32(*ys), symbols=i32(*ys), y_hat=f32(*ys), x_hat=f32(N, D, H, W))
    if desc.version == 2:
        t.update(z=f32(*zs), z_symbols=i32(*zs), z_hat=f32(*zs), sigma_hat=f32(*ys), indexes=i32(*ys))
    xyz = counts = None
    cap = D * H * W if cap is None else int(cap)
    if thr is not None:
        assert thr.dtype == torch.float32 and thr.numel() == N
        xyz, counts = torch.empty((N, cap, 3), dtype=torch.float32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
        n_scratch = L.lib().pcc_threshold_scratch_ints(N, D, H, W)
        if scratch is None:
            scratch = torch.empty((n_scratch,), dtype=torch.int32, device=dev)
        assert scratch.dtype == torch.int32 and scratch.numel() >= n_scratch and scratch.device == dev
        t.update(xyz=xyz, counts=counts)
    ws = ctx.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), N, D, H, W))
    L.check(L.lib().pcc_codec_encode(ctx.handle, C.byref(desc), _ptr(x), N, D, H, W, _ptr(t['y']), _ptr(t.get('z')),
                                     _ptr(t.get('z_symbols')), _ptr(t.get('z_hat')), _ptr(t.get('sigma_hat')),
                                     _ptr(t.get('indexes')), _ptr(t['symbols']), _ptr(t['y_hat']), _ptr(t['x_hat']), _ptr(thr),
                                     _ptr(xyz), _ptr(counts), cap, _ptr(scratch), _ptr(ws), ws.numel(),
                                     getattr(ctx, 'conv_flags', 0), 0, None if staging is None else C.byref(staging.sink()),
                                     None if symbols_ready is None else C.c_void_p(symbols_ready.cuda_event), ctx.stream),
            'pcc_codec_encode')
    return t


def _packed_io(packed, channels_first, idx_out=None):
    """pcc_symbol_io for the decoder calls: `packed` = stream-order symbols on the device (int16 / int32) as the host->device
    copy delivered them, idx_out = device tensor (uint8 / int32) that receives the packed CDF-row indexes."""
    k = L.SymbolSink()
    k.sym_bytes = _ITEM[packed.dtype]
    k.idx_bytes = 1 if idx_out is None else _ITEM[idx_out.dtype]
    k.channels_first = int(bool(channels_first))
    k.idx = None if idx_out is None else idx_out.data_ptr()
    return k


def codec_decode_hyper(ctx, desc, zsym, dhw, packed=None, channels_first=True, idx_packed=None):
    """z symbols (N,D/16,H/16,W/16,F) int32 -> z_hat, sigma_hat, indexes (src/model_types.py:403-406), one ABI call.
    packed: instead of zsym, the stream-order symbols (N, ...) int16 / int32 on the device -- the library unpacks them (the
    int32 tensor comes back as 'z_symbols'); idx_packed: device tensor (uint8 / int32, stream order) that receives the indexes."""
    (D, H, W), F, dev = dhw, desc.filters, ctx.device
    N = (zsym if packed is None else packed).shape[0]
    zs, ys = (N, D // 16, H // 16, W // 16, F), (N, D // 8, H // 8, W // 8, F)
    io = None
    if packed is not None or idx_packed is not None:
        src = packed if packed is not None else torch.empty((0,), dtype=torch.int16)
        io = _packed_io(src, channels_first, idx_packed)
        if packed is not None:
            assert packed.is_contiguous() and packed.device == dev and packed.numel() == int(np.prod(zs))
            io.zsym = packed.data_ptr()
            zsym = torch.empty(zs, dtype=torch.int32, device=dev)
        assert idx_packed is None or (idx_packed.is_contiguous() and idx_packed.numel() == int(np.prod(ys)))
    assert zsym.dtype == torch.int32 and zsym.is_contiguous() and tuple(zsym.shape) == zs
    t = dict(z_hat=torch.empty(zs, dtype=torch.float32, device=dev), sigma_hat=torch.empty(ys, dtype=torch.float32, device=dev),
             indexes=torch.empty(ys, dtype=torch.int32, device=dev), z_symbols=zsym)
    ws = ctx.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), N, D, H, W))
    L.check(L.lib().pcc_codec_decode_hyper(ctx.handle, C.byref(desc), _ptr(zsym), N, D, H, W, _ptr(t['z_hat']), _ptr(t['sigma_hat']),
                                           _ptr(t['indexes']), _ptr(ws), ws.numel(), getattr(ctx, 'conv_flags', 0),
                                           None if io is None else C.byref(io), ctx.stream),
            'pcc_codec_decode_hyper')
    return t


def codec_decode_main(ctx, desc, ysym, dhw, thr=None, cap=None, packed=None, channels_first=True, scratch=None):
    """y symbols -> y_hat -> x_hat (+ thresholding and compaction when `thr` (N,) float32 is given), one ABI call
    (src/model_types.py:305-307 / :407-408, :232-234).  packed: instead of ysym, the stream-order symbols on the device (see
    codec_decode_hyper); the int32 tensor comes back as 'symbols'."""
    (D, H, W), F, dev = dhw, desc.filters, ctx.device
    N = (ysym if packed is None else packed).shape[0]
    ys = (N, D // 8, H // 8, W // 8, F)
    io = None
    if packed is not None:
        assert packed.is_contiguous() and packed.device == dev and packed.numel() == int(np.prod(ys))
        io = _packed_io(packed, channels_first)
        io.ysym = packed.data_ptr()
        ysym = torch.empty(ys, dtype=torch.int32, device=dev)
    assert ysym.dtype == torch.int32 and ysym.is_contiguous() and tuple(ysym.shape) == ys
    t = dict(y_hat=torch.empty(ys, dtype=torch.float32, device=dev), x_hat=torch.empty((N, D, H, W), dtype=torch.float32, device=dev),
             symbols=ysym)
    xyz = counts = None
    cap = D * H * W if cap is None else int(cap)
    if thr is not None:
        assert thr.dtype == torch.float32 and thr.numel() == N
        xyz = torch.empty((N, cap, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        n_scratch = L.lib().pcc_threshold_scratch_ints(N, D, H, W)
        if scratch is None:
            scratch = torch.empty((n_scratch,), dtype=torch.int32, device=dev)
        assert scratch.dtype == torch.int32 and scratch.numel() >= n_scratch and scratch.device == dev
        t.update(xyz=xyz, counts=counts)
    ws = ctx.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), N, D, H, W))
    L.check(L.lib().pcc_codec_decode_main(ctx.handle, C.byref(desc), _ptr(ysym), N, D, H, W, _ptr(t['y_hat']), _ptr(t['x_hat']),
                                          _ptr(thr), _ptr(xyz), _ptr(counts), cap, _ptr(scratch), _ptr(ws), ws.numel(),
                                          getattr(ctx, 'conv_flags', 0), None if io is None else C.byref(io), ctx.stream),
            'pcc_codec_decode_main')
    return t


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


def quantize(ctx, v, medians=None, mode=L.PCC_ROUND_FLOOR_HALF, want_sym=True, want_deq=True, channels=None):
    """channels: the channel count when it is not v's last dimension (the channel of element i is i % channels)."""
    assert v.dtype == torch.float32 and v.is_contiguous()
    Cn = v.shape[-1] if channels is None else int(channels)
    sym = torch.empty(v.shape, dtype=torch.int32, device=v.device) if want_sym else None
    deq = torch.empty_like(v) if want_deq else None
    L.check(L.lib().pcc_quantize(ctx.handle, _ptr(v), _ptr(medians), _ptr(sym), _ptr(deq), v.numel(), Cn, mode,
                                 ctx.stream), 'pcc_quantize')
    return sym, deq


def dequantize(ctx, sym, medians=None, channels=None):
    assert sym.dtype == torch.int32 and sym.is_contiguous()
    deq = torch.empty(sym.shape, dtype=torch.float32, device=sym.device)
    L.check(L.lib().pcc_dequantize(ctx.handle, _ptr(sym), _ptr(medians), _ptr(deq), sym.numel(),
                                   sym.shape[-1] if channels is None else int(channels), ctx.stream), 'pcc_dequantize')
    return deq


def scale_to_index(ctx, sigma, table):
    assert sigma.dtype == torch.float32 and sigma.is_contiguous() and table.dtype == torch.float32
    idx = torch.empty(sigma.shape, dtype=torch.int32, device=sigma.device)
    L.check(L.lib().pcc_scale_to_index(ctx.handle, _ptr(sigma), _ptr(table), table.numel(), _ptr(idx), sigma.numel(),
                                       ctx.stream), 'pcc_scale_to_index')
    return idx


def threshold_compact(ctx, x, thr, clip=False, cap=None):
    """x: (B,D,H,W) float32; thr: (B,) float32 device tensor.  Returns (xyz (B,cap,3), counts (B,))."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    B, D, H, W = x.shape
    cap = D * H * W if cap is None else int(cap)
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device=x.device)
    counts = torch.empty((B,), dtype=torch.int32, device=x.device)
    scratch = torch.empty((L.lib().pcc_threshold_scratch_ints(B, D, H, W),), dtype=torch.int32, device=x.device)
    L.check(L.lib().pcc_threshold_compact(ctx.handle, _ptr(x), B, D, H, W, _ptr(thr), int(clip), _ptr(xyz),
                                          _ptr(counts), cap, _ptr(scratch), ctx.stream), 'pcc_threshold_compact')
    return xyz, counts


def voxelize(ctx, pts, block_of, B, D, H, W):
    """pts (n,3) int32, block_of (n,) int32 (device) -> dense (B,D,H,W) float32 of {0,1}."""
    dense = torch.zeros((B, D, H, W), dtype=torch.float32, device=ctx.device)
    if pts.numel():
        assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32
        L.check(L.lib().pcc_voxelize(ctx.handle, _ptr(pts), _ptr(block_of), pts.shape[0], B, D, H, W, _ptr(dense),
                                     ctx.stream), 'pcc_voxelize')
    return dense


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
        workspace = torch.empty((int(nbytes),), dtype=torch.uint8, device=x.device)
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
    ws = torch.empty((int(L.lib().pcc_tensor_histogram_workspace_bytes()),), dtype=torch.uint8, device=ctx.device)
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


def d1_threshold_stats(ctx, x_hat, thr, pts, block_of, clip=True):
    """Exact D1 sums for every threshold of every block (see include/pcc_geo.h).  x_hat (B,D,H,W) float32,
    thr (T<=256,) float32, pts (n,3) int32 grouped by block, block_of (n,) int32 -- all on the device.
    Returns int64 numpy arrays s_ab (B,256), s_ba (B,256), n_b (B,256) indexed by threshold, and tcount (B,)."""
    assert x_hat.dtype == torch.float32 and x_hat.is_contiguous() and x_hat.dim() == 4
    assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32 and block_of.is_contiguous()
    assert thr.dtype == torch.float32 and thr.is_contiguous()
    B, D, H, W = x_hat.shape
    ws = torch.empty((L.lib().pcc_d1_search_workspace_bytes(B, D, H, W),), dtype=torch.uint8, device=x_hat.device)
    s_ab = torch.empty((B, 256), dtype=torch.int64, device=x_hat.device)
    hsum, hcnt = torch.empty_like(s_ab), torch.empty_like(s_ab)
    tcount = torch.empty((B,), dtype=torch.int32, device=x_hat.device)
    L.check(L.lib().pcc_d1_threshold_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip),
                                           _ptr(pts), _ptr(block_of), pts.shape[0], _ptr(ws), _ptr(s_ab), _ptr(hsum),
                                           _ptr(hcnt), _ptr(tcount), ctx.stream), 'pcc_d1_threshold_stats')
    hs, hc = hsum.cpu().numpy(), hcnt.cpu().numpy()
    # suffix sums over levels k > t
    s_ba = np.concatenate([np.cumsum(hs[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    n_b = np.concatenate([np.cumsum(hc[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    return s_ab.cpu().numpy(), s_ba, n_b, tcount.cpu().numpy()


def d12_threshold_stats(ctx, x_hat, thr, pts, block_of, block_start, normals, clip=True):
    """d1_threshold_stats plus the D2 sums of every threshold (include/pcc_geo.h: pcc_d12_threshold_stats).  normals (n,3) float32,
    block_start (B+1,) int32 -- on the device.  Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba); d2_* float64 (B,256)."""
    assert x_hat.dtype == torch.float32 and x_hat.is_contiguous() and x_hat.dim() == 4
    assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32 and block_of.is_contiguous()
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.shape == pts.shape
    assert block_start.dtype == torch.int32 and block_start.is_contiguous() and thr.dtype == torch.float32 and thr.is_contiguous()
    B, D, H, W = x_hat.shape
    assert block_start.numel() == B + 1
    dev = x_hat.device
    ws = torch.empty((L.lib().pcc_d1_search_workspace_bytes(B, D, H, W),), dtype=torch.uint8, device=dev)
    ws2 = torch.empty((L.lib().pcc_d12_search_workspace_bytes(B, D, H, W, pts.shape[0]),), dtype=torch.uint8, device=dev)
    s_ab = torch.empty((B, 256), dtype=torch.int64, device=dev)
    hsum, hcnt = torch.empty_like(s_ab), torch.empty_like(s_ab)
    d2_ab = torch.empty((B, 256), dtype=torch.float64, device=dev)
    d2_ba = torch.empty_like(d2_ab)
    tcount = torch.empty((B,), dtype=torch.int32, device=dev)
    L.check(L.lib().pcc_d12_threshold_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts), _ptr(block_of),
                                            _ptr(block_start), pts.shape[0], _ptr(normals), _ptr(ws), _ptr(ws2), _ptr(s_ab), _ptr(hsum), _ptr(hcnt),
                                            _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba), ctx.stream), 'pcc_d12_threshold_stats')
    hs, hc = hsum.cpu().numpy(), hcnt.cpu().numpy()
    s_ba = np.concatenate([np.cumsum(hs[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    n_b = np.concatenate([np.cumsum(hc[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    return s_ab.cpu().numpy(), s_ba, n_b, tcount.cpu().numpy(), d2_ab.cpu().numpy(), d2_ba.cpu().numpy()


class SearchTiePairOverflow(L.PccError):
    """d12_threshold_stats_ties met more equidistant pairs in one chunk of thresholds than the stated capacity; `.pairs` suffices."""

    def __init__(self, pairs, max_pairs):
        super().__init__(f'd12_threshold_stats_ties: a chunk of thresholds needs {pairs} tie pairs, the workspace holds {max_pairs}; '
                         f'pass max_pairs >= {pairs}')
        self.pairs, self.max_pairs = int(pairs), int(max_pairs)


def search_tie_pair_capacity(B, D, H, W, npts):
    """Default pair capacity of d12_threshold_stats_ties (workspace rule): room for four equidistant voxels per row
    and threshold on average over one chunk of thresholds, 4 npts chunk + 1024, capped at the engine's limit of 2^31 - 1 pairs."""
    return min(4 * int(npts) * int(L.lib().pcc_d12_search_ties_chunk(B, D, H, W)) + 1024, (1 << 31) - 1)


def d12_threshold_stats_ties_launch(ctx, x_hat, thr, pts, block_of, block_start, normals64, clip=True, max_pairs=None):
    """d12_threshold_stats_ties without the host copies: the device tensors (s_ab, hsum, hcnt, tcount, d2_ab, d2_ba, status)."""
    assert x_hat.dtype == torch.float32 and x_hat.is_contiguous() and x_hat.dim() == 4
    assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32 and block_of.is_contiguous()
    assert pts.dim() == 2 and pts.shape[1] == 3 and pts.shape[0] > 0 and block_of.numel() == pts.shape[0]
    assert normals64.dtype == torch.float64 and normals64.is_contiguous() and normals64.shape == pts.shape, \
        'd12_threshold_stats_ties: normals must be (n,3) float64'
    assert block_start.dtype == torch.int32 and block_start.is_contiguous() and thr.dtype == torch.float32 and thr.is_contiguous()
    B, D, H, W = x_hat.shape
    assert block_start.numel() == B + 1
    lo, hi = pts.min(0).values.cpu(), pts.max(0).values.cpu()
    assert int(lo.min()) >= 0 and bool((hi < torch.tensor([D, H, W])).all()), f'block-local coordinates outside the {(D, H, W)} grid'
    n = pts.shape[0]
    max_pairs = search_tie_pair_capacity(B, D, H, W, n) if max_pairs is None else int(max_pairs)
    if not 1 <= max_pairs <= (1 << 31) - 1:
        raise L.PccError(f'd12_threshold_stats_ties: max_pairs = {max_pairs} outside [1, 2^31)')
    dev = x_hat.device
    ws = torch.empty((L.lib().pcc_d1_search_workspace_bytes(B, D, H, W),), dtype=torch.uint8, device=dev)
    ws2 = torch.empty((L.lib().pcc_d12_search_ties_workspace_bytes(B, D, H, W, n, max_pairs),), dtype=torch.uint8, device=dev)
    s_ab = torch.empty((B, 256), dtype=torch.int64, device=dev)
    hsum, hcnt = torch.empty_like(s_ab), torch.empty_like(s_ab)
    d2_ab = torch.empty((B, 256), dtype=torch.float64, device=dev)
    d2_ba = torch.empty_like(d2_ab)
    tcount = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    L.check(L.lib().pcc_d12_threshold_stats_ties(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts), _ptr(block_of),
                                                 _ptr(block_start), n, _ptr(normals64), max_pairs, _ptr(status), _ptr(ws), _ptr(ws2), _ptr(s_ab),
                                                 _ptr(hsum), _ptr(hcnt), _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba), ctx.stream),
            'pcc_d12_threshold_stats_ties')
    return s_ab, hsum, hcnt, tcount, d2_ab, d2_ba, status


def d12_threshold_stats_ties(ctx, x_hat, thr, pts, block_of, block_start, normals64, clip=True, max_pairs=None, return_status=False):
    """d12_threshold_stats under the tie-averaged D2 definition (include/pcc_geo.h: pcc_d12_threshold_stats_ties): D2 of every
    (block, threshold) averages over ALL equidistant nearest points, so it equals the host restatement
    (model_opt.host_threshold_stats(ties='mean')) up to float64 rounding.  normals64 (n,3) float64 -- on the device like the rest.
    The pair list of a chunk of thresholds holds max_pairs pairs (default search_tie_pair_capacity): with the default, a call that
    needs more runs once more with the number the first run reported; an explicit max_pairs that is too small raises
    SearchTiePairOverflow -- or, with return_status=True, returns what the engine wrote (D2 all NaN, D1 valid) with the status.
    Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba) and, with return_status=True, (pairs needed, overflowed) appended."""
    args = (ctx, x_hat, thr, pts, block_of, block_start, normals64, clip)
    out = d12_threshold_stats_ties_launch(*args, max_pairs=max_pairs)
    pairs, over = (int(v) for v in out[-1].cpu())
    if over and not return_status:
        if max_pairs is not None or pairs > (1 << 31) - 1:
            B, D, H, W = x_hat.shape
            raise SearchTiePairOverflow(pairs, search_tie_pair_capacity(B, D, H, W, pts.shape[0]) if max_pairs is None else max_pairs)
        out = d12_threshold_stats_ties_launch(*args, max_pairs=pairs)
        pairs, over = (int(v) for v in out[-1].cpu())
        assert not over, 'd12_threshold_stats_ties: the reported pair capacity did not suffice'
    s_ab, hsum, hcnt, tcount, d2_ab, d2_ba, _ = out
    B = x_hat.shape[0]
    hs, hc = hsum.cpu().numpy(), hcnt.cpu().numpy()
    s_ba = np.concatenate([np.cumsum(hs[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    n_b = np.concatenate([np.cumsum(hc[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((B, 1), np.int64)], 1)
    res = (s_ab.cpu().numpy(), s_ba, n_b, tcount.cpu().numpy(), d2_ab.cpu().numpy(), d2_ba.cpu().numpy())
    return res + ((pairs, bool(over)),) if return_status else res


NORMALS_COORD_LIMIT = 1 << 21        # include/pcc_geo.h "point normals": coordinates are integers in [0, 2^21)


def _voxel_points(points, what='estimate_normals'):
    """The input contract of estimate_normals and the cloud metrics (`what` names the caller in the messages), checked before anything reaches the GPU: an (N,3) cloud of integer coordinates in
    [0, 2^21), 1 <= N < 2^31.  Returns an int32 array (numpy input) or an int32 contiguous device tensor (torch input)."""
    if isinstance(points, torch.Tensor):
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise L.PccError(f'{what}: points must be (N, 3) with N >= 1, got {tuple(points.shape)}')
        if points.is_floating_point():
            if not bool(torch.isfinite(points).all()) or not bool((points == torch.round(points)).all()):
                raise L.PccError(f'{what}: coordinates must be integers (voxelised cloud); got non-integer values')
        elif points.dtype == torch.bool or points.is_complex():
            raise L.PccError(f'{what}: unsupported dtype {points.dtype}')
        if bool((points < 0).any()) or bool((points >= NORMALS_COORD_LIMIT).any()):
            raise L.PccError(f'{what}: coordinates must lie in [0, {NORMALS_COORD_LIMIT})')
        return points.to(torch.int32).contiguous()
    a = np.asarray(points)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise L.PccError(f'{what}: points must be (N, 3) with N >= 1, got {a.shape}')
    if a.shape[0] >= 1 << 31:
        raise L.PccError(f'{what}: at most 2^31 - 1 points per call')
    if a.dtype.kind == 'f':
        if not np.isfinite(a).all() or not np.array_equal(a, np.round(a)):
            raise L.PccError(f'{what}: coordinates must be integers (voxelised cloud); got non-integer values')
    elif a.dtype.kind not in 'iu':
        raise L.PccError(f'{what}: unsupported dtype {a.dtype}')
    if (a < 0).any() or (a >= NORMALS_COORD_LIMIT).any():
        raise L.PccError(f'{what}: coordinates must lie in [0, {NORMALS_COORD_LIMIT})')
    return np.ascontiguousarray(a, dtype=np.int32)


def estimate_normals(ctx, points, k=16, viewpoint=None, return_knn=False):
    """Point normals of a voxelised cloud (include/pcc_geo.h "point normals"): (N,3) float32 numpy array, oriented away from
    `viewpoint` (3 numbers) or, by default, from the cloud's centroid.  points: (N,3) numpy array or device tensor of integer
    coordinates in [0, 2^21).  return_knn=True also returns the (N, min(k, N)) int32 neighbour rows (nearest first, ties by
    row index).  Deterministic: the same cloud gives the same bits on every call."""
    k = int(k)
    if not 3 <= k <= 64:
        raise L.PccError(f'estimate_normals: k = {k} outside [3, 64]')
    vp = None
    if viewpoint is not None:
        vp = np.asarray(viewpoint, np.float64).reshape(-1)
        if vp.shape != (3,) or not np.isfinite(vp).all():
            raise L.PccError(f'estimate_normals: viewpoint must be 3 finite numbers, got {viewpoint!r}')
    pts_d = _device_points(ctx, points, 'estimate_normals')
    dev = ctx.device
    n = pts_d.shape[0]
    vp_d = None if vp is None else torch.from_numpy(vp).to(dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    knn = torch.empty((n, k), dtype=torch.int32, device=dev) if return_knn else None
    ws = torch.empty((L.lib().pcc_normals_workspace_bytes(n, k),), dtype=torch.uint8, device=dev)
    L.check(L.lib().pcc_estimate_normals(ctx.handle, _ptr(pts_d), n, k, _ptr(vp_d), _ptr(normals), _ptr(knn), _ptr(ws), ctx.stream),
            'pcc_estimate_normals')
    out = normals.cpu().numpy()
    if return_knn:
        return out, knn[:, :min(k, n)].cpu().numpy()
    return out


CLOUD_TALLY_SLOTS = 9      # include/pcc_geo.h "cloud metrics": N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA


def _device_points(ctx, points, what):
    pts = _voxel_points(points, what)
    return pts.to(ctx.device) if isinstance(pts, torch.Tensor) else torch.from_numpy(pts).to(ctx.device)


class CloudIndex:
    """Nearest-neighbour index over a voxelised cloud on the GPU (include/pcc_geo.h "cloud metrics"): Morton-sorted cells, exact
    integer distances, ties to the lowest row.  points: (N,3) numpy array or device tensor of integer coordinates in [0, 2^21),
    1 <= N < 2^31.  Built once, reusable by any number of cloud_nearest / cloud_distortion calls on the same context."""

    def __init__(self, ctx, points):
        pts = _device_points(ctx, points, 'CloudIndex')
        self.n = int(pts.shape[0])
        self.device = ctx.device
        self.buffer = torch.empty((L.lib().pcc_cloud_index_bytes(self.n),), dtype=torch.uint8, device=ctx.device)
        L.check(L.lib().pcc_cloud_index_build(ctx.handle, _ptr(pts), self.n, _ptr(self.buffer), ctx.stream), 'pcc_cloud_index_build')

    def __len__(self):
        return self.n


def cloud_nearest(ctx, index, queries):
    """For every query point, the row of its nearest point in `index` (ties: the lowest row) and the exact squared distance:
    (int32[nq], int64[nq]) numpy arrays.  queries: (nq,3) integer coordinates in [0, 2^21); nq = 0 gives empty arrays."""
    if len(queries) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    q = _device_points(ctx, queries, 'cloud_nearest')
    nq = int(q.shape[0])
    nn = torch.empty((nq,), dtype=torch.int32, device=ctx.device)
    sq = torch.empty((nq,), dtype=torch.int64, device=ctx.device)
    L.check(L.lib().pcc_cloud_nearest(ctx.handle, _ptr(index.buffer), index.n, _ptr(q), nq, _ptr(nn), _ptr(sq), ctx.stream),
            'pcc_cloud_nearest')
    return nn.cpu().numpy(), sq.cpu().numpy()


def _normals64(a_normals, n):
    """Host-side check of the normals of cloud_distortion; returns them as float64 (numpy) or as a float64 tensor."""
    if a_normals is None:
        return None
    if isinstance(a_normals, torch.Tensor):
        if not a_normals.is_floating_point():
            raise L.PccError(f'cloud_distortion: normals must be floating point, got {a_normals.dtype}')
        nrm = a_normals.to(torch.float64)
    else:
        nrm = np.asarray(a_normals)
        if nrm.dtype.kind != 'f':
            raise L.PccError(f'cloud_distortion: normals must be floating point, got {nrm.dtype}')
        nrm = np.ascontiguousarray(nrm, np.float64)
    if tuple(nrm.shape) != (n, 3):
        raise L.PccError(f'cloud_distortion: normals must be ({n}, 3), got {tuple(nrm.shape)}')
    return nrm


TIE_MODES = {'pick': 0, 'mean': 1}      # include/pcc_geo.h PCC_TIES_*: which of several equidistant nearest points D2 reads
_PAIR_LIMIT = (1 << 31) - 1


def tie_pair_capacity(n_a):
    """Default pair capacity of ties='mean' (DESIGN.md "Tie-averaged D2", workspace rule): room for four equidistant decoded points
    per original point on average, 4 N_A + 1024, capped at the engine's limit of 2^31 - 1 pairs."""
    return min(4 * int(n_a) + 1024, _PAIR_LIMIT)


def _tie_mode(ties):
    if ties not in TIE_MODES:
        raise L.PccError(f'cloud_distortion: ties must be one of {tuple(TIE_MODES)}, got {ties!r}')
    return TIE_MODES[ties]


def cloud_distortion_launch(ctx, index_a, b, a_normals=None, links=False, ties='pick', max_pairs=None):
    """cloud_distortion without the host copy: returns the float64[9] device tally (and the int32 to_b, to_a device tensors with
    links=True), queued on the context's stream.  b: (N_B,3) decoded points, N_B >= 1; a_normals: (N_A,3) or None.  ties='mean'
    (pcc_cloud_distortion_ties) appends the int64[2] device status (pairs needed, 1 = more than max_pairs: the D2 / H2 slots are
    then NaN) to what is returned; max_pairs defaults to tie_pair_capacity(N_A)."""
    mode = _tie_mode(ties)
    b = _voxel_points(b, 'cloud_distortion')
    nrm = _normals64(a_normals, index_a.n)
    dev = ctx.device
    if nrm is not None:
        nrm = (nrm.to(dev) if isinstance(nrm, torch.Tensor) else torch.from_numpy(nrm).to(dev)).contiguous()
    if mode:
        max_pairs = tie_pair_capacity(index_a.n) if max_pairs is None else int(max_pairs)
        if not 1 <= max_pairs <= _PAIR_LIMIT:
            raise L.PccError(f'cloud_distortion: max_pairs = {max_pairs} outside [1, 2^31)')
    index_b = CloudIndex(ctx, b)
    tally = torch.empty((CLOUD_TALLY_SLOTS,), dtype=torch.float64, device=dev)
    to_b = torch.empty((index_a.n,), dtype=torch.int32, device=dev) if links else None
    to_a = torch.empty((index_b.n,), dtype=torch.int32, device=dev) if links else None
    if not mode:
        ws = torch.empty((L.lib().pcc_cloud_distortion_workspace_bytes(index_a.n, index_b.n),), dtype=torch.uint8, device=dev)
        L.check(L.lib().pcc_cloud_distortion(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(index_b.buffer), index_b.n, _ptr(nrm),
                                             _ptr(tally), _ptr(to_b), _ptr(to_a), _ptr(ws), ctx.stream), 'pcc_cloud_distortion')
        return (tally, to_b, to_a) if links else tally
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((L.lib().pcc_cloud_distortion_ties_workspace_bytes(index_a.n, index_b.n, mode, max_pairs),), dtype=torch.uint8,
                     device=dev)
    L.check(L.lib().pcc_cloud_distortion_ties(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(index_b.buffer), index_b.n, _ptr(nrm), mode,
                                              max_pairs, _ptr(tally), _ptr(status), _ptr(to_b), _ptr(to_a), _ptr(ws), ctx.stream),
            'pcc_cloud_distortion_ties')
    return (tally, to_b, to_a, status) if links else (tally, status)


class TiePairOverflow(L.PccError):
    """ties='mean' met more equidistant pairs than the stated capacity; `.pairs` is the capacity that suffices."""

    def __init__(self, pairs, max_pairs):
        super().__init__(f'cloud_distortion: ties=\'mean\' needs {pairs} tie pairs, the workspace holds {max_pairs}; '
                         f'pass max_pairs >= {pairs}')
        self.pairs, self.max_pairs = int(pairs), int(max_pairs)


def cloud_distortion(ctx, a, b, a_normals=None, index_a=None, return_links=False, ties='pick', max_pairs=None):
    """Distortion tally of decoded cloud b against original cloud a on the GPU (include/pcc_geo.h "cloud metrics"): float64[9] =
    N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA (utils/pc_metric.pair_tally's five slots plus the Hausdorff maxima).
    a, b: (N,3) integer coordinates in [0, 2^21), N >= 1; a_normals: (N_A,3) normals of a (None: the D2 / H2 slots are 0);
    index_a: a CloudIndex of a to reuse (a is then not read).  return_links=True also returns to_b (int32[N_A]) and to_a
    (int32[N_B]), the nearest rows across (ties: the lowest row).  Deterministic: the same inputs give the same bits.
    ties='mean': D2 / H2 average over ALL equidistant nearest points (DESIGN.md "Tie-averaged D2"), independent of either cloud's
    row order up to float64 rounding.  Its pair workspace holds max_pairs pairs (default tie_pair_capacity(N_A)); with the default,
    a cloud that needs more is run once more with the exact number the first run reported, an explicit max_pairs that is too small
    raises TiePairOverflow."""
    mode = _tie_mode(ties)
    if index_a is None:                     # every input is checked before the first GPU call
        a = _voxel_points(a, 'cloud_distortion')
        b = _voxel_points(b, 'cloud_distortion')
        _normals64(a_normals, len(a))
        index_a = CloudIndex(ctx, a)
    out = cloud_distortion_launch(ctx, index_a, b, a_normals, links=return_links, ties=ties, max_pairs=max_pairs)
    if mode:
        pairs, over = (int(v) for v in out[-1].cpu())
        if over:
            if max_pairs is not None or pairs > _PAIR_LIMIT:
                raise TiePairOverflow(pairs, tie_pair_capacity(index_a.n) if max_pairs is None else max_pairs)
            out = cloud_distortion_launch(ctx, index_a, b, a_normals, links=return_links, ties=ties, max_pairs=pairs)
        out = out[:-1] if return_links else out[0]
    if return_links:
        return tuple(t.cpu().numpy() for t in out)
    return out.cpu().numpy()


COLOR_TALLY_SLOTS = 6      # include/pcc_geo.h "cloud colours": Y, U, V sums of A->B, then of B->A


def _colors_u8(colors, n, what):
    """Host-side check of an (n,3) colour array (numpy or tensor, integer values in 0..255); returns it as uint8 of the same kind."""
    if isinstance(colors, torch.Tensor):
        if colors.is_floating_point() or colors.is_complex() or colors.dtype == torch.bool:
            raise L.PccError(f'{what}: colours must be integers in 0..255, got {colors.dtype}')
        if tuple(colors.shape) != (n, 3):
            raise L.PccError(f'{what}: colours must be ({n}, 3), got {tuple(colors.shape)}')
        if colors.dtype != torch.uint8 and n and (bool((colors < 0).any()) or bool((colors > 255).any())):
            raise L.PccError(f'{what}: colours must be integers in 0..255')
        return colors.to(torch.uint8).contiguous()
    c = np.asarray(colors)
    if c.dtype.kind not in 'iu':
        raise L.PccError(f'{what}: colours must be integers in 0..255, got {c.dtype}')
    if c.shape != (n, 3):
        raise L.PccError(f'{what}: colours must be ({n}, 3), got {c.shape}')
    if c.dtype != np.uint8 and c.size and (c.min() < 0 or c.max() > 255):
        raise L.PccError(f'{what}: colours must be integers in 0..255')
    return np.ascontiguousarray(c, np.uint8)


def _device_u8(ctx, colors):
    return (colors.to(ctx.device) if isinstance(colors, torch.Tensor) else torch.from_numpy(colors).to(ctx.device)).contiguous()


def _index_or_points(index, what):
    """A CloudIndex, or points checked by _voxel_points (the index is then built by the caller after every check)."""
    if isinstance(index, CloudIndex):
        return index, index.n
    pts = _voxel_points(index, what)
    return pts, int(pts.shape[0])


def map_colors(ctx, index_a, a_colors, queries, rank=2, return_rows=False):
    """Colour of every query point taken from the original cloud (include/pcc_geo.h "cloud colours"): for each query, the colour of
    its rank-th nearest point of the original cloud, points ordered by (squared distance, row).  rank=2 (the default) is the
    reference's map_color.py (the second of a k = 2 KD-tree query), rank=1 the nearest point (cloud_nearest's row).
    index_a: a CloudIndex of the original cloud or its (N,3) points; a_colors: (N,3) integer colours in 0..255; queries: (nq,3)
    integer coordinates in [0, 2^21).  Returns (nq,3) uint8 numpy colours (and the int32 rows with return_rows=True); nq = 0 gives
    empty arrays.  Every input is checked before the first GPU call."""
    if rank not in (1, 2):
        raise L.PccError(f'map_colors: rank = {rank!r}, must be 1 or 2')
    index_a, n = _index_or_points(index_a, 'map_colors')
    if rank > n:
        raise L.PccError(f'map_colors: rank {rank} needs at least {rank} original points, got {n}')
    colors = _colors_u8(a_colors, n, 'map_colors')
    if len(queries) == 0:
        out = np.zeros((0, 3), np.uint8)
        return (out, np.zeros(0, np.int32)) if return_rows else out
    q = _voxel_points(queries, 'map_colors')
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    index_q = CloudIndex(ctx, q)
    nq = index_q.n
    colors_d = _device_u8(ctx, colors)          # held in a local: a temporary's block could be handed out again before the launch
    out = torch.empty((nq, 3), dtype=torch.uint8, device=ctx.device)
    rows = torch.empty((nq,), dtype=torch.int32, device=ctx.device) if return_rows else None
    L.check(L.lib().pcc_cloud_map_colors(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(colors_d), _ptr(index_q.buffer), nq, rank, _ptr(out),
                                         _ptr(rows), ctx.stream), 'pcc_cloud_map_colors')
    if return_rows:
        return out.cpu().numpy(), rows.cpu().numpy()
    return out.cpu().numpy()


def cloud_color_distortion(ctx, index_a, a_colors, b_points, b_colors):
    """Colour distortion tally of a decoded coloured cloud B against the original A on the GPU (include/pcc_geo.h "cloud colours"):
    float64[6] = the sums of the squared BT.709 Y, U, V errors over A (against the mean colour of each point's equidistant nearest
    points of B), then over B against A.  index_a: a CloudIndex of A or its (N_A,3) points; colours (N,3) integers in 0..255;
    b_points (N_B,3), N_B >= 1.  utils/pc_metric.color_table turns it into mse / psnr.  Every input is checked before the first GPU
    call; the same inputs give the same bits."""
    index_a, n = _index_or_points(index_a, 'cloud_color_distortion')
    colors_a = _colors_u8(a_colors, n, 'cloud_color_distortion')
    b = _voxel_points(b_points, 'cloud_color_distortion')
    colors_b = _colors_u8(b_colors, int(b.shape[0]), 'cloud_color_distortion')
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    index_b = CloudIndex(ctx, b)
    dev = ctx.device
    ca_d, cb_d = _device_u8(ctx, colors_a), _device_u8(ctx, colors_b)     # both alive until the launch (see map_colors)
    tally = torch.empty((COLOR_TALLY_SLOTS,), dtype=torch.float64, device=dev)
    ws = torch.empty((L.lib().pcc_cloud_color_workspace_bytes(index_a.n, index_b.n),), dtype=torch.uint8, device=dev)
    L.check(L.lib().pcc_cloud_color_distortion(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(ca_d), _ptr(index_b.buffer), index_b.n,
                                               _ptr(cb_d), _ptr(tally), _ptr(ws), ctx.stream), 'pcc_cloud_color_distortion')
    return tally.cpu().numpy()


def mesh_to_points(ctx, vertices, faces, n_samples=500000, vg_size=64, seed=0, return_samples=False):
    """A triangle mesh to a voxelised point cloud on the GPU (include/pcc_geo.h "mesh sampling"): the reference's ds_mesh_to_pc
    (area-weighted sampling with pyntcloud's barycentrics, one scalar min / max over all axes, rint onto a vg_size^3 grid, the first
    sample of every voxel), reproducible from `seed` (0 <= seed < 2^64).  vertices (V,3) float64, faces (F,3) integer indices.
    Returns (M,3) float32 voxels in sample order (and the (n,3) float32 raw samples with return_samples=True): the same bits as
    utils/mesh_sampling.mesh_to_points.  Every input is checked on the host before the first GPU call (ValueError)."""
    from .utils import mesh_sampling
    v, f = mesh_sampling.check_mesh(vertices, faces, n_samples, vg_size, seed)
    n, vg = int(n_samples), int(vg_size)
    dev = ctx.device
    v_d, f_d = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    samples = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_samples else None
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):            # hipCUB sizes its temporary storage for the current device
        ws_bytes = L.lib().pcc_mesh_sample_workspace_bytes(f.shape[0], n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    L.check(L.lib().pcc_mesh_to_points(ctx.handle, _ptr(v_d), v.shape[0], _ptr(f_d), f.shape[0], n, C.c_uint64(int(seed)), vg,
                                       _ptr(samples), _ptr(points), _ptr(count), _ptr(ws), ctx.stream), 'pcc_mesh_to_points')
    m = int(count.item())
    out = points[:m].cpu().numpy()
    return (out, samples.cpu().numpy()) if return_samples else out


def render_points(ctx, points, camera, colors=None, point_size=1, background=(255, 255, 255), return_rows=False):
    """A z-buffered square splat of a point cloud through a pinhole camera on the GPU (include/pcc_geo.h "point rendering").
    points: (n,3) float32, float64 or integer coordinates (any values: points behind the camera or off-screen are dropped);
    camera: a utils.render.Camera; colors: (n,3) integers in 0..255, or None for flat grey (128); point_size: integer side of each
    point's square in [1, 64]; background: RGB.  Returns the (H,W,3) uint8 numpy image (and the (H,W) int32 row of every pixel,
    -1 for the background, with return_rows=True): the same bytes as utils.render.render_host.  Every limit is checked on the
    host before any GPU call (ValueError); n = 0 gives the background without a launch."""
    from .utils import render
    p, c, s, bg = render.check_render_args(points, colors, camera, point_size, background)
    W, H = camera.width, camera.height
    n = int(p.shape[0])
    if n == 0:
        img = np.broadcast_to(bg, (H, W, 3)).copy()
        return (img, np.full((H, W), -1, np.int32)) if return_rows else img
    dev = ctx.device
    p_d = torch.from_numpy(p).to(dev)
    c_d = None if c is None else torch.from_numpy(c).to(dev)
    img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    rows = torch.empty((H, W), dtype=torch.int32, device=dev) if return_rows else None
    ws = torch.empty((L.lib().pcc_render_workspace_bytes(W, H),), dtype=torch.uint8, device=dev)
    E = (C.c_double * 16)(*camera.extrinsic.ravel().tolist())
    K = (C.c_double * 9)(*camera.intrinsic.ravel().tolist())
    bgc = (C.c_uint8 * 3)(*bg.tolist())
    L.check(L.lib().pcc_render_points(ctx.handle, _ptr(p_d), n, _ptr(c_d), E, K, W, H, s, bgc, _ptr(img), _ptr(rows), _ptr(ws),
                                      ctx.stream), 'pcc_render_points')
    if return_rows:
        return img.cpu().numpy(), rows.cpu().numpy()
    return img.cpu().numpy()


def error_map(ctx, index_a, b_points):
    """The squared D1 residual of every decoded point: for each row of b_points, the exact squared distance to its nearest point of
    the original cloud (int64 numpy array; cloud_nearest's distance, so the reference's compute_d1_res_ba whatever the tie rule).
    index_a: a CloudIndex of the original or its (N,3) points; b_points: (nb,3) integer coordinates in [0, 2^21)."""
    index_a, _ = _index_or_points(index_a, 'error_map')
    if len(b_points) == 0:
        return np.zeros(0, np.int64)
    _voxel_points(b_points, 'error_map')
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    return cloud_nearest(ctx, index_a, b_points)[1]


# ---------------------------------------------------------------------------------------------
# octree anchor (include/pcc_geo.h "octree anchor"; the codec is anchor_octree.py)
# ---------------------------------------------------------------------------------------------
def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def anchor_code_bits(models, bits):
    """The anchor's binary range coder on raw decisions: models (n) in [0, 2048), bits (n) in {0, 1} -> bytes (host)."""
    m, b = np.ascontiguousarray(models, dtype=np.uint16), _u8(bits)
    assert m.ndim == 1 and m.shape == b.shape, 'anchor_code_bits: models and bits must be 1-d and of one length'
    out = np.empty(2 * m.size + 16, np.uint8)
    n = C.c_int64()
    L.check(L.lib().pcc_anchor_code_bits(m.ctypes.data, b.ctypes.data, m.size, out.ctypes.data, out.size, C.byref(n)), 'pcc_anchor_code_bits')
    return out[:n.value].tobytes()


def anchor_decode_bits(data, models):
    m = np.ascontiguousarray(models, dtype=np.uint16)
    buf = np.frombuffer(bytes(data), np.uint8)
    out = np.empty(m.size, np.uint8)
    L.check(L.lib().pcc_anchor_decode_bits(buf.ctypes.data if buf.size else None, buf.size, m.ctypes.data, m.size, out.ctypes.data),
            'pcc_anchor_decode_bits')
    return out


def anchor_encode_nodes(occ, n6, no_context=False):
    """All occupancy bytes of a tree (breadth first) with their neighbour masks -> the payload bytes (host)."""
    occ, n6 = _u8(occ), _u8(n6)
    assert occ.ndim == 1 and occ.shape == n6.shape, 'anchor_encode_nodes: occ and n6 must be 1-d and of one length'
    out = np.empty(2 * occ.size + 16, np.uint8)
    n = C.c_int64()
    L.check(L.lib().pcc_anchor_encode(occ.ctypes.data, n6.ctypes.data, occ.size, L.PCC_ANCHOR_NO_CONTEXT if no_context else 0, out.ctypes.data,
                                      out.size, C.byref(n)), 'pcc_anchor_encode')
    return out[:n.value].tobytes()


class AnchorDecoder:
    """The host decoder of one payload: level(n6) returns the occupancy bytes of the next level.  A payload that ends early raises
    PccError."""

    def __init__(self, payload, no_context=False):
        self._data = np.frombuffer(bytes(payload), np.uint8)          # kept alive: the C state points into it
        self._state = np.zeros(L.lib().pcc_anchor_decoder_bytes() + 8, np.uint8)
        L.check(L.lib().pcc_anchor_decoder_init(self._state.ctypes.data, self._data.ctypes.data if self._data.size else None, self._data.size,
                                                L.PCC_ANCHOR_NO_CONTEXT if no_context else 0), 'pcc_anchor_decoder_init')

    def level(self, n6):
        n6 = _u8(n6)
        occ = np.empty(n6.size, np.uint8)
        L.check(L.lib().pcc_anchor_decode_level(self._state.ctypes.data, n6.ctypes.data, n6.size, occ.ctypes.data), 'pcc_anchor_decode_level')
        return occ

    @property
    def consumed(self):
        return int(L.lib().pcc_anchor_decoder_consumed(self._state.ctypes.data))

    def __len__(self):
        return int(self._data.size)


def anchor_tree_launch(ctx, points, num, den, depth):
    """Enqueues the tree of anchor_octree.encode for an int32 (n,3) numpy cloud already checked by the caller; returns the pinned
    host buffer the result is being copied into and a function that waits for it and returns (counts[depth + 1], occ, n6): the nodes
    per level with the leaves last, and the bytes of all levels, breadth first.  Nothing is read back before that one copy."""
    lib, dev = L.lib(), ctx.device
    n, depth = int(points.shape[0]), int(depth)
    cap = int(lib.pcc_anchor_tree_capacity(n, depth))
    if cap <= 0:
        raise L.PccError(f'anchor_tree: {n} points at depth {depth} are outside the contract')
    hdr_bytes = 8 * L.PCC_ANCHOR_HDR_WORDS
    pts_d = torch.from_numpy(points).to(dev, non_blocking=True)
    out = torch.empty((hdr_bytes + 2 * cap,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):            # hipCUB sizes its temporary storage for the current device
        ws = torch.empty((lib.pcc_anchor_tree_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    L.check(lib.pcc_anchor_tree(ctx.handle, _ptr(pts_d), n, int(num), int(den), depth, C.c_void_p(base), C.c_void_p(base + hdr_bytes),
                                C.c_void_p(base + hdr_bytes + cap), _ptr(ws), ctx.stream), 'pcc_anchor_tree')
    pin = getattr(ctx, '_anchor_pin', None)             # one launch in flight per context: the pinned landing buffer is reused
    if pin is None or pin.numel() < out.numel():
        ctx._anchor_pin = pin = torch.empty((out.numel(),), dtype=torch.uint8, pin_memory=True)
    host = pin[:out.numel()]
    host.copy_(out, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    alive = (pts_d, out, ws)

    def finish():
        assert alive
        done.synchronize()                  # pts_d, out and ws stay alive until here
        raw = host.numpy()
        counts = raw[:hdr_bytes].view(np.int64)[:depth + 1].copy()
        offs = [int(lib.pcc_anchor_tree_level_offset(n, l)) for l in range(depth + 1)]
        for l in range(depth):
            if not 1 <= counts[l] <= offs[l + 1] - offs[l]:
                raise L.PccError(f'anchor_tree: level {l} reports {counts[l]} nodes for a slot of {offs[l + 1] - offs[l]}')
        occ = np.concatenate([raw[hdr_bytes + offs[l]:hdr_bytes + offs[l] + counts[l]] for l in range(depth)])
        n6 = np.concatenate([raw[hdr_bytes + cap + offs[l]:hdr_bytes + cap + offs[l] + counts[l]] for l in range(depth)])
        return counts, occ, n6
    return finish


def anchor_tree(ctx, points, num, den, depth):
    return anchor_tree_launch(ctx, points, num, den, depth)()


def anchor_expand(ctx, parents, occ, child_level, want_n6=True):
    """One decoder step on the device: parents (device uint64 keys of a level, ascending; None for the root), occ (numpy uint8, the
    level's decoded bytes) -> (child keys on the device, their n6 as numpy or None).  One copy in, one copy out."""
    dev = ctx.device
    occ = _u8(occ)
    if parents is None:
        parents = torch.zeros((1,), dtype=torch.int64, device=dev)
    npar = int(parents.shape[0])
    assert occ.shape == (npar,), 'anchor_expand: one occupancy byte per parent'
    nch = int(np.unpackbits(occ).sum())
    occ_d = torch.from_numpy(occ).to(dev)
    children = torch.empty((nch,), dtype=torch.int64, device=dev)
    n6 = torch.empty((nch,), dtype=torch.uint8, device=dev) if want_n6 else None
    with torch.cuda.device(dev):
        ws = torch.empty((L.lib().pcc_anchor_expand_workspace_bytes(npar),), dtype=torch.uint8, device=dev)
    L.check(L.lib().pcc_anchor_expand(ctx.handle, _ptr(parents), _ptr(occ_d), npar, int(child_level), _ptr(children), nch, _ptr(n6), _ptr(ws),
                                      ctx.stream), 'pcc_anchor_expand')
    return children, (n6.cpu().numpy() if want_n6 else None)


def anchor_points(ctx, keys, num, den, resolution):
    """Leaf keys (device) -> the decoded (n,3) int32 points (numpy), in key order."""
    n = int(keys.shape[0])
    pts = torch.empty((n, 3), dtype=torch.int32, device=ctx.device)
    L.check(L.lib().pcc_anchor_points(ctx.handle, _ptr(keys), n, int(num), int(den), int(resolution), _ptr(pts), ctx.stream), 'pcc_anchor_points')
    return pts.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# surface anchor (include/pcc_geo.h "surface anchor"; the codec is anchor_surface.py)
# ---------------------------------------------------------------------------------------------
def surface_encode_vertices(edge_keys, flags, t, k):
    """The vertex payload: edge keys (n) uint64, flags (n) in {0, 1}, t (n) in [0, 2^k) -> bytes (host)."""
    keys, flags, t = np.ascontiguousarray(edge_keys, dtype=np.uint64), _u8(flags), _u8(t)
    assert keys.ndim == 1 and keys.shape == flags.shape == t.shape, 'surface_encode_vertices: one flag and one t per edge'
    out = np.empty(8 * keys.size + 16, np.uint8)
    n = C.c_int64()
    L.check(L.lib().pcc_surface_encode_vertices(keys.ctypes.data, flags.ctypes.data, t.ctypes.data, keys.size, int(k), out.ctypes.data, out.size,
                                                C.byref(n)), 'pcc_surface_encode_vertices')
    return out[:n.value].tobytes()


def surface_decode_vertices(data, edge_keys, k):
    """-> (flags, t, set flags, bytes read) of a vertex payload over the given edge list (host); PccError when it ends early."""
    keys = np.ascontiguousarray(edge_keys, dtype=np.uint64)
    buf = np.frombuffer(bytes(data), np.uint8)
    flags, t = np.zeros(keys.size, np.uint8), np.zeros(keys.size, np.uint8)
    nflags, consumed = C.c_int64(), C.c_int64()
    L.check(L.lib().pcc_surface_decode_vertices(buf.ctypes.data if buf.size else None, buf.size, keys.ctypes.data, keys.size, int(k), flags.ctypes.data,
                                                t.ctypes.data, C.byref(nflags), C.byref(consumed)), 'pcc_surface_decode_vertices')
    return flags, t, nflags.value, consumed.value


def _surface_ws(ctx, name, n):
    nbytes = getattr(L.lib(), f'pcc_surface_{name}_workspace_bytes')(int(n))
    if nbytes == 0:
        raise L.PccError(f'surface_{name}: a count of {n} is outside the contract')
    with torch.cuda.device(ctx.device):         # hipCUB sizes its temporary storage for the current device
        return torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)


def _surface_hdr(ctx):
    return torch.zeros((L.PCC_SURFACE_HDR_WORDS,), dtype=torch.int64, device=ctx.device)


def surface_leaves(ctx, points, k):
    """int32 (n,3) numpy cloud already checked by the caller -> (Morton keys of its distinct points, leaf keys), device int64, ascending."""
    n = int(points.shape[0])
    pts_d = torch.from_numpy(points).to(ctx.device)
    pkeys = torch.empty((n,), dtype=torch.int64, device=ctx.device)
    leaves = torch.empty((n,), dtype=torch.int64, device=ctx.device)
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'leaves', n)
    L.check(L.lib().pcc_surface_leaves(ctx.handle, _ptr(pts_d), n, int(k), _ptr(hdr), _ptr(pkeys), _ptr(leaves), _ptr(ws), ctx.stream),
            'pcc_surface_leaves')
    ndistinct, nleaves = (int(v) for v in hdr.cpu()[:2])
    if not 1 <= nleaves <= ndistinct <= n:
        raise L.PccError(f'surface_leaves: {ndistinct} distinct points and {nleaves} leaves from {n} points')
    return pkeys[:ndistinct], leaves[:nleaves]


def surface_edges(ctx, leaf_keys):
    """Leaf keys (device int64, ascending) -> the edge list (device int64, ascending)."""
    n = int(leaf_keys.shape[0])
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'edges', n)
    edges = torch.empty((12 * n,), dtype=torch.int64, device=ctx.device)
    L.check(L.lib().pcc_surface_edges(ctx.handle, _ptr(leaf_keys), n, _ptr(hdr), _ptr(edges), _ptr(ws), ctx.stream), 'pcc_surface_edges')
    nedges = int(hdr.cpu()[0])
    if not 1 <= nedges <= 12 * n:
        raise L.PccError(f'surface_edges: {nedges} edges from {n} leaves')
    return edges[:nedges]


def surface_vertices(ctx, pkeys, k, edge_keys):
    """Distinct point keys and the edge list (device) -> (flags, t) per edge, numpy uint8."""
    n, nedges = int(pkeys.shape[0]), int(edge_keys.shape[0])
    out = torch.empty((2, nedges), dtype=torch.uint8, device=ctx.device)
    ws = _surface_ws(ctx, 'vertices', n)
    L.check(L.lib().pcc_surface_vertices(ctx.handle, _ptr(pkeys), n, int(k), _ptr(edge_keys), nedges, _ptr(out[0]), _ptr(out[1]), _ptr(ws),
                                         ctx.stream), 'pcc_surface_vertices')
    out = out.cpu().numpy()
    return out[0], out[1]


def surface_reconstruct(ctx, leaf_keys, edge_keys, flags, t, k, resolution):
    """Leaves, edge list (device int64) and the vertices (numpy uint8 per edge) -> the decoded (n,3) int32 cloud (numpy), in Morton order."""
    dev = ctx.device
    nleaves, nedges = int(leaf_keys.shape[0]), int(edge_keys.shape[0])
    flags, t = _u8(flags), _u8(t)
    assert flags.shape == t.shape == (nedges,), 'surface_reconstruct: one flag and one t per edge'
    ft = torch.from_numpy(np.stack([flags, t])).to(dev)
    pos = torch.empty((nleaves,), dtype=torch.int64, device=dev)
    hdr, ws = _surface_hdr(ctx), _surface_ws(ctx, 'count', nleaves)
    L.check(L.lib().pcc_surface_count(ctx.handle, _ptr(leaf_keys), nleaves, _ptr(edge_keys), _ptr(ft[0]), _ptr(ft[1]), nedges, int(k), _ptr(pos),
                                      _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_surface_count')
    total = int(hdr.cpu()[0])
    if not nleaves <= total < 1 << 31:
        raise L.PccError(f'surface_reconstruct: {total} voxels from {nleaves} leaves')
    pts = torch.empty((total, 3), dtype=torch.int32, device=dev)
    ws = _surface_ws(ctx, 'reconstruct', total)
    L.check(L.lib().pcc_surface_reconstruct(ctx.handle, _ptr(leaf_keys), nleaves, _ptr(edge_keys), _ptr(ft[0]), _ptr(ft[1]), nedges, int(k),
                                            int(resolution), _ptr(pos), total, _ptr(pts), _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_surface_reconstruct')
    n = int(hdr.cpu()[0])
    if not 1 <= n <= total:
        raise L.PccError(f'surface_reconstruct: {n} distinct voxels of {total}')
    return pts[:n].cpu().numpy()


# ---------------------------------------------------------------------------------------------
# colour anchor (include/pcc_geo.h "colour anchor"; the codec is anchor_color.py)
# ---------------------------------------------------------------------------------------------
def _color_counts(counts):
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    assert counts.ndim == 1 and counts.size <= 63, 'colour anchor: one count per step, at most 63 steps'
    return counts


def color_anchor_encode_coefficients(coef, counts):
    """Coefficients (n,3) int16 in coding order and the per-step counts -> the payload bytes (host)."""
    coef, counts = np.ascontiguousarray(coef, dtype=np.int16), _color_counts(counts)
    assert coef.ndim == 2 and coef.shape[1] == 3, 'color_anchor_encode_coefficients: coefficients must be (n, 3)'
    n = C.c_int64()
    for per_coef in (6, 48):                 # 48 bytes a coefficient always fit; the first try spares the memory
        out = np.empty(per_coef * coef.shape[0] + 16, np.uint8)
        rc = L.lib().pcc_color_anchor_encode(coef.ctypes.data, coef.shape[0], counts.ctypes.data, counts.size, out.ctypes.data, out.size, C.byref(n))
        if rc != L.PCC_ERR_SPACE:
            break
    L.check(rc, 'pcc_color_anchor_encode')
    return out[:n.value].tobytes()


def color_anchor_decode_coefficients(data, counts, ncoef):
    """-> (coefficients (ncoef,3) int16, bytes read) of a payload (host); PccError when it is damaged or ends early."""
    counts = _color_counts(counts)
    buf = np.frombuffer(bytes(data), np.uint8)
    coef = np.zeros((int(ncoef), 3), np.int16)
    consumed = C.c_int64()
    L.check(L.lib().pcc_color_anchor_decode(buf.ctypes.data if buf.size else None, buf.size, counts.ctypes.data, counts.size, coef.ctypes.data,
                                            int(ncoef), C.byref(consumed)), 'pcc_color_anchor_decode')
    return coef, consumed.value


def _color_ws(ctx, n):
    nbytes = L.lib().pcc_color_anchor_workspace_bytes(int(n))
    if nbytes == 0:
        raise L.PccError(f'color_anchor: {n} points are outside the contract')
    with torch.cuda.device(ctx.device):         # hipCUB sizes its temporary storage for the current device
        return torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)


def _color_hdr(raw, n):
    hdr = raw[:8 * L.PCC_COLOR_HDR_WORDS].view(np.int64)
    counts, dups = hdr[:64].copy(), int(hdr[64])
    if dups == 0 and (counts.min() < 0 or int(counts.sum()) != n - 1):
        raise L.PccError(f'color_anchor: the per-step counts sum to {int(counts.sum())} for {n} points')
    return counts, dups, hdr[65:68].copy()


def color_anchor_plan(ctx, points, depth):
    """int32 (n,3) numpy cloud already checked by the caller -> (the planned workspace for color_anchor_inverse (device), per-step
    counts int64[64], number of adjacent equal keys: nonzero = duplicate positions).  One copy back."""
    n = int(points.shape[0])
    pts_d = torch.from_numpy(points).to(ctx.device)
    hdr = torch.empty((L.PCC_COLOR_HDR_WORDS,), dtype=torch.int64, device=ctx.device)
    ws = _color_ws(ctx, n)
    L.check(L.lib().pcc_color_anchor_plan(ctx.handle, _ptr(pts_d), n, int(depth), _ptr(hdr), _ptr(ws), ctx.stream), 'pcc_color_anchor_plan')
    counts, dups, _ = _color_hdr(hdr.cpu().numpy().view(np.uint8), n)
    return ws, counts, dups


def color_anchor_transform(ctx, points, colors, depth, qstep):
    """Plan and forward transform of an int32 (n,3) cloud and its uint8 (n,3) colours, both already checked by the caller ->
    (counts int64[64], adjacent equal keys, DC int64[3], coefficients (n - 1, 3) int16 in coding order).  Both calls are enqueued
    before the one copy back."""
    lib, dev = L.lib(), ctx.device
    n = int(points.shape[0])
    hdr_bytes = 8 * L.PCC_COLOR_HDR_WORDS
    pts_d, col_d = torch.from_numpy(points).to(dev), torch.from_numpy(colors).to(dev)
    out = torch.empty((hdr_bytes + 6 * (n - 1),), dtype=torch.uint8, device=dev)
    ws = _color_ws(ctx, n)
    base = out.data_ptr()
    L.check(lib.pcc_color_anchor_plan(ctx.handle, _ptr(pts_d), n, int(depth), C.c_void_p(base), _ptr(ws), ctx.stream), 'pcc_color_anchor_plan')
    L.check(lib.pcc_color_anchor_forward(ctx.handle, _ptr(col_d), n, int(depth), int(qstep), C.c_void_p(base),
                                         C.c_void_p(base + hdr_bytes) if n > 1 else None, _ptr(ws), ctx.stream), 'pcc_color_anchor_forward')
    raw = out.cpu().numpy()
    counts, dups, dc = _color_hdr(raw, n)
    return counts, dups, dc, raw[hdr_bytes:].view(np.int16).reshape(n - 1, 3).copy()


def color_anchor_inverse(ctx, plan, coef, dc, n, depth, qstep):
    """A workspace color_anchor_plan filled for the same n points, coefficients (n - 1, 3) int16 in coding order and the DC triple ->
    the (n,3) uint8 colours (numpy) in the row order of the planned points."""
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    assert coef.shape == (n - 1, 3), 'color_anchor_inverse: one coefficient triple per point but the first'
    coef_d = torch.from_numpy(coef).to(ctx.device) if n > 1 else None
    dc = np.ascontiguousarray(dc, dtype=np.int32)
    assert dc.shape == (3,), 'color_anchor_inverse: the DC is a triple'
    out = torch.empty((n, 3), dtype=torch.uint8, device=ctx.device)
    L.check(L.lib().pcc_color_anchor_inverse(ctx.handle, _ptr(coef_d), dc.ctypes.data, int(n), int(depth), int(qstep), _ptr(out), _ptr(plan),
                                             ctx.stream), 'pcc_color_anchor_inverse')
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# host range coder
# ---------------------------------------------------------------------------------------------
class HostCdfTable:
    """Quantised CDF table (rows, stride) + per-row size/offset, as the reference's
    `quantized_cdf` / `cdf_length` / `offset` (src/utils/patch_gaussian_conditional.py:91-97,118)."""

    def __init__(self, cdf, cdf_size, offset, precision=16, overflow_width=4):
        self.cdf = np.ascontiguousarray(cdf, np.int32)
        self.cdf_size = np.ascontiguousarray(cdf_size, np.int32)
        self.offset = np.ascontiguousarray(offset, np.int32)
        assert self.cdf.ndim == 2 and len(self.cdf_size) == len(self.offset) == self.cdf.shape[0]
        self.struct = L.CdfTable(self.cdf.ctypes.data_as(C.POINTER(C.c_int32)),
                                 self.cdf_size.ctypes.data_as(C.POINTER(C.c_int32)),
                                 self.offset.ctypes.data_as(C.POINTER(C.c_int32)),
                                 self.cdf.shape[0], self.cdf.shape[1], precision, overflow_width)


def _np_i32(a):
    if isinstance(a, torch.Tensor):
        a = a.numpy()
    a = np.ascontiguousarray(a, np.int32).reshape(-1)
    return a


def _np_host(a, allowed):
    """flat contiguous host array; keeps a dtype in `allowed` (narrow staging buffers), anything else becomes int32"""
    if isinstance(a, torch.Tensor):
        a = a.numpy()
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype in allowed else a.astype(np.int32)).reshape(-1)


def _uniform_dtype(arrs, allowed):
    """one dtype for all streams of a call (the ABI takes one element size per call)"""
    if all(a.dtype == arrs[0].dtype for a in arrs) and arrs[0].dtype in allowed:
        return arrs, arrs[0].dtype.itemsize
    return [np.ascontiguousarray(a, np.int32) for a in arrs], 4


_SYM, _ROW = (np.dtype(np.int16), np.dtype(np.int32)), (np.dtype(np.uint8), np.dtype(np.int32))


def _rows_2d(x, allowed):
    """x: a 2-D (streams, symbols) host array / CPU tensor whose dtype the ABI takes as it is -> C-contiguous numpy 2-D, else None."""
    if isinstance(x, torch.Tensor):
        x = x.numpy()
    if isinstance(x, np.ndarray) and x.ndim >= 2 and x.dtype in allowed:
        return np.ascontiguousarray(x.reshape(x.shape[0], -1))
    return None


def _row_ptrs(a2d):
    """uint64[streams]: the address of every row of a C-contiguous 2-D array -- what the ABI's `const void* const*` wants, without a
    Python loop over the streams (the per-stream ctypes bookkeeping was 0.4 ms per coder call: 1.6 ms of GIL-holding time per step)."""
    return np.uint64(a2d.ctypes.data) + np.arange(a2d.shape[0], dtype=np.uint64) * np.uint64(a2d.strides[0])


def _pp(ptrs):
    return ptrs.ctypes.data_as(C.POINTER(C.c_void_p))


def _sz(a):
    return a.ctypes.data_as(C.POINTER(C.c_size_t))


def range_encode_batch(table, data_list, index_list=None, index_mod=0, n_threads=0):
    """data_list: per-stream symbol arrays, int32 or int16 -- a list, or ONE 2-D (streams, symbols) array / CPU tensor (fast path: no
    per-stream Python work); index_list: per-stream CDF rows, int32 or uint8: a list, a 2-D array, or a single 1-D array shared by all
    streams.  Returns list of bytes."""
    d2 = _rows_2d(data_list, _SYM)
    if d2 is not None:
        S, n_sym = d2.shape
        if S == 0:
            return []
        if index_list is None:
            ip, ib, keep = None, 4, None
        else:
            i2 = _rows_2d(index_list, _ROW)
            if i2 is not None:
                assert i2.shape == d2.shape
                keep, ib = i2, i2.dtype.itemsize
                ip = _row_ptrs(i2)
            else:                                   # one row vector for every stream
                keep = _np_host(index_list, _ROW)
                assert keep.size == n_sym
                ib, ip = keep.dtype.itemsize, np.full(S, keep.ctypes.data, np.uint64)
        cap = n_sym * 8 + 64
        outs = np.empty((S, cap), np.uint8)
        n = np.full(S, n_sym, np.uint64)
        caps = np.full(S, cap, np.uint64)
        olen = np.zeros(S, np.uint64)
        dp, op = _row_ptrs(d2), _row_ptrs(outs)
        L.check(L.lib().pcc_range_encode_batch_n(C.byref(table.struct), S, _pp(dp), d2.dtype.itemsize, None if ip is None else _pp(ip), ib, index_mod,
                                                 _sz(n), _pp(op), _sz(caps), _sz(olen), n_threads), 'pcc_range_encode_batch_n')
        del keep
        return [outs[s_, :int(olen[s_])].tobytes() for s_ in range(S)]
    S = len(data_list)
    if S == 0:
        return []
    data, db = _uniform_dtype([_np_host(d, _SYM) for d in data_list], _SYM)
    idx, ib = (None, 4) if index_list is None else _uniform_dtype([_np_host(i, _ROW) for i in index_list], _ROW)
    n = (C.c_size_t * S)(*[d.size for d in data])
    caps = [d.size * 8 + 64 for d in data]
    outs = [np.empty(c, np.uint8) for c in caps]
    dp = (C.c_void_p * S)(*[d.ctypes.data for d in data])
    ip = None if idx is None else (C.c_void_p * S)(*[i.ctypes.data for i in idx])
    op = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
    cap = (C.c_size_t * S)(*caps)
    olen = (C.c_size_t * S)()
    if db == 4 and ib == 4:
        L.check(L.lib().pcc_range_encode_batch(C.byref(table.struct), S, dp, ip, index_mod, n, op, cap, olen, n_threads),
                'pcc_range_encode_batch')
    else:
        L.check(L.lib().pcc_range_encode_batch_n(C.byref(table.struct), S, dp, db, ip, ib, index_mod, n, op, cap, olen, n_threads),
                'pcc_range_encode_batch_n')
    return [outs[s][:olen[s]].tobytes() for s in range(S)]


def range_decode_batch(table, strings, n_list, index_list=None, index_mod=0, n_threads=0, out=None):
    """strings: list of bytes; n_list: symbols per stream; index_list: int32 or uint8 CDF rows (list, 2-D array, or one shared 1-D
    array).  Returns list of int32 numpy arrays, or fills the provided `out` -- a list of arrays, or ONE 2-D (streams, symbols) array /
    CPU tensor (fast path); int32, or int16: then a symbol that does not fit raises OverflowError and the caller decodes into int32."""
    S = len(strings)
    if S == 0:
        return []
    o2 = _rows_2d(out, _SYM) if out is not None and not isinstance(out, (list, tuple)) else None
    if o2 is not None:
        n_sym = o2.shape[1]
        assert o2.shape[0] == S and all(int(k) == n_sym for k in n_list)
        assert o2.ctypes.data == (out.numpy() if isinstance(out, torch.Tensor) else out).ctypes.data, 'out must be C-contiguous (it is filled in place)'
        if index_list is None:
            ip, ib, keep = None, 4, None
        else:
            # one row per stream (2-D) or ONE row shared by all streams (1-D); a list of per-stream arrays belongs to the legacy path
            # below (flattened here it would decode every stream with stream 0's rows)
            assert not isinstance(index_list, (list, tuple)), 'range_decode_batch: a 2-D `out` takes a 2-D (or one shared 1-D) index array'
            i2 = _rows_2d(index_list, _ROW)
            if i2 is not None:
                assert i2.shape == o2.shape, f'range_decode_batch: index rows {i2.shape} for symbols {o2.shape}'
                keep, ib, ip = i2, i2.dtype.itemsize, _row_ptrs(i2)
            else:
                keep = _np_host(index_list, _ROW)
                assert keep.ndim == 1 and keep.size == n_sym, f'range_decode_batch: shared index of {keep.size} rows for {n_sym} symbols'
                ib, ip = keep.dtype.itemsize, np.full(S, keep.ctypes.data, np.uint64)
        lens = np.fromiter((len(s_) for s_ in strings), np.uint64, S)
        blob = np.frombuffer(b''.join(strings) + b'\0', np.uint8)            # all strings in one buffer: pointers by offset
        sp = np.uint64(blob.ctypes.data) + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        n = np.full(S, n_sym, np.uint64)
        rc = L.lib().pcc_range_decode_batch_n(C.byref(table.struct), S, _pp(sp), _sz(lens), None if ip is None else _pp(ip), ib, index_mod, _sz(n),
                                              _pp(_row_ptrs(o2)), o2.dtype.itemsize, n_threads)
        del keep, blob
        if rc == L.PCC_ERR_SPACE and o2.dtype.itemsize == 2:
            raise OverflowError('a decoded symbol does not fit int16')
        L.check(rc, 'pcc_range_decode_batch_n')
        return out
    bufs = [np.frombuffer(s, np.uint8) if len(s) else np.zeros(1, np.uint8) for s in strings]
    idx, ib = (None, 4) if index_list is None else _uniform_dtype([_np_host(i, _ROW) for i in index_list], _ROW)
    outs = [np.empty(int(k), np.int32) for k in n_list] if out is None else out
    ob = outs[0].dtype.itemsize
    assert all(o.dtype == outs[0].dtype and o.flags['C_CONTIGUOUS'] for o in outs) and outs[0].dtype in _SYM
    sp = (C.c_void_p * S)(*[b.ctypes.data for b in bufs])
    sl = (C.c_size_t * S)(*[len(s) for s in strings])
    ip = None if idx is None else (C.c_void_p * S)(*[i.ctypes.data for i in idx])
    n = (C.c_size_t * S)(*[int(k) for k in n_list])
    op = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
    if ob == 4 and ib == 4:
        L.check(L.lib().pcc_range_decode_batch(C.byref(table.struct), S, sp, sl, ip, index_mod, n, op, n_threads),
                'pcc_range_decode_batch')
    else:
        rc = L.lib().pcc_range_decode_batch_n(C.byref(table.struct), S, sp, sl, ip, ib, index_mod, n, op, ob, n_threads)
        if rc == L.PCC_ERR_SPACE and ob == 2:
            raise OverflowError('a decoded symbol does not fit int16')
        L.check(rc, 'pcc_range_decode_batch_n')
    return outs


def pmf_to_quantized_cdf(pmf, precision=16):
    pmf = np.ascontiguousarray(pmf, np.float32)
    cdf = np.zeros(pmf.size + 1, np.int32)
    L.check(L.lib().pcc_pmf_to_quantized_cdf(pmf.ctypes.data_as(C.c_void_p), pmf.size, precision,
                                             cdf.ctypes.data_as(C.c_void_p)), 'pcc_pmf_to_quantized_cdf')
    return cdf


# ---------------------------------------------------------------------------------------------
# device rANS coder (the opt-in "rans1" string format, include/pcc_geo.h "rANS coder (DEVICE)")
# ---------------------------------------------------------------------------------------------
def rans_stream_cap(n):
    return int(L.lib().pcc_rans_stream_cap(int(n)))


def _rans_counts(ctx, n_list):
    """symbols per stream on the device; one cached tensor per (streams, n) when all streams are as long (the codec's case)"""
    n_list = [int(k) for k in n_list]
    if len(set(n_list)) > 1:
        return torch.tensor(n_list, dtype=torch.int32).to(ctx.device)
    cache = ctx.__dict__.setdefault('_rans_counts', {}) if isinstance(ctx, Context) else ctx._base.__dict__.setdefault('_rans_counts', {})
    key = (len(n_list), n_list[0])
    if key not in cache:
        cache[key] = torch.tensor(n_list, dtype=torch.int32).to(ctx.device)
    return cache[key]


def _rans_index(ctx, index, S, n_max):
    """-> (tensor or None, elements between the rows of two streams): (S, ...) int32 device tensor, or ONE row vector for all streams"""
    if index is None:
        return None, 0
    assert index.dtype == torch.int32 and index.is_contiguous() and index.device == ctx.device
    if index.numel() == n_max and (index.dim() == 1 or S == 1):
        return index, 0
    assert index.shape[0] == S and index.numel() == S * n_max, f'rans: index of shape {tuple(index.shape)} for {S} streams of {n_max}'
    return index, n_max


def rans_encode_launch(ctx, table, data, n_list=None, index=None, index_mod=0, channels=0, lanes=0):
    """Enqueues the encode of S streams on the current stream.  data: (S, ...) int32 device tensor, stream s = data[s] flattened (its
    first n_list[s] elements; default all); index: int32 device rows of the same shape, or one 1-D vector shared by all streams, or
    None with index_mod; channels > 0: data[s] is (vox, channels) in memory and the stream is channel-major (see the header).
    lanes: 0 = the lane rule.  Returns (out (S, cap) uint8, meta (2, S) int32: lengths, status) -- rans_encode_fetch(out, meta)."""
    assert data.dtype == torch.int32 and data.is_contiguous() and data.device == ctx.device and data.dim() >= 2
    S = data.shape[0]
    n_max = data[0].numel() if S else 0
    n_list = [n_max] * S if n_list is None else [int(k) for k in n_list]
    assert len(n_list) == S and all(0 <= k <= n_max for k in n_list)
    cap = rans_stream_cap(n_max)
    out = torch.empty((S, cap), dtype=torch.uint8, device=ctx.device)
    meta = torch.zeros((2, S), dtype=torch.int32, device=ctx.device)
    if S == 0:
        return out, meta
    idx, idx_stride = _rans_index(ctx, index, S, n_max)
    ws = torch.empty((int(L.lib().pcc_rans_workspace_bytes(S, n_max)) + 16,), dtype=torch.uint8, device=ctx.device)
    n_dev = _rans_counts(ctx, n_list)
    L.check(L.lib().pcc_rans_encode_batch(ctx.handle, C.byref(table.struct), S, _ptr(data), n_max, _ptr(idx), idx_stride, index_mod, channels,
                                          _ptr(n_dev), n_max, lanes, _ptr(out), cap, _ptr(meta[0]), _ptr(meta[1]), _ptr(ws), ws.numel(),
                                          ctx.stream), 'pcc_rans_encode_batch')
    return out, meta


def rans_encode_fetch(out, meta):
    """The strings of a rans_encode_launch: the lengths first, then only the used part of the byte buffer.  Waits for the device."""
    if out.shape[0] == 0:
        return []
    m = meta.cpu().numpy()
    if m[1].any():
        raise AssertionError('pcc_rans_encode_batch: CDF row index out of range (or a stream that is no multiple of its channels)')
    used = int(m[0].max())
    b = out[:, :used].cpu().numpy() if used else np.zeros((out.shape[0], 0), np.uint8)
    return [b[s, :int(m[0, s])].tobytes() for s in range(out.shape[0])]


def rans_encode_batch(ctx, table, data, n_list=None, index=None, index_mod=0, channels=0, lanes=0):
    """-> list of bytes (rans_encode_launch + rans_encode_fetch)"""
    return rans_encode_fetch(*rans_encode_launch(ctx, table, data, n_list, index, index_mod, channels, lanes))


def rans_check_status(status):
    """the per-stream flags of a rans_decode_batch(check=False), fetched now: raises like the checked call"""
    st = status.cpu().numpy()
    if (st & 5).any():
        raise AssertionError('pcc_rans_decode_batch: CDF row index out of range (or a stream that is no multiple of its channels)')
    if st.any():
        raise L.PccError(f'pcc_rans_decode_batch: string {int(np.flatnonzero(st)[0])} is corrupt (status {L.PCC_ERR_CORRUPT})')


def rans_decode_batch(ctx, table, strings, n_list, index=None, index_mod=0, channels=0, out=None, check=True):
    """strings: list of bytes -> (out, status).  The headers are checked on the host, then ONE pinned buffer (offsets, lengths, counts,
    bytes) goes to the device on the current stream and one wave decodes each string into out[s] ((S, n_max) int32, or the caller's
    (S, ...) int32 device tensor).  index / index_mod / channels: as for rans_encode_launch.  check: wait and raise PccError (status
    PCC_ERR_CORRUPT) when a string did not decode; False: the flags stay in `status` (device int32) for rans_check_status."""
    S = len(strings)
    n_list = [int(k) for k in n_list]
    assert len(n_list) == S
    n_max = max(n_list) if out is None else (out[0].numel() if S else 0)
    if out is None:
        out = torch.zeros((S, n_max), dtype=torch.int32, device=ctx.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.device == ctx.device and out.shape[0] == S and all(k <= n_max for k in n_list)
    status = torch.zeros((S,), dtype=torch.int32, device=ctx.device)
    if S == 0:
        return out, status
    lens = np.fromiter((len(s_) for s_ in strings), np.int64, S)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    head = 16 * S
    host = torch.empty((head + total + 16,), dtype=torch.uint8, pin_memory=True)
    h = host.numpy()
    h[:8 * S].view(np.int64)[:] = offs
    h[8 * S:12 * S].view(np.int32)[:] = lens
    h[12 * S:16 * S].view(np.int32)[:] = n_list
    h[head:head + total] = np.frombuffer(b''.join(strings), np.uint8)
    h[head + total:] = 0
    base = h.ctypes.data
    L.check(L.lib().pcc_rans_check_strings(S, C.c_void_p(base + head), C.c_void_p(base), C.c_void_p(base + 8 * S), C.c_void_p(base + 12 * S)),
            'pcc_rans_check_strings')
    dev = host.to(ctx.device, non_blocking=True)
    idx, idx_stride = _rans_index(ctx, index, S, n_max)
    p = dev.data_ptr()
    st_host = np.zeros(S, np.int32) if check else None
    L.check(L.lib().pcc_rans_decode_batch(ctx.handle, C.byref(table.struct), S, C.c_void_p(p + head), total, C.c_void_p(p), C.c_void_p(p + 8 * S),
                                          _ptr(idx), idx_stride, index_mod, channels, C.c_void_p(p + 12 * S), n_max, _ptr(out), n_max,
                                          _ptr(status), None if st_host is None else st_host.ctypes.data_as(C.c_void_p), ctx.stream),
            'pcc_rans_decode_batch')
    return out, status
