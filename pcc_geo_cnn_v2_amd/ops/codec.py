"""The codec's device side (include/pcc_geo.h): symbol staging and packing, quantisers, the one-call encode / decode graphs,
thresholding and voxelisation."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _ptr, _workspace


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


# ---- the latent step: the stepped twins of the three fused kernels and the rate ladder.  q: (N,) uint8 device tensor,
# one ladder index (model_syntax.latent_step) per block; the caller has checked q <= 63.
def _steps(ctx, q, N):
    assert q.dtype == torch.uint8 and q.is_contiguous() and q.device == ctx.device and q.numel() == N, \
        'latent steps: one uint8 ladder index per block, on the context\'s device'
    return _ptr(q)


def quantize_step_pack(ctx, v, medians, mode, channels_first, dst_ptr, dst_bytes, q, tile_max_ptr=None, want_deq=True, sym=None, deq=None):
    """quantize_pack on v / step(q[n]) with deq = float(sym) * step(q[n]) (+ medians) (pcc_quantize_step_pack).  dst_ptr None: no packed copy."""
    assert v.dtype == torch.float32 and v.is_contiguous() and v.device == ctx.device
    N, Cc = v.shape[0], v.shape[-1]
    sym = _out(sym, v.shape, torch.int32, v)
    deq = _out(deq, v.shape, torch.float32, v) if want_deq else None
    L.check(L.lib().pcc_quantize_step_pack(ctx.handle, _ptr(v), _ptr(medians), _ptr(sym), _ptr(deq), N, v[0].numel() // Cc, Cc, mode,
                                           int(bool(channels_first)), C.c_void_p(dst_ptr), dst_bytes,
                                           None if tile_max_ptr is None else C.c_void_p(tile_max_ptr), _steps(ctx, q, N), ctx.stream),
            'pcc_quantize_step_pack')
    return sym, deq


def index_pack_step(ctx, sigma, table, channels_first, dst_ptr, dst_bytes, q, idx=None):
    """index_pack on sigma / step(q[n]) (pcc_index_pack_step).  dst_ptr None: no packed copy."""
    assert sigma.dtype == torch.float32 and sigma.is_contiguous() and sigma.device == ctx.device and table.dtype == torch.float32
    N, Cc = sigma.shape[0], sigma.shape[-1]
    idx = _out(idx, sigma.shape, torch.int32, sigma)
    L.check(L.lib().pcc_index_pack_step(ctx.handle, _ptr(sigma), _ptr(table), table.numel(), _ptr(idx), N, sigma[0].numel() // Cc, Cc,
                                        int(bool(channels_first)), C.c_void_p(dst_ptr), dst_bytes, _steps(ctx, q, N), ctx.stream),
            'pcc_index_pack_step')
    return idx


def unpack_dequantize_step(ctx, src, ndhwc_shape, channels_first, q, medians=None, sym=None, deq=None):
    """unpack_dequantize with deq = float(sym) * step(q[n]) (+ medians) (pcc_unpack_dequantize_step)."""
    assert src.is_contiguous() and src.device == ctx.device and src.dtype in _ITEM
    sym = _out(sym, ndhwc_shape, torch.int32, src)
    deq = _out(deq, ndhwc_shape, torch.float32, src)
    N, Cc = sym.shape[0], sym.shape[-1]
    assert src.numel() == sym.numel()
    L.check(L.lib().pcc_unpack_dequantize_step(ctx.handle, _ptr(src), _ITEM[src.dtype], N, sym[0].numel() // Cc, Cc,
                                               int(bool(channels_first)), _ptr(sym), _ptr(medians), _ptr(deq), _steps(ctx, q, N), ctx.stream),
            'pcc_unpack_dequantize_step')
    return sym, deq


def cost16_table(cdf, cdf_size, precision=16):
    """Host: cost16[row][b] = rint(65536 * (precision - log2(cdf[b + 1] - cdf[b]))) in float64, as uint32 (rows, stride - 1); bins a row
    does not have stay 0.  A zero frequency is an AssertionError."""
    cdf, cdf_size = np.asarray(cdf, np.int64), np.asarray(cdf_size, np.int64)
    assert cdf.ndim == 2 and cdf_size.shape == (cdf.shape[0],) and cdf.shape[1] >= 2
    cost = np.zeros((cdf.shape[0], cdf.shape[1] - 1), np.uint32)
    for r, sz in enumerate(cdf_size.tolist()):
        assert 2 <= sz <= cdf.shape[1], f'cost table: row {r} has cdf_size {sz} for a stride of {cdf.shape[1]}'
        freq = np.diff(cdf[r, :sz])
        assert np.all(freq > 0), f'cost table: row {r} has a bin of frequency {int(freq.min())}: its cost would be infinite'
        cost[r, :sz - 1] = np.rint(65536.0 * (np.float64(precision) - np.log2(freq.astype(np.float64)))).astype(np.uint32)
    return cost


def device_cost_table(ctx, table):
    """The cost table of a coders.HostCdfTable on the context's device, built and uploaded once per (context, table) and kept -- like the
    rANS coder keeps its CDF tables; a table whose arrays were rebuilt in place is uploaded again.  -> (cost16, offset, cdf_size)."""
    cache = ctx.cache('cost16')
    e = cache.get(id(table))
    if e is None or e[0] is not table or not (np.array_equal(e[1], table.cdf) and np.array_equal(e[2], table.cdf_size) and np.array_equal(e[3], table.offset)):
        cost = cost16_table(table.cdf, table.cdf_size, table.struct.precision)
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in (cost.view(np.int32), table.offset, table.cdf_size))
        cache[id(table)] = e = (table, table.cdf.copy(), table.cdf_size.copy(), table.offset.copy(), dev)      # (the table stays alive: its id is the key)
    return e[4]


def rate_ladder(ctx, y, sigma, steps, scale_table, cdf_table, mode=L.PCC_ROUND_FLOOR_HALF, groups_per_block=0):
    """The exact size of every block's y string under every step of a ladder (pcc_rate_ladder): y, sigma (N, ..., C) float32 on the device,
    steps: 1 to 64 ladder indexes (host), scale_table: float32 device tensor, cdf_table: the coders.HostCdfTable whose rows the scale
    table selects.  -> int64 (N, J) device tensor in units of 2^-16 bit.  groups_per_block: launch geometry, no effect on the result."""
    assert y.dtype == torch.float32 and y.is_contiguous() and y.device == ctx.device and sigma.dtype == torch.float32 and sigma.is_contiguous()
    assert sigma.shape == y.shape and sigma.device == ctx.device and scale_table.dtype == torch.float32
    steps = np.ascontiguousarray(np.asarray(steps).reshape(-1))
    assert 1 <= steps.size <= 64 and np.issubdtype(steps.dtype, np.integer) and steps.min() >= 0 and steps.max() <= 63, \
        'rate_ladder: a ladder of 1 to 64 indexes in [0, 63]'
    steps = steps.astype(np.uint8)
    assert cdf_table.cdf.shape[0] == scale_table.numel(), 'rate_ladder: one CDF row per scale table entry'
    cost, offset, size = device_cost_table(ctx, cdf_table)
    N, Cc = y.shape[0], y.shape[-1]
    out = torch.empty((N, steps.size), dtype=torch.int64, device=ctx.device)
    L.check(L.lib().pcc_rate_ladder(ctx.handle, _ptr(y), _ptr(sigma), N, y[0].numel() // Cc, Cc, _ptr(scale_table), scale_table.numel(), mode,
                                    steps.ctypes.data_as(C.c_void_p), steps.size, _ptr(cost), cost.shape[1], _ptr(offset), _ptr(size),
                                    cdf_table.struct.overflow_width, int(groups_per_block), _ptr(out), ctx.stream), 'pcc_rate_ladder')
    return out


def _threshold_outputs(ctx, t, thr, cap, scratch, N, D, H, W):
    """What a codec call that also thresholds and compacts needs (`thr` (N,) float32 given): the point lists xyz (N,cap,3) and counts
    (N,), entered into the result dict t, and the compaction scratch, the caller's or a fresh one.  Returns (xyz, counts, cap,
    scratch), xyz and counts None without thr."""
    cap = D * H * W if cap is None else int(cap)
    if thr is None:
        return None, None, cap, scratch
    assert thr.dtype == torch.float32 and thr.numel() == N
    dev = ctx.device
    xyz, counts = torch.empty((N, cap, 3), dtype=torch.float32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
    n_scratch = L.lib().pcc_threshold_scratch_ints(N, D, H, W)
    if scratch is None:
        scratch = torch.empty((n_scratch,), dtype=torch.int32, device=dev)
    assert scratch.dtype == torch.int32 and scratch.numel() >= n_scratch and scratch.device == dev
    t.update(xyz=xyz, counts=counts)
    return xyz, counts, cap, scratch


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
    xyz, counts, cap, scratch = _threshold_outputs(ctx, t, thr, cap, scratch, N, D, H, W)
    ws = ctx.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), N, D, H, W))
    L.check(L.lib().pcc_codec_encode(ctx.handle, C.byref(desc), _ptr(x), N, D, H, W, _ptr(t['y']), _ptr(t.get('z')),
                                     _ptr(t.get('z_symbols')), _ptr(t.get('z_hat')), _ptr(t.get('sigma_hat')),
                                     _ptr(t.get('indexes')), _ptr(t['symbols']), _ptr(t['y_hat']), _ptr(t['x_hat']), _ptr(thr),
                                     _ptr(xyz), _ptr(counts), cap, _ptr(scratch), _ptr(ws), ws.numel(),
                                     ctx.conv_flags, 0, None if staging is None else C.byref(staging.sink()),
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
                                           _ptr(t['indexes']), _ptr(ws), ws.numel(), ctx.conv_flags,
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
    xyz, counts, cap, scratch = _threshold_outputs(ctx, t, thr, cap, scratch, N, D, H, W)
    ws = ctx.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), N, D, H, W))
    L.check(L.lib().pcc_codec_decode_main(ctx.handle, C.byref(desc), _ptr(ysym), N, D, H, W, _ptr(t['y_hat']), _ptr(t['x_hat']),
                                          _ptr(thr), _ptr(xyz), _ptr(counts), cap, _ptr(scratch), _ptr(ws), ws.numel(),
                                          ctx.conv_flags, None if io is None else C.byref(io), ctx.stream),
            'pcc_codec_decode_main')
    return t


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


def topk_compact(ctx, x, k, cap=None):
    """Count-matched thresholding (include/pcc_geo.h "top-k selection"): block b keeps its k[b] highest-scoring voxels
    (scores <= 0 never; ties at the cut to the lowest voxel index).  x: (B,D,H,W) float32 on the context's device, each block contiguous,
    blocks at least D*H*W elements apart (a slice of a wider buffer is fine); k: (B,) int32 device tensor.  Returns (xyz (B,cap,3),
    counts (B,)) like threshold_compact: points in voxel order, counts[b] = min(max(k[b], 0), positive voxels of b)."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.device == ctx.device, 'topk_compact: x is a (B,D,H,W) float32 tensor on the context\'s device'
    B, D, H, W = x.shape
    n = D * H * W
    assert B == 0 or n == 0 or x[0].is_contiguous(), 'topk_compact: the voxels of a block must be contiguous'
    stride = x.stride(0) if B > 1 and n > 0 else n
    assert stride >= n, 'topk_compact: blocks overlap'
    assert k.dtype == torch.int32 and tuple(k.shape) == (B,) and k.is_contiguous() and k.device == ctx.device, \
        'topk_compact: k is a (B,) int32 tensor on the context\'s device'
    cap = n if cap is None else int(cap)
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device=x.device)
    counts = torch.zeros((B,), dtype=torch.int32, device=x.device)
    if B == 0 or n == 0:
        return xyz, counts
    ws = _workspace(ctx, int(L.lib().pcc_topk_workspace_bytes(B, n)), 'topk_compact: more than 2^28 voxels per block')
    L.check(L.lib().pcc_topk_compact(ctx.handle, _ptr(x), stride, B, D, H, W, _ptr(k), _ptr(xyz), _ptr(counts), cap, _ptr(ws), ws.numel(),
                                     ctx.stream), 'pcc_topk_compact')
    return xyz, counts


def voxelize(ctx, pts, block_of, B, D, H, W):
    """pts (n,3) int32, block_of (n,) int32 (device) -> dense (B,D,H,W) float32 of {0,1}."""
    assert pts.dtype == torch.int32 and pts.dim() == 2 and pts.shape[1] == 3, 'voxelize: pts is an (n, 3) int32 tensor'
    assert pts.is_contiguous() and pts.device == ctx.device, 'voxelize: pts is contiguous and on the context\'s device'
    assert block_of.dtype == torch.int32 and tuple(block_of.shape) == (pts.shape[0],), 'voxelize: block_of is an (n,) int32 tensor'
    assert block_of.is_contiguous() and block_of.device == ctx.device, 'voxelize: block_of is contiguous and on the context\'s device'
    dense = torch.zeros((B, D, H, W), dtype=torch.float32, device=ctx.device)
    if pts.numel():
        L.check(L.lib().pcc_voxelize(ctx.handle, _ptr(pts), _ptr(block_of), pts.shape[0], B, D, H, W, _ptr(dense),
                                     ctx.stream), 'pcc_voxelize')
    return dense
