"""The entropy coders (include/pcc_geo.h): the host range coder and its CDF tables, and the opt-in device rANS coder ("rans1")."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _ptr, _workspace


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


def _index_rows(index_list, shape, what):
    """The CDF rows of a 2-D fast path over `shape` = (streams, symbols): one row of indexes per stream (2-D) or ONE row shared by all
    streams (1-D) -> (uint64 address of every stream's row or None, bytes per index, the array to keep alive during the call)."""
    if index_list is None:
        return None, 4, None
    S, n_sym = shape
    i2 = _rows_2d(index_list, _ROW)
    if i2 is not None:
        assert i2.shape == shape, f'{what}: index rows {i2.shape} for symbols {shape}'
        return _row_ptrs(i2), i2.dtype.itemsize, i2
    keep = _np_host(index_list, _ROW)
    assert keep.ndim == 1 and keep.size == n_sym, f'{what}: shared index of {keep.size} rows for {n_sym} symbols'
    return np.full(S, keep.ctypes.data, np.uint64), keep.dtype.itemsize, keep


def range_encode_batch(table, data_list, index_list=None, index_mod=0, n_threads=0):
    """data_list: per-stream symbol arrays, int32 or int16 -- a list, or ONE 2-D (streams, symbols) array / CPU tensor (fast path: no
    per-stream Python work); index_list: per-stream CDF rows, int32 or uint8: a list, a 2-D array, or a single 1-D array shared by all
    streams.  Returns list of bytes."""
    d2 = _rows_2d(data_list, _SYM)
    if d2 is not None:
        S, n_sym = d2.shape
        if S == 0:
            return []
        ip, ib, keep = _index_rows(index_list, d2.shape, 'range_encode_batch')
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
        # a list of per-stream index arrays belongs to the legacy path below (flattened here it would decode every stream with stream
        # 0's rows)
        assert not isinstance(index_list, (list, tuple)), 'range_decode_batch: a 2-D `out` takes a 2-D (or one shared 1-D) index array'
        ip, ib, keep = _index_rows(index_list, o2.shape, 'range_decode_batch')
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
    cache = ctx.cache('rans_counts')
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
    ws = _workspace(ctx, int(L.lib().pcc_rans_workspace_bytes(S, n_max)) + 16)
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


# ---------------------------------------------------------------------------------------------
# device occupancy coder (the "occ1" string format, include/pcc_geo.h "occupancy coder (DEVICE)")
# ---------------------------------------------------------------------------------------------
def occ_stream_cap(n):
    return int(L.lib().pcc_occ_stream_cap(int(n)))


def _occ_grid(ctx, t, what):
    """(S, ...) fp32 device tensor whose rows are contiguous -> (streams, voxels per stream, elements between two rows)"""
    assert t.dtype == torch.float32 and t.device == ctx.device and t.dim() >= 2, f'{what}: an (S, ...) float32 tensor on the context\'s device'
    S = t.shape[0]
    n = t[0].numel() if S else 0
    assert S == 0 or t[0].is_contiguous(), f'{what}: the voxels of a block must be contiguous'
    stride = t.stride(0) if S > 1 else n
    assert stride >= n
    return S, n, stride


def occ_encode_launch(ctx, x_hat, occ, lanes=0):
    """Enqueues the encode of S blocks on the current stream.  x_hat, occ: (S, ...) float32 device tensors of the same shape, block s =
    row s flattened (rows may be further apart than their voxels: a slice of a larger tensor); occupied = occ != 0.  lanes: 0 = the
    lane rule.  Returns (out (S, cap) uint8, meta (2, S) int32: lengths, status) -- occ_encode_fetch(out, meta)."""
    S, n, xs = _occ_grid(ctx, x_hat, 'occ_encode_launch: x_hat')
    S2, n2, os_ = _occ_grid(ctx, occ, 'occ_encode_launch: occ')
    assert (S, n) == (S2, n2), f'occ_encode_launch: x_hat {tuple(x_hat.shape)} and occ {tuple(occ.shape)}'
    cap = occ_stream_cap(n)
    out = torch.empty((S, cap), dtype=torch.uint8, device=ctx.device)
    meta = torch.zeros((2, S), dtype=torch.int32, device=ctx.device)
    if S == 0 or n == 0:                            # (an empty block codes as b'': lengths 0, nothing to launch)
        return out, meta
    ws = _workspace(ctx, int(L.lib().pcc_occ_workspace_bytes(S, n)) + 16)
    L.check(L.lib().pcc_occ_encode_batch(ctx.handle, _ptr(x_hat), xs, _ptr(occ), os_, S, n, lanes, _ptr(out), cap, _ptr(meta[0]), _ptr(meta[1]),
                                         _ptr(ws), ws.numel(), ctx.stream), 'pcc_occ_encode_batch')
    return out, meta


def occ_encode_fetch(out, meta):
    """The strings of an occ_encode_launch: the lengths first, then only the used part of the byte buffer.  Waits for the device."""
    if out.shape[0] == 0:
        return []
    m = meta.cpu().numpy()
    if m[1].any():
        raise AssertionError('pcc_occ_encode_batch: bad voxel count')
    used = int(m[0].max())
    b = out[:, :used].cpu().numpy() if used else np.zeros((out.shape[0], 0), np.uint8)
    return [b[s, :int(m[0, s])].tobytes() for s in range(out.shape[0])]


def occ_encode_batch(ctx, x_hat, occ, lanes=0):
    """-> list of bytes (occ_encode_launch + occ_encode_fetch)"""
    return occ_encode_fetch(*occ_encode_launch(ctx, x_hat, occ, lanes))


def occ_check_status(status):
    """the per-stream flags of an occ_decode_batch(check=False), fetched now: raises like the checked call"""
    st = status.cpu().numpy()
    if (st & 4).any():
        raise AssertionError('pcc_occ_decode_batch: bad voxel count')
    if st.any():
        raise L.PccError(f'pcc_occ_decode_batch: string {int(np.flatnonzero(st)[0])} is corrupt (status {L.PCC_ERR_CORRUPT})')


def occ_decode_batch(ctx, x_hat, strings, out=None, check=True):
    """strings: list of bytes, one per row of x_hat ((S, ...) float32 device tensor, the decoder's own) -> (out, status).  The lane
    bytes and lengths are checked on the host, then ONE pinned buffer (offsets, lengths, bytes) goes to the device on the current
    stream and one workgroup decodes each string into out[s]: float32 0 / 1 of x_hat's shape (or the caller's tensor of that shape).
    check: wait and raise PccError (status PCC_ERR_CORRUPT) when a string did not decode; False: the flags stay in `status` (device
    int32) for occ_check_status."""
    S, n, xs = _occ_grid(ctx, x_hat, 'occ_decode_batch: x_hat')
    assert len(strings) == S
    if out is None:
        out = torch.empty(tuple(x_hat.shape), dtype=torch.float32, device=ctx.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.device == ctx.device and out.shape == x_hat.shape
    status = torch.zeros((S,), dtype=torch.int32, device=ctx.device)
    if S == 0:
        return out, status
    lens = np.fromiter((len(s_) for s_ in strings), np.int64, S)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    head = 12 * S + (-12 * S) % 16
    host = torch.empty((head + total + 16,), dtype=torch.uint8, pin_memory=True)
    h = host.numpy()
    h[:8 * S].view(np.int64)[:] = offs
    h[8 * S:12 * S].view(np.int32)[:] = lens
    h[head:head + total] = np.frombuffer(b''.join(strings), np.uint8)
    h[head + total:] = 0
    base = h.ctypes.data
    L.check(L.lib().pcc_occ_check_strings(S, C.c_void_p(base + head), C.c_void_p(base), C.c_void_p(base + 8 * S), n), 'pcc_occ_check_strings')
    if n == 0:                                      # (the check above took nothing but empty strings)
        return out, status
    dev = host.to(ctx.device, non_blocking=True)
    ws = _workspace(ctx, int(L.lib().pcc_occ_workspace_bytes(S, n)) + 16)
    p = dev.data_ptr()
    st_host = np.zeros(S, np.int32) if check else None
    L.check(L.lib().pcc_occ_decode_batch(ctx.handle, _ptr(x_hat), xs, S, n, C.c_void_p(p + head), total, C.c_void_p(p), C.c_void_p(p + 8 * S),
                                         _ptr(out), n, _ptr(status), None if st_host is None else st_host.ctypes.data_as(C.c_void_p),
                                         _ptr(ws), ws.numel(), ctx.stream), 'pcc_occ_decode_batch')
    return out, status
