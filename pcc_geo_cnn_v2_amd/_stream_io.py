"""Host <-> device plumbing of the codec's block loops (model_types.py): pinned staging buffers, the copy streams beside the main
one, and the copies that run there.  Nothing here knows a model; every function takes the ops.Context it works on."""
import os
from contextlib import contextmanager

import numpy as np
import torch

_SIDE_STREAMS = {}


class _Immediate:
    """A future-like wrapper that runs its function when the result is asked for (the caller's thread)."""

    def __init__(self, fn):
        self.fn = fn

    def result(self):
        return self.fn()


def _host_dtypes(levels=64):
    """(symbol dtype, CDF-row dtype) of the host staging buffers: int16 / uint8 (uint8 rows cover scale tables of up to 256
    levels; larger tables keep int32 rows); PCC_WIDE_SYMBOLS=1 keeps int32 for both (A/B runs)."""
    if os.environ.get('PCC_WIDE_SYMBOLS'):
        return torch.int32, torch.int32
    return torch.int16, (torch.uint8 if levels <= 256 else torch.int32)


class _Pinned:
    """Cache of pinned host staging buffers keyed by (tag, shape, dtype)."""

    def __init__(self):
        self._b = {}
        self._rings = {}

    def get(self, tag, shape, dtype):
        key = (tag, tuple(shape), dtype)
        if key not in self._b:
            self._b[key] = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
        return self._b[key]

    def ring(self, tag, shape, dtype, depth=4):
        """Next buffer of a ring of `depth` pinned buffers (the decoder's staging buffers: a chunk's buffer is still the source
        of an asynchronous host->device copy while the host already fills the next chunk's).  Returns (buffer, release):
        call release(stream) after enqueuing the last device operation that reads the buffer; the ring waits for that event
        before it hands the buffer out again -- no pinned allocation (a device-synchronising call) in the steady state."""
        key = (tag, tuple(shape), dtype)
        r = self._rings.setdefault(key, {'next': 0, 'buf': [None] * depth, 'busy': [None] * depth})
        i = r['next']
        r['next'] = (i + 1) % depth
        if r['busy'][i] is not None:
            r['busy'][i].synchronize()
            r['busy'][i] = None
        if r['buf'][i] is None:
            r['buf'][i] = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)

        def release(stream):
            ev = torch.cuda.Event()
            ev.record(stream)
            r['busy'][i] = ev
        return r['buf'][i], release


def side_stream(ctx, which='_copy_stream'):
    """Copy streams beside the main one.  Work on one stream runs in order, so copies with different dependencies get
    different streams: '_copy_stream' (encoder symbols and decoded points to the host: each waits for an event of the main
    stream), '_up_stream' (decoder symbols to the device: no GPU-side dependency, they run as soon as the host has decoded
    them), '_idx_stream' (the decoder's CDF-row indexes to the host)."""
    # one set per device for the whole process (streams are a runtime resource: every model on the device shares them)
    key = (ctx.device.index, which)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(ctx.device)
    return _SIDE_STREAMS[key]


@contextmanager
def on_side_stream(ctx, which='_copy_stream', after=None):
    """The body runs with side stream `which` current, behind `after`: an event (default: one recorded now on the main stream),
    or False when the work depends on nothing the GPU does.  Yields the stream; `stream.record_event()` at the end of the body
    is the event whoever needs the results waits for."""
    side = side_stream(ctx, which)
    if after is None:
        after = torch.cuda.Event()
        after.record(torch.cuda.current_stream(ctx.device))
    with torch.cuda.stream(side):
        if after is not False:
            side.wait_event(after)
        yield side


def ship(ctx, staging, ready=None):
    """ONE device->pinned-host copy of a packed staging buffer on the side stream (no kernel runs there: the permutation
    into stream order, the narrowing and the max|symbol| tiles were written in order on the main stream by the library);
    returns the event the host has to wait for.  `ready`: event after which the staging buffer is final (default: now,
    on the main stream)."""
    with on_side_stream(ctx, after=ready) as side:
        staging.copy_out()
        return side.record_event()


def symbols_to_device(ctx, sym_host, release):
    """Stream-order host symbols -> the device, as they are (one host->device copy of the narrow integers: half the PCIe
    bytes of int32).  The copy runs on the SIDE stream -- a copy on the main stream would hold back every kernel queued
    behind it for its 20-60 us, and the decoder calls of a chunk are enqueued long before the GPU gets to them -- on a
    stream of their own (nothing there ever waits for the GPU), and the main stream only waits for the copy's event.  The
    library unpacks the symbols into the int32 (B,D,H,W,C) tensor inside the decoder call (pcc_symbol_io); the per-layer path
    calls ops.symbols_unpack."""
    main = torch.cuda.current_stream(ctx.device)
    with on_side_stream(ctx, '_up_stream', after=False) as side:
        dev = sym_host.to(ctx.device, non_blocking=True)
        release(side)
        arrived = side.record_event()
    main.wait_event(arrived)
    dev.record_stream(main)
    return dev


def indexes_to_host(ctx, idx_dev, idx_host):
    """The decoder's packed CDF-row indexes -> a pinned buffer, behind everything queued on the main stream so far; returns the
    event the host waits for."""
    with on_side_stream(ctx, '_idx_stream') as side:      # (not on the main stream: the copy would delay the kernels queued behind it)
        idx_dev.record_stream(side)
        idx_host.copy_(idx_dev, non_blocking=True)
        return side.record_event()


def to_host(ctx, ready, *tensors):
    """Blocking copies of small device tensors to numpy arrays, on the side stream behind `ready`: never a blocking copy on the
    main stream."""
    with on_side_stream(ctx, after=ready) as side:
        for t in tensors:
            t.record_stream(side)
        return [t.cpu().numpy() for t in tensors]


def gather_points(xyz, counts, ctx=None, ready=None):
    """Point lists to the host.  When `ready` (an event recorded after the compaction kernels) is given, the
    copies run on the side stream and wait only for that event, so the host never drains the main queue."""
    def fetch():
        cnt = counts.cpu().numpy()
        parts = [xyz[b, :int(cnt[b])] for b in range(len(cnt))]
        return cnt, (torch.cat(parts).cpu().numpy() if len(parts) else np.zeros((0, 3), np.float32))

    if ready is None or ctx is None:
        cnt, flat = fetch()
    else:
        with on_side_stream(ctx, after=ready) as side:
            xyz.record_stream(side)
            counts.record_stream(side)
            cnt, flat = fetch()
    out, p = [], 0
    for n in cnt:
        out.append(flat[p:p + int(n)].copy())
        p += int(n)
    return out
