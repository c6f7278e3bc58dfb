"""The context (one per process and GPU) and the helpers every other module of the package shares."""
import contextlib
import ctypes as C
import os

import torch

from .. import _lib as L


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

    def cache(self, name):
        """The dict this context keeps under `name`, created empty on first use.  A view hands out its base's, so what one of them
        caches the other finds."""
        return self.__dict__.setdefault('_caches', {}).setdefault(name, {})

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
        views = self.cache('views')
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

    def __getattr__(self, name):          # handle, device, num_cu, stream, workspace, cache, ...
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


def usable_cores():
    """Cores this process may use: the affinity mask capped by the cgroup CPU quota (cgroup v2 cpu.max, v1 cfs_quota_us).  A container
    that sees 256 cores may be throttled to 16 CPUs' worth of time per period: more threads than that get the whole process paused."""
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


def _workspace(ctx, nbytes, what=None):
    """The scratch of one call: nbytes uint8 on ctx.device, allocated with that device current.  hipCUB sizes its temporary storage
    for the current device, so a *_workspace_bytes query that asks hipCUB is passed as a callable and runs here, under the same
    guard.  what: the PccError message when the query answered 0, its word for an input outside the contract."""
    with torch.cuda.device(ctx.device):
        if callable(nbytes):
            nbytes = nbytes()
        if what is not None and nbytes == 0:
            raise L.PccError(what)
        return torch.empty((int(nbytes),), dtype=torch.uint8, device=ctx.device)


class _PairOverflow(L.PccError):
    """A tie-averaged D2 engine met more equidistant pairs than the stated capacity; `.pairs` is the capacity that suffices.  A
    subclass names in `_who` who needs them."""
    _who = ''

    def __init__(self, pairs, max_pairs):
        super().__init__(f'{self._who} needs {pairs} tie pairs, the workspace holds {max_pairs}; pass max_pairs >= {pairs}')
        self.pairs, self.max_pairs = int(pairs), int(max_pairs)
