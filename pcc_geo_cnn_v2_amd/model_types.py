"""Compression models -- the interface of /root/reference/src/model_types.py:179-416
(CompressionModel / CompressionModelV1 / CompressionModelV2: compress(), decompress(),
compress_blocks(), decompress_blocks()) on top of the HIP kernels.

MI355X-first differences (results identical):
  * blocks are processed `batch_size` at a time, resident in HBM, instead of one sess.run per block
    (reference: model_types.py:192-198,224-230);
  * sparse_to_dense, thresholding and np.argwhere run on the GPU (voxelize / threshold_compact);
  * the range coder runs on host threads, one stream per block, overlapped with the synthesis
    transform of the same (encoder) or previous (decoder) chunk;
  * the encoder obtains z_hat / y_hat from the quantiser directly instead of range-decoding the
    string it just produced (model_types.py:383,387): the values are identical by construction.
`sess` in the reference's signatures is an `ops.Context` here (None = the default GPU context).
Here: the whole-cloud selection, the models, their batch graph and the block loops of one process.  Beside it: _stream_io.py (pinned
buffers, copy streams and the copies on them), block_search.py (the schedule of the adaptive threshold search), sharded_blocks.py (the
block loops over the ranks of torch.distributed), stream_layers.py (the layers a stream carries behind the y/z strings and their place
in a block's strings; which options of an encode exclude each other: `plan_encode`, asked by both encoder entry points).
"""
import logging
import os
import pprint
import sys
import time
from enum import Enum

import numpy as np
import torch
from scipy.spatial import cKDTree

from . import _lib as L
from . import model_transforms as MT
from . import ops
from .entropy_models import EntropyBottleneck, GaussianConditional, scale_table
from ._stream_io import _Immediate, _Pinned, _host_dtypes, gather_points, indexes_to_host, on_side_stream, ship, side_stream, symbols_to_device, to_host
from .block_search import SearchSchedule
from . import stream_layers as SL
from .model_opt import count_rows, count_tallies_gpu, d2_on_gpu, decide_counts_from_tallies
from .model_transforms import TransformType
from .utils.octree_coding import departition_octree
from .utils.pc_metric import cloud_metrics_batch, cloud_metrics_batch_gpu, wants_hausdorff

logger = logging.getLogger(__name__)

CHECKPOINT_FILE = 'model.npz'


def sparse_to_dense(block, x_shape, data_format):
    """Host version of the dense occupancy scatter (model_types.py:108-114), kept for API parity and as the test oracle of
    ops.voxelize, which the codec uses.  x_shape is the 5-D shape of ONE block in `data_format`."""
    assert data_format in ('channels_first', 'channels_last')
    grid = np.zeros(x_shape, dtype=np.float32)
    occupancy = grid[0, 0] if data_format == 'channels_first' else grid[0, ..., 0]      # (D, H, W) view of the single channel
    occupancy[tuple(np.asarray(block)[:, :3].astype(np.uint32).T)] = 1.0                 # out-of-range coordinate: IndexError
    return grid


def get_normals_if(x, with_normals):
    return x[:, x.shape[1] - 3:x.shape[1]] if with_normals else None


def rank_candidates(names, cand_metrics, opt_groups=('d1', 'd2')):
    """The selection rule of model_types.py:128-176 on already-computed metrics: per optimisation group ('d1', 'd2') the
    candidate -- among those whose metric name starts with the group -- with the highest '{group}_psnr'; an empty decoded
    cloud (metrics None) scores -inf.  Returns [(group, winning candidate index, its metrics)].  Shared by the single-process
    and the sharded encoder (the latter feeds all_reduce'd metrics, so every rank takes the same decision)."""
    picks = []
    for group in opt_groups:
        members = [i for i, n in enumerate(names) if n.startswith(group)]
        if not members:
            continue
        key = f'{group}_psnr'
        score = {i: (-np.inf if cand_metrics[i] is None else cand_metrics[i][key]) for i in members}
        winner = members[int(np.argmax([score[i] for i in members]))]
        picks.append((group, winner, cand_metrics[winner] if cand_metrics[winner] is not None else {key: -np.inf}))
        logger.info(f'Group {group} : {key} best idx {winner} {names[winner]}\n' +
                    pprint.pformat({names[i]: f'{score[i]:.2f}' for i in members}))
    return picks


def select_best_per_opt_metric(binstr, x_hat_list, level, opt_metrics, points, resolution, with_normals,
                               opt_groups=('d1', 'd2'), tree=None, metrics_device='host', ctx=None, d2_ties='pick', hausdorff=False):
    """Per optimisation group, which candidate reconstruction of the whole cloud to keep (the reference's function of the same
    name, model_types.py:128-176; results pinned by tests/golden/select_best.npz).  x_hat_list[m] = the decoded blocks of
    candidate m (block-local coordinates).  Returns one dict per non-empty group: 'idx', 'metrics', 'x_hat_list',
    'blocks_depart' (blocks in cloud coordinates), 'blocks_full' (one array).  metrics_device='gpu': the whole-cloud metrics come
    from pc_metric.cloud_metrics_batch_gpu on context `ctx` (neighbour ties to the lowest row) instead of the KD-trees.
    d2_ties='mean': either engine averages D2 over all equidistant nearest points (pc_metric.tie_mean_tally).
    hausdorff=True (a Hausdorff opt metric was named; single process): every 'metrics' also carries pc_metric.hausdorff_table's keys, from
    the 9-slot whole-cloud tally of the same engine (cloud_tallies_gpu / cloud_tally_host: the same neighbour links, so the other keys
    keep their values); the ranking is unchanged."""
    if metrics_device not in SL.METRICS_DEVICES:
        raise AssertionError(f'metrics_device must be one of {SL.METRICS_DEVICES}, got {metrics_device!r}')
    assert len(opt_metrics) == len(x_hat_list), f'lengths of opt_metrics {len(opt_metrics)} and x_hat_list' + \
                                                f' {len(x_hat_list)} should be equal'
    grouped = [m for m, n in enumerate(opt_metrics) if any(n.startswith(g) for g in opt_groups)]
    placed = {m: departition_octree(x_hat_list[m], binstr, [0, 0, 0], [resolution] * 3, level) for m in grouped}
    clouds = {m: np.vstack(placed[m]) for m in grouped}
    original = points[:, :3]
    # `tree`: the KD-tree over the original points when the caller built it meanwhile (compress_blocks: beside the block loop)
    if hausdorff:
        from .utils import pc_metric as PM
        normals, peak = get_normals_if(points, with_normals), resolution - 1
        if metrics_device == 'gpu':
            from . import ops
            tallies = PM.cloud_tallies_gpu(ctx if ctx is not None else ops.get_context(), original, [clouds[m] for m in grouped], normals, ties=d2_ties)
        else:
            tree = tree if tree is not None else cKDTree(original)
            tallies = [PM.cloud_tally_host(original, clouds[m], normals, t1=tree, ties=d2_ties) if len(clouds[m]) else None for m in grouped]
        scored = [None if t is None else dict(PM.metrics_table(len(original), t[:5], peak, PM.GROUPS if with_normals else PM.GROUPS[:1]),
                                              **PM.hausdorff_table(t, peak, with_normals)) for t in tallies]
    elif metrics_device == 'gpu':
        from . import ops
        scored = cloud_metrics_batch_gpu(ctx if ctx is not None else ops.get_context(), original, [clouds[m] for m in grouped],
                                         resolution - 1, get_normals_if(points, with_normals), ties=d2_ties)
    else:
        scored = cloud_metrics_batch(original, [clouds[m] for m in grouped], resolution - 1, get_normals_if(points, with_normals),
                                     tree if tree is not None else cKDTree(original), ties=d2_ties)
    cand_metrics = [None] * len(opt_metrics)
    for m, met in zip(grouped, scored):
        cand_metrics[m] = met
    return [{'idx': m, 'metrics': met, 'x_hat_list': x_hat_list[m], 'blocks_depart': placed[m], 'blocks_full': clouds[m]}
            for _, m, met in rank_candidates(opt_metrics, cand_metrics, opt_groups)]


ENTROPY_CODERS = ('range', 'rans')


def block_count(n_rows, count_scale, n_voxels):
    """Count-matched thresholding: how many voxels the decoder keeps of a block with `n_rows` input rows under the scale
    rho = `count_scale`: min(n_voxels, floor(rho * n_rows + 0.5)), in float64."""
    return int(min(np.float64(n_voxels), np.floor(np.float64(count_scale) * np.float64(n_rows) + 0.5)))


# The margin of the rate target's prediction, in units of 2^-16 bit.  The host range coder's string is longer than the
# cost model's sum: it never writes fewer than two bytes and its termination depends on the final range state (16.000 bits measured on a
# one-symbol stream, plus 8), and its interval arithmetic truncates, which costs in proportion to the bits coded (largest ratio measured:
# 938.2 parts per million, 32768 symbols that mostly sit on frequency-1 bins of the four narrowest rows; rounded up here).  Both figures
# are MEASURED on seeded streams (tests/test_latent_step_cpu.py holds them against the real coder), not proven bounds.
RATE_MARGIN_FIXED_BITS = 24
RATE_MARGIN_PPM = 939


def rate_margin_bits16(bits16):
    """What choose_latent_step adds to a block's predicted y bits before it rounds them up to bytes (int64 array or int, units of 2^-16 bit)."""
    return (RATE_MARGIN_FIXED_BITS << 16) + (bits16 * RATE_MARGIN_PPM + 999999) // 1000000


def _np(t):
    return t.detach().cpu().numpy()


def _debug_dicts(B, debug, tensors, keys):
    """Per block the device tensors `keys` of `tensors` as numpy arrays (batch dimension kept; x_hat with its channel axis), or None per
    block without `debug`."""
    if not debug:
        return [None] * B
    return [{k: _np((tensors[k].unsqueeze(-1) if k == 'x_hat' else tensors[k])[b:b + 1]) for k in keys} for b in range(B)]


class CompressionModel:
    """What V1 and V2 share: the block loops and the structure of the batch graph.  A subclass states, as data: `n_strings` (strings per
    block, without the occupancy layer), `codec_abi` (the version of the batched-graph ABI), `encode_debug_keys` / `decode_debug_keys`;
    and, as methods, its transforms and entropy models and the steps of the batch graph that differ (`_analysis_layerwise`,
    `_string_jobs`, `_decode_phase_a`, `_decode_phase_b_host`, `_y_rans_decode`, `_y_medians`)."""
    n_strings = codec_abi = None
    encode_debug_keys = decode_debug_keys = ()

    def __init__(self, n_thresholds=2 ** 8, data_format='channels_first', batch_size=32,
                 round_mode=L.PCC_ROUND_FLOOR_HALF, coder_threads=0, seed=42, precision='fp32', search_threads=0,
                 entropy_coder='range', lossless=False):
        assert precision in ('fp32', 'fp16'), "precision: 'fp32' (the reference's arithmetic) or 'fp16' (fp16 matrix instructions, fp32 accumulate)"
        assert entropy_coder in ENTROPY_CODERS, f"entropy_coder: 'range' (the host range coder, tfc's bytes) or 'rans' (the device coder), not {entropy_coder!r}"
        # which string format compress() writes and decompress() reads: part of the stream (the CLIs record it in the numerics tag)
        self.entropy_coder = entropy_coder
        # lossless: every block carries one more string, LAST, that codes its true occupancy under the decoder's x_hat ("occ1", DESIGN.md
        # 4.19); the y/z strings and the threshold byte in front of it are what they are without it.  The CLIs name the layer in the tag.
        self.lossless = bool(lossless)
        self.precision = precision
        self.thresholds = np.linspace(0, 1.0, n_thresholds)
        self.data_format = data_format
        self.batch_size = int(batch_size)
        self.round_mode = round_mode
        self.coder_threads = coder_threads
        self.search_threads = search_threads      # worker processes of the host KD-tree threshold search (0 = min(cores, 64))
        self.seed = seed
        self.x_shape = None
        # the adaptive threshold search (block_search.py): set by the CLIs' --search_ties / --d2_search
        self.search_ties = 'pick'
        self.d2_search = None                     # None: model_opt.D2_SEARCH, then the environment (model_opt.d2_on_gpu)
        # ... and what it counts: blocks handed to the host pool, the kind of the last ones, A->B trees built / level sets ('tally_pruned')
        self.host_search_jobs = self.search_trees_built = self.search_trees_total = 0
        self.last_host_job_kind = None
        self._host_search_pool = None
        self._helper_pools = {}
        self._pinned = _Pinned()
        self._dev_cache = {}
        self._host_cache = {}
        self._stagings = {}
        self._codec_cache = (None,)

    # ------------------------------------------------------------------ helpers
    def _bind_transforms(self, **kinds):
        """`<kind>_transform_class` from the TransformType members of the ctor; `<kind>_transform` (the instance) is created by
        compress() / decompress()."""
        for kind, member in kinds.items():
            setattr(self, f'{kind}_transform_class', member.value)
            setattr(self, f'{kind}_transform', None)

    def _ctx(self, sess):
        ctx = sess if isinstance(sess, (ops.Context, ops._ContextView)) else ops.get_context(None)
        # BASELINE.json configs[4]: the fp16 mode.  Encoder and decoder must agree on it (the decoder recomputes sigma_hat):
        # like the checkpoint, it is part of the codec configuration, not of the stream.  A VIEW of the context carries the
        # flag: the caller's context is not modified.
        return ctx.view(L.PCC_CONV_F16 if self.precision == 'fp16' else 0)

    def _dev(self, ctx, name, arr):
        key = (ctx.device.index, name)
        if key not in self._dev_cache:
            self._dev_cache[key] = torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device)
        return self._dev_cache[key]

    def _spatial(self, x_shape):
        x_shape = [int(v) for v in x_shape]
        if len(x_shape) == 3:
            return tuple(x_shape)
        assert len(x_shape) == 5
        return tuple(x_shape[2:5]) if self.data_format == 'channels_first' else tuple(x_shape[1:4])

    def _staging(self, ctx, slot, B, y_dhw, z_dhw=None):
        """Per pipeline slot: the device + pinned staging buffers of one encode (ops.SymbolStaging), cached."""
        sym_t, row_t = _host_dtypes(len(getattr(self, 'scale_table', ())) or 64)
        F = self.num_filters
        key = (ctx.device.index, slot, B, tuple(y_dhw), None if z_dhw is None else tuple(z_dhw), sym_t, self.data_format)
        if key not in self._stagings:
            self._stagings[key] = ops.SymbolStaging(ctx.device, B, self._stream_shape(B, y_dhw, F),
                                                    None if z_dhw is None else self._stream_shape(B, z_dhw, F), F, sym_t, row_t,
                                                    self.data_format == 'channels_first')
        return self._stagings[key]

    # ---- symbol order of the range-coded streams.  tfc 1.3 codes each batch item's tensor flattened in ITS memory order:
    # with the reference's default data_format='channels_first' (model_types.py:180,254,377) that is (C,D,H,W), i.e.
    # channel-major streams; 'channels_last' gives (D,H,W,C).  Internally everything is NDHWC, so for channels_first the
    # int32 symbols / indexes are permuted on the GPU before they leave (and after they come back).
    def _to_stream_order(self, t):
        """(B,D,H,W,C) device tensor -> contiguous tensor in the stream's flattening order."""
        return t.permute(0, 4, 1, 2, 3).contiguous() if self.data_format == 'channels_first' else t

    def _from_stream_order(self, t):
        """inverse of _to_stream_order: returns (B,D,H,W,C) contiguous."""
        return t.permute(0, 2, 3, 4, 1).contiguous() if self.data_format == 'channels_first' else t

    def _stream_shape(self, B, dhw, C):
        return (B, C) + tuple(dhw) if self.data_format == 'channels_first' else (B,) + tuple(dhw) + (C,)

    def _eb_rows(self, n_per_block, C):
        """EntropyBottleneck CDF row (= channel) of every symbol of one stream: (index_list, index_mod) for the range coder."""
        if self.data_format != 'channels_first':
            return None, C                          # row = i % C
        key = ('eb_rows', n_per_block, C)
        if key not in self._host_cache:
            self._host_cache[key] = np.repeat(np.arange(C, dtype=np.int32), n_per_block // C)
        return self._host_cache[key], 0

    def _thr32(self, idx):
        # the reference compares float32 x_hat with a float64 scalar under numpy 1.18 value-based
        # casting, i.e. in float32
        return np.float32(self.thresholds[idx])

    def _voxelize(self, ctx, blocks, dhw):
        D, H, W = dhw
        B = len(blocks)
        pts = np.ascontiguousarray(np.concatenate([np.asarray(b)[:, :3] for b in blocks]).astype(np.uint32).astype(np.int32))
        # the reference's dense scatter raises IndexError on an out-of-range coordinate (model_types.py:108-114)
        assert pts.size == 0 or (pts.min() >= 0 and np.all(pts.max(0) < np.array(dhw))), \
            f'block-local coordinates outside the {dhw} grid'
        bof = np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(blocks)])
        return ops.voxelize(ctx, torch.from_numpy(pts).to(ctx.device), torch.from_numpy(bof).to(ctx.device), B, D, H, W)

    def _search_pool(self, n_jobs):
        from .model_opt import HostSearchPool
        # default: the cores this process may run on, at most 64 (measured on a 256-thread box whose container gets far fewer: 64
        # workers 17.5 s per 190-block cloud with d2 metrics, 128 workers 23.6 s -- the KD-tree work is host-bound)
        usable = ops.usable_cores() * 4          # (KD-tree queries wait on memory: 64 workers on a 16-CPU quota measured best)
        want = max(1, min(n_jobs, self.search_threads or min(usable, 64)))
        pool = self._host_search_pool
        if pool is None or len(pool.procs) < want:
            if pool is not None:
                pool.close()
            self._host_search_pool = pool = HostSearchPool(want)
        return pool

    def _helper_thread(self, name):
        """Single helper threads: 'coder' (host range-coder work of roundtrip_stream's encoder that may overlap the calling thread's),
        'ydec' (its decoder's y range-decode), 'gather' (point lists to the host), 'tree' (compress_blocks' KD-tree over the original
        cloud).  One thread each: the jobs of a kind complete in submission order."""
        if name not in self._helper_pools:
            from concurrent.futures import ThreadPoolExecutor
            self._helper_pools[name] = ThreadPoolExecutor(max_workers=1, thread_name_prefix=f'pcc-{name}')
        return self._helper_pools[name]

    def _thr_tensor(self, ctx, thr_idx):
        """float32 thresholds of the blocks of a chunk as a device tensor."""
        # cached on the device: a pageable host->device copy here would block the host until the GPU drains
        # and serialise the pipeline
        thr_idx = [int(t) for t in thr_idx]
        if len(set(thr_idx)) == 1:     # fixed threshold: one cached vector per (value, batch)
            thr = self._dev(ctx, ('thr', thr_idx[0], len(thr_idx)), np.full(len(thr_idx), self._thr32(thr_idx[0]), np.float32))
        else:                          # adaptive thresholds vary per chunk: gather from the cached 256-entry table
            table = self._dev(ctx, 'thr_table', np.array([self._thr32(t) for t in range(len(self.thresholds))], np.float32))
            thr = table[torch.tensor(thr_idx, dtype=torch.int64).to(ctx.device, non_blocking=True)]
        return thr

    def _extract_points(self, ctx, x_hat, thr_idx, clip):
        """x_hat (B,D,H,W) device; thr_idx list of ints -> (xyz (B,cap,3), counts (B,)) device tensors."""
        return ops.threshold_compact(ctx, x_hat, self._thr_tensor(ctx, thr_idx), clip=clip)

    _gather_points = staticmethod(gather_points)

    def _codec(self, ctx):
        """pcc_codec_desc of this model on ctx's GPU (the batched-graph ABI), or None when a transform is not one of the
        plain reference stacks (then the per-layer path is used)."""
        nets = {}
        for prefix, tr, _ in self._transforms():
            nets[prefix] = tr.network() if hasattr(tr, 'network') else None
            if nets[prefix] is None:
                return None
        key = (ctx.device.index,) + tuple(id(n) for n in nets.values())
        if self._codec_cache[0] != key:
            med = self._dev(ctx, 'medians', self.entropy_bottleneck.medians)
            tab = self._scale_table_dev(ctx)
            # the NetworkWeights objects are kept alive with the entry: their id()s are the key and must not be recycled
            self._codec_cache = (key, ops.codec_desc(ctx, self.codec_abi, self.num_filters, nets, med, tab, self.round_mode),
                                 list(nets.values()))
        return self._codec_cache[1][0]

    def _scale_table_dev(self, ctx):
        return None                                # (a model with a conditional bottleneck has one)

    def _range_decode(self, table, strings, n, index_list, index_mod, sym_h):
        """Range-decodes one stream per block into the narrow pinned buffer `sym_h` (B, ...) in stream order; returns sym_h, or
        -- when a symbol does not fit it (OverflowError from the coder: never seen in practice) -- an int32 array of the same
        shape."""
        B = len(strings)
        try:
            # 2-D fast paths of the wrapper: sym_h (B, ...) is filled in place, the rows come as one 2-D tensor or one shared vector
            ops.range_decode_batch(table, strings, [n] * B, index_list, index_mod, self.coder_threads, out=sym_h.view(B, -1))
            return sym_h
        except OverflowError:
            if index_list is not None and not isinstance(index_list, (list, tuple)):     # the list form of the wrapper
                index_list = [index_list[b] for b in range(B)] if getattr(index_list, 'ndim', 1) >= 2 else [index_list] * B
            wide = ops.range_decode_batch(table, strings, [n] * B, index_list, index_mod, self.coder_threads)
            return torch.from_numpy(np.stack(wide).reshape(sym_h.shape))

    def _range_decode_eb(self, tag, strings, shape):
        """One EntropyBottleneck-coded stream per block -> (stream-order symbols in the next pinned buffer of ring `tag`, its release)."""
        # per-slot cached pinned buffers (like the encoder's): nothing is allocated in the steady state
        sym_h, release = self._pinned.ring(tag, shape, _host_dtypes()[0])
        n = int(np.prod(shape[1:]))
        rows, mod = self._eb_rows(n, self.num_filters)
        return self._range_decode(self.entropy_bottleneck.table, strings, n, rows, mod, sym_h), release

    def _host_symbols(self, staging, kind, sym):
        """The staged stream-order symbols of tensor `kind` ('y' | 'z') for the host coder.  A symbol beyond the narrow host type (never
        seen in practice) shows in the tile maxima: then `sym`, the int32 tensor on the device, is fetched instead."""
        narrow, tile_max = getattr(staging, f'{kind}sym'), getattr(staging, f'{kind}tm')
        fits = staging.sym_dtype == torch.int32 or int(tile_max.max()) <= 32767
        return narrow if fits else self._to_stream_order(sym).cpu()

    # ---- entropy_coder='rans': the strings are coded on the device from the int32 (B,D,H,W,C) tensors as the codec leaves them.  Under
    # channels_first the kernels walk them channel-major (`channels`), and the EntropyBottleneck rows are one cached row vector in
    # that memory order; nothing is narrowed, staged in pinned rings or handed to the host coder pool.
    def _rans_layout(self, ctx, n_per_block, eb):
        """(index, index_mod, channels) of ops.rans_*: eb = the EntropyBottleneck's per-channel rows, else the caller's index tensor"""
        F = self.num_filters
        cf = self.data_format == 'channels_first'
        if not eb:
            return None, 0, F if cf else 0
        if not cf:
            return None, F, 0
        name = ('rans_rows', n_per_block, F)
        rows = self._dev_cache.get((ctx.device.index, name))
        if rows is None:
            rows = self._dev(ctx, name, np.tile(np.arange(F, dtype=np.int32), n_per_block // F))
        return rows, 0, F

    def _rans_encode(self, ctx, ready, jobs):
        """jobs: (kind, table, symbols, index or None) per string (`_string_jobs`); no index = the EntropyBottleneck's rows.  The launches run on the side
        stream once `ready` (default: now, on the main stream) has passed, beside the synthesis transform.  Returns fetch() -> one
        list of strings per job."""
        with on_side_stream(ctx, after=ready) as side:
            launched = []
            for _, table, sym, index in jobs:
                rows, mod, channels = self._rans_layout(ctx, sym[0].numel(), index is None)
                for t in (sym, index):
                    if t is not None:
                        t.record_stream(side)
                launched.append(ops.rans_encode_launch(ctx, table, sym, None, rows if index is None else index, mod, channels))

        def fetch():
            with torch.cuda.stream(side):           # (the copies wait for the side stream only, never for the main queue)
                return [ops.rans_encode_fetch(out, meta) for out, meta in launched]
        return fetch

    def _rans_decode(self, ctx, table, strings, shape, index=None):
        """strings -> (symbols (B,D,H,W,C) int32 on the device, status flags for ops.rans_check_status), on the current stream; no
        index = the EntropyBottleneck's rows"""
        sym = torch.empty(tuple(shape), dtype=torch.int32, device=ctx.device)
        n = sym[0].numel()
        rows, mod, channels = self._rans_layout(ctx, n, index is None)
        return ops.rans_decode_batch(ctx, table, strings, [n] * len(strings), rows if index is None else index, mod, channels, out=sym, check=False)

    def _unpack(self, ctx, packed, dhw):
        return ops.symbols_unpack(ctx, packed, (packed.shape[0],) + tuple(dhw) + (self.num_filters,), self.data_format == 'channels_first')

    # ------------------------------------------------------------------ weights / checkpoints
    def _transforms(self):
        raise NotImplementedError

    def train(self, x, gamma, alpha, lmbda, **trainer_args):
        """The training model (src/model_types.py:250-277 / :327-369) as a train.Trainer: `x` is unused (the trainer
        voxelises its own batches from `train_blocks` / `val_blocks`); see train.Trainer for the other arguments."""
        from .train import Trainer
        return Trainer(self, gamma=gamma, alpha=alpha, lmbda=lmbda, **trainer_args)

    def init_weights(self, seed=None):
        """Seeded Glorot-uniform kernels / zero biases (Keras defaults) and tfc default entropy models:
        what tf.global_variables_initializer() gives before saver.restore (compress_octree.py:83-92)."""
        rng = np.random.default_rng(self.seed if seed is None else seed)
        for prefix, tr, cin in self._transforms():
            MT.init_transform(tr, cin, rng)
        self._init_entropy(None)
        self._drop_device_state()

    def _drop_device_state(self):
        """Everything on the GPU that was derived from the weights / entropy tables (new ones have just been set): the cached
        medians / scale table tensors and the pcc_codec_desc, which holds raw device pointers to them."""
        self._dev_cache.clear()
        self._codec_cache = (None,)
        self._stagings = {}

    def get_weights(self):
        out = {}
        for prefix, tr, _ in self._transforms():
            out.update(MT.get_weights(tr, prefix))
        out.update(self._entropy_weights())
        return out

    def set_weights(self, params):
        for prefix, tr, _ in self._transforms():
            MT.set_weights(tr, prefix, params)
        self._init_entropy(params)
        self._drop_device_state()

    def save_checkpoint(self, checkpoint_dir):
        os.makedirs(checkpoint_dir, exist_ok=True)
        np.savez(os.path.join(checkpoint_dir, CHECKPOINT_FILE), **self.get_weights())

    def restore(self, checkpoint_dir):
        """tf.train.Saver().restore(sess, tf.train.latest_checkpoint(dir)) (compress_octree.py:82,90-92): `model.npz`, or
        -- when the directory holds the reference's own TF1 checkpoint -- its TensorBundle files (tf_checkpoint.py)."""
        path = os.path.join(checkpoint_dir, CHECKPOINT_FILE)
        if not os.path.exists(path) and os.path.isdir(checkpoint_dir):
            from . import tf_checkpoint
            prefix = tf_checkpoint.latest_checkpoint(checkpoint_dir)
            if prefix is not None and os.path.exists(prefix + '.index'):
                tf_checkpoint.import_checkpoint(checkpoint_dir, self)
                return
        assert os.path.exists(path), f'Checkpoint {checkpoint_dir} was not found'
        with np.load(path) as f:
            self.set_weights({k: f[k] for k in f.files})

    # ------------------------------------------------------------------ block loops
    def encode_block_range(self, sess, blocks, resolution, with_normals=False, opt_metrics=('d1_mse',),
                           max_deltas=(np.inf,), fixed_threshold=False, debug=False, count_scale=None, count_search=None, latent_step=None):
        """The per-block part of compress_blocks (model_types.py:192-212) for a list of blocks: returns (strings per block, best-threshold
        list per block, candidate point lists per block, metric names, debug).  This is the unit that shards across GPUs
        (sharded_blocks.py).  A block's strings are the model's y/z strings, then those of the layers, in the order of stream_layers.LAYERS.
        count_scale = rho: count-matched thresholding instead of the search: the block's candidate is the k =
        block_count(its input rows, rho, voxels) highest-scoring voxels of x_hat (ops.topk_compact), its threshold byte the fixed one, and
        k its cnt1 string.
        count_search = (lo, hi, steps): the count search: the candidates of a block are the top-k sets for k =
        block_count(its input rows, rho_j, voxels) over model_opt.count_ladder(lo, hi, steps), scored exactly on the GPU (ops.d1_count_stats
        / d12_count_stats) and chosen per metric name by the threshold search's own decision rule (model_opt.decide_counts_from_tallies).
        In the cnt1 place stands ONE COUNT STRING PER METRIC NAME, in the order of the returned names (compress_blocks keeps the one of
        each output); the threshold byte is the fixed one.
        latent_step = q or one q per block (V2 only): block b's y is quantised with the step stream_layers.latent_step(q[b])
        and coded under the scales divided by it, and the byte q[b] is its qs1 string.  Everything behind the transform sees only another
        x_hat."""
        dhw = self._spatial(self.x_shape)
        plan = self._plan_encode('encode_block_range', 1, len(blocks), dhw, opt_metrics, fixed_threshold=fixed_threshold, count_scale=count_scale,
                                 count_search=count_search, latent_step=latent_step)
        ctx = self._ctx(sess)
        want_d2 = any(m.startswith('d2_') for m in opt_metrics)
        if not fixed_threshold:
            # once per call what the reference asserts per block (model_opt.py:22-24): unknown metric names, d2_* without normals
            from .utils.pc_metric import validate_opt_metrics
            validate_opt_metrics(opt_metrics, with_normals)
        strings_list, debug_t_list = [], []
        # adaptive search (model_opt.py:33-73): every chunk's x_hat goes to the schedule, the decisions come a few chunks later
        search = SearchSchedule(self, ctx, dhw, len(blocks), resolution, with_normals, opt_metrics, max_deltas)
        half, n_voxels = len(self.thresholds) // 2, int(np.prod(dhw))

        def topk(x_hat, ks):
            return ops.topk_compact(ctx, x_hat, torch.tensor(ks, dtype=torch.int32).to(ctx.device, non_blocking=True))

        def one_candidate(xyz, counts, extra=None):
            # compute_optimal_thresholds' fixed branch (model_opt.py:27-31): index len//2 and the same points for every metric name
            n_m = len(max_deltas) * len(opt_metrics)
            for pts in self._gather_points(xyz, counts):
                search.thresholds.append([half] * n_m)
                search.points.append([pts] * n_m)
            return extra

        # The four candidate policies.  Each is called once the chunk's occupancy launch is queued, launches what it can before the host
        # codes the strings, and returns decide(): called after enc['finish'](), it leaves the chunk's thresholds and candidate points
        # with `search` and returns the layer strings the policy adds ({layer: one entry per block}), if any.
        def searched(chunk, enc):
            return lambda: search.add(chunk, enc['x_hat'])

        def fixed(chunk, enc):
            return lambda: one_candidate(enc['xyz'], enc['counts'])

        def counted(chunk, enc):      # the candidate is the top-k one, the byte the fixed one
            ks = [block_count(len(b), count_scale, n_voxels) for b in chunk]
            xyz, counts = topk(enc['x_hat'], ks)
            return lambda: one_candidate(xyz, counts, {'cnt1': [SL.count_to_bytes(k) for k in ks]})

        def count_searched(chunk, enc):
            def decide():
                rows = count_rows(chunk, plan.ladder, n_voxels)
                tallies = count_tallies_gpu(ctx, chunk, enc['x_hat'], rows, d2=want_d2, hausdorff=wants_hausdorff(opt_metrics))
                search.names, ks_m, _ = decide_counts_from_tallies(chunk, tallies, rows, resolution, opt_metrics, max_deltas, with_normals=want_d2)
                per_name = [self._gather_points(*topk(enc['x_hat'], [k[m] for k in ks_m])) for m in range(len(search.names))]
                for j in range(len(chunk)):
                    search.thresholds.append([half] * len(search.names))
                    search.points.append([pts_m[j] for pts_m in per_name])
                return {'cnt1': [[SL.count_to_bytes(k) for k in ks] for ks in ks_m]}      # one count string per metric name
            return decide

        policy = {'search': searched, 'fixed': fixed, 'count': counted, 'count_search': count_searched}[plan.policy]
        for c0 in range(0, len(blocks), self.batch_size):
            chunk = blocks[c0:c0 + self.batch_size]
            x = self._voxelize(ctx, chunk, dhw)
            q = None if plan.steps is None else plan.steps[c0:c0 + len(chunk)]
            # (`steps` only where there are some: tests/test_round6_gpu.py and two tools replace _encode_batch by doubles without the keyword)
            stepped = {} if q is None else {'steps': torch.from_numpy(q).to(ctx.device)}
            enc = self._encode_batch(ctx, x, debug, thr=self._thr_tensor(ctx, [half] * len(chunk)) if plan.policy == 'fixed' else None, **stepped)
            # the occupancy layer: the chunk's dense input under the x_hat the decoder will compute (same bits: the numerics tag); the
            # policy neither sees nor changes it
            occ_job = ops.occ_encode_launch(ctx, enc['x_hat'], x) if self.lossless else None
            decide = policy(chunk, enc)
            strings = enc['finish']()
            extra = decide() or {}
            if q is not None:
                extra['qs1'] = [SL.step_to_bytes(v) for v in q.tolist()]
            if occ_job is not None:
                extra['occ1'] = ops.occ_encode_fetch(*occ_job)
            if extra:
                strings = [SL.compose_strings(ss, **{name: per_block[j] for name, per_block in extra.items()}) for j, ss in enumerate(strings)]
            strings_list.extend(strings)
            debug_t_list.extend(enc['debug'])
        search.drain()
        return strings_list, search.thresholds, search.points, search.names, debug_t_list

    def _plan_encode(self, entry, world, n_blocks, dhw, opt_metrics, **options):
        """stream_layers.plan_encode with what the model itself fixes (version, precision, coder, occupancy layer, search settings)"""
        return SL.plan_encode(entry=entry, world=world, n_blocks=n_blocks, dhw=dhw, opt_metrics=opt_metrics, version=self.codec_abi,
                              precision=self.precision, entropy_coder=self.entropy_coder, lossless=self.lossless, search_ties=self.search_ties,
                              d2_gpu=lambda: d2_on_gpu(self.d2_search, 'pick'), **options)

    def compress_blocks(self, sess, blocks, binstr, points, resolution, level, with_normals=False,
                        opt_metrics=('d1_mse',), max_deltas=(np.inf,), fixed_threshold=False, debug=False,
                        need_points=True, metrics_device='host', d2_ties='pick', count_scale=None, count_search=None, latent_step=None,
                        target_bpp=None):
        """Uses the compression model to compress a point cloud (model_types.py:184-218).  Under torch.distributed (one
        process per GPU) the block list is sharded (sharded_blocks.py): rank 0 returns the complete result, the other ranks
        return (None, metadata without point lists, local debug list).  `need_points=False` skips the gather of the
        decoded candidate point lists to rank 0 (they are only needed for --dec_files / --debug).  metrics_device='gpu'
        (single process only) computes the whole-cloud metrics on the GPU and builds no KD-tree.  d2_ties='mean' (single process
        only): the whole-cloud D2 averages over all equidistant nearest points; the per-block threshold search is not affected.
        count_scale, count_search (single process only): see encode_block_range; under count_search the data of output m carries, as every
        block's last string, the count chosen for that output's metric name.
        latent_step (V2, single process only): see encode_block_range.  target_bpp = R (instead of latent_step): the finest uniform step
        whose predicted container holds at most R * len(points) / 8 bytes (`choose_latent_step`; analysis and hyper run twice).  Under
        either, every metadata dict carries 'latent_step' (q, or the list of them) and, under a target, 'rate_target'."""
        from . import sharding
        rank, world = sharding.world_info()
        plan = self._plan_encode('compress_blocks', world, len(blocks), None if count_search is None else self._spatial(self.x_shape), opt_metrics,
                                 fixed_threshold=fixed_threshold, count_scale=count_scale, count_search=count_search, latent_step=latent_step,
                                 target_bpp=target_bpp, metrics_device=metrics_device, d2_ties=d2_ties)
        # The KD-tree over the ORIGINAL cloud (the whole-cloud metrics of every candidate query it: pc_metric.py:80) does not depend on the
        # encode: it is built on a helper thread while the GPU codes the blocks (0.11 s of a 614 k-point cloud's 0.30 s; scipy builds
        # without the GIL).  Same constructor call as before: the same tree, the same neighbour picks.  The GPU metrics need no tree.
        host_metrics = metrics_device == 'host'
        tree_future = self._helper_thread('tree').submit(cKDTree, points[:, :3]) if len(points) and host_metrics else None
        if world > 1:
            from .sharded_blocks import compress_blocks_sharded
            return compress_blocks_sharded(self, sess, blocks, binstr, points, resolution, level, with_normals, opt_metrics,
                                           max_deltas, fixed_threshold, debug, need_points, tree_future)
        rate_target = None
        try:
            if target_bpp is not None:
                latent_step, rate_target = self.choose_latent_step(sess, blocks, binstr, len(points), target_bpp)
            # (only the options that are set: tests/_shard_worker.py replaces encode_block_range by doubles without these keywords)
            options = {k: v for k, v in (('count_scale', count_scale), ('count_search', count_search), ('latent_step', latent_step)) if v is not None}
            strings_list, threshold_list, x_hat_list, opt_metrics_ret, debug_t_list = self.encode_block_range(
                sess, blocks, resolution, with_normals, opt_metrics, max_deltas, fixed_threshold, debug, **options)
        finally:
            tree = tree_future.result() if tree_future is not None else None
        # block -> opt metric to opt metric -> block
        threshold_list = list(zip(*threshold_list))
        x_hat_list = list(zip(*x_hat_list))
        metadata = select_best_per_opt_metric(binstr, x_hat_list, level, opt_metrics_ret, points, resolution, with_normals, tree=tree,
                                              metrics_device=metrics_device, ctx=None if host_metrics else self._ctx(sess),
                                              d2_ties=d2_ties, hausdorff=wants_hausdorff(opt_metrics) and not fixed_threshold)
        data_list = [list(zip(strings_list, threshold_list[x['idx']])) for x in metadata]
        if plan.policy == 'count_search':      # every block holds one count string per metric name: output m keeps its own
            def keep(strings, m):
                base, extra = SL.split_strings(strings, self.n_strings, plan.layers, candidates=len(opt_metrics_ret))
                return SL.compose_strings(base, **{**extra, 'cnt1': extra['cnt1'][m]})
            data_list = [[(keep(ss, x['idx']), t) for ss, t in data] for x, data in zip(metadata, data_list)]
        if latent_step is not None:
            q = np.asarray(latent_step)
            for x in metadata:
                x['latent_step'] = int(q) if q.ndim == 0 else [int(v) for v in q]
                if rate_target is not None:
                    x['rate_target'] = dict(rate_target)
        return data_list, metadata, debug_t_list

    def choose_latent_step(self, sess, blocks, binstr, n_points, target_bpp):
        raise AssertionError('target_bpp needs a hyperprior model (c3p and its siblings), drop --target_bpp')

    def roundtrip_stream(self, sess, dense_chunks, thr_idx=None, gather=True):
        """Streams chunks of dense occupancy grids (each (b,D,H,W) float32 on the GPU) through the compress
        graph and the decompress graph with fixed-threshold extraction on both sides -- the unit of work of
        SURVEY.md §8d -- as a 3-deep software pipeline:
            chunk k   : GPU analysis/hyper + synthesis(enc) | host range-encode + z-decode
            chunk k-1 : host y-decode | GPU synthesis(dec)
            chunk k-2 : decoded points gathered to the host
        Yields (strings, enc_counts, dec_points or dec_counts) per chunk, in order."""
        ctx = self._ctx(sess)
        thr_idx = len(self.thresholds) // 2 if thr_idx is None else thr_idx
        q_b, q_g = [], []

        def stage_b(item):
            strings, cnt_e, st, dhw, B, yfut = item
            kw = {} if yfut is None else {'host': yfut.result()}
            dec = self._decode_phase_b(ctx, st, dhw, False, thr=self._thr_tensor(ctx, [thr_idx] * B), **kw)
            xyz_d, cnt_d = dec['xyz'], dec['counts']
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(ctx.device))
            item_g = (strings, cnt_e, xyz_d, cnt_d, ready)
            # (round 5) few long streams per chunk: the gather (counts to the host, pack, 10 MB of points per 8-block chunk of 128^3 blocks:
            # 0.9 ms of blocking copies) runs on a helper thread too; results are still yielded in order
            return self._helper_thread('gather').submit(stage_g_work, item_g) if threaded else item_g

        def stage_g(item):
            return item.result() if threaded else stage_g_work(item)

        def stage_g_work(item):
            strings, cnt_e, xyz_d, cnt_d, ready = item
            if threaded:
                torch.cuda.set_device(ctx.device)
            if gather:
                pts = self._gather_points(xyz_d, cnt_d, ctx, ready)
                ce, = to_host(ctx, ready, cnt_e)
            else:
                ce, pts = to_host(ctx, ready, cnt_e, cnt_d)
            return strings, ce, pts

        def stage_a(item):
            enc, dhw, B = item
            strings = enc['strings'].result()
            st = self._decode_phase_a(ctx, strings, dhw)
            # (round 5) the y range-decode of this chunk -- host work only -- starts now on a helper thread and is collected one iteration
            # later by stage_b, when both coders fit the usable cores side by side (the rule of the encoder's helper thread below)
            host_coder = threaded and self.entropy_coder == 'range' and 'host' not in st      # (rans: no host part; 'host': done in phase a)
            yfut = self._helper_thread('ydec').submit(self._decode_phase_b_host, st) if host_coder else None
            q_b.append((strings, enc['counts'], st, dhw, B, yfut))
            if len(q_b) > 1:
                q_g.append(stage_b(q_b.pop(0)))

        # The GPU work of chunk k+1 (compress graph) is enqueued BEFORE the host waits for the symbols of chunk k: the device
        # queue then always holds at least one more compress graph than the host coder needs to stay ahead of, so a slow or
        # noisy host does not drain it.  Pinned symbol buffers are per slot (three chunks can be between enqueue and coding).
        # The range ENCODER of a chunk (wait for its symbols, code them) runs on a helper thread -- the coder is sequential per
        # stream, so at 128^3 one chunk's y streams cost the host milliseconds -- while this thread range-DECODES an older chunk
        # and feeds the GPU; the library calls release the GIL.
        q_a, k = [], 0
        threaded = None
        trace = os.environ.get('PCC_STAGE_TIMES')          # host time per pipeline stage and iteration (ms), to stderr
        try:
            for x in dense_chunks:
                B, dhw = x.shape[0], tuple(x.shape[1:4])
                if threaded is None:
                    threaded = (2 * B <= ops.usable_cores() or bool(os.environ.get('PCC_FORCE_HELPER_THREADS'))) and not os.environ.get('PCC_NO_HELPER_THREADS')
                t0 = time.perf_counter()
                enc = self._encode_batch(ctx, x, False, thr=self._thr_tensor(ctx, [thr_idx] * B), slot=k % 3)
                # (only when both coders fit the usable cores side by side: with 32 streams per call on a 16-core container the two
                # would just take turns, with scheduler jitter on top -- measured: 7-12 ms hiccups in the 64^3 headline)
                on_thread = 2 * B <= ops.usable_cores() and self.entropy_coder == 'range'        # (rans: finish only fetches bytes)
                enc['strings'] = self._helper_thread('coder').submit(enc['finish']) if on_thread else _Immediate(enc['finish'])
                k += 1
                q_a.append((enc, dhw, B))
                t1 = time.perf_counter()
                if len(q_a) > 1:
                    stage_a(q_a.pop(0))
                t2 = time.perf_counter()
                if len(q_g) > 1:
                    out = stage_g(q_g.pop(0))
                    if trace:
                        print(f'stage ms: enqueue {1e3 * (t1 - t0):.2f} decode+enqueue {1e3 * (t2 - t1):.2f} gather {1e3 * (time.perf_counter() - t2):.2f}',
                              file=sys.stderr)
                    yield out
            while q_a:
                stage_a(q_a.pop(0))
            while q_b:
                q_g.append(stage_b(q_b.pop(0)))
            while q_g:
                yield stage_g(q_g.pop(0))
        finally:
            # an abandoned generator (or a stage that raised) must not leave helper-thread jobs running against buffers the caller is
            # about to free: wait for whatever is still queued
            for enc_, _, _ in q_a:
                fut = enc_.get('strings')
                if hasattr(fut, 'cancel') and not fut.cancel():
                    try:
                        fut.result()
                    except Exception:
                        pass
            for item in list(q_b) + list(q_g):
                for fut in (item if isinstance(item, tuple) else (item,)):
                    if hasattr(fut, 'cancel') and hasattr(fut, 'result') and not fut.cancel():
                        try:
                            fut.result()
                        except Exception:
                            pass

    def decompress_blocks(self, sess, blocks, x_shape, debug=False, layers='all'):
        """Uses the decompression model to decompress a point cloud (model_types.py:220-238).  Under torch.distributed the block list
        is sharded and rank 0 returns the points (sharded_blocks.py).
        layers: 'all' decodes the occupancy string of a lossless stream (one string more per block than the model's y/z strings)
        against x_hat and returns the exact input voxels, the threshold byte is ignored; 'base' is the lossy decode of the same stream,
        as if the layer were not there.  A stream without the layer decodes the same under both.  'count' reads the extra string as the
        block's point count k ("cnt1") and returns the k highest-scoring voxels of x_hat; 'base' on such a stream is the
        decode by the threshold byte.  'step' reads the string behind the y/z strings as the block's latent step ("qs1", DESIGN.md 4.21;
        single process only): the stream cannot be decoded without it, so there is no 'base' form of it."""
        from . import sharding
        assert layers in ('all', 'base', 'count', 'step'), f"layers: 'all', 'base', 'count' or 'step', not {layers!r}"
        if layers == 'step' and sharding.world_info()[1] > 1:
            raise AssertionError('a stepped stream (qs1) is decoded by one process: the sharded path moves the y/z strings alone, run on one GPU')
        if sharding.world_info()[1] > 1:
            from .sharded_blocks import decompress_blocks_sharded
            return decompress_blocks_sharded(self, sess, blocks, x_shape, debug, layers)
        return self.decompress_block_range(sess, blocks, x_shape, debug, layers)

    def decompress_block_range(self, sess, blocks, x_shape, debug=False, layers='all'):
        """decompress_blocks for a list of blocks on this process' GPU: the unit that shards across GPUs.
        Software pipeline over chunks: the host range decoder of chunk k overlaps the synthesis of k-1."""
        dhw = self._spatial(x_shape)
        chunks = [blocks[c0:c0 + self.batch_size] for c0 in range(0, len(blocks), self.batch_size)]
        # the layer to read and its values, read and checked before anything is launched
        carried = SL.carried_layer(layers, blocks, self.n_strings)
        if carried == 'qs1' and self.codec_abi != 2:
            raise RuntimeError('the stream carries latent steps (qs1): only the hyperprior models (c3p and its siblings) read them')
        values = None if carried is None else SL.layer_values(carried, blocks, self.n_strings)
        ctx = self._ctx(sess)
        if carried == 'qs1':
            values = np.array(values, np.uint8)

        def of_chunk(k):
            return values[k * self.batch_size:k * self.batch_size + len(chunks[k])]

        # how the points of chunk k come out of x_hat, chosen once; by the threshold byte it is phase b's own last step
        by_threshold = carried in (None, 'qs1')
        if carried == 'occ1':
            def points(k, dec):
                B = len(chunks[k])
                occ, status = ops.occ_decode_batch(ctx, dec['x_hat'], of_chunk(k), check=False)
                out = ops.threshold_compact(ctx, occ, self._dev(ctx, ('thr_occ', B), np.full(B, 0.5, np.float32)), clip=False)
                ops.occ_check_status(status)                            # (after the chunk's launches)
                return out
        elif carried == 'cnt1':
            def points(k, dec):      # the stream is not trusted: a count above the block's voxels is the same request as all of them
                ks = [min(v, int(np.prod(dhw))) for v in of_chunk(k)]
                return ops.topk_compact(ctx, dec['x_hat'], torch.tensor(ks, dtype=torch.int32).to(ctx.device, non_blocking=True))
        else:
            def points(k, dec):
                return dec['xyz'], dec['counts']                        # the decoder does not clip (:232-233)
        state, results = [None] * len(chunks), [None] * len(chunks)
        for k in range(len(chunks) + 1):
            if k < len(chunks):
                stepped = {} if carried != 'qs1' else {'steps': torch.from_numpy(of_chunk(k)).to(ctx.device)}      # (V1 has no such keyword)
                state[k] = self._decode_phase_a(ctx, [s for s, _ in chunks[k]], dhw, **stepped)
            if k >= 1:
                thr = self._thr_tensor(ctx, [int(t) for _, t in chunks[k - 1]]) if by_threshold else None
                dec = self._decode_phase_b(ctx, state[k - 1], dhw, debug, thr=thr)
                results[k - 1] = points(k - 1, dec) + (dec['debug'],)
                state[k - 1] = None
        dec_blocks, debug_t_list = [], []
        for xyz, counts, dbg in results:
            dec_blocks.extend(self._gather_points(xyz, counts))
            debug_t_list.extend(dbg)
        return dec_blocks, debug_t_list

    # ------------------------------------------------------------------ batched graph.  With a pcc_codec_desc (`_codec`) the GPU part
    # of each phase is ONE ABI call; otherwise the same steps run layer by layer.  Both leave the same tensors under the same names.
    def _synthesis_layerwise(self, ctx, t, thr, clip):
        """t['y_hat'] -S-> t['x_hat'] [-> thresholded points t['xyz'], t['counts']], layer by layer"""
        t['x_hat'] = self.synthesis_transform.forward_ndhwc(ctx, t['y_hat'])[..., 0].contiguous()
        if thr is not None:
            t['xyz'], t['counts'] = ops.threshold_compact(ctx, t['x_hat'], thr, clip=clip)

    def _analysis_stepped(self, ctx, x, steps, stg):
        raise AssertionError('latent_step needs a hyperprior model (c3p and its siblings), drop --latent_step')

    def _encode_batch(self, ctx, x, debug, thr=None, slot=0, steps=None):
        """The compress graph of a chunk x (B,D,H,W): returns x_hat (and, with `thr`, the encoder-side points xyz / counts), the per-block
        debug dicts and finish() -> the strings per block, which waits for the symbols and codes them.
        steps: (B,) uint8 device tensor of ladder indexes -- the stepped chunk path, layer by layer with the stepped
        kernels, which stage the symbols themselves."""
        B, dhw = x.shape[0], x.shape[1:4]
        codec = self._codec(ctx) if steps is None else None
        ready = None
        rans = self.entropy_coder == 'rans'
        stg = None if rans else self._staging(ctx, slot, B, [v // 8 for v in dhw], [v // 16 for v in dhw] if self.n_strings == 2 else None)
        if codec is not None:                      # the whole GPU part of compress() (model_types.py:289-293 / :379-388) in one ABI call
            ready = torch.cuda.Event()
            ready.record(side_stream(ctx, '_idx_stream'))            # creates the handle (on a stream that is idle now: a record costs the
                                                                     # main queue a few microseconds); re-recorded by the library on the main stream
            t = ops.codec_encode(ctx, codec, x.contiguous(), thr, symbols_ready=ready, staging=stg)
        elif steps is not None:
            t = self._analysis_stepped(ctx, x, steps, stg)
        else:
            t = self._analysis_layerwise(ctx, x)
        jobs = self._string_jobs(t)
        if codec is None and not rans and steps is None:
            stg.pack(ctx, *(t[k] for k in ('symbols', 'z_symbols', 'indexes') if k in t))
        # what crosses PCIe: ONE buffer per chunk -- symbols as int16, the 64 scale rows as uint8 (8.5 -> 3.3 MB per 32-block
        # chunk), packed in stream order by the library before `ready`, plus the per-tile max|symbol| that tells the host
        # afterwards whether a symbol exceeded int16 (then that tensor is fetched again as int32: never seen in practice).
        # The copy runs on a side stream so that it overlaps the synthesis transform.
        # entropy_coder='rans': nothing is narrowed or shipped; the strings are coded on the side stream from the int32 tensors.
        if rans:
            fetch = self._rans_encode(ctx, ready, jobs)
        else:
            ev = ship(ctx, stg, ready)
        if codec is None:
            self._synthesis_layerwise(ctx, t, thr, clip=True)
        eb_rows = {kind: self._eb_rows(sym[0].numel(), self.num_filters) for kind, _, sym, index in jobs if index is None}

        def finish():
            if rans:
                return list(zip(*fetch()))
            ev.synchronize()  # symbols are on the host
            coded = []
            for kind, table, sym, index in jobs:
                rows, mod = eb_rows[kind] if index is None else (stg.idx.view(B, -1), 0)
                coded.append(ops.range_encode_batch(table, self._host_symbols(stg, kind, sym).view(B, -1), rows, mod, self.coder_threads))
            return list(zip(*coded))  # strings = (y_string,) / (y_string, z_string), model_types.py:293,389

        dbg = _debug_dicts(B, debug, t, self.encode_debug_keys)
        return dict(x_hat=t['x_hat'], finish=finish, debug=dbg, xyz=t.get('xyz'), counts=t.get('counts'))

    def _decode_phase_a(self, ctx, strings, dhw):
        """What can be decoded of a chunk before its predecessor's synthesis is enqueued -> the state phase b continues from"""
        raise NotImplementedError

    def _decode_phase_b_host(self, st):
        """The host part of phase b, (stream-order y symbols on the host, their ring release), when phase a has not left it under
        'host' already.  No GPU work is enqueued here, so roundtrip_stream may run it on a helper thread."""
        return st['host']

    def _decode_phase_b(self, ctx, st, dhw, debug, thr=None, host=None):
        """y_string -> y symbols -> y_hat -S-> x_hat [-> thresholded points].  host: the result of _decode_phase_b_host when it already
        ran elsewhere."""
        rans = self.entropy_coder == 'rans'
        if rans:
            ysym, status = self._y_rans_decode(ctx, st, dhw)
            packed = None
        else:
            ysym, packed = None, symbols_to_device(ctx, *(self._decode_phase_b_host(st) if host is None else host))
        codec = self._codec(ctx)
        if st.get('steps') is not None:            # stepped stream: y_hat = float(symbol) * step of the block, then the layer-wise synthesis
            yshape = (len(st['strings']),) + tuple(v // 8 for v in dhw) + (self.num_filters,)
            sym, y_hat = ops.unpack_dequantize_step(ctx, ysym if rans else packed, yshape, not rans and self.data_format == 'channels_first',
                                                    st['steps'], self._y_medians(ctx))
            t = dict(symbols=sym, y_hat=y_hat)
            self._synthesis_layerwise(ctx, t, thr, clip=False)
        elif codec is not None:                    # unpack -> dequantise -> synthesis (-> threshold + compaction) in one ABI call
            t = ops.codec_decode_main(ctx, codec, ysym, dhw, thr, packed=packed, channels_first=self.data_format == 'channels_first')
        else:
            if not rans:
                ysym = self._unpack(ctx, packed, [v // 8 for v in dhw])
            t = dict(symbols=ysym, y_hat=ops.dequantize(ctx, ysym, self._y_medians(ctx)))
            self._synthesis_layerwise(ctx, t, thr, clip=False)
        if rans:                                    # (after the chunk's launches: the device works while the host waits for the flags)
            for flags in (st.get('zstatus'), status):
                if flags is not None:
                    ops.rans_check_status(flags)
        dbg = _debug_dicts(len(st['strings']), debug, {**st, **t}, self.decode_debug_keys)      # (st: what phase a decoded)
        return dict(x_hat=t['x_hat'], debug=dbg, xyz=t.get('xyz'), counts=t.get('counts'))


class CompressionModelV1(CompressionModel):
    n_strings, codec_abi = 1, 1
    encode_debug_keys = ('y', 'symbols', 'y_hat', 'x_hat')
    decode_debug_keys = ('y_hat', 'x_hat')

    def __init__(self, num_filters=32,
                 analysis_transform_type=TransformType.AnalysisTransformV1,
                 synthesis_transform_type=TransformType.SynthesisTransformV1, *args, **kwargs):
        self.num_filters = num_filters
        self._bind_transforms(analysis=analysis_transform_type, synthesis=synthesis_transform_type)
        self.entropy_bottleneck = None
        super().__init__(*args, **kwargs)

    def _transforms(self):
        t = []
        if self.analysis_transform is not None:
            t.append(('analysis', self.analysis_transform, 1))
        t.append(('synthesis', self.synthesis_transform, self.num_filters))
        return t

    def _init_entropy(self, params):
        eb_params = tables = None
        if params is not None and 'entropy_bottleneck/quantiles' in params:
            eb_params = {k.split('/', 1)[1]: params[k] for k in params if k.startswith('entropy_bottleneck/')}
            if 'quantized_cdf' in eb_params:
                tables = (eb_params.pop('quantized_cdf'), eb_params.pop('cdf_length'), eb_params.pop('offset'))
        self.entropy_bottleneck = EntropyBottleneck(self.num_filters, params=eb_params, tables=tables, seed=self.seed)

    def _entropy_weights(self):
        eb = self.entropy_bottleneck
        out = {f'entropy_bottleneck/{k}': v for k, v in eb.params.items()}
        out.update({'entropy_bottleneck/quantized_cdf': eb.quantized_cdf, 'entropy_bottleneck/cdf_length': eb.cdf_length,
                    'entropy_bottleneck/offset': eb.offset})
        return out

    def compress(self, x_shape):
        """Initializes the compression model (model_types.py:283-295)."""
        self.x_shape = [int(v) for v in x_shape]
        self.analysis_transform = self.analysis_transform_class(self.num_filters, data_format=self.data_format)
        self.synthesis_transform = self.synthesis_transform_class(self.num_filters, data_format=self.data_format)
        self.init_weights()

    def decompress(self):
        """Initializes the decompression model (model_types.py:297-309)."""
        self.analysis_transform = None
        self.synthesis_transform = self.synthesis_transform_class(self.num_filters, data_format=self.data_format)
        self.init_weights()

    # ---- batched graph: x -A-> y -EB-> y_string ; y_hat -S-> x_hat
    def _y_medians(self, ctx):
        return self._dev(ctx, 'medians', self.entropy_bottleneck.medians)

    def _analysis_layerwise(self, ctx, x):
        y = self.analysis_transform.forward_ndhwc(ctx, x.unsqueeze(-1))
        ysym, y_hat = ops.quantize(ctx, y, self._y_medians(ctx), self.round_mode)
        return dict(y=y, symbols=ysym, y_hat=y_hat)

    def _string_jobs(self, t):
        return [('y', self.entropy_bottleneck.table, t['symbols'], None)]

    def _decode_phase_a(self, ctx, strings, dhw):
        if self.entropy_coder == 'rans':           # the strings go to the device as they are, in phase b
            return dict(strings=strings)
        yshape = self._stream_shape(len(strings), [v // 8 for v in dhw], self.num_filters)
        return dict(strings=strings, host=self._range_decode_eb('dec_ysym', [s[0] for s in strings], yshape))

    def _y_rans_decode(self, ctx, st, dhw):
        B = len(st['strings'])
        return self._rans_decode(ctx, self.entropy_bottleneck.table, [s[0] for s in st['strings']],
                                 (B,) + tuple(v // 8 for v in dhw) + (self.num_filters,))


class CompressionModelV2(CompressionModel):
    n_strings, codec_abi = 2, 2
    encode_debug_keys = ('y', 'z', 'z_symbols', 'z_hat', 'sigma_hat', 'indexes', 'symbols', 'y_hat', 'x_hat')
    decode_debug_keys = ('z_hat', 'sigma_hat', 'indexes', 'symbols', 'y_hat', 'x_hat')

    def __init__(self, num_filters=32,
                 analysis_transform_type=TransformType.AnalysisTransformV1,
                 synthesis_transform_type=TransformType.SynthesisTransformV1,
                 hyper_analysis_transform_type=TransformType.HyperAnalysisTransform,
                 hyper_synthesis_transform_type=TransformType.HyperSynthesisTransform,
                 scales_min=0.11, scales_max=256, scales_levels=64, *args, **kwargs):
        self.num_filters = num_filters
        self._bind_transforms(analysis=analysis_transform_type, synthesis=synthesis_transform_type,
                              hyper_analysis=hyper_analysis_transform_type, hyper_synthesis=hyper_synthesis_transform_type)
        self.scale_table = scale_table(scales_min, scales_max, scales_levels)
        self.entropy_bottleneck = self.conditional_bottleneck = None
        super().__init__(*args, **kwargs)

    def _transforms(self):
        t = []
        if self.analysis_transform is not None:
            t.append(('analysis', self.analysis_transform, 1))
            t.append(('hyper_analysis', self.hyper_analysis_transform, self.num_filters))
        t.append(('hyper_synthesis', self.hyper_synthesis_transform, self.num_filters))
        t.append(('synthesis', self.synthesis_transform, self.num_filters))
        return t

    def _init_entropy(self, params):
        CompressionModelV1._init_entropy(self, params)
        tables = None
        if params is not None and 'gaussian_conditional/quantized_cdf' in params:
            tables = tuple(params[f'gaussian_conditional/{k}'] for k in ('quantized_cdf', 'cdf_length', 'offset'))
        if self.conditional_bottleneck is None or tables is not None:
            self.conditional_bottleneck = GaussianConditional(self.scale_table, tables=tables)

    def _entropy_weights(self):
        out = CompressionModelV1._entropy_weights(self)
        gc = self.conditional_bottleneck
        out.update({'gaussian_conditional/quantized_cdf': gc.quantized_cdf, 'gaussian_conditional/cdf_length': gc.cdf_length,
                    'gaussian_conditional/offset': gc.offset})
        return out

    def compress(self, x_shape):
        """Initializes the compression model (model_types.py:371-391)."""
        self.x_shape = [int(v) for v in x_shape]
        F, df = self.num_filters, self.data_format
        self.analysis_transform = self.analysis_transform_class(F, data_format=df)
        self.synthesis_transform = self.synthesis_transform_class(F, data_format=df)
        self.hyper_analysis_transform = self.hyper_analysis_transform_class(F, data_format=df)
        self.hyper_synthesis_transform = self.hyper_synthesis_transform_class(F, data_format=df)
        self.init_weights()

    def decompress(self):
        """Initializes the decompression model (model_types.py:393-411)."""
        F, df = self.num_filters, self.data_format
        self.analysis_transform = self.hyper_analysis_transform = None
        self.synthesis_transform = self.synthesis_transform_class(F, data_format=df)
        self.hyper_synthesis_transform = self.hyper_synthesis_transform_class(F, data_format=df)
        self.init_weights()

    # ---- batched graph: x -A-> y -HA-> z -EB-> z_string ; z_hat -HS-> sigma ; (y, sigma) -GC-> y_string ; y_hat -S-> x_hat
    def _y_medians(self, ctx):
        return None                                # (the conditional bottleneck quantises y around zero)

    def _scale_table_dev(self, ctx):
        return self._dev(ctx, 'scale_table', self.conditional_bottleneck.scale_table_f32)

    def _scales_layerwise(self, ctx, t):
        """t['z_hat'] -HS-> t['sigma_hat'] -> t['indexes'] (the CDF row of every y symbol), layer by layer"""
        t['sigma_hat'] = self.hyper_synthesis_transform.forward_ndhwc(ctx, t['z_hat'])
        t['indexes'] = ops.scale_to_index(ctx, t['sigma_hat'], self._scale_table_dev(ctx))
        return t

    def _analysis_layerwise(self, ctx, x):
        med = self._dev(ctx, 'medians', self.entropy_bottleneck.medians)
        y = self.analysis_transform.forward_ndhwc(ctx, x.unsqueeze(-1))
        z = self.hyper_analysis_transform.forward_ndhwc(ctx, y)
        zsym, z_hat = ops.quantize(ctx, z, med, self.round_mode)
        t = self._scales_layerwise(ctx, dict(y=y, z=z, z_symbols=zsym, z_hat=z_hat))
        t['symbols'], t['y_hat'] = ops.quantize(ctx, y, None, self.round_mode)
        return t

    def _string_jobs(self, t):
        return [('y', self.conditional_bottleneck.table, t['symbols'], t['indexes']), ('z', self.entropy_bottleneck.table, t['z_symbols'], None)]

    # ---- the latent step: y / step and sigma / step per block; z is quantised as ever
    def _analysis_hyper(self, ctx, x):
        """x -A-> y -HA-> z -> z symbols, z_hat -HS-> sigma_hat, layer by layer: what both passes of a rate target and the stepped encode share"""
        med = self._dev(ctx, 'medians', self.entropy_bottleneck.medians)
        y = self.analysis_transform.forward_ndhwc(ctx, x.unsqueeze(-1))
        z = self.hyper_analysis_transform.forward_ndhwc(ctx, y)
        zsym, z_hat = ops.quantize(ctx, z, med, self.round_mode)
        return dict(y=y, z=z, z_symbols=zsym, z_hat=z_hat, sigma_hat=self.hyper_synthesis_transform.forward_ndhwc(ctx, z_hat))

    @staticmethod
    def _step_dst(stg, name):
        """(device address, bytes per element) the stepped kernels pack tensor `name` to: the staging buffer, or -- under rans, which codes
        from the int32 tensors on the device -- no packed copy at all"""
        if stg is None:
            return None, 4
        return stg.dev_ptr(name), ops._ITEM[stg.idx_dtype if name == 'idx' else stg.sym_dtype]

    def _analysis_stepped(self, ctx, x, steps, stg):
        t = self._analysis_hyper(ctx, x)
        cf = self.data_format == 'channels_first'
        ptr, nbytes = self._step_dst(stg, 'idx')
        t['indexes'] = ops.index_pack_step(ctx, t['sigma_hat'], self._scale_table_dev(ctx), cf, ptr, nbytes, steps)
        ptr, nbytes = self._step_dst(stg, 'ysym')
        t['symbols'], t['y_hat'] = ops.quantize_step_pack(ctx, t['y'], None, self.round_mode, cf, ptr, nbytes, steps,
                                                          None if stg is None else stg.dev_ptr('ytm'))
        if stg is not None:
            ops.symbols_pack(ctx, t['z_symbols'], cf, stg.dev_ptr('zsym'), ops._ITEM[stg.sym_dtype], stg.dev_ptr('ztm'))
        return t

    def choose_latent_step(self, sess, blocks, binstr, n_points, target_bpp):
        """The rate target's first pass: analysis and hyper per chunk, the rate ladder over all 64 steps and the actual z strings.  The
        predicted container at q = its fixed bytes (header, binstr, per block the threshold byte, three length fields and the step byte)
        + the z bytes + sum over the blocks of ceil((bits16[b][q] + rate_margin_bits16(bits16[b][q])) / 2^19): the measured margin by
        which the coder's string exceeds the model's sum, so that the chosen step fits on every stream measured; it is no proven bound.
        Returns (q, dict(target_bpp, budget_bytes, predicted_bytes, predictions)): q the smallest (finest) whose prediction is at most
        target_bpp * n_points / 8, else 63 with a warning."""
        from .model_syntax import _HEADER, _U16
        from .stream_layers import LATENT_STEPS
        ctx = self._ctx(sess)
        dhw = self._spatial(self.x_shape)
        ladder = np.arange(LATENT_STEPS, dtype=np.uint8)
        ybytes = np.zeros(LATENT_STEPS, np.int64)
        zbytes = 0
        for c0 in range(0, len(blocks), self.batch_size):
            chunk = blocks[c0:c0 + self.batch_size]
            t = self._analysis_hyper(ctx, self._voxelize(ctx, chunk, dhw))
            bits = ops.rate_ladder(ctx, t['y'], t['sigma_hat'], ladder, self._scale_table_dev(ctx), self.conditional_bottleneck.table, self.round_mode)
            zs = self._to_stream_order(t['z_symbols']).cpu().numpy().reshape(len(chunk), -1)
            rows, mod = self._eb_rows(zs.shape[1], self.num_filters)
            zbytes += sum(len(s) for s in ops.range_encode_batch(self.entropy_bottleneck.table, zs, rows, mod, self.coder_threads))
            bits = bits.cpu().numpy()
            ybytes += ((bits + rate_margin_bits16(bits) + ((1 << 19) - 1)) >> 19).sum(0)
        layers = ('qs1',)         # per block: the threshold byte, a length field per string, the step byte
        fixed = _HEADER.size + len(binstr) + len(blocks) * (1 + (self.n_strings + len(layers)) * _U16.size + sum(SL.BY_NAME[n].size for n in layers))
        pred = fixed + zbytes + ybytes
        budget = float(target_bpp) * n_points / 8.0
        fits = np.flatnonzero(pred <= budget)
        q = int(fits[0]) if fits.size else LATENT_STEPS - 1
        if not fits.size:
            logger.warning('target_bpp %g (%d bytes for %d points) is out of reach: the coarsest step (q = %d, step %g) predicts %d bytes',
                           target_bpp, int(budget), n_points, q, SL.latent_step(q), int(pred[q]))
        return q, dict(target_bpp=float(target_bpp), budget_bytes=budget, predicted_bytes=int(pred[q]), predictions=[int(v) for v in pred])

    def _hyper_decode(self, ctx, dhw, zsym=None, zpacked=None, idx_packed=None, steps=None):
        """z symbols (int32 on the device) or `zpacked` (stream-order symbols as the host->device copy delivered them) -> z_hat,
        sigma_hat, indexes; idx_packed: device tensor that also receives the indexes in stream order, for the host coder.
        steps: the blocks' ladder indexes (uint8, device): the rows are those of sigma_hat / step, layer by layer as the stepped encoder."""
        codec = self._codec(ctx) if steps is None else None
        cf = self.data_format == 'channels_first'
        if steps is not None:
            if zpacked is not None:
                zsym = self._unpack(ctx, zpacked, [v // 16 for v in dhw])
            z_hat = ops.dequantize(ctx, zsym, self._dev(ctx, 'medians', self.entropy_bottleneck.medians))
            sigma = self.hyper_synthesis_transform.forward_ndhwc(ctx, z_hat)
            idx = ops.index_pack_step(ctx, sigma, self._scale_table_dev(ctx), cf, None if idx_packed is None else idx_packed.data_ptr(),
                                      4 if idx_packed is None else idx_packed.element_size(), steps)
            return dict(z_hat=z_hat, sigma_hat=sigma, indexes=idx, z_symbols=zsym)
        if codec is not None:                      # unpack z -> dequantise -> hyper-synthesis -> indexes -> pack, one ABI call
            return ops.codec_decode_hyper(ctx, codec, zsym, dhw, packed=zpacked, channels_first=cf, idx_packed=idx_packed)
        if zpacked is not None:
            zsym = self._unpack(ctx, zpacked, [v // 16 for v in dhw])
        t = self._scales_layerwise(ctx, dict(z_hat=ops.dequantize(ctx, zsym, self._dev(ctx, 'medians', self.entropy_bottleneck.medians))))
        if idx_packed is not None:
            ops.symbols_pack(ctx, t['indexes'], cf, idx_packed.data_ptr(), idx_packed.element_size())
        return t

    def _decode_phase_a(self, ctx, strings, dhw, steps=None):
        """z_string -EB.decompress-> z_hat -HS-> sigma -> indexes (async D2H).  steps: the ladder indexes of a stepped stream's blocks
        (uint8, device), kept in the state for phase b."""
        B, F = len(strings), self.num_filters
        zstrings = [s[1] for s in strings]
        stepped = {} if steps is None else {'steps': steps}
        if self.entropy_coder == 'rans':
            zsym, zstatus = self._rans_decode(ctx, self.entropy_bottleneck.table, zstrings, (B,) + tuple(v // 16 for v in dhw) + (F,))
            t = self._hyper_decode(ctx, dhw, zsym, **stepped)
            # the CDF rows stay on the device: phase b decodes the y strings there
            return dict(strings=strings, z_hat=t['z_hat'], sigma_hat=t['sigma_hat'], indexes=t['indexes'], zstatus=zstatus, device=ctx.device, **stepped)
        zsym_h, zsym_release = self._range_decode_eb('dec_zsym', zstrings, self._stream_shape(B, [v // 16 for v in dhw], F))
        zpacked = symbols_to_device(ctx, zsym_h, zsym_release)
        # the 64 scale rows leave in stream order, one byte each
        row_t = _host_dtypes(len(self.scale_table))[1]
        idx_s = torch.empty(self._stream_shape(B, [v // 8 for v in dhw], F), dtype=row_t, device=ctx.device)
        t = self._hyper_decode(ctx, dhw, zpacked=zpacked, idx_packed=idx_s, **stepped)
        # (the host reads idx_h synchronously in phase b, long before the ring comes round: no release event needed)
        idx_h, _ = self._pinned.ring('dec_idx', idx_s.shape, row_t)
        ev = indexes_to_host(ctx, idx_s, idx_h)
        return dict(strings=strings, idx_h=idx_h, ev=ev, z_hat=t['z_hat'], sigma_hat=t['sigma_hat'], indexes=t['indexes'], zsym_h=zsym_h,
                    device=ctx.device, **stepped)

    def _decode_phase_b_host(self, st):
        """Wait for the CDF-row indexes, range-decode the y strings into a pinned buffer (the coder is sequential per stream: 2 ms per
        8-block chunk of 128^3 blocks; on roundtrip_stream's helper thread the calling thread keeps feeding the device meanwhile)."""
        if self.entropy_coder == 'rans':           # nothing to do on the host
            return None
        strings, idx_h = st['strings'], st['idx_h']
        B = len(strings)
        # may run on the 'ydec' helper thread: pinned allocations below must be made with THIS model's device current (a helper thread
        # starts on device 0 and would touch or create a context there on a rank that owns another GPU)
        if st.get('device') is not None:
            torch.cuda.set_device(st['device'])
        st['ev'].synchronize()
        ysym_h, ysym_release = self._pinned.ring('dec_ysym', idx_h.shape, _host_dtypes()[0])
        n = int(np.prod(idx_h.shape[1:]))
        return self._range_decode(self.conditional_bottleneck.table, [s[0] for s in strings], n, idx_h.view(B, -1), 0, ysym_h), ysym_release

    def _y_rans_decode(self, ctx, st, dhw):
        return self._rans_decode(ctx, self.conditional_bottleneck.table, [s[0] for s in st['strings']], st['indexes'].shape, st['indexes'])


class ModelType(Enum):
    v1 = CompressionModelV1
    v2 = CompressionModelV2
