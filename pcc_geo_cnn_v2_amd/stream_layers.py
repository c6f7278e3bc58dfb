"""What a stream carries on top of the model's y/z strings, and what an encode may combine.

LAYERS names every layer: its part of the numerics tag, its place in a block's strings (the order of the table, behind the model's
`n_strings` strings), how its string is written and read, and which other layers it may stand beside.  The tag functions, the composition
of a block's strings and the decoder's mode are derived from it: a new layer is a new row.  RULES says which options of an encode exclude
each other; `plan_encode` walks it for compress_blocks, encode_block_range and the CLIs and returns what the encode will do.

No torch, no GPU: the CLIs ask before the process group is joined or a context made.
"""
import logging
import struct
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib as L
from .model_opt import check_hausdorff_search, count_ladder, gpu_search_supported
from .utils.pc_metric import check_ties

logger = logging.getLogger(__name__)

# ---- the strings of the layers ----------------------------------------------------------------------------------------------------------
_COUNT = struct.Struct('<I')             # the "cnt1" string of a block: how many voxels the decoder keeps


def count_to_bytes(k):
    return _COUNT.pack(int(k))


def count_from_bytes(payload):
    """The count string of a block -> k, or None when it is not exactly 4 bytes long."""
    return _COUNT.unpack(payload)[0] if len(payload) == _COUNT.size else None


def _count_of(payload, block):
    k = count_from_bytes(payload)
    if k is None:
        raise _corrupt(f'block {block}: the count string holds {len(payload)} bytes, a "cnt1" stream carries {_COUNT.size} per block')
    return k


def _corrupt(message):
    return L.PccError(f'{message} (status {L.PCC_ERR_CORRUPT})')


LATENT_STEPS = 64                        # the latent step: one ladder index q per block, one byte


def latent_step(q):
    """Step size of ladder index q in [0, 63]: (8 + (q & 7)) * 2^((q >> 3) - 5) -- 0.25 ... 60, latent_step(16) = 1; integer times a
    power of two, so every value is exact in float32 (and no libm is involved)."""
    if not (isinstance(q, (int, np.integer)) and not isinstance(q, bool) and 0 <= q < LATENT_STEPS):
        raise AssertionError(f'latent_step: the ladder index is an integer in [0, {LATENT_STEPS - 1}], got {q!r}')
    q = int(q)
    e = (q >> 3) - 5
    return float(8 + (q & 7)) * (float(1 << e) if e >= 0 else 1.0 / float(1 << -e))


def step_to_bytes(q):
    latent_step(q)
    return bytes([int(q)])


def step_from_bytes(payload, block):
    """The step string of block `block` -> q.  A string that is not one byte, or a q beyond the ladder, is a RuntimeError."""
    if len(payload) != 1:
        raise RuntimeError(f'block {block}: the step string holds {len(payload)} bytes, a "qs1" stream carries one byte per block')
    if payload[0] >= LATENT_STEPS:
        raise RuntimeError(f'block {block}: step index {payload[0]} is beyond the ladder (0 to {LATENT_STEPS - 1})')
    return payload[0]


# ---- the layer table ---------------------------------------------------------------------------------------------------------------------
# name: the part of the tag, behind the coder part; the strings of a block's layers follow its y/z strings in the order of the rows
# to_bytes / from_bytes(payload, block): the string of one block; size: its bytes where they are fixed
# corrupt: the error of a block whose strings do not fit the layer; what: how messages call it
# mode: decompress_blocks' `layers` value that reads it; optional: whether the stream decodes without it ('base')
# beside: the layers it may share a stream with -- none yet, for any of them
Layer = namedtuple('Layer', 'name to_bytes from_bytes size corrupt what mode optional beside')
LAYERS = (
    Layer('qs1', step_to_bytes, step_from_bytes, 1, RuntimeError, 'latent steps', 'step', False, ()),
    Layer('occ1', bytes, lambda payload, block: payload, None, _corrupt, 'occupancy layer', 'all', True, ()),
    Layer('cnt1', count_to_bytes, _count_of, _COUNT.size, _corrupt, 'point counts', 'count', True, ()),
)
BY_NAME = {layer.name: layer for layer in LAYERS}


def ordered_layers(names, error=AssertionError, where=''):
    """`names` in the order of the table, after the check that they may share a stream (`error` otherwise)."""
    names = tuple(names)
    out = tuple(layer.name for layer in LAYERS if layer.name in names)
    if len(out) != len(names):
        raise error(f'the layers of a stream are of {[layer.name for layer in LAYERS]}, each at most once, not {list(names)}{where}')
    for a in out:
        for b in out:
            if a != b and b not in BY_NAME[a].beside:
                raise error(f'a stream carries the {BY_NAME[a].what} ({a}) or the {BY_NAME[b].what} ({b}), not both{where}')
    return out


def stream_tag(tag, entropy_coder, lossless=False, count=False, step=False, layers=()):
    """The numerics tag of a stream written with `entropy_coder`, with its layers named as final parts in the order of the table:
    '/qs1' the per-block latent steps, '/occ1' the occupancy layer, '/cnt1' the per-block point counts -- given as `layers` or by the
    three flags."""
    from .model_syntax import coder_tag
    flagged = [name for name, on in (('occ1', lossless), ('cnt1', count), ('qs1', step)) if on and name not in layers]
    return '/'.join((coder_tag(tag, entropy_coder),) + ordered_layers(tuple(layers) + tuple(flagged)))


def split_stream_tag(tag):
    """(numerics tag without coder and layer parts, entropy coder, tuple of layers) of a stream's tag; (tag, None, ()) for a stream
    without a tag of ours.  Unknown parts are refused like split_coder_tag refuses them, and so are layers in another order than the
    table's or layers that no build writes together."""
    from .model_syntax import split_coder_tag
    if tag is None or not tag.startswith('pcc_geo_cnn_v2_amd/'):
        return tag, None, ()
    parts = tag.split('/')
    found = []
    while len(parts) > 4 and parts[-1] in BY_NAME:
        found.insert(0, parts.pop())
    layers = ordered_layers(found, RuntimeError, f' ({tag}); this build reads each of them alone')
    if list(layers) != found:
        raise RuntimeError(f'the stream names its layers as {found} ({tag}); their order is {[layer.name for layer in LAYERS]}')
    base, coder = split_coder_tag('/'.join(parts))
    return base, coder, layers


def stream_layers(tag, expected, override=None, ignore=False):
    """Decoder side: (entropy coder, layers) the stream names; the rest of the tag is compared as stream_coder does."""
    from .model_syntax import coder_tag, stream_coder
    base, coder, layers = split_stream_tag(tag)
    return stream_coder(tag if coder is None else coder_tag(base, coder), expected, override, ignore), layers


def decode_mode(layers, base_only=False, name='the stream'):
    """decompress_blocks' `layers` value ('all' | 'base' | 'count' | 'step') for a stream that names `layers`.  base_only: the decode by
    the threshold byte alone; logged as without effect where the stream has no layer to leave out or cannot be decoded without one."""
    own = [BY_NAME[n] for n in layers]
    needed = [layer for layer in own if not layer.optional]
    if base_only and (not own or needed):
        logger.warning('--base_only has no effect on %s: the stream carries no occupancy layer', name)
    if needed:
        return needed[0].mode
    return 'base' if base_only else own[-1].mode if own else 'all'


def carried_layer(mode, blocks, n_strings):
    """The layer that decompress_blocks' `layers` value `mode` reads from `blocks` ([(strings, threshold byte)]), or None.  'all' reads
    the occupancy string only where the blocks carry one: a stream without the layer decodes the same under 'all' and 'base'."""
    found = [layer.name for layer in LAYERS if layer.mode == mode]
    absent = mode == 'all' and not (len(blocks) > 0 and len(blocks[0][0]) == n_strings + 1)
    return found[0] if found and not absent else None


def compose_strings(base, **strings):
    """The strings of a block: the model's `base` strings, then the string of every layer named in `strings`, in the order of the table.
    A list stands for several strings in the layer's place (the count search: one count per metric name until compress_blocks keeps one)."""
    assert set(strings) <= set(BY_NAME), f'unknown layers {sorted(set(strings) - set(BY_NAME))}'
    out = tuple(base)
    for layer in LAYERS:
        s = strings.get(layer.name)
        if s is not None:
            out += tuple(s) if isinstance(s, (list, tuple)) else (s,)
    return out


def split_strings(strings, n_strings, layers, block=0, candidates=None):
    """The inverse of compose_strings: (base strings, {layer: its string}) of block `block` of a stream that carries `layers` behind
    `n_strings` model strings; with `candidates` the last layer's entry is the list of that many strings.  A block with another number
    of strings is the corrupt-stream error of its last layer."""
    want = n_strings + len(layers) + (candidates or 1) - 1
    if len(strings) != want:
        layer = BY_NAME[layers[-1]]
        raise layer.corrupt(f'block {block}: {len(strings)} strings, a stream with the {layer.what} ({layer.name}) carries {want} per block')
    out = dict(zip(layers, strings[n_strings:]))
    if candidates is not None:
        out[layers[-1]] = list(strings[want - candidates:])
    return tuple(strings[:n_strings]), out


def layer_values(name, blocks, n_strings, layers=None):
    """The decoded string of layer `name` of every block ([(strings, threshold byte)]) of a stream that carries `layers` (default: that
    layer alone), read before anything is launched.  The stream is not trusted: see the layer's from_bytes and split_strings."""
    layers = (name,) if layers is None else layers
    return [BY_NAME[name].from_bytes(split_strings(strings, n_strings, layers, b)[1][name], b) for b, (strings, _) in enumerate(blocks)]


# ---- what an encode may combine ----------------------------------------------------------------------------------------------------------
METRICS_DEVICES = ('host', 'gpu')      # where the encoder's whole-cloud metrics run (compress_octree --metrics_device)

# policy: how a block's candidate points and threshold byte are chosen, 'search' | 'fixed' | 'count' | 'count_search'; ladder: the count
# scales of the count search (model_opt.count_ladder) or None; steps: the ladder index of the latent step per block (uint8) or None --
# also None under a rate target, which chooses it later; layers: what the stream will carry, in the order of the table
EncodePlan = namedtuple('EncodePlan', 'policy ladder steps layers')


def _d2_missing(o):
    return any(str(m).startswith('d2_') for m in o.opt_metrics or ()) and not (o.d2_gpu() if callable(o.d2_gpu) else o.d2_gpu)


def _set_ladder(o):
    if isinstance(o.count_search, AssertionError):      # a command line that could not be read as (lo, hi, steps): the reader's own words
        raise o.count_search
    if not (isinstance(o.count_search, (tuple, list)) and len(o.count_search) == 3):
        return f'count_search must be (lo, hi, steps), got {o.count_search!r}'
    o.ladder = count_ladder(*o.count_search)


def _set_steps(o):
    if o.latent_step is None:
        return None
    q = np.asarray(o.latent_step)
    if not (np.issubdtype(q.dtype, np.integer) and q.ndim <= 1 and q.size and q.min() >= 0 and q.max() < LATENT_STEPS):
        return f'latent_step is a ladder index in [0, {LATENT_STEPS - 1}] or one per block, got {o.latent_step!r}'
    if q.ndim == 1 and o.n_blocks is not None and q.size != o.n_blocks:
        return f'latent_step: {q.size} ladder indexes for {o.n_blocks} blocks'
    o.steps = (np.full(o.n_blocks, q) if q.ndim == 0 and o.n_blocks is not None else q).astype(np.uint8)


def _number_above_0(v):
    return isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool) and np.isfinite(v) and v > 0


def _count_policy(name, flag):
    """what either count policy excludes"""
    return [lambda o: o.fixed_threshold and f'{name} and fixed_threshold are two policies for the same decision, drop --{flag} or --fixed_threshold',
            lambda o: o.lossless and f'{name} and lossless: a stream carries the point counts or the occupancy layer, drop --{flag} or --lossless',
            lambda o: o.world > 1 and f'{name} is single-process only ' + ONE_PROCESS.format(o=o, flag=flag)]


ONE_PROCESS = '(world size {o.world}): the sharded path moves the y/z strings alone, drop --{flag} or run on one GPU'

# group -> (the flag in front of its messages on the command line, whether the group applies).  `what`: latent_step or target_bpp, the one given;
# the Hausdorff objectives and the tie rule of the whole-cloud D2 keep their rules where they are (model_opt, pc_metric)
GROUPS = {
    'step': ('--{o.what}', lambda o: o.latent_step is not None or o.target_bpp is not None),
    'count_scale': ('--count_threshold', lambda o: o.count_scale is not None),
    'count_flags': ('--count_threshold', lambda o: o.count_scale is not None),
    'count_search': ('--count_search', lambda o: o.count_search is not None),
    'lossless': ('--lossless', lambda o: o.lossless),
    'hausdorff': ('--opt_metrics', lambda o: not o.fixed_threshold),      # (a fixed threshold runs no search)
    'd2_ties': ('--d2_ties', lambda o: True),
    'metrics_device': ('--metrics_device', lambda o: True),
}
# group -> its rules: rule(o) returns the refusal's message -- the Python name, the reason, the flag to drop -- or nothing; the first rule
# of a group that speaks is the refusal
RULES = {
    'step': [
        lambda o: o.latent_step is not None and o.target_bpp is not None and
        'latent_step and target_bpp: the rate target chooses the step itself, drop --latent_step or --target_bpp',
        lambda o: o.version != 2 and f'{o.what} needs a hyperprior model (c3p and its siblings): the factorized prior of a V1 model has no '
        f'parametric rescale, drop --{o.what}',
        lambda o: o.precision == 'fp16' and f'{o.what} is built on the fp32 layer-wise path, drop --precision fp16 (or --{o.what})',
        lambda o: o.world > 1 and f'{o.what} is single-process only ' + ONE_PROCESS.format(o=o, flag=o.what),
        lambda o: o.lossless and f'{o.what} and lossless: a stepped stream carries no occupancy layer yet, drop --lossless (or --{o.what})',
        lambda o: o.count_scale is not None and f'{o.what} and count_scale: a stepped stream carries no point counts yet, drop --count_threshold (or --{o.what})',
        lambda o: o.count_search is not None and f'{o.what} and count_search: a stepped stream carries no point counts yet, drop --count_search (or --{o.what})',
        lambda o: o.target_bpp is not None and not _number_above_0(o.target_bpp) and f'target_bpp must be a finite number above 0, got {o.target_bpp!r}',
        lambda o: o.target_bpp is not None and o.entropy_coder == 'rans' and 'target_bpp predicts the size of range-coded strings, the escapes of the '
        'rANS coder cost otherwise: drop --entropy_coder rans (or --target_bpp)',
        _set_steps],
    'd2_ties': [lambda o: check_ties(o.d2_ties, o.world)],
    'lossless': [lambda o: o.world > 1 and f'lossless is single-process only (world size {o.world}): the sharded path does not carry the '
                 'occupancy strings, drop --lossless or run on one GPU'],
    'count_scale': [
        lambda o: not (isinstance(o.count_scale, (int, float, np.floating)) and np.isfinite(o.count_scale) and o.count_scale > 0) and
        f'count_scale must be a finite float above 0, got {o.count_scale!r}',
        *_count_policy('count_scale', 'count_threshold')],
    # (the command line alone: flags that would have no effect; the model's entry points accept the settings they stand for)
    'count_flags': [lambda o: o.search_ties == 'mean' and 'count_scale runs no threshold search, drop --search_ties mean',
                    lambda o: o.d2_gpu is True and 'count_scale runs no threshold search, drop --d2_search gpu'],
    'count_search': [
        _set_ladder,
        lambda o: o.count_scale is not None and 'count_search and count_scale are two policies for the same decision, drop --count_search or --count_threshold',
        *_count_policy('count_search', 'count_search'),
        lambda o: o.search_ties == 'mean' and "count_search with search_ties 'mean': the tie-averaged D2 engine has no count source, drop --search_ties mean",
        lambda o: _d2_missing(o) and "count_search with a d2_* metric needs the D2 statistics from the GPU (d2_search 'gpu'): the host KD-tree path "
        'has no count source, pass --d2_search gpu',
        lambda o: o.dhw is not None and not gpu_search_supported(o.opt_metrics, o.dhw) and
        f'count_search covers block grids up to 128^3 (the GPU search engines), not {tuple(o.dhw)}: raise --octree_level'],
    'hausdorff': [lambda o: check_hausdorff_search(o.opt_metrics, o.search_ties, o.d2_gpu, o.world)],
    'metrics_device': [
        lambda o: o.metrics_device not in METRICS_DEVICES and f'metrics_device must be one of {METRICS_DEVICES}, got {o.metrics_device!r}',
        lambda o: o.metrics_device == 'gpu' and o.world > 1 and f'metrics_device gpu is single-process only (world size {o.world}): the sharded '
        'metric path runs on the host, drop --metrics_device gpu or run on one GPU'],
}
# Which groups an entry point asks, in which order: when several rules refuse, each entry point goes on naming first the option it named
# first before the table existed.  encode_block_range is the per-rank unit: what needs the whole cloud or the world is not its business.
ENTRY_ORDER = {
    'compress_blocks': ('step', 'd2_ties', 'lossless', 'count_scale', 'count_search', 'hausdorff', 'metrics_device'),
    'encode_block_range': ('count_search', 'step', 'count_scale'),
    'cli': ('count_scale', 'count_flags', 'count_search', 'hausdorff', 'step', 'lossless', 'metrics_device', 'd2_ties'),
}


def plan_encode(*, count_scale=None, count_search=None, fixed_threshold=False, lossless=False, latent_step=None, target_bpp=None, version=2,
                precision='fp32', entropy_coder='range', world=1, search_ties='pick', opt_metrics=(), d2_gpu=None, dhw=None, n_blocks=None,
                metrics_device='host', d2_ties='pick', entry='compress_blocks'):
    """Checks the options of an encode against RULES (an AssertionError names the option, the reason and the flag to drop; for the
    command line it begins with the flag of the option it is about) and returns the EncodePlan.  version: 1 or 2, the model's codec_abi; d2_gpu: whether the D2 statistics of the search come
    from the GPU -- a callable is asked only when a d2_* metric stands beside the count search; dhw: the block grid, when known;
    n_blocks: the number of blocks, when known; entry: who asks (ENTRY_ORDER)."""
    o = SimpleNamespace(**locals(), what='latent_step' if latent_step is not None else 'target_bpp', ladder=None, steps=None)
    for group in ENTRY_ORDER[entry]:
        flag, applies = GROUPS[group]
        for rule in RULES[group] if applies(o) else ():
            try:
                message = rule(o)
            except AssertionError as e:
                message = str(e)
            if message:
                raise AssertionError(f'{flag.format(o=o)}: {message}' if entry == 'cli' else message)
    policy = 'count_search' if count_search is not None else 'count' if count_scale is not None else 'fixed' if fixed_threshold else 'search'
    carried = [name for name, on in (('qs1', GROUPS['step'][1](o)), ('occ1', lossless), ('cnt1', policy in ('count', 'count_search'))) if on]
    return EncodePlan(policy, o.ladder, o.steps, ordered_layers(carried))
