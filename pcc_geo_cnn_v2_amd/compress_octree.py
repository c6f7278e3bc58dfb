"""Encoder CLI -- same flags and files as /root/reference/src/compress_octree.py:130-185.

  python -m pcc_geo_cnn_v2_amd.compress_octree --input_files a.ply --output_files a.ply.bin \\
         --checkpoint_dir models/c3p/1.00e-04 --model_config c3p --resolution 1024 --octree_level 4 \\
         [--dec_files a.dec.ply] [--fixed_threshold] [--opt_metrics d1_mse] [--max_deltas inf] [--debug]
         [--estimate_normals [--normals_k 16]] [--metrics_device host|gpu] [--d2_ties pick|mean] [--search_ties pick|mean]
         [--entropy_coder range|rans] [--lossless] [--count_threshold [RHO]] [--count_search [LO HI STEPS]]

Differences: `--checkpoint_dir` holds `model.npz` (this framework's weight container) instead of a TF1
checkpoint; `--batch_size` (blocks resident per GPU pass) is new.  Under
`python -m torch.distributed.run --nproc-per-node N` the blocks are sharded over N GPUs and rank 0 writes
the files.  `--num_filters` is accepted and ignored, like in the reference.  `--estimate_normals` is new: the
normals of the D2 metrics come from the GPU (include/pcc_geo.h "point normals") instead of an `--input_normals` file.
`--metrics_device gpu` is new: the whole-cloud metrics of the final candidate selection run on the GPU (include/pcc_geo.h "cloud
metrics", neighbour ties to the lowest row) instead of scipy KD-trees; single process only.
`--lossless` is new: every block carries one more string that codes its true occupancy under the decoder's x_hat, so
decompress_octree returns the input voxels exactly; the y/z strings stay the lossy base; single process only.
`--count_threshold [RHO]` is new: count-matched thresholding instead of the threshold search: every block carries one more
string with k = round(RHO x its input points) (RHO = 1 when omitted) and decompress_octree keeps its k highest-scoring voxels; single
process only.
"""
import argparse
import json
import logging
import os

import numpy as np

logging.basicConfig(level=logging.INFO,
                    format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                    datefmt='%Y-%m-%d %H:%M:%S')
logger = logging.getLogger(__name__)


def _dump_clouds(folder, clouds):
    """--debug: one PLY per block under `folder` (0.ply, 1.ply, ...)."""
    from .utils import pc_io
    os.makedirs(folder, exist_ok=True)
    for n, cloud in enumerate(clouds):
        pc_io.write_df(os.path.join(folder, f'{n}.ply'), pc_io.pa_to_df(cloud))


class _Cloud:
    """One input file of the command line and the files its rate points go to (one per optimisation metric)."""
    __slots__ = ('source', 'targets', 'decoded')

    def __init__(self, source, targets, decoded):
        self.source, self.targets, self.decoded = source, targets, decoded


def _plan(args):
    """Command-line contract of /root/reference/src/compress_octree.py:131-183 -> (clouds, with_normals).  Every input file owns
    len(opt_metrics) consecutive entries of --output_files (and of --dec_files when given)."""
    from .model_configs import ModelConfigType
    from .utils.pc_metric import validate_opt_metrics
    if args.resolution <= 0:
        raise AssertionError('resolution must be positive')
    if args.data_format not in ('channels_first', 'channels_last'):
        raise AssertionError(f'unknown data_format {args.data_format}')
    if args.model_config not in ModelConfigType.keys():
        raise AssertionError(f'unknown model_config {args.model_config}: one of {list(ModelConfigType.keys())}')
    estimate = getattr(args, 'estimate_normals', False)
    if estimate and args.input_normals is not None:
        raise AssertionError('--estimate_normals and --input_normals are mutually exclusive')
    with_normals = args.input_normals is not None or estimate
    # the reference's own default '--opt_metrics d1_psnr' is not in avail_opt_metrics, so its CLI asserts unless the flag is
    # given (compress_octree.py:37,154).  psnr is monotone in mse (pc_metric.py:55), so '<g>_psnr' is taken as '<g>_mse' here
    metrics = []
    for name in args.opt_metrics:
        if name in ('d1_psnr', 'd2_psnr'):
            logger.warning(f"--opt_metrics {name}: not an optimisation metric of the reference; using the equivalent {name[:3]}mse")
            name = name[:3] + 'mse'
        metrics.append(name)
    args.opt_metrics = metrics
    validate_opt_metrics(metrics, with_normals=with_normals)
    check_search_ties(getattr(args, 'search_ties', 'pick'), metrics, with_normals, getattr(args, 'fixed_threshold', False))
    per_cloud = len(metrics) if len(metrics) > 1 else 1
    n_in = len(args.input_files)
    if len(args.output_files) != per_cloud * n_in:
        raise AssertionError(f'{n_in} input file(s) x {per_cloud} metric(s) need {per_cloud * n_in} output files, got {len(args.output_files)}')
    if per_cloud > 1 and not estimate and len(args.input_normals or ()) * per_cloud != len(args.output_files):
        raise AssertionError('several optimisation metrics need one normals file per input file')
    if args.dec_files is not None and len(args.dec_files) != per_cloud * n_in:
        raise AssertionError(f'--dec_files: expected {per_cloud * n_in} paths, got {len(args.dec_files)}')
    clouds = []
    for k, source in enumerate(args.input_files):
        span = slice(k * per_cloud, (k + 1) * per_cloud)
        targets = list(args.output_files[span])
        if len(set(targets)) != len(targets):
            raise AssertionError(f'{targets} should have no duplicates')
        clouds.append(_Cloud(source, targets, None if args.dec_files is None else list(args.dec_files[span])))
    return clouds, with_normals


COUNT_SEARCH_DEFAULT = (0.5, 2.0, 33)      # a design choice (half to twice the input count, 33 geometric steps), not a tuned value


def count_search_of(args):
    """--count_search [LO HI STEPS] as (lo, hi, steps), None without the flag; the bare flag is COUNT_SEARCH_DEFAULT."""
    v = getattr(args, 'count_search', None)
    if v is None:
        return None
    if len(v) == 0:
        return COUNT_SEARCH_DEFAULT
    try:
        lo, hi, steps = (float(x) for x in v)
    except ValueError:
        lo = hi = steps = None
    if steps is None or not steps.is_integer():
        raise AssertionError(f'--count_search takes no value or LO HI STEPS (two scales and an integer), got {list(v)}')
    return lo, hi, int(steps)


def check_encode_options(args, world):
    """What the parsed flags may combine (stream_layers.plan_encode), before the process group and the GPU are touched:
    returns the plan of the encode; a refusal names the flag in front of its message."""
    from .model_configs import ModelConfigType
    from .model_types import CompressionModelV2
    from .stream_layers import plan_encode
    try:
        search = count_search_of(args)
    except AssertionError as e:
        search = e      # (plan_encode raises it where the rules of the count search stand)
    config = ModelConfigType[args.model_config] if args.model_config in ModelConfigType.keys() else None      # (unknown: _plan's to refuse)
    return plan_encode(
        entry='cli', world=world, count_scale=getattr(args, 'count_threshold', None), count_search=search,
        fixed_threshold=getattr(args, 'fixed_threshold', False), lossless=getattr(args, 'lossless', False),
        latent_step=getattr(args, 'latent_step', None), target_bpp=getattr(args, 'target_bpp', None),
        version=1 if config is not None and not issubclass(config.value.model_type.value, CompressionModelV2) else 2,
        precision=getattr(args, 'precision', 'fp32'), entropy_coder=getattr(args, 'entropy_coder', 'range'),
        search_ties=getattr(args, 'search_ties', 'pick'), opt_metrics=getattr(args, 'opt_metrics', None) or (),
        d2_gpu=getattr(args, 'd2_search', None) == 'gpu', dhw=(int(args.resolution) >> int(args.octree_level),) * 3 if isinstance(search, tuple) else None,
        metrics_device=getattr(args, 'metrics_device', 'host'), d2_ties=getattr(args, 'd2_ties', 'pick'))


def check_search_ties(search_ties, opt_metrics, with_normals, fixed_threshold=False):
    """--search_ties mean changes the d2_* statistics of the per-block threshold search: refused where it could not do anything."""
    from .model_opt import check_search_ties as check
    try:
        check(search_ties, opt_metrics, with_normals)
        if search_ties == 'mean' and fixed_threshold:
            raise AssertionError('--fixed_threshold runs no threshold search, drop one of the two flags')
    except AssertionError as e:
        raise AssertionError(f'--search_ties: {e}') from None


def _block_grid(resolution, level, data_format):
    """Octree geometry: the bounding box of the whole cloud and the dense shape of one leaf block."""
    from .utils import pc_io
    _, _, shape = pc_io.get_shape_data(resolution, data_format)
    spatial = slice(1, 4) if data_format == 'channels_first' else slice(0, 3)
    box = shape[spatial].copy()
    shape[spatial] = shape[spatial] // (1 << level)
    return box, shape


def _write_rate_point(target, decoded_path, binstr, streams, info, args, blocks, debug_t_list):
    """The files of one rate point: <target> (gzip'd container), <target>.enc.metric.json, optionally the decoded cloud and the
    --debug dumps (/root/reference/src/compress_octree.py:109-125 lists them)."""
    from .model_syntax import save_compressed_file, split_stream_tag, write_tagged_gzip
    from .stream_layers import latent_step as step_size, split_strings
    from .utils import pc_io
    folder = os.path.dirname(target)
    if folder:
        os.makedirs(folder, exist_ok=True)
    payload = save_compressed_file(binstr, streams, args.resolution, args.octree_level, strict=True)
    write_tagged_gzip(target, payload, info['numerics_tag'])      # = gzip.open(target, 'wb').write(payload) + the tag in the member header
    with open(target + '.enc.metric.json', 'w') as fh:
        # the reference's keys (floats) + the tag of the kernels that computed sigma-hat (a string: a tool that re-gzips the payload drops the
        # header comment, this file keeps it; readers of the reference's JSON iterate over known metric names)
        record = dict({name: float(val) for name, val in info['metrics'].items()}, codec_numerics=info['numerics_tag'])
        if getattr(args, 'metrics_device', 'host') != 'host':      # host mode writes exactly the keys it always wrote
            record['metrics_device'] = args.metrics_device
        if getattr(args, 'd2_ties', 'pick') != 'pick':
            record['d2_ties'] = args.d2_ties
        if getattr(args, 'search_ties', 'pick') != 'pick':
            record['search_ties'] = args.search_ties
        # the bytes of the stream's layers, by name (the tag names them; what stands in front of them are the model's y/z strings)
        layers = split_stream_tag(info['numerics_tag'])[2]
        split = [split_strings(strings, len(strings) - len(layers), layers, b) for b, (strings, _) in enumerate(streams)] if layers else []
        if getattr(args, 'count_threshold', None) is not None:
            record.update(threshold_policy='count', count_scale=float(args.count_threshold))
        if count_search_of(args) is not None:
            record.update(threshold_policy='count_search', count_ladder=list(count_search_of(args)))
        if 'threshold_policy' in record:
            record['count_bytes'] = sum(len(extra['cnt1']) for _, extra in split)      # (4 per block)
        if 'latent_step' in info:
            q = info['latent_step']
            record['latent_step'] = q
            record['latent_step_size'] = step_size(q) if isinstance(q, int) else [step_size(v) for v in q]
            if 'rate_target' in info:      # the size is the container's before gzip
                record['target_bpp'] = info['rate_target']['target_bpp']
                record['predicted_bytes'] = info['rate_target']['predicted_bytes']
                record['container_bytes'] = len(payload)
        if getattr(args, 'lossless', False):
            # the rate of the exact cloud counts the whole file as written
            n_points = sum(len(b) for b in blocks)
            record['lossless'] = True
            record['base_bytes'] = sum(len(x) for base, _ in split for x in base)
            record['occ_bytes'] = sum(len(extra['occ1']) for _, extra in split)
            record['bits_per_input_point_lossless'] = 8.0 * os.path.getsize(target) / max(n_points, 1)
        json.dump(record, fh, sort_keys=True, indent=4)
    if decoded_path is not None:
        pc_io.write_df(decoded_path, pc_io.pa_to_df(info['blocks_full']))
    if args.debug:
        pc_io.write_df(target + '.enc.ply', pc_io.pa_to_df(info['blocks_full']))
        _dump_clouds(target + '.ori.blocks', blocks)
        _dump_clouds(target + '.enc.blocks', info['x_hat_list'])
        _dump_clouds(target + '.enc.blocks.depart', info['blocks_depart'])
        np.savez_compressed(target + '.enc.data.npz', data=np.array(streams, dtype=object), debug_t_list=np.array(debug_t_list, dtype=object))


def encode_cloud(args, model, sess, cloud, blocks, binstr, points, plan, with_normals, want_points, write=True):
    """One cloud of the command line: compress_blocks on its blocks under the parsed options, then -- where `write` (rank 0: the other
    ranks only take part in the collectives) -- the files of every rate point, tagged with the layers of `plan`."""
    from .model_syntax import stream_tag
    from .utils import cli_timing as T
    logger.info(f'Starting {cloud.source} to {", ".join(cloud.targets)} with {len(blocks)} blocks')
    streams, infos, debug_t_list = model.compress_blocks(
        sess, blocks, binstr, points, args.resolution, args.octree_level, with_normals=with_normals, opt_metrics=args.opt_metrics,
        max_deltas=args.max_deltas, fixed_threshold=args.fixed_threshold, debug=args.debug, need_points=want_points,
        metrics_device=getattr(args, 'metrics_device', 'host'), d2_ties=getattr(args, 'd2_ties', 'pick'),
        count_scale=getattr(args, 'count_threshold', None), count_search=count_search_of(args), latent_step=getattr(args, 'latent_step', None),
        target_bpp=getattr(args, 'target_bpp', None))
    T.mark('compress_blocks', sess.device)
    if write:
        if len(streams) != len(cloud.targets):
            raise AssertionError(f'{len(streams)} rate points for {len(cloud.targets)} output files')
        tag = stream_tag(sess.numerics_tag(args.precision), model.entropy_coder, layers=plan.layers)
        for n, target in enumerate(cloud.targets):
            infos[n]['numerics_tag'] = tag
            _write_rate_point(target, None if cloud.decoded is None else cloud.decoded[n], binstr, streams[n], infos[n], args, blocks, debug_t_list)
        logger.info(f'Finished {cloud.source} to {", ".join(cloud.targets)} with {len(blocks)} blocks')
    T.mark('container_gzip_write')


def compress(args):
    from .utils import cli_timing as T
    T.mark('process_start_to_main')
    import torch
    from . import ops
    from .model_configs import ModelConfigType
    from .sharding import join_process_group
    from .utils import pc_io
    from .utils.octree_coding import partition_octree
    T.mark('imports')

    plan = check_encode_options(args, int(os.environ.get('WORLD_SIZE', '1')))      # (first: its messages name the flags, not what _plan meets)
    clouds, with_normals = _plan(args)
    rank, world, local = join_process_group()
    if args.debug and world > 1:
        raise AssertionError('--debug dumps every intermediate of every block: run it on one GPU')
    sess = ops.get_context(torch.device('cuda', local))        # what tf.Session is to the reference (compress_octree.py:84)
    T.mark('context', sess.device)

    geometry = pc_io.load_points(args.input_files, batch_size=args.read_batch_size)
    if getattr(args, 'estimate_normals', False):
        # once per cloud, before partitioning; every rank of a sharded run estimates from its own copy (deterministic: same bits)
        geometry = [np.hstack((xyz, ops.estimate_normals(sess, xyz, k=args.normals_k))) for xyz in geometry]
        T.mark('estimate_normals', sess.device)
    elif with_normals:
        geometry = [np.hstack((xyz, pc_io.load_normals(path))) for xyz, path in zip(geometry, args.input_normals)]
    T.mark('ply_read')
    box, block_shape = _block_grid(args.resolution, args.octree_level, args.data_format)
    logger.info('Performing octree partitioning')
    partitions = [partition_octree(cloud, [0, 0, 0], box, args.octree_level) for cloud in geometry]
    T.mark('partition')
    logger.info(f'Processing resolution {args.resolution} with octree level {args.octree_level} resulting in dense_tensor_shape '
                f'{block_shape} and {sum(len(blocks) for blocks, _ in partitions)} blocks')

    model = ModelConfigType[args.model_config].build(data_format=args.data_format, batch_size=args.batch_size, precision=args.precision,
                                                    entropy_coder=getattr(args, 'entropy_coder', 'range'), lossless=getattr(args, 'lossless', False))
    model.d2_search = getattr(args, 'd2_search', None)      # per model, not a module global
    model.search_ties = getattr(args, 'search_ties', 'pick')
    model.compress(np.concatenate(((1,), block_shape)))
    model.restore(args.checkpoint_dir)      # asserts 'Checkpoint ... was not found' like compress_octree.py:91
    T.mark('checkpoint_restore')
    if T.enabled():      # the weight repack + upload happens on the first codec call: make it a phase of its own
        model._codec(sess)
        T.mark('weights_repack_upload', sess.device)

    for cloud, points, (blocks, binstr) in zip(clouds, geometry, partitions):
        encode_cloud(args, model, sess, cloud, blocks, binstr, points, plan, with_normals, clouds[0].decoded is not None or args.debug, write=rank == 0)
    T.dump()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def build_parser():
    from .utils.pc_metric import avail_opt_metrics, hausdorff_opt_metrics
    parser = argparse.ArgumentParser(prog='compress_octree.py', description='Compress a file.',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('--input_files', nargs='+', help='Input files.', required=True)
    parser.add_argument('--output_files', nargs='+', required=True,
                        help='Output files. If input normals are provided, specify two output files per input file.')
    parser.add_argument('--input_normals', nargs='+',
                        help='Input normals. If provided, two output paths are needed for each input file for D1 and D2 optimization.')
    parser.add_argument('--estimate_normals', default=False, action='store_true',
                        help='Estimate the normals of each input cloud on the GPU instead of reading --input_normals (new; enables the '
                             'd2_* metrics like a normals file does).')
    parser.add_argument('--normals_k', type=int, default=16, help='Neighbours per point of --estimate_normals (3..64).')
    parser.add_argument('--metrics_device', choices=('host', 'gpu'), default='host',
                        help='Where the whole-cloud metrics of the final candidate selection run (new): host = scipy KD-trees, '
                             'gpu = the HIP engine (ties to the lowest row; single process only).')
    parser.add_argument('--d2_ties', choices=('pick', 'mean'), default='pick',
                        help='Which of several equidistant nearest points the whole-cloud D2 reads (the metrics that rank the candidates '
                             'and go to .enc.metric.json; new): pick = one of them, mean = the average over all of them (row-order '
                             'independent, the same on host and gpu; single process only).  The per-block threshold search keeps its '
                             'own rules either way (its flag: --search_ties).')
    parser.add_argument('--search_ties', choices=('pick', 'mean'), default='pick',
                        help='Which of several equidistant nearest points the d2_* statistics of the per-block threshold search read '
                             '(new): pick = one of them (each engine its own, see --d2_search), mean = the average over all of them: '
                             'row-order independent, the same sums on the GPU (the default engine for mean) and with --d2_search kdtree '
                             '(or PCC_D2_HOST=1: the slow host restatement, for checking; PCC_D2_GPU has no effect under mean), and the function '
                             '--d2_ties mean reports.  Needs a d2 metric '
                             'in --opt_metrics and normals.')
    parser.add_argument('--dec_files', nargs='*',
                        help='Decoded files. Allows compression/decompression in a single execution.  Under --lossless they still hold the '
                             'lossy base candidate (what decompress_octree --base_only writes).')
    parser.add_argument('--checkpoint_dir', help='Directory where to save/load model checkpoints.', required=True)
    parser.add_argument('--model_config', help='Model used: c1, c2, c3, c3p.', required=True)
    # the reference's default (compress_octree.py:156); translated to d1_mse in compress(), see there
    parser.add_argument('--opt_metrics', nargs='+', default=['d1_psnr'],
                        help=f'Optimization metrics used. Available: {avail_opt_metrics}; worst-point objectives (new): '
                             f'{hausdorff_opt_metrics} -- the largest per-point error instead of the sum (GPU search, one process, '
                             '--search_ties pick; d2_hausdorff* needs --d2_search gpu); .enc.metric.json then also carries the '
                             'whole-cloud Hausdorff keys.')
    parser.add_argument('--max_deltas', nargs='+', default=[np.inf], type=float, help='Max deltas tested during optimization.')
    parser.add_argument('--fixed_threshold', default=False, action='store_true', help='Enable fixed thresholding.')
    parser.add_argument('--read_batch_size', type=int, default=1, help='Batch size for parallel reading.')
    parser.add_argument('--resolution', type=int, help='Dataset resolution.', default=64)
    parser.add_argument('--octree_level', type=int, help='Octree level.', default=4)
    parser.add_argument('--num_filters', type=int, default=32, help='Number of filters per layer (ignored, as in the reference).')
    parser.add_argument('--data_format', default='channels_first', help='Data format used: channels_first or channels_last')
    parser.add_argument('--debug', default=False, action='store_true', help='Output debug data for point cloud.')
    parser.add_argument('--batch_size', type=int, default=32, help='Blocks resident on the GPU per pass (new).')
    parser.add_argument('--d2_search', default=None, choices=['gpu', 'kdtree'],
                        help='Where the d2_* statistics of the adaptive threshold search come from (new): gpu = nearest-index transforms, ties '
                             'between equidistant neighbours go to the lowest (x, y, z); kdtree = scipy KD-trees on the host, the '
                             "reference's own picks and decisions (8-18x slower per cloud).  Default: kdtree (PCC_D2_GPU=1 = gpu).")
    parser.add_argument('--precision', default='fp32', choices=['fp32', 'fp16'],
                        help='fp16: fp16 matrix instructions with fp32 accumulation on the conv layers (new; must match between '
                             'compress and decompress).')
    parser.add_argument('--entropy_coder', default='range', choices=['range', 'rans'],
                        help="String format (new): range = the host range coder (tfc's algorithm, the default: files unchanged), "
                             'rans = the interleaved rANS coded on the GPU; the stream names it (numerics tag suffix /rans1), so '
                             'decompress_octree needs no flag.')
    parser.add_argument('--lossless', default=False, action='store_true',
                        help='Add the occupancy layer (new): one more string per block codes its true occupancy under the decoded x_hat, '
                             'so decompress_octree returns the input voxels exactly and --base_only the lossy cloud.  The stream names the '
                             'layer (numerics tag suffix /occ1); .enc.metric.json gains lossless, base_bytes, occ_bytes and '
                             'bits_per_input_point_lossless (8 x file size / input points).  Single process only.')
    parser.add_argument('--count_threshold', nargs='?', type=float, const=1.0, default=None, metavar='RHO',
                        help='Count-matched thresholding (new) instead of the threshold search: every block carries one more string, its '
                             'point count k = floor(RHO x input points + 0.5) (RHO = 1 when omitted), and decompress_octree keeps its k '
                             'highest-scoring voxels.  The stream names the layer (numerics tag suffix /cnt1); .enc.metric.json gains '
                             'threshold_policy, count_scale and count_bytes.  Not with --fixed_threshold, --lossless, --search_ties mean or '
                             '--d2_search gpu; single process only.')
    parser.add_argument('--count_search', nargs='*', default=None, metavar='LO HI STEPS',
                        help='Count search (new) instead of the threshold search: every block tries the point counts k = floor(RHO x input '
                             'points + 0.5) over STEPS scales RHO spaced geometrically from HI down to LO, scores each top-k set exactly '
                             '(D1, and D2 with --d2_search gpu) on the GPU and keeps, per output file, the count its metric prefers; the '
                             'stream is the one of --count_threshold (tag suffix /cnt1, one 4-byte count per block).  The bare flag means '
                             f'{" ".join(map(str, COUNT_SEARCH_DEFAULT))}: a design choice, not a tuned value.  .enc.metric.json gains threshold_policy, '
                             'count_ladder and count_bytes.  Not with --count_threshold, --fixed_threshold, --lossless or --search_ties mean; '
                             'd2_* metrics need --d2_search gpu; blocks up to 128^3; single process only.')
    parser.add_argument('--latent_step', type=int, default=None, metavar='Q',
                        help='Quality knob on the checkpoint at hand (new): quantise the latents y with the step (8 + (Q & 7)) x 2^((Q >> 3) - 5), '
                             'Q in 0..63 (0.25 ... 60; Q = 16 is the step 1 of the plain stream) and code them under the scales divided by '
                             'it.  Every block carries one more string, the byte Q, and the stream names it (numerics tag suffix /qs1), so '
                             'decompress_octree needs no flag; .enc.metric.json gains latent_step and latent_step_size.  Hyperprior models '
                             '(c2, c3, c3p) in fp32 only; not with --lossless, --count_threshold or --count_search; single process only.')
    parser.add_argument('--target_bpp', type=float, default=None, metavar='R',
                        help='Rate target (new): the finest --latent_step whose PREDICTED container (before gzip) holds at most R bits per '
                             'input point; the prediction is the cost model plus a measured margin, not a proven bound, so the written '
                             'container can exceed the target by the coder\'s excess on unusual streams; analysis runs twice.  Out of reach: the coarsest step, with a warning.  .enc.metric.json also '
                             'gains target_bpp, predicted_bytes and container_bytes.  As --latent_step, and not with it or --entropy_coder rans.')
    return parser


if __name__ == '__main__':
    from . import want_hw_queues
    want_hw_queues()        # before torch (the HIP runtime) loads: compress() imports it
    compress(build_parser().parse_args())
    # everything is written and closed: leave without the interpreter / runtime teardown (0.4 - 0.5 s of a 2 - 3 s process,
    # profiles/r06_cli_wallclock.md); PCC_CLI_CLEAN_EXIT=1 keeps the ordinary exit
    if not os.environ.get('PCC_CLI_CLEAN_EXIT'):
        import sys
        logging.shutdown()
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)
