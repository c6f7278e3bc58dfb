"""One (cloud, checkpoint) experiment in this process -- the role of the reference's src/ev_experiment.py.

  python -m pcc_geo_cnn_v2_amd.ev_experiment --output_dir OUT --model_dir models/c3p/1.00e-04 --model_config c3p --pc_name loot
      --input_pc loot.ply [--input_norm loot_n.ply | --estimate_normals] --resolution 1024 [--octree_level 4]
      --opt_metrics d1_mse d2_mse --max_deltas inf [--fixed_threshold | --count_threshold [RHO] | --count_search [LO HI STEPS]] [--latent_step Q | --target_bpp R] [--no_merge_coding] [--metrics_device host|gpu]
      [--d2_ties pick|mean] [--consistency assert|warn] [--recolor rank2|transfer]

Files in OUT, per optimisation group g (d1 always; d2 only when a d2_* metric is asked for, which needs normals):

  <pc_name>_<g>.ply.bin (+ .enc.metric.json)   the encoder's output: compress_octree's files, byte for byte
  <pc_name>_<g>.ply.bin.ply                    the decoded cloud: written by the encoder (--dec_files, "merged coding") or, with
                                               no_merge_coding, by the decoder
  <pc_name>_<g>.ply.bin.ply.color.ply          the decoded cloud with the original's colours (map_color), when the input has colours
  report_<g>.json                              ev_report.build_report's dictionary of those files + enc_dec_d1_psnr_diff

--recolor picks the colour step: rank2 (default; the reference's map_color, ops.map_colors rank 2) or transfer (ops.transfer_colors,
DESIGN.md 4.9 "Colour transfer": the mean of the original points nearest to each decoded point; not TMC13-conformant).  With
transfer, and only then, the reports written gain "recolor": "transfer".

The reference starts one Python process per step and one pc_error per report.  Here every step runs in the calling process on
a `Resident`: the GPU context, the original cloud with its normals, octree partition, KD-tree and GPU cell index, and the
model of the current checkpoint with its uploaded weights stay in place between calls (ev_run_experiment makes one Resident
for a whole sweep).  With metrics_device='gpu' the decoded clouds of all groups are measured in one pass against the original's
one CloudIndex.

A step whose outputs exist is skipped, so a killed run resumes where it stopped; a decoded cloud that is missing next to its
.ply.bin is decoded again by the decoder (the same points: encoder and decoder are bit-consistent), which leaves the .ply.bin alone.

enc_dec_d1_psnr_diff is |d1_psnr of .enc.metric.json - d1_psnr of the report|, the reference's encoder / decoder check
(ev_experiment.py:158-162: below 0.01 dB).  consistency='assert' (default) raises AssertionError after all reports are written
when a group misses it, as the reference does; 'warn' logs it.

`resolution` is the size of the voxel grid (1024 for a vox10 cloud), as compress_octree and ev_report take it; --pcerror_cfg_path
may give it instead (a pc_error cfg file holds the peak value, one less).  --pcerror_path, --num_parallel and
--no_stream_redirection are accepted and ignored.
"""
import argparse
import gzip
import json
import logging
import os
import sys

import numpy as np

logger = logging.getLogger(__name__)

DIFF_KEY = 'enc_dec_d1_psnr_diff'
DIFF_BOUND = 0.01
CONSISTENCY = ('assert', 'warn')
RECOLOR = ('rank2', 'transfer')


class Original:
    """An original cloud and everything derived from it alone: read / built on first use, then kept."""

    def __init__(self, resident, input_pc, input_norm, estimate_normals, normals_k):
        assert os.path.exists(input_pc), f'{input_pc} not found'
        assert input_norm is None or os.path.exists(input_norm), f'{input_norm} not found'
        self.resident, self.input_pc, self.input_norm = resident, input_pc, input_norm
        self.estimate, self.normals_k = estimate_normals, normals_k
        self._cache = {}

    def _once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def points(self):
        from .utils import pc_io
        return self._once('points', lambda: pc_io.load_pc(self.input_pc))

    @property
    def normals(self):
        """(N,3) normals from the normals file or the GPU estimator; None without either."""
        def make():
            from . import ops
            from .utils import pc_io
            if self.estimate:
                return ops.estimate_normals(self.resident.ctx, self.points, k=self.normals_k)
            if self.input_norm is not None:
                n = pc_io.load_normals(self.input_norm)
                assert len(n) == len(self.points), 'normals file must have one normal per input point'
                return n
            return None
        return self._once('normals', make)

    @property
    def geometry(self):
        """What the encoder partitions: x y z (+ nx ny nz)."""
        return self._once('geometry', lambda: self.points if self.normals is None else np.hstack((self.points, self.normals)))

    @property
    def xyz64(self):
        return self._once('xyz64', lambda: np.asarray(self.points, np.float64)[:, :3])

    @property
    def colors(self):
        """(N,3) uint8 colours, or None when the file has none."""
        def make():
            from .utils import pc_io
            try:
                return pc_io.load_colors(self.input_pc)
            except ValueError:
                return None
        return self._once('colors', make)

    @property
    def index(self):
        from . import ops
        return self._once('index', lambda: ops.CloudIndex(self.resident.ctx, self.xyz64))

    @property
    def tree(self):
        from scipy.spatial import cKDTree
        return self._once('tree', lambda: cKDTree(self.xyz64, balanced_tree=False))

    def partition(self, box, level):
        from .utils.octree_coding import partition_octree
        return self._once(('partition', tuple(int(v) for v in box), level), lambda: partition_octree(self.geometry, [0, 0, 0], box, level))


class Resident:
    """What outlives one run_experiment call: the GPU context, the originals, and the models of ONE checkpoint (the weights of
    a checkpoint are packed and uploaded when its model first codes; a new checkpoint replaces the previous one's models)."""

    def __init__(self, device=None):
        if int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise AssertionError('the experiment loop runs in one process on one GPU: start it without torch.distributed.run')
        self.device = device
        self._ctx = None
        self.originals = {}
        self._models = {}
        self._checkpoint = None
        self.stats = {'clouds_loaded': 0, 'models_built': 0, 'jobs': 0}

    @property
    def ctx(self):
        if self._ctx is None:
            import torch
            from . import ops
            self._ctx = ops.get_context(torch.device('cuda', 0) if self.device is None else self.device)
        return self._ctx

    def original(self, input_pc, input_norm=None, estimate_normals=False, normals_k=16):
        key = (os.path.abspath(input_pc), None if input_norm is None else os.path.abspath(input_norm), bool(estimate_normals), normals_k)
        if key not in self.originals:
            self.originals[key] = Original(self, input_pc, input_norm, estimate_normals, normals_k)
            self.stats['clouds_loaded'] += 1
        return self.originals[key]

    def model(self, role, model_config, model_dir, batch_size, precision='fp32', block_shape=None):
        """The encoder (role 'enc', for blocks of block_shape) or decoder ('dec') model of a checkpoint, built as the CLIs do."""
        from .model_configs import ModelConfigType
        checkpoint = os.path.abspath(model_dir)
        if checkpoint != self._checkpoint:
            self._models, self._checkpoint = {}, checkpoint
        key = (role, model_config, batch_size, precision, None if block_shape is None else tuple(int(v) for v in block_shape))
        if key not in self._models:
            model = ModelConfigType[model_config].build(data_format='channels_first', batch_size=batch_size, precision=precision)
            if role == 'enc':
                model.compress(np.concatenate(((1,), block_shape)))
            else:
                model.decompress()
            model.restore(model_dir)
            self._models[key] = model
            self.stats['models_built'] += 1
        return self._models[key]


def _progress(src, dst, comment=''):
    join = lambda x: ', '.join(x) if isinstance(x, (list, tuple)) else x
    logger.info(f'[{join(src)}] -> [{join(dst)}] {comment}')


def _encode(res, original, enc_pcs, dec_pcs, model_dir, model_config, resolution, octree_level, opt_metrics, max_deltas,
            fixed_threshold, metrics_device, d2_ties, batch_size, count_threshold=None, count_search=None, latent_step=None, target_bpp=None):
    """compress_octree.compress for one cloud on the resident state: the same arguments, the same plan, the same writer."""
    from . import compress_octree as CO
    from .utils.pc_metric import hausdorff_opt_metrics
    argv = ['--input_files', original.input_pc, '--output_files', *enc_pcs, '--checkpoint_dir', model_dir, '--model_config', model_config,
            '--opt_metrics', *opt_metrics, '--max_deltas', *[str(d) for d in max_deltas], '--resolution', str(resolution),
            '--octree_level', str(octree_level), '--metrics_device', metrics_device, '--d2_ties', d2_ties, '--batch_size', str(batch_size)]
    if original.estimate:
        argv += ['--estimate_normals', '--normals_k', str(original.normals_k)]
    elif original.input_norm is not None:
        argv += ['--input_normals', original.input_norm]
    if dec_pcs is not None:
        argv += ['--dec_files', *dec_pcs]
    if fixed_threshold:
        argv += ['--fixed_threshold']
    if count_threshold is not None:
        argv += ['--count_threshold', repr(float(count_threshold))]
    if count_search is not None:
        # the count search scores d2_* metrics with the GPU engine alone: ask for it where one is requested
        argv += ['--count_search', *[repr(v) for v in count_search]]
        argv += ['--d2_search', 'gpu'] if any(m.startswith('d2_') for m in opt_metrics) else []
    elif any(m.startswith('d2_') and m in hausdorff_opt_metrics for m in opt_metrics):
        argv += ['--d2_search', 'gpu']      # likewise: the d2 Hausdorff terms exist in the GPU engine alone
    if latent_step is not None:
        argv += ['--latent_step', str(int(latent_step))]
    if target_bpp is not None:
        argv += ['--target_bpp', repr(float(target_bpp))]
    args = CO.build_parser().parse_args(argv)
    plan = CO.check_encode_options(args, 1)
    clouds, with_normals = CO._plan(args)
    box, block_shape = CO._block_grid(args.resolution, args.octree_level, args.data_format)
    blocks, binstr = original.partition(box, args.octree_level)
    model = res.model('enc', model_config, model_dir, args.batch_size, args.precision, block_shape)
    model.entropy_coder = args.entropy_coder
    model.d2_search = args.d2_search
    model.search_ties = args.search_ties
    CO.encode_cloud(args, model, res.ctx, clouds[0], blocks, binstr, original.geometry, plan, with_normals, clouds[0].decoded is not None)


def _decode(res, enc_pcs, dec_pcs, model_dir, model_config, batch_size, precision='fp32'):
    """decompress_octree.decompress for some files on the resident state."""
    from .model_syntax import load_compressed_file, read_gzip_tag, stream_layers
    from .stream_layers import decode_mode
    from .utils import pc_io
    from .utils.octree_coding import departition_octree
    sess = res.ctx
    model = res.model('dec', model_config, model_dir, batch_size, precision)
    for enc, dec in zip(enc_pcs, dec_pcs):
        model.entropy_coder, layers = stream_layers(read_gzip_tag(enc), sess.numerics_tag(precision))      # the stream names its coder and layer
        with gzip.open(enc, 'rb') as f:
            resolution, level, binstr, blocks = load_compressed_file(f)
        x_shape = np.array([resolution, resolution, resolution], dtype=np.uint32) // (2 ** level)
        dec_blocks, _ = model.decompress_blocks(sess, blocks, x_shape, debug=False, layers=decode_mode(layers))
        dec_blocks = departition_octree(dec_blocks, binstr, [0, 0, 0], x_shape * (2 ** level), level)
        pa = np.vstack(dec_blocks) if len(dec_blocks) else np.zeros((0, 3))
        pc_io.write_df(dec, pc_io.pa_to_df(pa))


def _recolor(res, original, dec, out, recolor='rank2'):
    """map_color.map_color (rank 2, or mode 'transfer') with the original's resident colours and index."""
    import pandas as pd
    from . import ops
    from .utils import pc_io
    assert recolor in RECOLOR, f'recolor must be one of {RECOLOR}, got {recolor!r}'
    target = pc_io.read_ply(dec)[['x', 'y', 'z']]
    if recolor == 'transfer':
        mapped = ops.transfer_colors(res.ctx, original.index, original.colors, target.values)
    else:
        mapped = ops.map_colors(res.ctx, original.index, original.colors, target.values, rank=2)
    pc_io.write_ply(out, pd.concat([target.reset_index(drop=True),
                                    pd.DataFrame({c: mapped[:, k] for k, c in enumerate(pc_io.COLOR_COLUMNS)})], axis=1))


def measure(res, original, decoded_pcs, enc_pcs, resolution, metrics_device='host', d2_ties='pick'):
    """ev_report.build_report(original, decoded, enc, resolution, normals...) for several decoded clouds of one original, from
    the resident points, normals, KD-tree / CloudIndex: the same dictionaries."""
    from .utils import pc_io
    from .utils.pc_metric import check_ties, cloud_tallies_gpu, cloud_tally_host, compute_metrics, metrics_table
    check_ties(d2_ties)
    a, n1 = original.xyz64, original.normals
    groups = ('d1', 'd2') if n1 is not None else ('d1',)
    clouds = [np.asarray(pc_io.load_pc(p), np.float64)[:, :3] for p in decoded_pcs]
    for b in clouds:
        assert len(b), 'compute_metrics: empty decoded cloud'
    if metrics_device == 'gpu':
        tallies = cloud_tallies_gpu(res.ctx, a, clouds, n1, index_a=original.index, ties=d2_ties)
        tables = [metrics_table(len(a), t[:5], resolution - 1, groups) for t in tallies]
    elif metrics_device == 'host':
        if d2_ties == 'pick':
            tables = [compute_metrics(a, b, resolution - 1, p1_n=n1, t1=original.tree) for b in clouds]
        else:
            tables = [metrics_table(len(a), cloud_tally_host(a, b, n1, t1=original.tree, ties=d2_ties)[:5], resolution - 1, groups)
                      for b in clouds]
    else:
        raise AssertionError(f'metrics_device must be host or gpu, got {metrics_device!r}')
    reports = []
    for m, enc in zip(tables, enc_pcs):
        size = os.stat(enc).st_size
        data = {'pos_total_size_in_bytes': size, 'pos_bits_per_input_point': size * 8 / len(a), 'input_point_count': len(a)}
        data.update({k: float(v) for k, v in m.items() if k in ('d1_mse', 'd1_psnr', 'd2_mse', 'd2_psnr')})
        if d2_ties != 'pick':
            data['d2_ties'] = d2_ties
        reports.append(data)
    return reports


def enc_dec_diff(enc_pc, report):
    """|d1_psnr of <enc_pc>.enc.metric.json - d1_psnr of the report|; 0.0 when both are the same infinity (a lossless point)."""
    with open(enc_pc + '.enc.metric.json') as f:
        enc = json.load(f)
    if enc['d1_psnr'] == report['d1_psnr']:
        return 0.0
    return abs(enc['d1_psnr'] - report['d1_psnr'])


def run_experiment(output_dir, model_dir, model_config, pc_name, input_pc, input_norm=None, estimate_normals=False,
                   opt_metrics=('d1_mse',), max_deltas=(np.inf,), fixed_threshold=False, no_merge_coding=False, metrics_device='host',
                   d2_ties='pick', consistency='assert', resolution=None, octree_level=4, batch_size=32, normals_k=16, resident=None,
                   count_threshold=None, count_search=None, recolor='rank2', latent_step=None, target_bpp=None):
    """See the module docstring.  Returns {group: report dictionary} of the reports that exist afterwards."""
    from .utils.experiment import opt_groups
    from .utils.pc_metric import validate_opt_metrics
    assert consistency in CONSISTENCY, f'consistency must be one of {CONSISTENCY}, got {consistency!r}'
    assert recolor in RECOLOR, f'recolor must be one of {RECOLOR}, got {recolor!r}'
    assert resolution is not None and int(resolution) > 0, 'resolution (the size of the voxel grid) is needed'
    assert not (input_norm and estimate_normals), 'estimate_normals and input_norm are mutually exclusive'
    assert os.path.isdir(model_dir), f'{model_dir} not found'
    opt_metrics, resolution = list(opt_metrics), int(resolution)
    validate_opt_metrics(opt_metrics, with_normals=bool(input_norm) or estimate_normals)
    res = resident if resident is not None else Resident()
    res.stats['jobs'] += 1
    original = res.original(input_pc, input_norm, estimate_normals, normals_k)

    groups = opt_groups(opt_metrics)
    enc_pcs = [os.path.join(output_dir, f'{pc_name}_{g}.ply.bin') for g in groups]
    dec_pcs = [x + '.ply' for x in enc_pcs]
    color_pcs = [x + '.color.ply' for x in dec_pcs]
    report_paths = [os.path.join(output_dir, f'report_{g}.json') for g in groups]
    os.makedirs(output_dir, exist_ok=True)

    # encoding, or encoding + decoding with merged coding
    if all(os.path.exists(x) and os.path.exists(x + '.enc.metric.json') for x in enc_pcs):
        _progress(input_pc, enc_pcs, '(exists)')
    else:
        _progress(input_pc, enc_pcs)
        _encode(res, original, enc_pcs, None if no_merge_coding else dec_pcs, model_dir, model_config, resolution, octree_level,
                opt_metrics, max_deltas, fixed_threshold, metrics_device, d2_ties, batch_size, count_threshold, count_search, latent_step, target_bpp)

    # decoding: whatever the encoder did not leave behind
    todo = [(e, d) for e, d in zip(enc_pcs, dec_pcs) if not os.path.exists(d)]
    if not todo:
        _progress(enc_pcs, dec_pcs, '(exists)')
    else:
        _progress([e for e, _ in todo], [d for _, d in todo])
        _decode(res, [e for e, _ in todo], [d for _, d in todo], model_dir, model_config, batch_size)

    # colour mapping
    for dec, col in zip(dec_pcs, color_pcs):
        if os.path.exists(col):
            _progress(dec, col, '(exists)')
        elif original.colors is not None:
            _progress(dec, col)
            _recolor(res, original, dec, col, recolor)

    # reports: every missing one in one pass over the original
    todo = [k for k, r in enumerate(report_paths) if not os.path.exists(r)]
    failures = []
    if todo:
        _progress('all', [report_paths[k] for k in todo])
        new = measure(res, original, [dec_pcs[k] for k in todo], [enc_pcs[k] for k in todo], resolution, metrics_device, d2_ties)
        for k, data in zip(todo, new):
            data[DIFF_KEY] = diff = enc_dec_diff(enc_pcs[k], data)
            if recolor != 'rank2':
                data['recolor'] = recolor
            tmp = report_paths[k] + '.tmp'
            with open(tmp, 'w') as f:
                json.dump(data, f, sort_keys=True, indent=4)
            os.replace(tmp, report_paths[k])
            logger.info(f'D1 PSNR diff between encoder and decoder: {diff}')
            if not diff < DIFF_BOUND:
                with open(enc_pcs[k] + '.enc.metric.json') as f:
                    failures.append(f'encoded {enc_pcs[k]} with D1 {json.load(f)["d1_psnr"]} but decoded {dec_pcs[k]} with D1 '
                                    f'{data["d1_psnr"]}dB')
    out = {}
    for g, r in zip(groups, report_paths):
        with open(r) as f:
            out[g] = json.load(f)
    for msg in failures:
        logger.warning(msg)
    if failures and consistency == 'assert':
        raise AssertionError('; '.join(failures))
    logger.info('Done')
    return out


def build_parser():
    from .utils.pc_metric import avail_opt_metrics, hausdorff_opt_metrics
    p = argparse.ArgumentParser(prog='ev_experiment.py', description='Run experiment for a point cloud.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--output_dir', help='Output directory', required=True)
    p.add_argument('--model_dir', help='Model directory', required=True)
    p.add_argument('--model_config', help='Model configuration', required=True)
    p.add_argument('--pc_name', help='Point cloud name', required=True)
    p.add_argument('--input_pc', help='Path to input point cloud', required=True)
    p.add_argument('--input_norm', help='Path to input point cloud normals (enables the d2 group)')
    p.add_argument('--estimate_normals', default=False, action='store_true', help='Estimate the normals on the GPU instead (new)')
    p.add_argument('--resolution', type=int, help='Size of the voxel grid, e.g. 1024 (new; or --pcerror_cfg_path)')
    p.add_argument('--octree_level', type=int, default=4, help='Octree level of the encoder (new)')
    p.add_argument('--pcerror_path', help='Accepted and ignored: no external pc_error is run')
    p.add_argument('--pcerror_cfg_path', help='pc_error configuration: its resolution (a peak value) + 1 is the grid size')
    p.add_argument('--opt_metrics', nargs='+', required=True,
                   help=f'Optimization metrics used. Available: {avail_opt_metrics}; worst-point objectives (new): {hausdorff_opt_metrics} '
                        '(one process, --search_ties pick; the d2 ones read the GPU search engine)')
    p.add_argument('--max_deltas', nargs='+', type=float, help='Max deltas tested during optimization.', required=True)
    p.add_argument('--fixed_threshold', help='Enable fixed thresholding.', default=False, action='store_true')
    p.add_argument('--count_threshold', nargs='?', type=float, const=1.0, default=None, metavar='RHO',
                   help='Count-matched thresholding instead of the threshold search, passed to the compress step (new)')
    p.add_argument('--count_search', nargs='*', default=None, metavar='LO HI STEPS',
                   help='Count search instead of the threshold search, passed to the compress step (new; the bare flag is its default '
                        'ladder; d2_* metrics then take their search statistics from the GPU engine)')
    p.add_argument('--latent_step', type=int, default=None, metavar='Q',
                   help='Latent step of the hyperprior models (ladder index 0..63, 16 = the plain stream), passed to the compress step (new)')
    p.add_argument('--target_bpp', type=float, default=None, metavar='R',
                   help='Rate target in bits per input point of the container before gzip, passed to the compress step (new)')
    p.add_argument('--num_parallel', type=int, default=1, help='Accepted and ignored: the steps run in this process')
    p.add_argument('--no_stream_redirection', default=False, action='store_true', help='Accepted and ignored')
    p.add_argument('--no_merge_coding', help='Do not merge encoding and decoding.', default=False, action='store_true')
    p.add_argument('--metrics_device', choices=('host', 'gpu'), default='host', help='Where the whole-cloud metrics run (new)')
    p.add_argument('--d2_ties', choices=('pick', 'mean'), default='pick', help='Tie rule of the whole-cloud D2 (new)')
    p.add_argument('--consistency', choices=CONSISTENCY, default='assert',
                   help='Encoder / decoder D1 PSNR difference of 0.01 dB or more: assert = fail (the reference), warn = log (new)')
    p.add_argument('--batch_size', type=int, default=32, help='Blocks resident on the GPU per pass (new)')
    p.add_argument('--recolor', choices=RECOLOR, default='rank2',
                   help='Colour step of the decoded clouds: rank2 = the reference map_color, transfer = the mean of the nearest original '
                        'points (ops.transfer_colors; not TMC13-conformant; new)')
    return p


def main(argv=None):
    from . import want_hw_queues
    from .compress_octree import count_search_of
    want_hw_queues()
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = build_parser()
    a = p.parse_args(argv)
    resolution = a.resolution
    if resolution is None:
        if a.pcerror_cfg_path is None:
            p.error('--resolution or --pcerror_cfg_path is needed')
        import yaml
        with open(a.pcerror_cfg_path) as f:
            resolution = int(yaml.safe_load(f)['resolution']) + 1
    run_experiment(a.output_dir, a.model_dir, a.model_config, a.pc_name, a.input_pc, a.input_norm, a.estimate_normals, a.opt_metrics,
                   a.max_deltas, a.fixed_threshold, a.no_merge_coding, a.metrics_device, a.d2_ties, a.consistency, resolution,
                   a.octree_level, a.batch_size, count_threshold=a.count_threshold,
                   count_search=count_search_of(a), recolor=a.recolor, latent_step=a.latent_step, target_bpp=a.target_bpp)
    return 0


if __name__ == '__main__':
    sys.exit(main())
